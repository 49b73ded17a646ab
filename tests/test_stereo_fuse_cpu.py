"""CPU-side checks of the fusion of the lifted joints with the keypoint rays (egotap.h: egotap_stereo_fuse): the float64 restatement
spec.stereo_fuse_ref pinned by closed forms that do not depend on it, every mode bit on constructed inputs, and the ABI's exports and refusals
(fake pointers: nothing is launched).

The closed forms are compared in float64 (``dtype="float64"``: the records before their one rounding) on pinhole cameras, whose rays are exact to
rounding.  Each bound is BOUND_OPS * 2^-52 * cond * scale: the solve and what feeds it are a few dozen float64 operations (BOUND_OPS = 64 covers them
and the closed form's own rounding), a symmetric positive-definite 3 x 3 system amplifies a relative perturbation by at most its condition number, and
that number is computed from the weights: the eigenvalues of A = wp I + sum w (I - d d^T) lie in [wp, wp + sum w], so cond <= (wp + wL + wR) / wp.
scale is the largest coordinate involved.  Every check prints the value seen beside its bound."""
import ctypes as C
import math

import numpy as np
import pytest

import ocam_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec

EPS = 2.0 ** -52
BOUND_OPS = 64.0
F = 300.0
THAT = np.array([0.25, -0.5, 0.75], dtype=np.float32)       # exactly representable: x0 = pose + t_hat is one float64 addition of fp32 values
PIN = I.pinhole(F)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _frame(B, n=10.0, that=THAT):
    fr = np.zeros((B, 8), dtype=np.float32)
    fr[:, :3], fr[:, 3] = that, n
    return fr


def _pose_for(x0_wanted, that=THAT):
    """fp32 pose rows whose placed prior is near ``x0_wanted``, and the prior x0 they really give (float64)"""
    pose = (np.asarray(x0_wanted, dtype=np.float64) - that.astype(np.float64)).astype(np.float32)
    return pose, pose.astype(np.float64) + that.astype(np.float64)


def _pixel(d):
    """the pinhole pixel whose ray is along d (d_z > 0)"""
    return F * d[..., :2] / d[..., 2:3]


def _keypoints(B, J, left=None, right=None, score=(0.9, 0.9)):
    """[B, 2, J, 4] float64: points (or None: the centre pixel with score 0, not seen) seen by each eye through identity R"""
    kp = np.zeros((B, 2, J, 4))
    for e, (pts, o) in enumerate(((left, np.zeros(3)), (right, I.T))):
        if pts is not None:
            kp[:, e, :, :2] = _pixel(np.asarray(pts, dtype=np.float64) - o)
            kp[:, e, :, 2] = score[e]
    return kp


def _fuse(kp, pose, frame, prm=None, R=None, dtype="float64", **kw):
    return spec.stereo_fuse_ref(kp, pose, frame, PIN, PIN, I.T, prm or spec.FuseParams(sigma_prior=0.05), R=R, dtype=dtype, **kw)


def _weights(prm, x0, score, origin):
    rho = np.linalg.norm(x0 - origin, axis=-1)
    return score / (prm.sigma_ray * rho) ** 2


def _bound(cond, scale):
    return BOUND_OPS * EPS * cond * scale


def _report(what, seen, bound):
    print(f"{what}: seen {seen:.3e}, bound {bound:.3e}")
    assert seen <= bound, (what, seen, bound)


# ------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("eye", [0, 1], ids=["left", "right"])
def test_one_exact_ray_moves_the_prior_across_the_ray_and_keeps_its_depth_along_it(eye):
    prm = spec.FuseParams(sigma_prior=0.05)
    X = I.joints_in_view(3, 9, seed=11)
    rng = np.random.default_rng(12)
    pose, x0 = _pose_for(X + rng.normal(0, 0.02, X.shape))
    o = (np.zeros(3), I.T)[eye]
    kp = _keypoints(3, 9, left=X if eye == 0 else None, right=X if eye == 1 else None)
    pf, rec, st = _fuse(kp, pose, _frame(3), prm)
    assert (rec[..., 7] == 1 + (2, 4)[eye]).all()
    d = (X - o) / np.linalg.norm(X - o, axis=-1, keepdims=True)
    y0 = x0 - o
    a = (d * y0).sum(-1, keepdims=True)
    r = y0 - a * d
    w, wp = _weights(prm, x0, 0.9, o)[..., None], 1.0 / prm.sigma_prior ** 2
    want = x0 - (w / (wp + w)) * r
    cond = float(((wp + w) / wp).max())
    bound = _bound(cond, np.abs(x0).max())
    _report(f"one eye ({'LR'[eye]}): |x - closed form|, cond {cond:.2f}", np.abs(rec[..., :3] - want).max(), bound)
    _report("one eye: the component along the ray is the prior's", np.abs(((rec[..., :3] - o) * d).sum(-1) - a[..., 0]).max(), bound)
    _report("one eye: move = share |r|", np.abs(rec[..., 3] - (w / (wp + w))[..., 0] * np.linalg.norm(r, axis=-1)).max(), bound)
    _report("one eye: share", np.abs(rec[..., 6] - (w / (wp + w))[..., 0]).max(), BOUND_OPS * EPS)
    assert (rec[..., 5 - eye] == 0).all()                        # the other eye is not used: its res is 0
    np.testing.assert_array_equal(st[:, :4], [[9, 0, 9, 0]] * 3)
    want_rows = (rec[..., :3] - THAT.astype(np.float64)).astype(np.float32)
    assert np.array_equal(_bits(pf), _bits(want_rows))


def test_two_exact_rays_through_the_prior_leave_it_where_it_is():
    prm = spec.FuseParams(sigma_prior=0.05)
    X = I.joints_in_view(2, 7, seed=21).astype(np.float32).astype(np.float64)        # fp32 values: the prior is X itself
    pose, x0 = _pose_for(X, that=np.zeros(3, dtype=np.float32))
    assert np.array_equal(x0, X)
    pf, rec, st = _fuse(_keypoints(2, 7, left=X, right=X), pose, _frame(2, that=np.zeros(3, dtype=np.float32)), prm)
    assert (rec[..., 7] == 7).all()
    wp = 1.0 / prm.sigma_prior ** 2
    cond = float(((wp + _weights(prm, X, 0.9, 0.0) + _weights(prm, X, 0.9, I.T)) / wp).max())
    bound = _bound(cond, np.abs(X).max())
    _report(f"two eyes, prior = X: |x - X|, cond {cond:.2f}", np.abs(rec[..., :3] - X).max(), bound)
    _report("two eyes, prior = X: move", rec[..., 3].max(), bound)
    sr = prm.sigma_ray * np.linalg.norm(X - I.T, axis=-1).min()
    _report("two eyes, prior = X: res (in sigmas)", rec[..., 4:6].max(), bound / sr)
    np.testing.assert_array_equal(st[:, :4], [[7, 7, 0, 0]] * 2)


def test_two_exact_rays_and_a_wide_prior_give_the_analytic_point():
    """X on both rays: A X = wp X + wR M_R t, so x = X + wp A^-1 (x0 - X) -- solved here with numpy, not with the restatement's LDL^T"""
    prm = spec.FuseParams(sigma_prior=10.0)
    X = I.joints_in_view(2, 7, seed=31)
    rng = np.random.default_rng(32)
    pose, x0 = _pose_for(X + rng.normal(0, 0.03, X.shape))
    pf, rec, st = _fuse(_keypoints(2, 7, left=X, right=X), pose, _frame(2), prm)
    assert (rec[..., 7] == 7).all()
    wp = 1.0 / prm.sigma_prior ** 2
    wL, wR = _weights(prm, x0, 0.9, 0.0), _weights(prm, x0, 0.9, I.T)
    want = np.empty_like(X)
    for idx in np.ndindex(X.shape[:2]):
        dL, dR = X[idx] / np.linalg.norm(X[idx]), (X[idx] - I.T) / np.linalg.norm(X[idx] - I.T)
        A = wp * np.eye(3) + wL[idx] * (np.eye(3) - np.outer(dL, dL)) + wR[idx] * (np.eye(3) - np.outer(dR, dR))
        want[idx] = X[idx] + wp * np.linalg.solve(A, x0[idx] - X[idx])
    cond = float(((wp + wL + wR) / wp).max())
    _report(f"two eyes, sigma_prior = 10: |x - analytic|, cond {cond:.3e}", np.abs(rec[..., :3] - want).max(), _bound(cond, np.abs(X).max()))
    assert np.abs(rec[..., :3] - X).max() < np.abs(x0 - X).max()                      # and it did go towards X


@pytest.mark.parametrize("R", [None, I.SMALL_R], ids=["identity", "rotated"])
def test_without_a_gate_exact_rays_and_their_own_point_as_prior_agree_with_the_triangulation(R):
    """max_sigma = +inf, the prior the fp32 point the exact rays go through: the fused point is that point, and so is stereo_triangulate_ref's X"""
    prm = spec.FuseParams(sigma_prior=0.05, max_sigma=math.inf)
    X = I.joints_in_view(3, 17, seed=41).astype(np.float32).astype(np.float64)
    Rm = np.eye(3) if R is None else R
    kp = np.zeros((3, 2, 17, 4))
    kp[:, 0, :, :2], kp[:, 1, :, :2], kp[..., 2] = I.pinhole_pixels(X), I.pinhole_pixels((X - I.T) @ Rm), 0.9
    zero = np.zeros(3, dtype=np.float32)
    pose, x0 = _pose_for(X, that=zero)
    pf, rec, st = _fuse(kp, pose, _frame(3, that=zero), prm, R=R)
    tri, _ = spec.stereo_triangulate_ref(kp, PIN, PIN, I.T, R=R, dtype="float64")
    assert (rec[..., 7] == 7).all() and (tri[..., 7] == 1).all()
    wp = 1.0 / prm.sigma_prior ** 2
    cond = float(((wp + _weights(prm, X, 0.9, 0.0) + _weights(prm, X, 0.9, I.T)) / wp).max())
    _report(f"fused vs triangulated X, cond {cond:.2f}", np.abs(rec[..., :3] - tri[..., :3]).max(), _bound(cond, np.abs(X).max()))


def test_no_eye_seen_leaves_the_prior_and_the_pose_row_in_bits():
    X = I.joints_in_view(2, 5, seed=51)
    pose, x0 = _pose_for(X)
    pf, rec, st = _fuse(_keypoints(2, 5), pose, _frame(2))
    assert (rec[..., 7] == 1).all() and np.array_equal(_bits(rec[..., :3]), _bits(x0)) and (rec[..., 3:7] == 0).all()
    assert np.array_equal(_bits(pf), _bits(pose))
    np.testing.assert_array_equal(st, [[5, 0, 0, 0, 0, 0, 0, 0]] * 2)


# ------------------------------------------------------------------------------------------------ every mode bit, on constructed inputs
def _one_joint(x0_wanted, left=None, right=None, prm=None, score=(0.9, 0.9), kp_edit=None, frame=None, pose_edit=None):
    """one frame, one joint -> (mode, record, pose_fused row, pose row, x0, stats)"""
    pose, x0 = _pose_for(np.asarray(x0_wanted, dtype=np.float64).reshape(1, 1, 3))
    if pose_edit is not None:
        pose_edit(pose)
    kp = _keypoints(1, 1, left=None if left is None else np.reshape(left, (1, 1, 3)), right=None if right is None else np.reshape(right, (1, 1, 3)), score=score)
    if kp_edit is not None:
        kp_edit(kp)
    pf, rec, st = _fuse(kp, pose, _frame(1) if frame is None else frame, prm)
    return int(rec[0, 0, 7]), rec[0, 0], pf[0, 0], pose[0, 0], x0[0, 0], st[0]


X0 = np.array([0.2, -0.1, 1.0])


def _ray_at_g(x0, origin, g, prm):
    """a point whose ray from ``origin`` misses the prior x0 by exactly g prior-and-ray standard deviations (to rounding)"""
    y0 = x0 - origin
    rho = np.linalg.norm(y0)
    sin = g * math.sqrt((prm.sigma_ray * rho) ** 2 + prm.sigma_prior ** 2) / rho
    u = np.cross(y0, [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return origin + y0 / rho * math.sqrt(1 - sin * sin) + u * sin


def _constructed_modes():
    """{name: mode} of the constructed single-joint inputs, each meant to give one named mode"""
    prm = spec.FuseParams(sigma_prior=0.05)
    out = {}
    near = X0 + [0.01, 0.02, 0.0]
    out["both used"] = _one_joint(X0, near, near)[0]
    out["low score left"] = _one_joint(X0, near, near, score=(0.49, 0.9))[0]
    out["low score right"] = _one_joint(X0, near, near, score=(0.9, 0.1))[0]
    out["nan score left"] = _one_joint(X0, near, near, score=(np.nan, 0.9))[0]
    for name, (e, c, v) in {"nan x right": (1, 0, np.nan), "inf y left": (0, 1, np.inf), "-inf x left": (0, 0, -np.inf)}.items():
        def edit(kp, e=e, c=c, v=v):
            kp[0, e, 0, c] = v
        out[name] = _one_joint(X0, near, near, kp_edit=edit)[0]
    for e, o in enumerate((np.zeros(3), I.T)):
        for tag, g in (("below", 3.0 * (1 - 1e-9)), ("above", 3.0 * (1 + 1e-9))):
            p = _ray_at_g(_pose_for(X0)[1], o, g, prm)
            out[f"gate {'LR'[e]} just {tag}"] = _one_joint(X0, p if e == 0 else None, p if e == 1 else None, prm)[0]
    # a prior behind a camera: the prior's depth is negative, every pinhole ray has d_z > 0
    out["prior behind both"] = _one_joint([0.05, 0.05, -0.5], near, near)[0]
    # the prior far to the side: one eye's ray points at it, the other's ray away from it by more than a right angle
    side, away = np.array([1.0, 0.0, 0.05]), np.array([-1.0, 0.0, 0.05])
    out["right not in front, left used"] = _one_joint(side, left=side, right=I.T + away)[0]
    out["left not in front, right used"] = _one_joint(side, left=away, right=side)[0]
    # two rays that each pass the pre-gate (0.15 from the prior, the gate is at 3 * sqrt(0.02^2 + 0.05^2) = 0.16) on opposite sides: no point is within
    # 3 sigma_ray of both
    out["inconsistent rays"] = _one_joint(X0, X0 + [0.0, 0.15, 0.0], X0 - [0.0, 0.15, 0.0])[0]
    return out


WANT_MODES = {"both used": 7, "low score left": 5, "low score right": 3, "nan score left": 5, "nan x right": 3, "inf y left": 5, "-inf x left": 5,
              "gate L just below": 3, "gate L just above": 9, "gate R just below": 5, "gate R just above": 17, "prior behind both": 97,
              "right not in front, left used": 67, "left not in front, right used": 37, "inconsistent rays": 135}


def test_every_mode_bit_on_a_constructed_input():
    got = _constructed_modes()
    assert got == WANT_MODES, {k: (got[k], WANT_MODES[k]) for k in got if got[k] != WANT_MODES[k]}


def test_a_rejected_fit_falls_back_to_the_prior_in_bits():
    mode, rec, row, pose_row, x0, st = _one_joint(X0, X0 + [0.0, 0.15, 0.0], X0 - [0.0, 0.15, 0.0])
    assert mode == 135 and np.array_equal(_bits(rec[:3]), _bits(x0)) and np.array_equal(_bits(row), _bits(pose_row))
    assert rec[3] == 0 and rec[6] == 0 and (rec[4:6] > 3.0).all(), rec          # the residuals of the fit that was tried stay: they say why
    np.testing.assert_array_equal(st, [1, 0, 0, 2, 0, 0, 0, 0])
    # a solve that is not finite (sigma_ray so small that sr^2 underflows: w = inf) falls back too, with res written as 0
    mode, rec, row, pose_row, x0, st = _one_joint(X0, X0, None, prm=spec.FuseParams(sigma_prior=0.05, sigma_ray=1e-200))
    assert mode == 131 and np.array_equal(_bits(rec[:3]), _bits(x0)) and np.array_equal(_bits(row), _bits(pose_row)) and (rec[3:7] == 0).all(), rec
    np.testing.assert_array_equal(st, [1, 0, 0, 1, 0, 0, 0, 0])


@pytest.mark.parametrize("cause", ["n below min_joints", "n NaN", "t_hat NaN", "t_hat inf"])
def test_a_frame_without_a_root_passes_through(cause):
    X = I.joints_in_view(2, 6, seed=61)
    pose, x0 = _pose_for(X + np.random.default_rng(62).normal(0, 0.02, X.shape))
    pose = np.concatenate([np.full((2, 1, 3), 7.0, dtype=np.float32), pose, np.full((2, 2, 3), -7.0, dtype=np.float32)], axis=1)
    fr = _frame(2)
    if cause == "n below min_joints":
        fr[1, 3] = 2.0
    elif cause == "n NaN":
        fr[1, 3] = np.nan
    else:
        fr[1, 1] = np.nan if cause == "t_hat NaN" else np.inf
    pf, rec, st = _fuse(_keypoints(2, 6, left=X, right=X), pose, fr, pose_row0=1)
    assert (rec[0, :, 7] == 7).all() and st[0, 0] == 6                           # the frame beside it is fused
    assert (rec[1] == 0).all() and (st[1] == 0).all() and np.array_equal(_bits(pf[1]), _bits(pose[1]))
    assert np.array_equal(_bits(pf[0, [0, 7, 8]]), _bits(pose[0, [0, 7, 8]]))    # rows outside the joint rows: the input's bits
    assert not np.array_equal(pf[0, 1:7], pose[0, 1:7])
    pf3, rec3, st3 = _fuse(_keypoints(2, 6, left=X, right=X), pose, _frame(2, n=2.0), spec.FuseParams(sigma_prior=0.05, min_joints=2), pose_row0=1)
    assert (rec3[..., 7] == 7).all()                                             # n >= min_joints: equality counts


def test_a_pose_row_that_is_not_finite_has_no_prior_and_keeps_its_bits():
    X = I.joints_in_view(1, 4, seed=71)
    pose, x0 = _pose_for(X)
    pose[0, 1, 2] = np.nan
    pose[0, 2, 0] = -np.inf
    _bits(pose)[0, 3, 1] = 0x7FC00123                                            # a NaN with a payload
    pf, rec, st = _fuse(_keypoints(1, 4, left=X, right=X), pose, _frame(1))
    assert rec[0, 0, 7] == 7 and (rec[0, 1:] == 0).all() and np.array_equal(_bits(pf[0, 1:]), _bits(pose[0, 1:]))
    np.testing.assert_array_equal(st[0, :4], [1, 1, 0, 0])


def _pinhole_mixed(seed, R):
    """tests/ocam_inputs.pinhole_case(5, 17, seed) with a prior = X + N(0, 0.03) noise"""
    kp, X, kind = I.pinhole_case(5, 17, seed, R=R)
    pose, x0 = _pose_for(X + np.random.default_rng(seed).normal(0, 0.03, X.shape))
    return kp.astype(np.float32), pose, _frame(5), R


def test_the_inputs_cover_every_mode_named_here():
    seen = set(_constructed_modes().values())
    for seed, R in ((3, None), (4, I.SMALL_R)):
        kp, pose, fr, R = _pinhole_mixed(seed, R)
        pf, rec, st = _fuse(kp, pose, fr, R=R, dtype="float32")
        mode = rec[..., 7].astype(int)
        seen |= set(mode.ravel().tolist())
        for e in range(2):                                        # an eye is used, gated or not in front: never two of them
            assert (((mode >> (1 + e)) & 1) + ((mode >> (3 + e)) & 1) + ((mode >> (5 + e)) & 1) <= 1).all()
        both, one, fb = (mode & 6) == 6, ((mode & 6) != 0) & ((mode & 6) != 6), (mode & 128) != 0
        rej = sum(((mode >> k) & 1) for k in (3, 4, 5, 6))
        np.testing.assert_array_equal(st[:, 0], (mode & 1).sum(1))
        np.testing.assert_array_equal(st[:, 1], (both & ~fb).sum(1))
        np.testing.assert_array_equal(st[:, 2], (one & ~fb).sum(1))
        np.testing.assert_array_equal(st[:, 3], (rej + np.where(fb, ((mode >> 1) & 1) + ((mode >> 2) & 1), 0)).sum(1))
    print("modes seen:", sorted(seen))
    assert {3, 5, 7, 13, 19, 25} <= seen, sorted(seen)            # from pinhole_case alone
    assert {37, 67, 97, 9, 17, 135} <= seen, sorted(seen)          # the constructed ones
    assert 35 not in seen                                         # left used AND left not in front: excluded by the definition


def test_permuting_frames_permutes_the_outputs():
    kp, pose, fr, R = _pinhole_mixed(4, I.SMALL_R)
    fr[2, 3] = 1.0                                                # one frame without a root
    perm = np.array([3, 0, 4, 2, 1])
    a = _fuse(kp, pose, fr, R=R, dtype="float32")
    b = _fuse(kp[perm], pose[perm], fr[perm], R=R, dtype="float32")
    for x, y in zip(a, b):
        assert np.array_equal(_bits(x[perm]), _bits(y))


def test_restatement_refusals_and_parameters():
    kp, pose, fr, R = _pinhole_mixed(3, None)
    with pytest.raises(TypeError):
        spec.FuseParams()                                         # sigma_prior has no default
    for bad in (dict(sigma_prior=0.0), dict(sigma_prior=math.inf), dict(sigma_prior=0.05, sigma_ray=-1.0), dict(sigma_prior=0.05, sigma_ray=math.nan),
                dict(sigma_prior=0.05, max_sigma=-1.0), dict(sigma_prior=0.05, max_sigma=math.nan), dict(sigma_prior=0.05, min_joints=-1)):
        with pytest.raises(ValueError, match="FuseParams"):
            spec.FuseParams(**bad)
    p = spec.FuseParams(sigma_prior=0.05)
    assert (p.sigma_ray, p.max_sigma, p.min_joints) == (0.02, 3.0, 3) and spec.FuseParams(sigma_prior=1.0, max_sigma=math.inf).max_sigma == math.inf
    with pytest.raises(ValueError, match="keypoints"):
        _fuse(kp[:, :1], pose, fr)
    with pytest.raises(ValueError, match="pose_row0"):
        _fuse(kp, pose, fr, pose_row0=1)
    with pytest.raises(ValueError, match="frame"):
        _fuse(kp, pose, fr[:, :4])
    with pytest.raises(ValueError, match="FuseParams"):
        spec.stereo_fuse_ref(kp, pose, fr, PIN, PIN, I.T, None)


# ------------------------------------------------------------------------------------------------ the ABI and the Python faces
def test_the_entry_is_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    assert "egotap_stereo_fuse" in L.exported_symbols() and hasattr(lib, "egotap_stereo_fuse") and "int egotap_stereo_fuse(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert C.sizeof(L.EgotapFuseParams) == 32
    o = L.fuse_params_struct(spec.FuseParams(sigma_prior=0.07, max_sigma=math.inf))
    assert (o.sigma_ray, o.sigma_prior, o.max_sigma, o.min_joints) == (0.02, 0.07, math.inf, 3)


def test_stereo_fuse_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    B, J, Pn = 3, 15, 16
    kp, pose, fr, fu, pf, st = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000
    D3, D9, D8 = C.c_double * 3, C.c_double * 9, C.c_double * 8
    cam = L.ocam_struct(I.calibration(1))

    def prm(**kw):
        o = L.fuse_params_struct(spec.FuseParams(sigma_prior=0.05))
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    ok = dict(kp=P(kp), B=B, J=J, left=cam, right=cam, R=None, t=D3(0.1, 0.0, 0.0), aff=None, ms=0.5, pose=P(pose), P=Pn, row0=1, fr=P(fr), prm=prm(), fu=P(fu),
              pf=P(pf), st=P(st))

    def call(**kw):
        a = dict(ok, **kw)
        by = lambda m: C.byref(m) if m is not None else None      # noqa: E731
        rc = lib.egotap_stereo_fuse(a["kp"], a["B"], a["J"], by(a["left"]), by(a["right"]), a["R"], a["t"], a["aff"], a["ms"], a["pose"], a["P"], a["row0"], a["fr"],
                                    by(a["prm"]), a["fu"], a["pf"], a["st"], None)
        return rc, lib.egotap_last_error().decode()
    nan, inf = float("nan"), float("inf")
    kp_b, pose_b, fr_b, fu_b = B * 2 * J * 16, B * Pn * 12, B * 32, B * J * 32
    bad_cam = L.ocam_struct(I.calibration(1))
    bad_cam.n_pol = 0
    cases = [(dict(kp=None), "null"), (dict(t=None), "null"), (dict(pose=None), "null"), (dict(fr=None), "null"), (dict(prm=None), "null"), (dict(fu=None), "null"),
             (dict(pf=None), "null"), (dict(st=None), "null"), (dict(left=None), "left: null camera model"), (dict(right=None), "right: null camera model"),
             (dict(left=bad_cam), "left: polynomialC2W"), (dict(right=bad_cam), "right: polynomialC2W"),
             (dict(B=0), "must be positive"), (dict(J=0), "must be positive"), (dict(B=-1), "must be positive"), (dict(J=65), "at most 64 joints"),
             (dict(kp=P(kp + 8)), "16-byte aligned"), (dict(fr=P(fr + 4)), "16-byte aligned"), (dict(fu=P(fu + 8)), "16-byte aligned"), (dict(st=P(st + 4)), "16-byte aligned"),
             (dict(pose=P(pose + 2)), "4-byte aligned"), (dict(pf=P(pf + 1)), "4-byte aligned"),
             (dict(row0=2), "pose rows"), (dict(row0=-1), "pose rows"), (dict(P=14, row0=0), "pose rows"),
             (dict(ms=nan), "must be finite"), (dict(ms=inf), "must be finite"), (dict(t=D3(0.1, nan, 0.0)), "must be finite"),
             (dict(R=D9(1, 0, 0, 0, 1, 0, 0, inf, 1)), "must be finite"), (dict(aff=D8(4, 0, 4, 0, 4, nan, 4, 0)), "must be finite"),
             (dict(prm=prm(sigma_ray=0.0)), "sigma_ray"), (dict(prm=prm(sigma_ray=nan)), "sigma_ray"), (dict(prm=prm(sigma_ray=inf)), "sigma_ray"),
             (dict(prm=prm(sigma_prior=-0.05)), "sigma_prior"), (dict(prm=prm(sigma_prior=nan)), "sigma_prior"), (dict(prm=prm(sigma_prior=inf)), "sigma_prior"),
             (dict(prm=prm(max_sigma=nan)), "max_sigma"), (dict(prm=prm(max_sigma=-1.0)), "max_sigma"), (dict(prm=prm(min_joints=-1)), "min_joints"),
             (dict(fu=P(kp)), "fused overlaps keypoints"), (dict(fu=P(kp + kp_b - 16)), "fused overlaps keypoints"), (dict(fu=P(pose + pose_b - 16)), "fused overlaps pose"),
             (dict(fu=P(fr)), "fused overlaps frame"), (dict(st=P(fr + fr_b - 32)), "stats overlaps frame"), (dict(st=P(kp + 32)), "stats overlaps keypoints"),
             (dict(st=P(pose)), "stats overlaps pose"), (dict(pf=P(kp)), "pose_fused overlaps keypoints"), (dict(pf=P(fr)), "pose_fused overlaps frame"),
             (dict(pf=P(pose + 12)), "pose_fused overlaps pose"), (dict(pf=P(pose - 12)), "pose_fused overlaps pose"),       # in place is pose_fused == pose only
             (dict(pf=P(fu + fu_b - 4)), "fused overlaps pose_fused"), (dict(st=P(fu)), "fused overlaps stats"), (dict(st=P(pf + 16)), "pose_fused overlaps stats")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_stereo_fuse:") and word in msg, (kw, rc, msg)


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch
    from egotap_amd import models as M
    cam = I.calibration(0)
    prm = spec.FuseParams(sigma_prior=0.05)
    kp, pose, fr = torch.zeros(2, 2, 15, 4), torch.zeros(2, 16, 3), torch.zeros(2, 8)
    t = (0.1, 0.0, 0.0)
    with pytest.raises(ValueError, match="FuseParams"):
        L.stereo_fuse(kp, pose, fr, cam, cam, t, None)
    with pytest.raises(ValueError, match="3 values"):
        L.stereo_fuse(kp, pose, fr, cam, cam, (0.1, 0.0), prm)
    with pytest.raises(ValueError, match=r"\[2, 4\]"):
        L.stereo_fuse(kp, pose, fr, cam, cam, t, prm, affine=[(4.0, 0.0, 4.0, 0.0)])
    with pytest.raises(ValueError, match="keypoints"):
        L.stereo_fuse(kp[:, :1], pose, fr, cam, cam, t, prm)
    with pytest.raises(ValueError, match="pose_row0"):
        L.stereo_fuse(kp, pose, fr, cam, cam, t, prm, pose_row0=2)
    with pytest.raises(ValueError, match="frame"):
        L.stereo_fuse(kp, pose, fr[:1], cam, cam, t, prm)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.stereo_fuse(kp, pose, fr, cam, cam, t, prm, pose_row0=1)
    fusion = M.StereoFusion(cam, cam, t, prm, pose_row0=1)
    with pytest.raises(ValueError, match="StereoFusion.update: keypoints"):
        fusion.update(pose, kp[:, :1], fr)
    with pytest.raises(L.EgotapError, match="StereoFusion.update runs on the GPU only"):
        fusion.update(pose, kp, fr)
    with pytest.raises(ValueError, match="FuseParams"):
        M.StereoFusion(cam, cam, t, None)
    # the model's factory: by name without a rig, sigma_prior required, the three kinds of affine
    model = M.EgoTAPAutoEncoderModel.__new__(M.EgoTAPAutoEncoderModel)
    torch.nn.Module.__init__(model)
    with pytest.raises(L.EgotapError, match="set_stereo_rig"):
        model.new_stereo_fusion(0.05)
    with pytest.raises(TypeError):
        model.new_stereo_fusion()
