"""CPU-side checks of the temporal filter in a world frame (egotap.h: egotap_pose_track_world): the float64 restatement spec.pose_track_world_ref pinned
by what does not depend on it -- the camera-frame restatement under an identity rig pose, a motionless world under a turning head, covariance under a
change of world, rig poses that do not count against "the frame removed", chunking and stream permutation -- then spec.rig_pose / rig_compose, and the
ABI's export and refusals (fake pointers: nothing is launched) and the Python faces' argument checks."""
import ctypes as C
import itertools

import numpy as np
import pytest

import pose_track_inputs as I
import pose_track_world_inputs as W
from egotap_amd import lib as L
from egotap_amd import spec

DT = W.DT
NK = spec.POSE_TRACK_STATE


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    view = np.int64 if a.dtype == np.float64 else np.int32
    assert np.array_equal(a.view(view), b.view(view)), np.argwhere(a.view(view) != b.view(view))[:8]


def _plus_zero(a):
    return None if a is None else a + 0.0                            # -0 + 0 is +0: what the identity transform makes of a negative zero


# ------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("shape", [(1, 1, 16, 15), (7, 1, 16, 15), (3, 5, 17, 0), (2, 4, 64, 64), (1, 9, 16, 15), (7, 2, 5, 4)], ids=lambda s: "T%d_S%d_P%d_J%d" % s)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_identity_rig_pose_gives_the_camera_frame_bits(shape, dtype):
    T, S, P, J = shape
    pose, frame, j3, state0 = (_plus_zero(a) for a in I.case(T, S, P, J))
    assert not any(np.signbit(a[a == 0]).any() for a in (pose, frame, j3, state0) if a is not None)
    want = spec.pose_track_ref(pose, state0, DT, I.PARAMS, frame=frame, joints3d=j3, streams=S, dtype=dtype)
    got = spec.pose_track_world_ref(pose, state0, np.tile(W.IDENTITY, (T * S, 1)), DT, I.PARAMS, frame=frame, joints3d=j3, streams=S, dtype=dtype)
    assert set(want[0][..., 7].ravel()) >= {1.0, 2.0}
    _bits(got[0], want[0])
    _bits(got[1], want[1])
    _bits(got[2], want[1])                                            # placed_cam: back through the identity
    _bits(got[3], want[2])


# ------------------------------------------------------------------------------------------------ 2. a motionless world under a moving rig
def test_a_motionless_world_stays_still_under_a_turning_head():
    w = W.still_world()
    P, J, T, top, dt = W.STILL_P, W.STILL_J, W.STILL_T, w["top"], w["dt"]
    assert 281.0 <= top <= 283.0
    prm = spec.TrackParams()
    z = np.zeros((1, P + 1 + J, NK))
    tracks, pw, pc, _ = spec.pose_track_world_ref(w["pose"], z, w["rig"], dt, prm, frame=w["frame"], joints3d=w["joints3d"], dtype="float64")
    truth = np.concatenate([w["pose_w"], w["root_w"][None], w["joints_w"]])
    assert (tracks[..., 7] == 1).all()
    ex = np.abs(tracks[..., 0:3] - truth).max()
    ev = np.abs(tracks[..., 3:6]).max()
    ec = np.abs(tracks[..., 6] - 1.0).max()                           # min_cutoff of the defaults
    epw, epc = np.abs(pw - w["placed_w"]).max(), np.abs(pc - w["placed_c"]).max()
    # the camera-frame filter on the same measurements
    _, placed_cam_frame, _ = spec.pose_track_ref(w["pose"], z, dt, prm, frame=w["frame"], joints3d=w["joints3d"], dtype="float64")
    off = np.linalg.norm(placed_cam_frame - w["placed_c"], axis=-1)
    print(f"world: |x^ - truth| {ex:.3g} ({ex / top:.3g} relative), |v^| {ev:.3g}, |cutoff - min_cutoff| {ec:.3g}, placed_world {epw:.3g}, placed_cam {epc:.3g};"
          f"  camera frame: placed off by up to {off.max():.3g}, mean {off.mean():.3g}")
    assert ex <= 1e-12 * top and epw <= 1e-12 * top and epc <= 1e-12 * top
    assert ev <= 1e-9 * top
    assert ec <= 1e-9
    assert off.max() > 1.0                                            # the contrast this entry exists for


# ------------------------------------------------------------------------------------------------ 3. covariance
def test_a_change_of_world_moves_the_outputs_with_it():
    T, S, P, J = 9, 2, 6, 5
    pose, frame, j3, rig = W.clean_case(T, S, P, J, seed=11)
    frame[3 * S, 3] = 0.0                                             # a held root, a held joint and a held pose row on the way
    j3[4 * S + 1, 2, 7] = 0.0
    pose[5 * S, 1, 0] = np.nan
    Wm = spec.rig_pose([3.0, -2.0, 0.5], R=W.rot(2, 0.7) @ W.rot(0, -1.1))
    z = np.zeros((S, P + 1 + J, NK))
    a = spec.pose_track_world_ref(pose, z, rig, DT, W.PARAMS, frame=frame, joints3d=j3, streams=S, dtype="float64")
    b = spec.pose_track_world_ref(pose, z, spec.rig_compose(Wm, rig), DT, W.PARAMS, frame=frame, joints3d=j3, streams=S, dtype="float64")
    Rw, tw = Wm.reshape(3, 4)[:, :3], Wm.reshape(3, 4)[:, 3]
    _bits(a[0][..., 7], b[0][..., 7])
    assert set(a[0][..., 7].ravel()) == {1.0, 2.0}
    live = a[0][..., 7:8] != 0
    point = (np.arange(P + 1 + J) >= P)[None, :, None]
    top = max(np.abs(a[0][..., 0:3]).max(), np.abs(b[0][..., 0:3]).max(), np.abs(a[1]).max(), np.abs(b[1]).max())
    moved = np.where(live, a[0][..., 0:3] @ Rw.T + np.where(point, tw, 0.0), 0.0)
    ex = np.abs(b[0][..., 0:3] - moved).max()
    ev = np.abs(b[0][..., 3:6] - a[0][..., 3:6] @ Rw.T).max()
    ec = np.abs(b[0][..., 6] - a[0][..., 6]).max() / np.abs(a[0][..., 6]).max()
    epw = np.abs(b[1] - (a[1] @ Rw.T + tw)).max()                     # every pose row here has its root: placed is a point
    epc = np.abs(b[2] - a[2]).max()
    print(f"covariance: x^ {ex:.3g}, v^ {ev:.3g}, cutoff {ec:.3g} relative, placed_world {epw:.3g}, placed_cam {epc:.3g}, bound {1e-12 * top:.3g}")
    assert (a[0][:, P, 7] != 0).all()
    assert max(ex, epw, epc, ev) <= 1e-12 * top
    assert ec <= 1e-12


# ------------------------------------------------------------------------------------------------ 4. a rig pose that is not seen
def _break(g, how):
    g = g.copy()
    if how == "nan":
        g[5] = np.nan
    elif how == "past_tol":
        g[0:3] *= 1.0 + 0.6 * W.ORTHO_TOL                             # |E_00| = 1.2 tol
    elif how == "inside_tol":
        g[0:3] *= 1.0 + 0.4 * W.ORTHO_TOL                             # |E_00| = 0.8 tol
    elif how == "reflection":
        g[8:11] *= -1.0
    return g


@pytest.mark.parametrize("how", ["nan", "past_tol", "inside_tol", "reflection"])
def test_a_rig_pose_that_is_not_seen_is_a_missing_frame(how):
    T, S, P, J = 12, 1, 4, 3
    pose, frame, j3, rig = W.clean_case(T, S, P, J, seed=21)
    bad = [5, 6]
    broken = rig.copy()
    for t in bad:
        broken[t] = _break(rig[t], how)
    z = np.zeros((S, P + 1 + J, NK))
    full = spec.pose_track_world_ref(pose, z, broken, np.full(T, DT), W.PARAMS, frame=frame, joints3d=j3, dtype="float64", ortho_tol=W.ORTHO_TOL)
    if how == "inside_tol":                                           # accepted: every track updates, and the pose is read as it is
        assert (full[0][..., 7] == 1).all() and (full[2][bad] != 0).all()
        plain = spec.pose_track_world_ref(pose, z, rig, np.full(T, DT), W.PARAMS, frame=frame, joints3d=j3, dtype="float64", ortho_tol=W.ORTHO_TOL)
        assert not np.array_equal(full[0][bad], plain[0][bad])
        return
    assert (full[0][bad][..., 7] == 2).all() and (np.delete(full[0], bad, axis=0)[..., 7] == 1).all()
    assert (full[0][bad][..., 6] == 0).all()
    _bits(full[0][5][:, 0:6], full[0][4][:, 0:6])                     # every track holds
    _bits(full[1][5], full[1][4])                                     # placed_world holds with them
    assert (full[2][bad] == 0).all() and (full[2][4] != 0).all()      # placed_cam: no camera to bring it back to
    dts = np.full(T - 2, DT)
    dts[5] = 3 * DT
    cut = lambda a: np.delete(a, bad, axis=0)                         # noqa: E731
    short = spec.pose_track_world_ref(cut(pose), z, cut(rig), dts, W.PARAMS, frame=cut(frame), joints3d=cut(j3), dtype="float64", ortho_tol=W.ORTHO_TOL)
    for k in range(3):
        _bits(cut(full[k]), short[k])
    _bits(full[3], short[3])
    assert np.isfinite(full[3]).all()


# ------------------------------------------------------------------------------------------------ 5. splits and streams
def _compositions(n):
    for cuts in itertools.product((0, 1), repeat=n - 1):
        parts, run = [], 1
        for c in cuts:
            if c:
                parts.append(run)
                run = 1
            else:
                run += 1
        yield parts + [run]


def test_any_chunking_gives_the_bits_of_one_call():
    T, S, P, J = 7, 2, 5, 4
    pose, frame, j3, rig, state0 = W.case(T, S, P, J, seed=8)
    dts = np.array([DT, 2 * DT, DT, 0.0, DT, DT / 2, DT], dtype=np.float32)
    kw = dict(streams=S, ortho_tol=W.ORTHO_TOL)
    start = state0.copy()
    whole = spec.pose_track_world_ref(pose, state0, rig, dts, W.PARAMS, frame=frame, joints3d=j3, **kw)
    _bits(state0, start)                                              # the state given is not written: in place equals out of place
    assert set(whole[0][..., 7].ravel()) == {0.0, 1.0, 2.0}
    seen = ~(whole[2] == 0).all(axis=(1, 2))
    assert seen.any() and not seen.all()
    n = 0
    for parts in _compositions(T):
        st, lo, outs = state0, 0, ([], [], [])
        for n_t in parts:
            sl = slice(lo * S, (lo + n_t) * S)
            *rec, st = spec.pose_track_world_ref(pose[sl], st, rig[sl], dts[lo:lo + n_t], W.PARAMS, frame=frame[sl], joints3d=j3[sl], **kw)
            for o, r in zip(outs, rec):
                o.append(r)
            lo += n_t
        for o, want in zip(outs, whole):
            _bits(np.concatenate(o), want)
        _bits(st, whole[3])
        n += 1
    assert n == 64


def test_permuting_the_streams_permutes_the_outputs():
    T, S, P, J = 5, 4, 6, 3
    pose, frame, j3, rig, state0 = W.case(T, S, P, J, seed=9)
    perm = np.array([2, 0, 3, 1])

    def by_stream(a):
        return a.reshape((T, S) + a.shape[1:])[:, perm].reshape(a.shape)
    a = spec.pose_track_world_ref(pose, state0, rig, DT, W.PARAMS, frame=frame, joints3d=j3, streams=S)
    b = spec.pose_track_world_ref(by_stream(pose), state0[perm], by_stream(rig), DT, W.PARAMS, frame=by_stream(frame), joints3d=by_stream(j3), streams=S)
    for k in range(3):
        _bits(by_stream(a[k]), b[k])
    _bits(a[3][perm], b[3])
    assert not np.array_equal(a[0], b[0])


def test_the_shared_case_meets_every_branch():
    """the inputs the device tests use: rig poses that count and every kind that does not, over tracks of every status, from a state under way"""
    pose, frame, j3, rig, state0 = W.case(7, 5, 17, 15, seed=1)
    assert (state0[..., 11] == 1).any() and (state0[..., 11] == 0).any() and (state0[..., 10] > 0).any() and (state0[..., 9] > 0).any()
    g = rig.reshape(-1, 3, 4)
    R = g[:, :, :3]
    with np.errstate(all="ignore"):
        finite = np.isfinite(g).all(axis=(1, 2))
        ortho = np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max(axis=(1, 2)) <= W.ORTHO_TOL
        right = np.linalg.det(np.where(np.isfinite(R), R, 0.0)) > 0
    assert (~finite).any() and np.isnan(g).any() and np.isinf(g).any() and (finite & ~ortho).any() and (finite & ortho & ~right).any() and (finite & ortho & right).any()
    tracks, pw, pc, _ = spec.pose_track_world_ref(pose, state0, rig, DT, W.PARAMS, frame=frame, joints3d=j3, streams=5, ortho_tol=W.ORTHO_TOL)
    seen = finite & ortho & right
    assert (pc[~seen] == 0).all() and (pw[~seen] != 0).any() and (pc[seen] != 0).any()
    assert (tracks[~seen][..., 7] != 1).all()
    st = tracks.reshape(7, 5, 33, 8)[..., 7]
    assert {(int(a), int(b)) for a, b in zip(st[:-1].ravel(), st[1:].ravel())} == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (2, 0)}


def test_the_restatement_refuses_by_name():
    z = np.zeros((1, 3, NK))
    pose = np.zeros((3, 2, 3))
    g = np.tile(W.IDENTITY, (3, 1))
    with pytest.raises(ValueError, match="rig_pose is"):
        spec.pose_track_world_ref(pose, z, g[:2], DT)
    with pytest.raises(ValueError, match="rig_pose is"):
        spec.pose_track_world_ref(pose, z, g[:, :9], DT)
    for tol in (-1e-9, np.nan):
        with pytest.raises(ValueError, match="ortho_tol"):
            spec.pose_track_world_ref(pose, z, g, DT, ortho_tol=tol)
    with pytest.raises(ValueError, match="pose_track_world_ref: state is"):
        spec.pose_track_world_ref(pose, np.zeros((1, 2, NK)), g, DT)
    with pytest.raises(ValueError, match="pose_track_world_ref: dts holds"):
        spec.pose_track_world_ref(pose, z, g, np.full(2, DT))
    assert (spec.pose_track_world_ref(pose, z, g, DT, ortho_tol=0.0)[0][:, :2, 7] == 1).all()        # the identity is exact
    assert (spec.pose_track_world_ref(pose, z, g * 3.0, DT, ortho_tol=np.inf)[0][:, :2, 7] == 1).all()      # +inf: any finite right-handed matrix


# ------------------------------------------------------------------------------------------------ 6. rig_pose / rig_compose
def test_rig_pose_from_quaternions_and_composition():
    h = np.sqrt(0.5)
    quarter = {(h, h, 0, 0): [[1, 0, 0], [0, 0, -1], [0, 1, 0]],      # about x: y -> z
               (h, 0, h, 0): [[0, 0, 1], [0, 1, 0], [-1, 0, 0]],      # about y: z -> x
               (h, 0, 0, h): [[0, -1, 0], [1, 0, 0], [0, 0, 1]],      # about z: x -> y
               (1, 0, 0, 0): np.eye(3)}
    t = np.array([1.0, -2.0, 3.0])
    for q, R in quarter.items():
        g = spec.rig_pose(t, quat=q)
        assert g.shape == (12,) and g.dtype == np.float64
        assert np.abs(g.reshape(3, 4)[:, :3] - np.array(R, dtype=np.float64)).max() <= 4e-16, q
        _bits(g.reshape(3, 4)[:, 3], t)
        assert np.abs(spec.rig_pose(t, quat=np.array(q) * -37.5) - g).max() <= 4e-16      # any scale, either sign: the same rotation
        _bits(spec.rig_pose(t, R=R), np.concatenate([np.array(R, dtype=np.float64), t[:, None]], axis=1).ravel())
    _bits(spec.rig_pose([0.0, 0.0, 0.0]), W.IDENTITY)
    many = spec.rig_pose(np.zeros((5, 2, 3)), quat=[h, 0, 0, h])      # leading dimensions broadcast
    assert many.shape == (5, 2, 12)
    for bad in ([0, 0, 0, 0], [np.nan, 0, 0, 1], [np.inf, 0, 0, 0], [1e200, 1e200, 0, 0]):
        with pytest.raises(ValueError, match="norm"):
            spec.rig_pose(t, quat=bad)
    with pytest.raises(ValueError, match="quat is"):
        spec.rig_pose(t, quat=[1, 0, 0])
    with pytest.raises(ValueError, match="R is"):
        spec.rig_pose(t, R=np.eye(4))
    with pytest.raises(ValueError, match="t is"):
        spec.rig_pose([1.0, 2.0], R=np.eye(3))
    with pytest.raises(ValueError, match="not both"):
        spec.rig_pose(t, R=np.eye(3), quat=[1, 0, 0, 0])
    # composition: b and then a
    rng = np.random.default_rng(12)
    a = spec.rig_pose(rng.normal(0, 1, (4, 3)), quat=rng.normal(0, 1, (4, 4)))
    b = spec.rig_pose(rng.normal(0, 1, (4, 3)), quat=rng.normal(0, 1, (4, 4)))
    x = rng.normal(0, 1, (4, 3))
    apply = lambda g, x: np.einsum("nij,nj->ni", g.reshape(-1, 3, 4)[:, :, :3], x) + g.reshape(-1, 3, 4)[:, :, 3]      # noqa: E731
    ab = spec.rig_compose(a, b)
    assert ab.shape == (4, 12) and np.abs(apply(ab, x) - apply(a, apply(b, x))).max() <= 1e-14
    assert np.abs(spec.rig_compose(a[0], b) - spec.rig_compose(np.tile(a[0], (4, 1)), b)).max() == 0      # broadcasts
    with pytest.raises(ValueError, match="rig_compose"):
        spec.rig_compose(a[:, :9], b)
    # the composed poses still count as rotations
    R = ab.reshape(-1, 3, 4)[:, :, :3]
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() <= 1e-14 and (np.linalg.det(R) > 0).all()


# ------------------------------------------------------------------------------------------------ 7. the ABI and the Python faces
def test_the_new_entry_is_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    assert "egotap_pose_track_world" in L.exported_symbols() and hasattr(lib, "egotap_pose_track_world") and "int egotap_pose_track_world(" in text
    assert "A STATE BELONGS TO THE FRAME IT WAS MADE IN" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert len(L._PROTOS["egotap_pose_track_world"][1]) == 18


def test_pose_track_world_refuses_by_name_before_any_launch():
    lib = L.load()
    V = C.c_void_p
    T, S, P, J = 3, 2, 16, 15
    B, K = T * S, P + 1 + J
    names = ("pose", "frame", "j3", "rig", "dts", "sin", "sout", "tracks", "pw", "pc")
    addr = {n: 0x100000 * (k + 1) for k, n in enumerate(names)}
    nbytes = dict(pose=B * P * 12, frame=B * 32, j3=B * J * 32, rig=B * 96, dts=T * 4, sin=S * K * 96, sout=S * K * 96, tracks=B * K * 32, pw=B * P * 12, pc=B * P * 12)
    ok = dict({n: V(a) for n, a in addr.items()}, T=T, S=S, P=P, J=J, dt=0.0, prm=L.track_params_struct(), tol=1e-6)

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_pose_track_world(a["pose"], a["frame"], a["j3"], a["rig"], a["T"], a["S"], a["P"], a["J"], a["dts"], a["dt"],
                                         C.byref(a["prm"]) if a["prm"] is not None else None, a["tol"], a["sin"], a["sout"], a["tracks"], a["pw"], a["pc"], None)
        return rc, lib.egotap_last_error().decode()

    def prm(**kw):
        o = L.track_params_struct()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    nan, inf = float("nan"), float("inf")
    at = lambda n, off=0: V(addr[n] + off)      # noqa: E731
    # everything egotap_pose_track refuses
    cases = [(dict(pose=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(tracks=None), "null"), (dict(pw=None), "null"),
             (dict(prm=None), "params"),
             (dict(pose=at("pose", 2)), "pose"), (dict(frame=at("frame", 1)), "frame"), (dict(j3=at("j3", 2)), "joints3d"), (dict(dts=at("dts", 3)), "dts"),
             (dict(pw=at("pw", 2)), "placed_world"), (dict(tracks=at("tracks", 8)), "tracks must be 16-byte"), (dict(tracks=at("tracks", 4)), "tracks must be 16-byte"),
             (dict(sin=at("sin", 4)), "state_in"), (dict(sout=at("sout", 4)), "state_out"),
             (dict(T=0), "T, S and P"), (dict(S=0), "T, S and P"), (dict(P=0), "T, S and P"), (dict(T=-1), "T, S and P"), (dict(P=65), "at most 64 pose rows"),
             (dict(J=-1), "J must be"), (dict(J=65), "J must be"), (dict(j3=None), "joints3d"), (dict(J=0), "joints3d"),
             (dict(dts=None, dt=0.0), "dt must be"), (dict(dts=None, dt=-1.0), "dt must be"), (dict(dts=None, dt=nan), "dt must be"), (dict(dts=None, dt=inf), "dt must be")]
    for c in spec.TRACK_CLASSES:
        cases += [(dict(prm=prm(**{f"{c}_min_cutoff": v})), f"{c}_min_cutoff") for v in (0.0, -1.0, nan, inf)]
        cases += [(dict(prm=prm(**{f"{c}_d_cutoff": v})), f"{c}_d_cutoff") for v in (0.0, nan, inf)]
        cases += [(dict(prm=prm(**{f"{c}_beta": v})), f"{c}_beta") for v in (-0.1, nan, inf)]
    for g in ("max_disagree", "max_gap", "max_joint_gap"):
        cases += [(dict(prm=prm(**{g: v})), g) for v in (nan, -1.0, -inf)]
    cases += [(dict(prm=prm(min_joints=-1)), "min_joints"), (dict(prm=prm(max_hold=-1)), "max_hold")]
    # and what is new here
    cases += [(dict(rig=None), "null"), (dict(pc=None), "null"), (dict(rig=at("rig", 4)), "rig_pose must be 8-byte"), (dict(pc=at("pc", 2)), "placed_cam must be 4-byte"),
              (dict(tol=nan), "ortho_tol"), (dict(tol=-1e-12), "ortho_tol"), (dict(tol=-inf), "ortho_tol")]
    # an output on an input, or on another output: first byte, last byte
    full = {"sout": "state_out", "tracks": "tracks", "pw": "placed_world", "pc": "placed_cam"}
    for out, name in full.items():
        for inp in ("pose", "frame", "j3", "rig", "dts", "sin"):
            if (out, inp) == ("sout", "sin"):
                continue
            cases += [({out: at(inp)}, f"{name} overlaps"), ({out: at(inp, (nbytes[inp] - 1) // 16 * 16)}, f"{name} overlaps"),
                      ({inp: at(out, (nbytes[out] - 1) // 16 * 16)}, f"{name} overlaps")]
    cases += [(dict(tracks=at("sout", 96)), "state_out overlaps tracks"), (dict(pw=at("sout")), "state_out overlaps placed_world"),
              (dict(pc=at("sout", 8)), "state_out overlaps placed_cam"), (dict(pw=at("tracks", nbytes["tracks"] - 16)), "tracks overlaps placed_world"),
              (dict(pc=at("tracks", 16)), "tracks overlaps placed_cam"), (dict(pc=at("pw", nbytes["pw"] - 4)), "placed_world overlaps placed_cam"),
              (dict(pc=at("pw")), "placed_world overlaps placed_cam"),
              (dict(sout=at("sin", 96)), "state_out overlaps state_in"), (dict(sout=at("sin", -8)), "state_out overlaps state_in")]
    # rig_pose on another input
    cases += [(dict(rig=at(inp)), f"rig_pose overlaps {nm}") for inp, nm in (("pose", "pose"), ("frame", "frame"), ("j3", "joints3d"), ("sin", "state_in"))]
    cases += [(dict(dts=at("rig", 8)), "rig_pose overlaps dts")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_pose_track_world:") and word in msg, (kw, rc, msg)
    # ortho_tol 0 and +inf, the state in place: not refused for those (the first refusal is a later one, made on purpose)
    for tol in (0.0, inf):
        rc, msg = call(tol=tol, sout=at("sin"), tracks=at("tracks", 8))
        assert rc == 1 and "tracks must be 16-byte" in msg


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch
    from egotap_amd import models
    P, J = 16, 15
    pose, state = torch.zeros(4, P, 3), torch.zeros(2, P + 1 + J, 12, dtype=torch.float64)
    j3, frame = torch.zeros(4, J, 8), torch.zeros(4, 8)
    rig = torch.from_numpy(np.tile(W.IDENTITY, (4, 1)))
    kw = dict(dt=0.1, joints3d=j3, frame=frame, streams=2)
    for bad in (rig.float(), rig[:3], rig[:, :9], rig.reshape(4, 3, 4), rig.numpy(), None):
        with pytest.raises(ValueError, match="pose_track_world: rig_pose is a float64 tensor"):
            L.pose_track_world(pose, state, bad, **kw)
    for tol in (-1.0, float("nan")):
        with pytest.raises(ValueError, match="ortho_tol"):
            L.pose_track_world(pose, state, rig, ortho_tol=tol, **kw)
    # the checks of lib.pose_track, under this entry's name
    with pytest.raises(ValueError, match="pose_track_world: pose is a tensor"):
        L.pose_track_world(torch.zeros(5, P, 3), state, rig, **kw)
    with pytest.raises(ValueError, match="pose_track_world: joints3d is a tensor"):
        L.pose_track_world(pose, state, rig, dt=0.1, joints3d=torch.zeros(4, J, 4), streams=2)
    with pytest.raises(ValueError, match="pose_track_world: frame is a tensor"):
        L.pose_track_world(pose, state, rig, dt=0.1, joints3d=j3, frame=torch.zeros(4, 4), streams=2)
    with pytest.raises(ValueError, match="pose_track_world: state is a contiguous float64"):
        L.pose_track_world(pose, state.float(), rig, **kw)
    with pytest.raises(ValueError, match="pose_track_world: give exactly one of dt"):
        L.pose_track_world(pose, state, rig, joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="pose_track_world: dts is a float32 tensor"):
        L.pose_track_world(pose, state, rig, dts=torch.zeros(3), joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="pose_track_world: dt must be finite"):
        L.pose_track_world(pose, state, rig, dt=0.0, joints3d=j3, streams=2)
    with pytest.raises(L.EgotapError, match="pose_track_world runs on the GPU only"):
        L.pose_track_world(pose, state, rig, **kw)
    with pytest.raises(L.EgotapError, match="pose, frame, joints3d, dts and state on one cuda device"):      # the camera-frame face's own words, as before
        L.pose_track(pose, state, **kw)
    # the tracker: a world tracker needs a rig pose, a camera tracker refuses one, each by name
    world, cam = models.PoseTracker(P, J, streams=2, world=True), models.PoseTracker(P, J, streams=2)
    assert world.world and not cam.world and world.ortho_tol == 1e-6
    assert models.PoseTracker(P, J, world=True, ortho_tol=0.0).ortho_tol == 0.0
    with pytest.raises(ValueError, match="ortho_tol goes with a world tracker"):
        models.PoseTracker(P, J, ortho_tol=1e-6)
    for tol in (-1e-9, float("nan")):
        with pytest.raises(ValueError, match="ortho_tol must be"):
            models.PoseTracker(P, J, world=True, ortho_tol=tol)
    with pytest.raises(ValueError, match="needs rig_pose"):
        world.update(pose, j3, frame, dt=0.1)
    with pytest.raises(ValueError, match="rig_pose goes with a world tracker"):
        cam.update(pose, j3, frame, dt=0.1, rig_pose=rig)
    with pytest.raises(ValueError, match="pose is a tensor"):
        world.update(torch.zeros(4, P + 1, 3), dt=0.1, rig_pose=rig)
    with pytest.raises(L.EgotapError, match="GPU only"):
        world.update(pose, j3, frame, dt=0.1, rig_pose=rig)
    with pytest.raises(L.EgotapError, match="GPU only"):
        cam.update(pose, j3, frame, dt=0.1)
    world.reset()
