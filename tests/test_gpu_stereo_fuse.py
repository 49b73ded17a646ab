"""The fusion of the lifted joints with the keypoint rays on the device: egotap_stereo_fuse (stereo_fuse.h), lib.stereo_fuse and the model's StereoFusion.

The expected values are the float64 restatement spec.stereo_fuse_ref on keypoints of every kind tests/ocam_inputs.py makes (valid, low score, NaN
score, NaN / inf coordinate, parallel, swapped eyes), priors 3 cm off the truth, frames without a root and pose rows that are not finite.  Device and
host run the same float64 operations in the same order; only the divisions and the square roots may differ in the last float64 bit, which the one
rounding to fp32 can turn into one fp32 ulp -- the gates are the project's for this class of arithmetic (test_gpu_stereo_triangulate.py):
  * equal in bits: mode, the all-zero records, every pose_fused row the definition passes through, the four counts of stats;
  * x, y, z and the fused pose_fused rows within 2 fp32 ulp of the frame's largest |x| component;
  * move, the residuals, the weight share and the rms / max statistics within 2 fp32 ulp of their own largest value in the frame.
Measured on the MI355X: every value of every case below came out EQUAL IN BITS (largest deviation / bound 0.0), so the gates have their whole width
to spare.
The serving test's expected value is lib.stereo_fuse on the same tensors: the same kernel on the same inputs, hence equal bits; the tracker and the
skeleton behind it are held to their own restatements by their own gates (test_gpu_pose_track.py, test_gpu_skeleton_fit.py)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import ocam_inputs as I
import test_gpu_pose_track as TP
import test_gpu_skeleton_fit as TS
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
CANARY = -12345.0
SHAPES = [(1, 15, 16), (5, 17, 17), (4, 64, 64), (9, 15, 16)]      # (B, J, P): one wave; two workgroups, the second ragged; every lane; three workgroups
RIGS = ["pinhole", "pinhole_rot", "fisheye_ue", "fisheye_cv"]
THAT = np.array([0.25, -0.5, 0.75], dtype=np.float32)
PRM = spec.FuseParams(sigma_prior=0.05)


def _bits(got, want):
    got, want = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32) for t in (got, want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got.view(np.int32) != want.view(np.int32))[:8]


def _between_canaries(n_floats, pad=64):
    flat = torch.full((n_floats + 2 * pad,), CANARY, device="cuda")

    def untouched():
        return bool((flat[:pad] == CANARY).all()) and bool((flat[pad + n_floats:] == CANARY).all())
    return flat[pad:pad + n_floats], untouched


@functools.lru_cache(maxsize=None)
def _case(shape, rig):
    """(rig arguments, inputs, the restatement's outputs): computed once per case, shared, never written"""
    B, J, P = shape
    row0 = P - J
    R = I.SMALL_R if rig in ("pinhole_rot", "fisheye_cv") else None
    if rig.startswith("pinhole"):
        kp64, X, kind = I.pinhole_case(B, J, seed=70 + B + J, R=R)
        left, right, affine = I.pinhole(), I.pinhole(), None
    else:
        kp64, affine, X, kind = I.fisheye_case(B, J, seed=80 + B + J, R=R, ue=rig == "fisheye_ue")
        left, right = I.rig_models(rig == "fisheye_ue")
    kp = np.ascontiguousarray(kp64.astype(np.float32))
    rng = np.random.default_rng(B * 100 + J)
    pose = np.full((B, P, 3), 1e6, dtype=np.float32)              # a row outside the joint rows is copied, never read into a record
    pose[:, row0:] = (X + rng.normal(0, 0.03, X.shape) - THAT).astype(np.float32)
    pose[0, row0 + J - 1, 1] = np.nan                             # a pose row that is not finite, in the last lane
    frame = np.zeros((B, 8), dtype=np.float32)
    frame[:, :3], frame[:, 3] = THAT, 4 + np.arange(B)
    frame[:, 4:] = rng.normal(0, 1, (B, 4))                       # the rest of the record is not read
    if B > 2:
        frame[2, 3] = 2.0                                         # frames without a root: too few joints, t_hat not finite
    if B > 7:
        frame[7, 0] = np.nan
        frame[4, 2] = -np.inf
    rig_args = dict(left=left, right=right, t=I.T, R=R, affine=affine)
    want = spec.stereo_fuse_ref(kp, pose, frame, left, right, I.T, PRM, R=R, affine=affine, pose_row0=row0)
    for a in (kp, pose, frame) + want:
        a.setflags(write=False)
    return rig_args, (kp, pose, frame, row0), want


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _launch(rig_args, prm, kp, pose, row0, frame, fused, pose_fused, stats):
    B, _, J, _ = kp.shape
    cl, cr, Rp, tp, ap, ms = L.stereo_triangulate_args(rig_args["left"], rig_args["right"], rig_args["t"], rig_args["R"], rig_args["affine"], 0.5)
    p = L.fuse_params_struct(prm)
    L.check(L.load().egotap_stereo_fuse(L.ptr(kp), B, J, C.byref(cl), C.byref(cr), Rp, tp, ap, ms, L.ptr(pose), pose.shape[1], row0, L.ptr(frame), C.byref(p),
                                        L.ptr(fused), L.ptr(pose_fused), L.ptr(stats), L.stream()))


def _compare(tag, got, want, pose, row0):
    """the gates of the module docstring; returns the largest deviation in units of its bound"""
    g_pf, g_fu, g_st = (t.detach().cpu().numpy() if torch.is_tensor(t) else t for t in got)
    w_pf, w_fu, w_st = want
    B, J, _ = w_fu.shape
    mode = w_fu[..., 7].astype(int)
    _bits(g_fu[..., 7], w_fu[..., 7])
    _bits(g_fu[mode == 0], w_fu[mode == 0])                       # zeros, in bits
    assert (w_fu[mode == 0] == 0).all()
    _bits(g_st[:, :4], w_st[:, :4])
    _bits(g_st[w_st[:, 0] == 0], w_st[w_st[:, 0] == 0])
    kept = ((mode & 6) != 0) & ((mode & 128) == 0)                # a fit was kept: the only rows that are written anew
    through = np.ones(pose.shape[:2], dtype=bool)
    through[:, row0:row0 + J] = ~kept
    _bits(g_pf[through], pose[through])                           # the pass-through rows are the INPUT's bits
    _bits(w_pf[through], pose[through])
    _bits(g_fu[..., :3][(mode != 0) & ~kept], w_fu[..., :3][(mode != 0) & ~kept])      # x = x0: one addition, no division
    ulp2 = lambda top: 2.0 * float(np.spacing(np.float32(top)))   # noqa: E731
    worst = 0.0
    for b in range(B):
        on = mode[b] != 0
        if not on.any():
            continue
        d = np.abs(g_fu[b].astype(np.float64) - w_fu[b].astype(np.float64))
        ds = np.abs(g_st[b].astype(np.float64) - w_st[b].astype(np.float64))
        dp = np.abs(g_pf[b, row0:row0 + J][kept[b]].astype(np.float64) - w_pf[b, row0:row0 + J][kept[b]].astype(np.float64))
        top_x = np.abs(w_fu[b, on, :3]).max()
        checks = [("x, y, z", d[on, :3], top_x), ("pose_fused", dp, top_x), ("move", d[on, 3], w_fu[b, on, 3].max()), ("res", d[on, 4:6], w_fu[b, on, 4:6].max()),
                  ("share", d[on, 6], w_fu[b, on, 6].max()), ("rms / max move", ds[4:6], w_fu[b, on, 3].max()), ("rms / max res", ds[6:8], w_fu[b, on, 4:6].max())]
        for name, dev, top in checks:
            if dev.size == 0:
                continue
            bound = ulp2(top)
            worst = max(worst, float(dev.max()) / bound)
            assert (dev <= bound).all(), (tag, b, name, float(dev.max()), bound)
    differ = int((g_fu.view(np.int32) != w_fu.view(np.int32)).sum() + (g_st.view(np.int32) != w_st.view(np.int32)).sum() + (g_pf.view(np.int32) != w_pf.view(np.int32)).sum())
    print(tag, "largest deviation / bound:", worst, "| values that differ in any bit:", differ, "| modes:", sorted(set(mode.ravel().tolist())))
    return worst


@pytest.mark.parametrize("rig", RIGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%d_J%d_P%d" % s)
def test_stereo_fuse_equals_the_float64_restatement(shape, rig):
    B, J, P = shape
    rig_args, (kp, pose, frame, row0), want = _case(shape, rig)
    mode = want[1][..., 7].astype(int)
    assert (mode & 6).any() and (B <= 2 or (mode[2] == 0).all()) and mode[0, J - 1] == 0      # fused joints, the frame without a root, the NaN row
    dkp, dpose, dframe = _dev(kp), _dev(pose), _dev(frame)
    fused, ok_f = _between_canaries(B * J * 8)
    pf, ok_p = _between_canaries(B * P * 3)
    stats, ok_s = _between_canaries(B * 8)
    _launch(rig_args, PRM, dkp, dpose, row0, dframe, fused, pf, stats)
    torch.cuda.synchronize()
    assert ok_f() and ok_p() and ok_s(), "a canary moved"
    got = (pf.view(B, P, 3), fused.view(B, J, 8), stats.view(B, 8))
    _compare(f"{rig} B={B} J={J} P={P}", got, want, pose, row0)
    _bits(dkp, kp), _bits(dpose, pose), _bits(dframe, frame)      # the inputs are read only
    face = L.stereo_fuse(dkp, dpose, dframe, params=PRM, pose_row0=row0, **rig_args)      # the Python face: the same launch
    for a, b in zip(face, got):
        _bits(a, b)
    # in place: pose_fused == pose gives the bits of out of place
    inplace = dpose.clone()
    fused2, stats2 = torch.empty_like(got[1]), torch.empty_like(got[2])
    _launch(rig_args, PRM, dkp, inplace, row0, dframe, fused2, inplace, stats2)
    torch.cuda.synchronize()
    for a, b in zip((inplace, fused2, stats2), got):
        _bits(a, b)


def test_no_gate_a_wide_prior_and_nothing_to_fuse():
    """max_sigma = +inf and sigma_prior = 10 take the other parameters through; a batch in which no frame has a root is all pass-through"""
    shape = (5, 17, 17)
    rig_args, (kp, pose, frame, row0), _ = _case(shape, "pinhole_rot")
    for prm in (spec.FuseParams(sigma_prior=0.05, max_sigma=math.inf), spec.FuseParams(sigma_prior=10.0, sigma_ray=0.005, min_joints=0)):
        want = spec.stereo_fuse_ref(kp, pose, frame, I.pinhole(), I.pinhole(), I.T, prm, R=rig_args["R"], pose_row0=row0)
        got = L.stereo_fuse(_dev(kp), _dev(pose), _dev(frame), params=prm, pose_row0=row0, **rig_args)
        torch.cuda.synchronize()
        _compare(f"max_sigma={prm.max_sigma} sigma_prior={prm.sigma_prior}", got, want, pose, row0)
    none = np.array(frame)
    none[:, 3] = 0.0
    pf, fu, st = L.stereo_fuse(_dev(kp), _dev(pose), _dev(none), params=PRM, pose_row0=row0, **rig_args)
    torch.cuda.synchronize()
    _bits(pf, pose)
    assert not fu.any() and not st.any()


# ------------------------------------------------------------------------------------------------------------ serving
def test_fusion_behind_the_serving_call_and_in_front_of_the_tracker():
    m, p = _model()
    left, right = I.rig_models(True)
    m.__dict__.pop("_stereo_rig", None)
    with pytest.raises(L.EgotapError, match="new_stereo_fusion: no stereo rig is set"):
        m.new_stereo_fusion(0.5)
    m.set_stereo_rig(left, right, I.T, R=I.SMALL_R, min_score=-1e30)             # the synthetic estimators' peaks are no probabilities: every joint is "seen"
    dev = torch.device("cuda", torch.cuda.current_device())
    B, S0, P, J = 2, 4 * p.hm_size, p.out_joints, p.n_joints_hm
    row0 = spec.stereo_pose_row0(p)
    g = torch.Generator().manual_seed(31)
    l8, r8 = (torch.randint(0, 256, (B, S0, S0, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2))
    flags = dict(return_keypoints=True, return_triangulation=True)
    # the synthetic weights know no unit: wide, ungated, and a frame in which nothing triangulates still places its prior (t_hat = 0)
    prm = spec.FuseParams(sigma_prior=0.5, max_sigma=math.inf, min_joints=0)
    affine = (spec.stereo_pixel_affine(left, p.hm_size), spec.stereo_pixel_affine(right, p.hm_size))
    with pytest.raises(ValueError, match="sigma_prior is the one given"):
        m.new_stereo_fusion(0.25, params=prm)
    with pytest.raises(ValueError, match='"identity"'):
        m.new_stereo_fusion(0.5, affine="sensor")
    try:
        for graphed in (False, True):
            m._rgb_state(dev).graphs.clear()
            before = tuple(t.clone() for t in m.predict_pose_from_camera(l8, r8, graphed=graphed, **flags))
            ws_bytes, n_graphs = m._rgb_state(dev).ws.numel(), len(m._rgb_state(dev).graphs)
            fusion = m.new_stereo_fusion(0.5, params=prm)
            pose, kp, j3, fr = m.predict_pose_from_camera(l8, r8, graphed=graphed, **flags)
            lib, h = L.load(), m._rgb_state(dev).handle.h
            L.check(lib.egotap_timing_enable(h, 1))
            try:
                fusion.update(pose, kp, fr)
                n, ms, fl = C.c_int(), C.c_double(), C.c_double()
                L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
                detail = lib.egotap_timing_detail(h).decode()
            finally:
                L.check(lib.egotap_timing_enable(h, 0))
            assert n.value == 1 and '"role": "stereo_fuse"' in detail and "stereo_fuse_kernel" in detail, detail      # one launch, recorded under its name
            pose_fused, fused, stats = fusion.update(pose, kp, fr)
            want = L.stereo_fuse(kp, pose, fr, left, right, I.T, prm, R=I.SMALL_R, affine=affine, min_score=-1e30, pose_row0=row0)
            torch.cuda.synchronize()
            assert tuple(pose_fused.shape) == (B, P, 3) and tuple(fused.shape) == (B, J, 8) and tuple(stats.shape) == (B, 8)
            for a, b in zip((pose_fused, fused, stats), want):
                _bits(a, b)
            for a, b in zip((pose, kp, j3, fr), before):                          # the serving call's own outputs: the fusion changes nothing
                assert torch.equal(a, b), graphed
            assert m._rgb_state(dev).ws.numel() == ws_bytes and len(m._rgb_state(dev).graphs) == n_graphs
            print("graphed" if graphed else "eager", "stats", stats.tolist(), "modes", sorted(set(fused[..., 7].int().flatten().tolist())))
            assert bool((stats[:, 0] > 0).all()) and not torch.equal(pose_fused, pose)
            # against the restatement, from the tensors the serving call returned
            ref = spec.stereo_fuse_ref(kp.cpu().numpy(), pose.cpu().numpy(), fr.cpu().numpy(), left, right, I.T, prm, R=I.SMALL_R, affine=affine, min_score=-1e30,
                                       pose_row0=row0)
            _compare(f"serving graphed={graphed}", (pose_fused, fused, stats), ref, pose.cpu().numpy(), row0)
            # the tracker and the skeleton take pose_fused in place of pose, each within its own gates
            tprm, sprm = spec.TrackParams(min_joints=1, max_hold=2), spec.SkeletonParams(window=3, min_samples=1)
            tracker, skeleton = m.new_pose_tracker(streams=1, params=tprm), m.new_skeleton(streams=1, params=sprm)
            placed, tracks = tracker.update(pose_fused, j3, fr, dt=1.0 / 30)
            rig = skeleton.set_rest_pose(pose[0])
            rigid, rotations, lengths = skeleton.update(placed, tracks)
            torch.cuda.synchronize()
            K = P + 1 + J
            ins = tuple(t.cpu().numpy() for t in (pose_fused, j3, fr))
            wt, wp, _ = spec.pose_track_ref(ins[0], np.zeros((1, K, TP.NK)), 1.0 / 30, tprm, frame=ins[2], joints3d=ins[1])
            TP._compare("tracker behind the fusion", (tracks, placed, torch.zeros(1, K, TP.NK, dtype=torch.float64)), (wt, wp, np.zeros((1, K, TP.NK))), ins, 1, 1.0 / 30)
            ws = spec.skeleton_fit_ref(placed.cpu().numpy(), np.zeros((1, P, 2)), rig, sprm, tracks=tracks.cpu().numpy())
            TS._compare("skeleton behind the fusion", (rigid, rotations, lengths, torch.from_numpy(ws[3])), ws, placed.cpu().numpy())
    finally:
        m._rgb_state(dev).graphs.clear()
    # affine="identity" and an explicit pair: the sensor entry's keypoints are already calibration pixels
    ident = m.new_stereo_fusion(0.5, params=prm, affine="identity").update(pose, kp, fr)
    explicit = m.new_stereo_fusion(0.5, params=prm, affine=spec.STEREO_IDENTITY_AFFINE).update(pose, kp, fr)
    want = L.stereo_fuse(kp, pose, fr, left, right, I.T, prm, R=I.SMALL_R, affine=None, min_score=-1e30, pose_row0=row0)
    for a, b, c in zip(ident, explicit, want):
        _bits(a, c)
        _bits(b, c)
