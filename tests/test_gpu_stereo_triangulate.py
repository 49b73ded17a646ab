"""The fisheye camera model and the stereo triangulation on the device: egotap_ocam_project / egotap_ocam_unproject / egotap_stereo_triangulate
(ocam.h) and ``return_triangulation`` of the three serving entries.

The operators' expected values are the float64 restatements of spec.py.  Device and host run the same float64 operations in the same order; only
atan and the divisions may differ in the last float64 bit, which the one rounding to fp32 can turn into one fp32 ulp:
  * project / unproject: every finite value within 1 fp32 ulp, the (xc, yc) branch and the non-finite pattern equal in bits;
  * triangulate: valid, n and the zeros of invalid records equal in bits; X, Y, Z, s, t_hat within 2 fp32 ulp of the largest |X| component of the
    frame; gap, disagree and the frame's rms / max -- differences of such values -- within the same absolute bound; den within 2 fp32 ulp of 1.
    Every joint meant to be valid has host den >= 1e-4: asserted, so none is excused.
The serving entries' expected value is lib.stereo_triangulate on the keypoints and pose the same configuration returns: the same kernel on the same
inputs, hence equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import ocam_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
CANARY = -12345.0


def _same_bits(got, want):
    got, want = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32) for t in (got, want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got.view(np.int32) != want.view(np.int32))[:8]


def _between_canaries(n_floats, pad=64):
    """(the whole buffer, the view an operator writes, a check that nothing else moved)"""
    flat = torch.full((n_floats + 2 * pad,), CANARY, device="cuda")

    def untouched():
        return bool((flat[:pad] == CANARY).all()) and bool((flat[pad + n_floats:] == CANARY).all())
    return flat, flat[pad:pad + n_floats], untouched


# ------------------------------------------------------------------------------------------------------------ 1. project / unproject
def _within_one_ulp(got, want64):
    want = want64.astype(np.float32)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    ulps = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64)) / np.spacing(np.abs(want[fin])).astype(np.float64)
    print("max ulp distance", ulps.max() if ulps.size else 0.0, "values off by one ulp:", int((ulps > 0).sum()), "of", ulps.size)
    assert (ulps <= 1.0).all(), ulps.max()


def _points(kind, k, N):
    """N float32 inputs of the fixture's (cycled), with the edge rows where there is room: on-axis / centre first, then NaN and inf rows"""
    src = I.golden()[f"c{k}_{kind}_in"]
    pts = np.ascontiguousarray(np.resize(src, (N, src.shape[1])).astype(np.float32))
    if N == 1:
        pts[0] = src[3]
    if N >= 63:
        pts[5, 0] = np.nan
        pts[6, -1] = np.inf
        pts[7, 0] = -np.inf
        pts[N - 1] = src[0]                                       # the on-axis point / the centre pixel in the last lane too
    return pts


@pytest.mark.parametrize("k", [0, 1], ids=["ue_flip", "no_flip"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_project_and_unproject_equal_the_float64_restatements_to_one_ulp(N, k):
    m = I.calibration(k)
    cam = L.ocam_struct(m)
    lib = L.load()
    for kind, fn, face, ref, n_out in (("w2c", lib.egotap_ocam_project, L.ocam_project, spec.ocam_world2cam_ref, 2),
                                       ("c2w", lib.egotap_ocam_unproject, L.ocam_unproject, spec.ocam_cam2world_ref, 3)):
        pts = _points(kind, k, N)
        want = ref(pts.astype(np.float64), m)
        dev_in = torch.from_numpy(pts).cuda()
        flat, out, untouched = _between_canaries(N * n_out)
        L.check(fn(L.ptr(dev_in), N, C.byref(cam), L.ptr(out), L.stream()))
        torch.cuda.synchronize()
        assert untouched(), kind
        got = out.view(N, n_out).cpu().numpy()
        _within_one_ulp(got, want)
        if kind == "w2c" and N > 1:                               # the (xc, yc) branch: equal bits
            centre = np.array([m.xc, m.yc]).astype(np.float32)
            assert np.array_equal(got[0].view(np.int32), centre.view(np.int32)) and np.array_equal(got[N - 1].view(np.int32), centre.view(np.int32))
            assert np.array_equal(got[1].view(np.int32), centre.view(np.int32))        # norm 5e-9 <= 1e-8
        _same_bits(face(dev_in.view(1, N, -1), m)[0], got)        # the Python face: the same launch


# ------------------------------------------------------------------------------------------------------------ 2. triangulate
def _compare(got3, gotf, want3, wantf, tag):
    """the gates of the module docstring; returns the largest deviation in units of the frame's bound"""
    got3, gotf = (t.cpu().numpy() if torch.is_tensor(t) else t for t in (got3, gotf))
    valid = want3[..., 7] == 1
    _same_bits(got3[..., 7], want3[..., 7])
    _same_bits(gotf[:, 3], wantf[:, 3])
    _same_bits(got3[~valid], want3[~valid])                       # zeros, in bits
    _same_bits(gotf[wantf[:, 3] == 0], wantf[wantf[:, 3] == 0])
    worst = 0.0
    for b in range(want3.shape[0]):
        if not valid[b].any():
            continue
        top = np.abs(want3[b, valid[b], :3]).max()
        bound = 2.0 * float(np.spacing(np.float32(top)))
        d3 = np.abs(got3[b, valid[b]].astype(np.float64) - want3[b, valid[b]].astype(np.float64))
        df = np.abs(gotf[b].astype(np.float64) - wantf[b].astype(np.float64))
        worst = max(worst, d3[:, [0, 1, 2, 3, 5, 6]].max() / bound, df[[0, 1, 2, 4, 5, 6, 7]].max() / bound, d3[:, 4].max() / 2.0 ** -22)
        assert (d3[:, [0, 1, 2, 5]] <= bound).all(), (tag, b, "X, Y, Z, s", d3.max(), bound)
        assert (d3[:, [3, 6]] <= bound).all(), (tag, b, "gap, disagree", d3.max(), bound)
        assert (d3[:, 4] <= 2.0 ** -22).all(), (tag, b, "den", d3[:, 4].max())
        assert (df[[0, 1, 2]] <= bound).all() and (df[[4, 5, 6, 7]] <= bound).all(), (tag, b, "frame", df, bound)
    print(tag, "largest deviation / bound:", worst)


@pytest.mark.parametrize("J", [15, 17])
@pytest.mark.parametrize("B", [1, 5])
def test_triangulate_equals_the_float64_restatement(B, J):
    lib = L.load()
    pin = I.pinhole()
    for model in ("pinhole", "fisheye_ue", "fisheye_cv"):
        for R in (None, I.SMALL_R):
            if model == "pinhole":
                kp64, X, kind = I.pinhole_case(B, J, seed=40 + B + J, R=R)
                left, right, affine = pin, pin, None
            else:
                kp64, affine, X, kind = I.fisheye_case(B, J, seed=50 + B + J, R=R, ue=model == "fisheye_ue")
                left, right = I.rig_models(model == "fisheye_ue")
            kp = np.ascontiguousarray(kp64.astype(np.float32))    # what both sides see
            rng = np.random.default_rng(B * 100 + J)
            pose_np = np.zeros((B, J + 2, 3), dtype=np.float32)
            pose_np[:, 1:J + 1] = (X - np.array([0.2, -0.4, 0.9]) + rng.normal(0, 0.02, X.shape)).astype(np.float32)
            pose_np[:, 0], pose_np[:, J + 1] = 1e6, -1e6          # rows outside pose_row0 .. pose_row0 + J - 1 are never read
            for pose in (None, pose_np):
                tag = f"{model} B={B} J={J} R={'I' if R is None else 'rot'} pose={'no' if pose is None else 'yes'}"
                want3, wantf = spec.stereo_triangulate_ref(kp, left, right, I.T, R=R, affine=affine, pose=pose, pose_row0=1)
                meant = kind == "valid"
                assert (want3[meant][:, 7] == 1).all() and (want3[meant][:, 4] >= 1e-4).all(), (tag, want3[meant][:, 4].min())
                assert (wantf[:, 3] >= 4).all() and (model != "pinhole" or R is not None or np.array_equal(want3[..., 7] == 1, meant)), tag
                if model != "pinhole":                            # the fp32 keypoints still meet near the truth (2e-3 of its size: pixels rounded to fp32)
                    assert np.abs(want3[meant][:, :3] - X[meant]).max() <= 2e-3 * np.abs(X).max(), tag
                dkp = torch.from_numpy(kp).cuda()
                dpose = None if pose is None else torch.from_numpy(pose).cuda()
                f3, out3, ok3 = _between_canaries(B * J * 8)
                ff, outf, okf = _between_canaries(B * 8)
                cl, cr, Rp, tp, ap, ms = L.stereo_triangulate_args(left, right, I.T, R, affine, 0.5)
                L.check(lib.egotap_stereo_triangulate(L.ptr(dkp), B, J, C.byref(cl), C.byref(cr), Rp, tp, ap, ms, L.ptr(dpose), J + 2 if pose is not None else 0, 1,
                                                      L.ptr(out3), L.ptr(outf), L.stream()))
                torch.cuda.synchronize()
                assert ok3() and okf(), tag
                _compare(out3.view(B, J, 8), outf.view(B, 8), want3, wantf, tag)
                g3, gf = L.stereo_triangulate(dkp, left, right, I.T, R=R, affine=affine, pose=dpose, pose_row0=1)      # the Python face: the same launch
                _same_bits(g3, out3.view(B, J, 8))
                _same_bits(gf, outf.view(B, 8))


def test_triangulate_nothing_valid_and_the_largest_frame():
    """a frame without a valid joint is all zeros; J = 64 fills the wave; min_score is compared as given"""
    pin = I.pinhole()
    kp64, X, _ = I.pinhole_case(6, 64, seed=77)
    kp64[2, :, :, 2] = 0.25                                       # frame 2: nothing seen
    kp = torch.from_numpy(kp64.astype(np.float32)).cuda()
    for ms in (0.5, 0.2):
        want3, wantf = spec.stereo_triangulate_ref(kp.cpu().numpy(), pin, pin, I.T, min_score=ms)
        got3, gotf = L.stereo_triangulate(kp, pin, pin, I.T, min_score=ms)
        torch.cuda.synchronize()
        _compare(got3, gotf, want3, wantf, f"J=64 min_score={ms}")
        assert (wantf[2] == 0).all() == (ms == 0.5) and (ms != 0.5 or (want3[2] == 0).all())


# ------------------------------------------------------------------------------------------------------------ 3. serving
B = 2
CROP, CROP_R = (8, 0, 112, 96), (0, 2, 110, 94)                     # of 96 x 120 sensor frames
MIN_SCORE = -1e30                                                   # the synthetic estimators' peaks are no probabilities: every joint is "seen"


def _rig(m):
    left, right = I.rig_models(True)
    m.set_stereo_rig(left, right, I.T, R=I.SMALL_R, min_score=MIN_SCORE)
    return dict(left=left, right=right, t=I.T, R=I.SMALL_R, min_score=MIN_SCORE)


def _bytes8(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda() for _ in range(2)]


def _entries(m, p, seed=11):
    """(name, call(**flags), the entry's keypoint -> calibration pixel affine) of the three serving entries on seeded frames"""
    S = p.hm_size
    l8, r8 = _bytes8(seed, (B, 4 * S, 4 * S, 3))
    left, right = L.rgb_u8_to_f32(l8, r8, m.camera_table(l8.device))
    lh, rh = _bytes8(seed + 21, (B, 96, 120, 3))
    x4 = [spec.stereo_pixel_affine(I.calibration(0), S), spec.stereo_pixel_affine(I.calibration(1), S)]
    return [("rgb", lambda **kw: m.predict_pose_from_rgb(left, right, **kw), x4),
            ("camera", lambda **kw: m.predict_pose_from_camera(l8, r8, **kw), x4),
            ("sensor", lambda **kw: m.predict_pose_from_sensor(lh, rh, crop=CROP, crop_right=CROP_R, mirror_right=True, **kw), spec.STEREO_IDENTITY_AFFINE)]


def _triangulated(rig, kp, pose, affine, p):
    return L.stereo_triangulate(kp, rig["left"], rig["right"], rig["t"], R=rig["R"], affine=affine, min_score=rig["min_score"], pose=pose,
                                pose_row0=spec.stereo_pose_row0(p))


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_serving_triangulation_is_the_operator_on_the_returned_keypoints_and_pose(graphed):
    m, p = _model()
    rig = _rig(m)
    J = p.n_joints_hm
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        for name, call, affine in _entries(m, p):
            m._rgb_state(dev).graphs.clear()
            pose0 = call().clone()
            _, hm0, kp0, lb0 = (t.clone() for t in call(return_heatmaps=True, return_keypoints=True, return_limbs=True))
            ws_bytes = m._rgb_state(dev).ws.numel()
            want3, wantf = _triangulated(rig, kp0, pose0, affine, p)
            out = call(return_heatmaps=True, return_keypoints=True, return_limbs=True, return_triangulation=True, graphed=graphed)
            torch.cuda.synchronize()
            assert len(out) == 6, name
            pose, hm, kp, lb, j3, fr = out
            assert tuple(j3.shape) == (B, J, 8) and tuple(fr.shape) == (B, 8), name
            assert torch.equal(pose, pose0) and torch.equal(hm, hm0), name
            _same_bits(kp, kp0)
            _same_bits(lb, lb0)
            _same_bits(j3, want3)
            _same_bits(fr, wantf)
            print(name, "valid joints per frame", fr[:, 3].tolist())
            # the keypoints are computed inside and not returned
            out = call(return_triangulation=True, graphed=graphed)
            torch.cuda.synchronize()
            assert len(out) == 3 and torch.equal(out[0], pose0), name
            _same_bits(out[1], want3)
            _same_bits(out[2], wantf)
            if not graphed:
                assert m.rgb_form() == "scratch", name
            assert m._rgb_state(dev).ws.numel() == ws_bytes, name               # the eager workspace is grow-only: the parents' size was enough
            if graphed:
                assert len(m._rgb_state(dev).graphs) == 2, name
    finally:
        m._rgb_state(dev).graphs.clear()


def test_a_second_graphed_call_replays_the_same_graph_and_the_key_holds_the_rig():
    m, p = _model()
    rig = _rig(m)
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        m._rgb_state(dev).graphs.clear()
        for k in range(2):                                          # the second call replays with other frames
            name, call, affine = _entries(m, p, seed=60 + k)[1]
            pose0, kp0 = (t.clone() for t in call(return_keypoints=True))
            want3, wantf = _triangulated(rig, kp0, pose0, affine, p)
            pose, j3, fr = call(return_triangulation=True, graphed=True)
            torch.cuda.synchronize()
            assert torch.equal(pose, pose0), k
            _same_bits(j3, want3)
            _same_bits(fr, wantf)
            assert len(m._rgb_state(dev).graphs) == 1, k
        call(graphed=True)                                          # without the flag: the key is the parent's, a graph of its own
        assert len(m._rgb_state(dev).graphs) == 2
        m.set_stereo_rig(rig["left"], rig["right"], I.T * 2.0, R=I.SMALL_R, min_score=MIN_SCORE)              # another rig: another graph
        pose, j3, fr = call(return_triangulation=True, graphed=True)
        torch.cuda.synchronize()
        assert len(m._rgb_state(dev).graphs) == 3
        want3, wantf = _triangulated(dict(rig, t=I.T * 2.0), kp0, pose0, affine, p)
        _same_bits(j3, want3)
        _same_bits(fr, wantf)
    finally:
        m._rgb_state(dev).graphs.clear()


def test_bf16_frozen_hand_off_stays_on():
    m, p = _model()
    rig = _rig(m)
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        m.set_precision("bf16")
        assert m.freeze_weights(batch=B) == {}
        for name, call, affine in _entries(m, p):
            pose0 = call().clone()
            assert m.rgb_form() == "handoff", name
            ws_bytes = m._rgb_state(dev).ws.numel()
            _, kp0 = (t.clone() for t in call(return_keypoints=True))
            pose, j3, fr = call(return_triangulation=True)
            torch.cuda.synchronize()
            assert m.rgb_form() == "handoff" and torch.equal(pose, pose0), name
            want3, wantf = _triangulated(rig, kp0, pose0, affine, p)
            _same_bits(j3, want3)
            _same_bits(fr, wantf)
            assert m._rgb_state(dev).ws.numel() == ws_bytes, name
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")


def test_without_a_rig_the_flag_raises_by_name_and_the_module_route_returns_the_same_records():
    m, p = _model()
    m.__dict__.pop("_stereo_rig", None)
    for name, call, _ in _entries(m, p):
        with pytest.raises(L.EgotapError, match="set_stereo_rig"):
            call(return_triangulation=True)
        assert torch.is_tensor(call())                              # without the flag nothing asks for a rig
    rig = _rig(m)
    try:
        m.net_HeatMap.set_precision("bf16")
        m.net_RotHeatMap.set_precision("bf16")                      # the head stays fp32: the networks cannot share one handle
        assert "different precisions" in m._rgb_one_call_refusal()
        for name, call, affine in _entries(m, p):
            pose0, kp0 = (t.clone() for t in call(return_keypoints=True))
            want3, wantf = _triangulated(rig, kp0, pose0, affine, p)
            pose, j3, fr = call(return_triangulation=True)
            torch.cuda.synchronize()
            assert torch.equal(pose, pose0), name
            _same_bits(j3, want3)
            _same_bits(fr, wantf)
            with pytest.raises(L.EgotapError, match="ungraphed"):
                call(return_triangulation=True, graphed=True)
    finally:
        m.set_precision("f32")


def test_the_timing_hook_records_the_three_operators():
    m, p = _model()
    dev = torch.device("cuda", torch.cuda.current_device())
    h = m._rgb_state(dev).handle.h
    lib = L.load()
    cam = I.calibration(0)
    pts = torch.from_numpy(I.golden()["c0_w2c_in"].astype(np.float32)).cuda()
    kp = torch.from_numpy(I.pinhole_case(2, 15, seed=3)[0].astype(np.float32)).cuda()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        pix = L.ocam_project(pts, cam)
        L.ocam_unproject(pix, cam)
        L.stereo_triangulate(kp, I.pinhole(), I.pinhole(), I.T)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 3 and all(f'"role": "{r}"' in detail for r in ("ocam_project", "ocam_unproject", "stereo_triangulate")), detail
    L.ocam_project(pts, cam)                                        # the hook is off: nothing is recorded
    L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
    assert n.value == 0
