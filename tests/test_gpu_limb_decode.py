"""Limb elevation angles and 2D segments from the sin/cos limb heatmaps on the device: egotap_limb_decode (limb_decode_kernel) and ``return_limbs`` of
the three serving entries (egotap_predict_pose_rgb_kpl / _rgb_u8_kpl / _sensor_u8_kpl).

The operator's expected value is spec.limb_decode_ref, the same definition in float64 numpy.  Both sides sum in float64 in different orders, so the
sums differ by at most S^2 2^-53 relative to the sum of the terms' magnitudes and every output is one fp32 rounding of nearly the same float64 value:
the tolerances of tests/limb_decode_inputs.py::compare (2 ulp; 2^-22 pi on the angles where they are conditioned; length^2 / 12 within
1e-4 max(ax^2, ay^2) + 2^-21 relative; empty records bit for bit).  The serving entries' expected value is the operator on the heatmaps the same
configuration returns: the same kernel on the same bytes, hence equal bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import limb_decode_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu


def _same_bits(got, want):
    got, want = (np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32) for t in (got, want))
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got.view(np.int32) != want.view(np.int32))[:8]


# ------------------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("mirrored", [False, True], ids=["identity", "mirror"])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [15, 17])
@pytest.mark.parametrize("S", [16, 48, 64, 128])
def test_operator_against_the_float64_definition(S, J, bf16, mirrored):
    affine = I.MIRROR if mirrored else None
    host = torch.from_numpy(I.tensor(J, S, bf16).copy())
    big = host.cuda().bfloat16() if bf16 else host.cuda()
    sl = big[:, 1:1 + 6 * J]                                      # a dim-1 slice: image stride (6J + 2) S*S
    want = I.reference(J, S, bf16, affine)
    # the raw entry into a view with canary records in front of and behind it
    n, pad, canary = I.B * 2 * J, 4, -12345.0
    flat = torch.full(((n + 2 * pad) * 8,), canary, device="cuda")
    out = flat[8 * pad:8 * (pad + n)]
    aff = None if affine is None else (C.c_float * 8)(*[float(v) for row in affine for v in row])
    L.check(L.load().egotap_limb_decode(L.ptr(sl), L.BF16 if bf16 else L.F32, I.B, S, sl.stride(0), 2 * J, J, 2, aff, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    assert bool((flat[:8 * pad] == canary).all()) and bool((flat[8 * (pad + n):] == canary).all())
    I.check_gates(I.compare(out.view(I.B, 2, J, 8).cpu().numpy(), want, J, affine))
    # the Python face: the same launch, the same bits.  (The fp32 kernel on the upcast maps splits the pixels over the lanes differently, so it agrees
    # with the bf16 kernel to rounding only -- both are held against the float64 definition above.)
    _same_bits(L.limb_decode(sl, 2 * J, J, eyes=2, affine=affine), out.view(I.B, 2, J, 8))


def test_one_eye_and_a_first_channel_of_zero():
    """eyes = 1, c0 = 0 on a contiguous tensor of exactly the pairs' channels (image stride = 2 n S*S)"""
    J, S = 15, 48
    host = np.ascontiguousarray(I.tensor(J, S, False)[:, 1 + 2 * J:1 + 4 * J])
    got = L.limb_decode(torch.from_numpy(host).cuda(), 0, J, eyes=1).cpu().numpy()
    want = spec.limb_decode_ref(host, 0, J, 1)
    assert np.array_equal(want, I.reference(J, S, False, None)[:, :1], equal_nan=True)
    full = np.concatenate([got, I.reference(J, S, False, None)[:, 1:]], axis=1)     # compare() takes both eyes: the second is the reference's own
    I.compare(full, I.reference(J, S, False, None), J, None)


# ------------------------------------------------------------------------------------------------------------ 2. serving
X4 = [(4.0, 0.0, 4.0, 0.0)] * 2
B = 2
CROP, CROP_R = (8, 0, 112, 96), (0, 2, 110, 94)                     # of 96 x 120 sensor frames


def _bytes8(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).cuda() for _ in range(2)]


def _decode(hm, J, affine=X4):
    return L.limb_decode(hm, 2 * J, J, eyes=2, affine=affine)


def _entries(m, p):
    """(name, call(**flags), affine) of the three serving entries on seeded frames"""
    S = p.hm_size
    l8, r8 = _bytes8(11, (B, 4 * S, 4 * S, 3))
    left, right = L.rgb_u8_to_f32(l8, r8, m.camera_table(l8.device))
    lh, rh = _bytes8(32, (B, 96, 120, 3))
    aff = [spec.sensor_keypoint_affine(CROP, False, S), spec.sensor_keypoint_affine(CROP_R, True, S)]
    return [("rgb", lambda **kw: m.predict_pose_from_rgb(left, right, **kw), X4),
            ("camera", lambda **kw: m.predict_pose_from_camera(l8, r8, **kw), X4),
            ("sensor", lambda **kw: m.predict_pose_from_sensor(lh, rh, crop=CROP, crop_right=CROP_R, mirror_right=True, **kw), aff)]


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_serving_limbs_are_the_decode_of_the_returned_heatmaps_and_nothing_else_moves(graphed):
    m, p = _model()
    J = p.n_joints_hm
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        for name, call, affine in _entries(m, p):
            m._rgb_state(dev).graphs.clear()
            pose0 = call().clone()
            _, hm0, kp0 = (t.clone() for t in call(return_heatmaps=True, return_keypoints=True))
            ws_bytes = m._rgb_state(dev).ws.numel()
            pose, hm, kp, lb = call(return_heatmaps=True, return_keypoints=True, return_limbs=True, graphed=graphed)
            torch.cuda.synchronize()
            assert tuple(lb.shape) == (B, 2, J, 8), name
            assert torch.equal(pose, pose0) and torch.equal(hm, hm0), name
            _same_bits(kp, kp0)
            want = _decode(hm, J, affine)
            _same_bits(lb, want)
            assert bool(torch.isfinite(lb).all()) and bool((lb[..., 7] > 0).all()), name
            # the heatmaps stay in the workspace: the limbs alone, and limbs with keypoints
            pose2, lb2 = call(return_limbs=True, graphed=graphed)
            torch.cuda.synchronize()
            assert torch.equal(pose2, pose0), name
            _same_bits(lb2, want)
            if not graphed:
                assert m.rgb_form() == "scratch", name
            pose3, kp3, lb3 = call(return_keypoints=True, return_limbs=True, graphed=graphed)
            torch.cuda.synchronize()
            assert torch.equal(pose3, pose0), name
            _same_bits(kp3, kp0)
            _same_bits(lb3, want)
            assert m._rgb_state(dev).ws.numel() == ws_bytes, name               # the eager workspace is grow-only: the parents' size was enough
            if graphed:
                assert len(m._rgb_state(dev).graphs) == 3, name                 # one graph per flag combination (the cache holds eight)
    finally:
        m._rgb_state(dev).graphs.clear()


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
def test_bf16_frozen_hand_off_stays_on_and_reads_the_bf16_operand(graphed):
    m, p = _model()
    J = p.n_joints_hm
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        m.set_precision("bf16")
        assert m.freeze_weights(batch=B) == {}
        m._rgb_state(dev).graphs.clear()
        for name, call, affine in _entries(m, p):
            pose0 = call().clone()
            assert m.rgb_form() == "handoff", name
            ws_bytes = m._rgb_state(dev).ws.numel()
            _, hm = call(return_heatmaps=True)
            pose, lb = call(return_limbs=True, graphed=graphed)
            torch.cuda.synchronize()
            if not graphed:
                assert m.rgb_form() == "handoff", name
            assert torch.equal(pose, pose0), name
            _same_bits(lb, _decode(hm.bfloat16(), J, affine))                   # the hand-off buffer holds bf16(heatmaps): DESIGN 3.17
            assert m._rgb_state(dev).ws.numel() == ws_bytes, name
    finally:
        m._rgb_state(dev).graphs.clear()
        m.unfreeze_weights()
        m.set_precision("f32")


def test_workspace_queries_are_the_parents():
    """the _kpl entries have no size query of their own: they run in what the parents' queries return, to the byte"""
    m, p = _model()
    dev = torch.device("cuda", torch.cuda.current_device())
    name, call, _ = _entries(m, p)[0]
    call()
    st = m._rgb_state(dev)
    need = C.c_size_t()
    L.check(L.load().egotap_predict_pose_rgb_workspace_bytes(st.handle.h, B, B, C.byref(need)))
    ws = torch.empty(need.value, dtype=torch.uint8, device=dev)
    l8, r8 = _bytes8(11, (B, 256, 256, 3))
    left, right = L.rgb_u8_to_f32(l8, r8, m.camera_table(dev))
    pose, kp, lb = (torch.empty(s, device=dev) for s in ((B, p.out_joints, 3), (B, 2, p.n_joints_hm, 4), (B, 2, p.n_joints_hm, 8)))
    lib = L.load()
    L.check(lib.egotap_predict_pose_rgb_kpl(st.handle.h, L.ptr(left), L.ptr(right), B, L.ptr(pose), None, B, L.ptr(ws), need.value, L.stream(), L.ptr(kp), L.ptr(lb)))
    torch.cuda.synchronize()
    want_pose, want_kp, want_lb = call(return_keypoints=True, return_limbs=True)
    assert torch.equal(pose, want_pose)
    _same_bits(kp, want_kp)
    _same_bits(lb, want_lb)
    rc = lib.egotap_predict_pose_rgb_kpl(st.handle.h, L.ptr(left), L.ptr(right), B, L.ptr(pose), None, B, L.ptr(ws), need.value - 1, L.stream(), L.ptr(kp), L.ptr(lb))
    assert rc != 0 and "workspace too small" in lib.egotap_last_error().decode()      # one byte less is refused, as for the parent
