"""2D joints and confidences from the heatmaps on the device: egotap_heatmap_peaks (heatmap_peaks_kernel) and ``return_keypoints`` of the three
serving entries (egotap_predict_pose_rgb_kp / _rgb_u8_kp / _sensor_u8_kp).

The operator's expected value is spec.heatmap_peaks_ref, the same definition in numpy: equal bits (a NaN score is compared with isnan).  The serving
entries' expected value is the operator on the heatmaps the same configuration returns: equal bits again; only the sensor route's comparison with the
float64 affine image of the camera route's keypoints has a tolerance, 1e-3 sensor pixels (fp32 rounding of one fmaf at coordinates below 4096)."""
import ctypes as C

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model

pytestmark = pytest.mark.gpu


def _same_records(got, want):
    """equal bits, except that a NaN score equals any NaN score"""
    got, want = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float32) for t in (got, want))
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = (got.view(np.int32) != want.view(np.int32)) & ~nan
    assert not bad.any(), (np.argwhere(bad)[:8], got[bad][:8], want[bad][:8])


# ------------------------------------------------------------------------------------------------------------ 1. the operator
KINDS = ["random", "two_equal", "plateau", "first", "last", "wave0", "wave1", "wave2", "wave3", "zero", "negative", "nan_beside", "inf", "only_nan", "random"]


def _maps(S, B, n, bf16, seed):
    """[B, n, S, S] float32 on the host (bf16-representable when asked): map k of the flat list is of kind KINDS[k]"""
    g = torch.Generator().manual_seed(seed + S)
    h = torch.randn((B * n, S, S), generator=g)
    if bf16:
        h = h.bfloat16().float()
    HW, flat = S * S, h.view(B * n, -1)
    top = float(flat.abs().max()) + 1.0          # above every random value (every place set to it is rounded to the same bf16 value below)
    # maps of 4096 elements and more are read by four waves, 64 consecutive 16-byte vectors of every 256 each: a maximum in each wave's part of the
    # second pass; smaller maps are read by one wave: a maximum in each quarter
    span = 256 * (8 if bf16 else 4)
    wave_at = [span + (span // 4) * w + 37 if HW >= 4096 else (HW // 4) * w + 37 for w in range(4)]
    for k in range(B * n):
        kind, m = KINDS[k % len(KINDS)], flat[k]
        if kind == "two_equal":
            m[HW // 5] = m[HW - 7] = top                          # far apart: the first in scan order wins
        elif kind == "plateau":
            m[3 * S - 2:3 * S + 3] = top                          # equal maxima across a row boundary
        elif kind == "first":
            m[0] = top
        elif kind == "last":
            m[HW - 1] = top                                       # the last lane of the last vector
        elif kind.startswith("wave"):
            m[wave_at[int(kind[4])]] = top
        elif kind == "zero":
            m.zero_()
        elif kind == "negative":
            m.copy_(-m.abs() - 1.0)
        elif kind == "nan_beside":
            at = 5 * S + 9
            m[at] = top
            m[at + 1] = m[at - S] = m[0] = float("nan")           # NaN neighbours: no step; a NaN first element never wins
        elif kind == "inf":
            m[7 * S + 3] = float("inf")
            m[7 * S + 4] = float("inf")                           # inf - x on one axis, and a tie of infinities
        elif kind == "only_nan":
            m.fill_(float("nan"))
    if bf16:
        h = h.bfloat16().float()
    return h.view(B, n, S, S)


def _run_operator(S, bf16, c0, n, groups, affine):
    B, C_slice, C_big = 3, 8, 10
    assert c0 + n <= C_slice
    host = _maps(S, B, C_big, bf16, seed=17)
    big = host.cuda().bfloat16() if bf16 else host.cuda()
    sl = big[:, 1:1 + C_slice]                                    # a dim-1 slice: image stride C_big * S*S > n * S*S
    want = spec.heatmap_peaks_ref(host[:, 1 + c0:1 + c0 + n].numpy(), groups=groups, affine=affine)
    # the raw entry into a view with canary records in front of and behind it
    pad, canary = 8, -12345.0
    flat = torch.full(((B * n + 2 * pad) * 4,), canary, device="cuda")
    out = flat[4 * pad:4 * (pad + B * n)]
    aff = None if affine is None else (C.c_float * (4 * groups))(*[float(v) for row in affine for v in row])
    L.check(L.load().egotap_heatmap_peaks(L.ptr(sl), L.BF16 if bf16 else L.F32, B, S, sl.stride(0), c0, n, groups, aff, L.ptr(out), L.stream()))
    torch.cuda.synchronize()
    _same_records(out.view(B, n, 4), want)
    assert bool((flat[:4 * pad] == canary).all()) and bool((flat[4 * (pad + B * n):] == canary).all())
    # the Python face: the same records
    got = L.heatmap_peaks(sl, c0, n, groups=groups, affine=affine)
    _same_records(got, want)
    if bf16:                                                      # the bf16 kernel computes what the fp32 kernel computes on the upcast maps
        _same_records(got, L.heatmap_peaks(sl.float(), c0, n, groups=groups, affine=affine))
    return got


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("S", [16, 48, 64, 128])
def test_operator_equals_the_numpy_definition_bit_for_bit(S, bf16):
    got = _run_operator(S, bf16, c0=2, n=5, groups=1, affine=None)
    # the kinds did what they are for (map k of the slice's n maps of image b is flat map (b * 10 + 1 + 2 + k) of the host tensor)
    idx = {KINDS[(b * 10 + 3 + k) % len(KINDS)]: int(got[b, k, 3]) for b in range(3) for k in range(5)}
    assert idx.get("first", 0) == 0 and idx.get("last", S * S - 1) == S * S - 1 and idx.get("only_nan", 0) == 0


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_operator_with_an_affine_per_group(bf16):
    _run_operator(64, bf16, c0=2, n=6, groups=2, affine=[(4.6875, 70.0, 3.125, 30.0), (-4.6875, 370.0, 3.3, 2.0)])
    _run_operator(32, bf16, c0=0, n=6, groups=3, affine=[(4.0, 0.0, 4.0, 0.0), (-1.7, 3.3, 0.1, -9.0), (1e-3, 4095.7, 123.4, 0.5)])


def test_ground_truth_maps_read_out_their_joints():
    """on the synthesised ground-truth maps of the training loader: a joint in view peaks in its own pixel with a unit score, one out of view scores 0"""
    g = torch.Generator().manual_seed(3)
    pts = torch.rand((2, 16, 2), generator=g) * 1024.0
    pts[0, 5] = torch.tensor([1500.0, 300.0])                       # out of view
    maps = L.synth_heatmaps(pts.cuda(), pts.cuda(), torch.randn((2, 16, 3), generator=g).cuda())["cat"]
    rec = L.heatmap_peaks(maps, 0, 15).cpu()
    _same_records(rec, spec.heatmap_peaks_ref(maps[:, :15].cpu().numpy()))
    for b in range(2):
        for j in range(15):
            x, y = (pts[b, j + 1] / 1024.0 * 64).tolist()
            if b == 0 and j == 4:
                assert rec[b, j, 2] == 0 and rec[b, j, 3] == 0
            else:
                assert int(rec[b, j, 3]) == int(y) * 64 + int(x) and rec[b, j, 2] > 0.9, (b, j, rec[b, j], x, y)


# ------------------------------------------------------------------------------------------------------------ 2. serving
def _model(preset="UnrealEgo", hm=64):
    m, p = serving_model(preset, hm)
    m.opt.hm_chunk = 2                                              # B = 3: pieces of 2 and 1 frames
    return m, p


X4 = [(4.0, 0.0, 4.0, 0.0)] * 2
B = 3


def _bytes8(seed, shape):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, shape, generator=g, dtype=torch.uint8) for _ in range(2)]


def _frames(m, seed=11, S0=256):
    """(bytes left, right on the device; the table-normalised float frames of the same bytes)"""
    l8, r8 = (t.cuda() for t in _bytes8(seed, (B, S0, S0, 3)))
    left, right = L.rgb_u8_to_f32(l8, r8, m.camera_table(l8.device))
    return l8, r8, left, right


def _peaks_of(hm, J, affine=X4):
    return L.heatmap_peaks(hm, 0, 2 * J, groups=2, affine=affine).view(hm.shape[0], 2, J, 4)


def test_rgb_f32_keypoints_are_the_peaks_of_the_returned_heatmaps_and_the_pose_keeps_its_bits():
    m, p = _model()
    _, _, left, right = _frames(m)
    want_pose = m.predict_pose_from_rgb(left, right).clone()
    pose, hm, kp = m.predict_pose_from_rgb(left, right, return_heatmaps=True, return_keypoints=True)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (B, 2, p.n_joints_hm, 4) and torch.equal(pose, want_pose)
    want_kp = _peaks_of(hm, p.n_joints_hm)
    _same_records(kp, want_kp)
    _same_records(kp, spec.heatmap_peaks_ref(hm[:, :2 * p.n_joints_hm].cpu().numpy(), groups=2, affine=X4).reshape(kp.shape))
    pose2, kp2 = m.predict_pose_from_rgb(left, right, return_keypoints=True)          # the heatmaps stay in the workspace
    torch.cuda.synchronize()
    assert m.rgb_form() == "scratch" and torch.equal(pose2, want_pose)
    _same_records(kp2, want_kp)


def test_bf16_frozen_hand_off_stays_on_and_reads_the_bf16_operand():
    m, p = _model()
    try:
        m.set_precision("bf16")
        assert m.freeze_weights(batch=2) == {}
        _, _, left, right = _frames(m)
        want_pose = m.predict_pose_from_rgb(left, right).clone()
        assert m.rgb_form() == "handoff"
        _, hm = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        pose, kp = m.predict_pose_from_rgb(left, right, return_keypoints=True)
        torch.cuda.synchronize()
        assert m.rgb_form() == "handoff" and torch.equal(pose, want_pose)
        _same_records(kp, _peaks_of(hm.bfloat16(), p.n_joints_hm))                   # the hand-off buffer holds bf16(heatmaps): DESIGN 3.17
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")


def test_graphed_replays_the_eager_keypoints():
    m, p = _model()
    try:
        m._rgb_state(torch.device("cuda", torch.cuda.current_device())).graphs.clear()
        for k in range(2):                                          # the second call replays with other frames
            _, _, left, right = _frames(m, seed=20 + k)
            want_pose, want_kp = (t.clone() for t in m.predict_pose_from_rgb(left, right, return_keypoints=True))
            pose, kp = m.predict_pose_from_rgb(left, right, return_keypoints=True, graphed=True)
            torch.cuda.synchronize()
            assert torch.equal(pose, want_pose), k
            _same_records(kp, want_kp)
        assert len(m._rgb["graphs"]) == 1
        m.predict_pose_from_rgb(left, right, graphed=True)          # without keypoints: a graph of its own
        assert len(m._rgb["graphs"]) == 2
    finally:
        m._rgb["graphs"].clear()


CROP, CROP_R = (8, 0, 112, 96), (0, 2, 110, 94)                     # of 96 x 120 sensor frames


def test_camera_and_sensor_entries():
    m, p = _model()
    J, S = p.n_joints_hm, p.hm_size
    l8, r8, left, right = _frames(m, seed=31)
    want_pose, want_kp = (t.clone() for t in m.predict_pose_from_rgb(left, right, return_keypoints=True))
    pose, kp = m.predict_pose_from_camera(l8, r8, return_keypoints=True)
    torch.cuda.synchronize()
    assert torch.equal(pose, want_pose)
    _same_records(kp, want_kp)
    # the sensor's frames: each eye's (x, y) is the affine image of what the camera route reads out of the host-resized frames
    lh, rh = _bytes8(32, (B, 96, 120, 3))
    c8l, c8r = spec.resize_u8(lh, CROP, False, 4 * S).cuda(), spec.resize_u8(rh, CROP_R, True, 4 * S).cuda()
    cam_pose, cam_kp = (t.clone() for t in m.predict_pose_from_camera(c8l, c8r, return_keypoints=True))
    pose, hm, kp = m.predict_pose_from_sensor(lh.cuda(), rh.cuda(), crop=CROP, crop_right=CROP_R, mirror_right=True, return_heatmaps=True, return_keypoints=True)
    torch.cuda.synchronize()
    assert torch.equal(pose, cam_pose)
    cam, got = cam_kp.cpu().double().numpy(), kp.cpu().numpy()
    assert np.array_equal(got[..., 2:], cam_kp.cpu().numpy()[..., 2:])               # score and index
    for eye, (rect, mirror) in enumerate(((CROP, False), (CROP_R, True))):
        ax, bx, ay, by = (float(v) for v in spec.sensor_keypoint_affine(rect, mirror, S))
        x, y = ax * (cam[:, eye, :, 0] / 4.0) + bx, ay * (cam[:, eye, :, 1] / 4.0) + by
        print("sensor eye", eye, "max |dx|, |dy|", np.abs(got[:, eye, :, 0] - x).max(), np.abs(got[:, eye, :, 1] - y).max())
        assert np.abs(got[:, eye, :, 0] - x).max() <= 1e-3 and np.abs(got[:, eye, :, 1] - y).max() <= 1e-3
        x0, y0, w, h = rect
        assert (got[:, eye, :, 0] >= x0).all() and (got[:, eye, :, 0] <= x0 + w).all() and (got[:, eye, :, 1] >= y0).all() and (got[:, eye, :, 1] <= y0 + h).all()
    # and bit for bit the operator with that affine on the heatmaps the call returns
    aff = [spec.sensor_keypoint_affine(CROP, False, S), spec.sensor_keypoint_affine(CROP_R, True, S)]
    _same_records(kp, _peaks_of(hm, J, affine=aff))


def test_side_128_egocap():
    m, p = _model("EgoCap", 128)
    g = torch.Generator().manual_seed(41)
    left, right = (torch.randn((1, 3, 512, 512), generator=g).cuda() for _ in range(2))
    want_pose = m.predict_pose_from_rgb(left, right).clone()
    pose, hm, kp = m.predict_pose_from_rgb(left, right, return_heatmaps=True, return_keypoints=True)
    torch.cuda.synchronize()
    assert tuple(kp.shape) == (1, 2, 17, 4) and torch.equal(pose, want_pose)
    _same_records(kp, _peaks_of(hm, 17))
