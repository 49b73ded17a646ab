"""Frames from another lens on the device: egotap_lens_remap (lens_remap_kernel) and EgoTAPAutoEncoderModel.predict_pose_from_lens
(egotap_predict_pose_lens / _kp / _kpl).

The expected value of the operator is spec.lens_remap_u8 (for NV12 / YUYV: of spec.yuv_to_rgb_u8(frames)), the integer restatement of the same
arithmetic: the comparison is torch.equal.  The expected value of the one call is predict_pose_from_camera on the restatement's bytes: torch.equal
again, no tolerance anywhere.  The operator writes into a canary-filled buffer whose bytes around the outputs must stay untouched."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model, timed_launches as _launches
import ocam_inputs as OI
import yuv_cases as Y_

pytestmark = pytest.mark.gpu
POISON, ONE = 0xEE, 2048


def _helper(f, xc, yc, size):
    return dataclasses.replace(OI.pinhole(f, "helper"), xc=xc, yc=yc, size=size)


def _helper_maps(H, W, S0, f2):
    """two different maps that run over the far edges of an H x W frame (the helper lenses of test_lens_map_cpu.py): the left one rotated, the
    right one mirrored"""
    model = _helper(20.0, 31.25, 23.75, (48, 64))
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    left = spec.lens_map(model, _helper(f2, W - 1.5 - 0.5 * f2, H - 1.25 - 0.5 * f2, (H, W)), S0, R=R)
    right = spec.lens_map(model, _helper(f2, 0.45 * f2, 0.55 * f2, (H, W)), S0, mirror=True)
    for m in (left, right):
        assert 0.05 < m.valid.mean() < 0.95
    assert not np.array_equal(left.taps, right.taps)
    return left, right


def _odd(host):
    """the frames on the device at an odd address"""
    store = torch.full((host.numel() + 16,), POISON, dtype=torch.uint8, device="cuda")
    dev = store[1:1 + host.numel()].view(host.shape).copy_(host)
    assert dev.data_ptr() % 2 == 1 and dev.is_contiguous()
    return dev


def _run_between_canaries(l8, r8, B, maps, layout=None, colour=None):
    S0 = maps.S0
    n, pad, canary = B * S0 * S0 * 3, 1024, 0xA5
    flat = torch.full((2 * (n + pad) + pad,), canary, dtype=torch.uint8, device="cuda")
    out_l, out_r = flat[pad:pad + n], flat[2 * pad + n:2 * pad + 2 * n]          # canaries in front of, between and behind the outputs
    assert out_l.data_ptr() % 4 == 0 and out_r.data_ptr() % 4 == 0
    L.check(L.load().egotap_lens_remap(L.ptr(l8), L.ptr(r8), B, C.byref(L.lens_source(maps, layout, colour)), S0, L.ptr(out_l), L.ptr(out_r), L.stream()))
    torch.cuda.synchronize()
    for lo, hi in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, flat.numel())):
        assert bool((flat[lo:hi] == canary).all()), (lo, hi)
    return out_l.view(B, S0, S0, 3), out_r.view(B, S0, S0, 3)


def _rgb(seed, B, H, W):
    x = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    x[:, 0, 0], x[:, -1, -1] = 0, 255
    return x


def _check_rgb(lh, rh, l8, r8, maps):
    B = lh.shape[0]
    got_l, got_r = _run_between_canaries(l8, r8, B, maps)
    for got, host, m, fill in ((got_l, lh, maps.left, maps.fill[0]), (got_r, rh, maps.right, maps.fill[1])):
        want = spec.lens_remap_u8(host, m, fill)
        assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    return got_l, got_r


# ------------------------------------------------------------------------------------------------------------ 1. the operator, packed RGB
def test_hand_made_map_corners_fractions_and_fill():
    B, H, W, S0 = 1, 5, 7, 4
    left = np.full((S0, S0, 2), -1, dtype=np.int32)
    left[0, 0] = (0, 0)                                       # the first pixel
    left[0, 1] = (6 * ONE, 4 * ONE)                           # the last pixel: both second taps are clamped onto it
    left[0, 3] = (6 * ONE, 0)
    left[1, 0] = (0, 4 * ONE)
    left[1, 2] = (2 * ONE + 512, 1 * ONE + 1536)
    left[2, 1] = (5 * ONE + 2047, 3 * ONE + 2047)             # the last fraction below the last pixel
    left[3, 3] = (1, 1)
    right = np.full((S0, S0, 2), -1, dtype=np.int32)
    right[:, :, 0] = (np.arange(16).reshape(4, 4) * 797) % (6 * ONE + 1)
    right[:, :, 1] = (np.arange(16).reshape(4, 4) * 523) % (4 * ONE + 1)
    right[1, 1] = right[2, 3] = -1
    maps = L.lens_maps(spec.LensMap(left, S0, H, W, (8, 8)), spec.LensMap(right, S0, H, W, (8, 8)), fill=((9, 200, 31), (255, 0, 128)))
    lh, rh = _rgb(1, B, H, W), _rgb(2, B, H, W)
    got_l, got_r = _check_rgb(lh, rh, lh.cuda(), rh.cuda(), maps)
    assert torch.equal(got_l[0, 0, 0].cpu(), lh[0, 0, 0]) and torch.equal(got_l[0, 0, 1].cpu(), lh[0, 4, 6])
    assert got_l[0, 3, 0].tolist() == [9, 200, 31] and got_r[0, 1, 1].tolist() == [255, 0, 128]


def test_odd_addresses_and_a_map_per_eye():
    B, H, W, S0 = 2, 37, 53, 8
    maps = L.lens_maps(*_helper_maps(H, W, S0, 40.0), fill=(7, 7, 7))
    lh, rh = _rgb(3, B, H, W), _rgb(4, B, H, W)
    _check_rgb(lh, rh, _odd(lh), _odd(rh), maps)
    a, b = L.lens_remap(lh.cuda(), rh.cuda(), maps, S0)          # the Python face: the same bytes
    assert torch.equal(a.cpu(), spec.lens_remap_u8(lh, maps.left, (7, 7, 7))) and torch.equal(b.cpu(), spec.lens_remap_u8(rh, maps.right, (7, 7, 7)))


def test_grid_stride_loop_takes_a_second_turn():
    B, H, W, S0 = 33, 64, 64, 256
    assert B * S0 * (S0 // 4) > 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256          # more thread groups than the grid holds
    maps = L.lens_maps(*_helper_maps(H, W, S0, 40.0), fill=((1, 2, 3), (4, 5, 6)))
    l8, r8 = _rgb(5, B, H, W).cuda(), _rgb(6, B, H, W).cuda()
    got_l, got_r = _run_between_canaries(l8, r8, B, maps)
    # (the restatement in torch integers on the device's copy of the same bytes: exact wherever it runs, and quick at this size)
    assert torch.equal(got_l, spec.lens_remap_u8(l8, maps.left, (1, 2, 3))) and torch.equal(got_r, spec.lens_remap_u8(r8, maps.right, (4, 5, 6)))


def test_identity_lens_equals_the_resize_kernel_inside_the_circle():
    """the identity-lens map of the anchor test against rgb_u8_resize_kernel's bytes: the two kernels tied together on the device"""
    B, S0 = 3, 256
    cam = OI.calibration(0)
    plain, mirrored = spec.lens_map(cam, cam, S0), spec.lens_map(cam, cam, S0, mirror=True)
    maps = L.lens_maps(plain, mirrored)
    l8, r8 = _rgb(7, B, 1024, 1024).cuda(), _rgb(8, B, 1024, 1024).cuda()
    got_l, got_r = _run_between_canaries(l8, r8, B, maps)
    want_l, want_r = L.rgb_u8_resize(l8, r8, S0, mirror_right=True)
    for got, want, m, src in ((got_l, want_l, plain, l8), (got_r, want_r, mirrored, r8)):
        ok = torch.from_numpy(m.valid).cuda()
        assert 0.74 <= float(ok.float().mean()) <= 0.76
        assert torch.equal(got[:, ok], want[:, ok]) and not bool(got[:, ~ok].any())
        assert torch.equal(got, spec.lens_remap_u8(src, m))


# ------------------------------------------------------------------------------------------------------------ 2. the operator, NV12 / YUYV
def _yuv_layout(fmt, H, W, pitch):
    return spec.YuvLayout.nv12(H, W, pitch, pitch * H + 6, pitch * H + 6 + pitch * (H // 2) + 4) if fmt == "nv12" else spec.YuvLayout.yuyv(H, W, pitch, pitch * H + 8)


def _at_minimum_alignment(host, layout):
    a = layout.base_alignment
    store = torch.full((host.numel() + 16,), POISON, dtype=torch.uint8, device="cuda")
    dev = store[a:a + host.numel()].view(host.shape).copy_(host)
    assert dev.data_ptr() % (2 * a) == a and dev.is_contiguous()
    return dev


def _check_yuv(lh, rh, layout, colour, maps):
    B = lh.shape[0]
    got_l, got_r = _run_between_canaries(_at_minimum_alignment(lh, layout), _at_minimum_alignment(rh, layout), B, maps, layout, colour)
    for got, host, m, fill in ((got_l, lh, maps.left, maps.fill[0]), (got_r, rh, maps.right, maps.fill[1])):
        want = spec.lens_remap_u8(spec.yuv_to_rgb_u8(host, layout, colour), m, fill)
        assert torch.equal(got.cpu(), want), (layout.format, colour, int((got.cpu() != want).sum()))


@pytest.mark.parametrize("fmt,pitch", [("nv12", 16), ("yuyv", 32)])
def test_small_yuv_frames_with_a_padded_pitch(fmt, pitch):
    B, H, W, S0 = 2, 6, 8, 4
    layout = _yuv_layout(fmt, H, W, pitch)
    assert bool(Y_.padding_mask(layout).any())
    left, right = _helper_maps(H, W, 16, 4.0)
    # every fourth row and column of a denser map, and by hand the frame's two corners: the last chroma block and pixel pair are read
    lt, rt = np.array(left.taps[1::4, 2::4]), np.array(right.taps[2::4, 1::4])
    lt[0, 0], lt[3, 3], rt[0, 3] = (0, 0), ((W - 1) * ONE, (H - 1) * ONE), ((W - 2) * ONE + 1024, (H - 2) * ONE + 1024)
    maps = L.lens_maps(spec.LensMap(lt, S0, H, W, (48, 64)), spec.LensMap(rt, S0, H, W, (48, 64)), fill=((50, 60, 70), (0, 0, 0)))
    assert maps.left.valid.sum() >= 4 and maps.right.valid.sum() >= 4 and not maps.left.valid.all()
    lh, rh = Y_.frames(11, B, layout, POISON), Y_.frames(12, B, layout, POISON)
    for colour in (Y_.COLOURS[0], Y_.COLOURS[3]):
        _check_yuv(lh, rh, layout, colour, maps)


@pytest.fixture(scope="module")
def rig_maps():
    """calibration 0 seen through calibration 1, 0.02 rad about the axis apart, on 480 x 640 frames: the valid share is about 0.65"""
    cam, sensor = OI.rig_models(True)
    left = spec.lens_map(cam, sensor, 256, OI.SMALL_R, frame_size=(480, 640))
    right = spec.lens_map(cam, sensor, 256, OI.SMALL_R.T, frame_size=(480, 640), mirror=True)
    for m in (left, right):
        assert 0.6 < m.valid.mean() < 0.7
    return L.lens_maps(left, right, fill=((0, 0, 0), (128, 128, 128)))


@pytest.mark.parametrize("colour", Y_.COLOURS, ids=[f"{c.matrix}-{c.range}" for c in Y_.COLOURS])
@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_fisheye_rig_on_camera_buffers(rig_maps, fmt, colour):
    B, H, W = 2, 480, 640
    layout = _yuv_layout(fmt, H, W, W + 10 if fmt == "nv12" else 2 * W + 12)
    lh, rh = Y_.frames(21, B, layout, POISON), Y_.frames(22, B, layout, POISON)
    _check_yuv(lh, rh, layout, colour, rig_maps)


# ------------------------------------------------------------------------------------------------------------ 3. one call
def _clones(out):
    return tuple(t.clone() for t in out)


def _serving_maps(m, hm, model_size, mirror_right):
    """the rig's maps at the estimators' side; ``model_size`` replaces the calibration image's size (the keypoint affine reads nothing else of it)"""
    cam, sensor = OI.rig_models(True)
    left = spec.lens_map(cam, sensor, 4 * hm, OI.SMALL_R, frame_size=(96, 80))
    right = spec.lens_map(cam, sensor, 4 * hm, OI.SMALL_R.T, frame_size=(96, 80), mirror=mirror_right)
    left, right = (dataclasses.replace(x, model_size=model_size) for x in (left, right))
    return m.lens_maps(left, right, fill=((0, 0, 0), (90, 100, 110)))


def _other_entries_sizes(m, B, chunk):
    lib, h = L.load(), m._rgb_state(torch.device("cuda", torch.cuda.current_device())).handle.h
    out = []
    for fn, args in ((lib.egotap_predict_pose_rgb_workspace_bytes, (B, chunk)), (lib.egotap_predict_pose_rgb_u8_workspace_bytes, (B, chunk)),
                     (lib.egotap_predict_pose_sensor_u8_workspace_bytes, (B, 96, 80, chunk))):
        n = C.c_size_t()
        L.check(fn(h, *args, C.byref(n)))
        out.append(n.value)
    return out


def test_one_call_fp32_equals_the_camera_entry_on_the_restatement():
    """B = 2 in one piece, packed RGB, a model camera of the frame's own size and no mirror: the keypoint affine is the camera entry's, so every output
    is the camera entry's in bits; graphed equals ungraphed; the triangulation is the operator on the returned keypoints"""
    hm, B = 32, 2
    m, p = _model("UnrealEgo", hm)
    S0 = 4 * hm
    maps = _serving_maps(m, hm, (S0, S0), False)
    lh, rh = _rgb(31, B, 96, 80), _rgb(32, B, 96, 80)
    l8, r8 = lh.cuda(), rh.cuda()
    cam_l, cam_r = spec.lens_remap_u8(lh, maps.left, maps.fill[0]).cuda(), spec.lens_remap_u8(rh, maps.right, maps.fill[1]).cuda()
    every = dict(return_heatmaps=True, return_keypoints=True, return_limbs=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    try:
        graphs = m._rgb_state(dev).graphs
        graphs.clear()
        sizes = _other_entries_sizes(m, B, 256)
        want = _clones(m.predict_pose_from_camera(cam_l, cam_r, **every))
        want_graphed = _clones(m.predict_pose_from_camera(cam_l, cam_r, graphed=True, **every))
        assert len(graphs) == 1
        for graphed in (False, True):
            got = m.predict_pose_from_lens(l8, r8, maps, graphed=graphed, **every)
            torch.cuda.synchronize()
            assert len(got) == 4
            for name, a, b in zip(("pose", "heatmaps", "keypoints", "limbs"), got, want):
                assert torch.equal(a, b), (graphed, name, float((a - b).abs().max()))
        assert len(graphs) == 2 and sum("lens" in k for k in graphs) == 1
        # the triangulation: the operator on the keypoints and the pose this call returns, the identity as the pixel affine
        left, right = OI.rig_models(True)
        m.set_stereo_rig(left, right, OI.T, R=OI.SMALL_R, min_score=0.0)
        pose, kp, j3, fr = m.predict_pose_from_lens(l8, r8, maps, return_keypoints=True, return_triangulation=True)
        torch.cuda.synchronize()
        w3, wf = L.stereo_triangulate(kp, left, right, OI.T, R=OI.SMALL_R, affine=spec.STEREO_IDENTITY_AFFINE, min_score=0.0, pose=pose,
                                      pose_row0=spec.stereo_pose_row0(p))
        assert torch.equal(pose, want[0]) and torch.equal(kp, want[2])
        assert torch.equal(j3.view(torch.int32), w3.view(torch.int32)) and torch.equal(fr.view(torch.int32), wf.view(torch.int32))
        # the other entries afterwards: their sizes, their graph, their bits
        assert _other_entries_sizes(m, B, 256) == sizes
        again = m.predict_pose_from_camera(cam_l, cam_r, graphed=True, **every)
        torch.cuda.synchronize()
        assert len(graphs) == 2 and all(torch.equal(a, b) for a, b in zip(again, want_graphed)) and all(torch.equal(a, b) for a, b in zip(again, want))
        launches = _launches(m, lambda: m.predict_pose_from_lens(l8, r8, maps, **every))
        assert [x for x in launches if "lens" in x[0] or "resize" in x[0]] == [("lens_remap", "lens_remap_kernel", 1)], launches
    finally:
        m._rgb["graphs"].clear()
        m.__dict__.pop("_stereo_rig", None)


def test_one_call_bf16_frozen_in_pieces_from_nv12_with_a_mirrored_eye():
    """B = 3 in pieces of one frame, NV12 frames, frozen bf16 weights, a 1024 x 1024 model camera and a mirrored right eye: pose and heatmaps are the
    camera entry's on the restatement's bytes, keypoints and limbs the standalone operators' on those heatmaps with the model camera's affine"""
    hm, B = 64, 3
    m, p = _model("UnrealEgo", hm)
    J = p.n_joints_hm
    maps = _serving_maps(m, hm, (1024, 1024), True)
    layout, colour = spec.YuvLayout.nv12(96, 80, pitch=96), spec.YuvColour("bt709", "full")
    lh, rh = Y_.frames(41, B, layout, POISON), Y_.frames(42, B, layout, POISON)
    l8, r8 = lh.cuda(), rh.cuda()
    cam_l = spec.lens_remap_u8(spec.yuv_to_rgb_u8(lh, layout, colour), maps.left, maps.fill[0]).cuda()
    cam_r = spec.lens_remap_u8(spec.yuv_to_rgb_u8(rh, layout, colour), maps.right, maps.fill[1]).cuda()
    affine = [spec.sensor_keypoint_affine((0, 0, 1024, 1024), False, hm), spec.sensor_keypoint_affine((0, 0, 1024, 1024), True, hm)]
    assert [tuple(float(v) for v in a) for a in affine] == [(16.0, 0.0, 16.0, 0.0), (-16.0, 1024.0, 16.0, 0.0)]
    try:
        m.set_precision("bf16")
        assert m.freeze_weights(batch=1) == {}
        m.opt.hm_chunk = 1
        dev = torch.device("cuda", torch.cuda.current_device())
        graphs = m._rgb_state(dev).graphs
        graphs.clear()
        want_pose, want_hm = _clones(m.predict_pose_from_camera(cam_l, cam_r, return_heatmaps=True))
        want_kp = L.heatmap_peaks(want_hm, 0, 2 * J, groups=2, affine=affine).view(B, 2, J, 4)
        want_lb = L.limb_decode(want_hm, 2 * J, J, eyes=2, affine=affine)
        lean_pose = m.predict_pose_from_camera(cam_l, cam_r).clone()          # no heatmaps asked for: the hand-off route
        assert m.rgb_form() == "handoff"
        for graphed in (False, True):
            got = m.predict_pose_from_lens(l8, r8, maps, layout, colour, graphed=graphed, return_heatmaps=True, return_keypoints=True, return_limbs=True)
            torch.cuda.synchronize()
            for name, a, b in zip(("pose", "heatmaps", "keypoints", "limbs"), got, (want_pose, want_hm, want_kp, want_lb)):
                assert torch.equal(a, b), (graphed, name, float((a - b).abs().max()))
            got = m.predict_pose_from_lens(l8, r8, maps, layout, colour, graphed=graphed)
            torch.cuda.synchronize()
            assert torch.equal(got, lean_pose) and (graphed or m.rgb_form() == "handoff")
        assert len(graphs) == 2 and all("lens" in k and "nv12" in k for k in graphs)
        # another colour is another graph: the key holds the layout and the colour
        m.predict_pose_from_lens(l8, r8, maps, layout, spec.YuvColour("bt601", "limited"), graphed=True)
        assert len(graphs) == 3
        launches = _launches(m, lambda: m.predict_pose_from_lens(l8, r8, maps, layout, colour))
        assert [x for x in launches if "lens" in x[0] or "resize" in x[0]] == [("lens_remap", "lens_remap_kernel", 3)], launches      # one per piece
        camera = _launches(m, lambda: m.predict_pose_from_camera(cam_l, cam_r))
        assert sorted(x for x in launches if x[0] != "lens_remap") == sorted(camera)
    finally:
        m._rgb["graphs"].clear()
        m.unfreeze_weights()
        m.set_precision("f32")
        m.opt.hm_chunk = 256


def test_mixed_precisions_run_the_module_route_by_name():
    m, p = _model("UnrealEgo", 64)
    maps = _serving_maps(m, 64, (256, 256), False)
    lh, rh = _rgb(51, 2, 96, 80), _rgb(52, 2, 96, 80)
    l8, r8 = lh.cuda(), rh.cuda()
    cam_l, cam_r = spec.lens_remap_u8(lh, maps.left, maps.fill[0]).cuda(), spec.lens_remap_u8(rh, maps.right, maps.fill[1]).cuda()
    every = dict(return_heatmaps=True, return_keypoints=True, return_limbs=True)
    try:
        m.net_HeatMap.set_precision("bf16")
        m.net_RotHeatMap.set_precision("bf16")                      # the head stays fp32
        assert "different precisions" in m._rgb_one_call_refusal()
        want = _clones(m.predict_pose_from_camera(cam_l, cam_r, **every))
        got = m.predict_pose_from_lens(l8, r8, maps, **every)
        torch.cuda.synchronize()
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
        with pytest.raises(L.EgotapError, match=r"predict_pose_from_lens\(graphed=True\).*the lens remap.*ungraphed"):
            m.predict_pose_from_lens(l8, r8, maps, graphed=True)
    finally:
        m.eval()
        m.set_precision("f32")
