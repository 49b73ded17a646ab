"""NV12 / YUYV sensor frames on the device: egotap_yuv_u8_resize (yuv_u8_resize_kernel) and EgoTAPAutoEncoderModel.predict_pose_from_sensor_yuv
(egotap_predict_pose_sensor_yuv / _kp / _kpl).

The expected value of the operator is spec.yuv_resize_u8 = spec.resize_u8(spec.yuv_to_rgb_u8(frames)), the integer restatement of the same
arithmetic: the comparison is torch.equal.  The expected value of the one call is predict_pose_from_sensor on spec.yuv_to_rgb_u8(frames):
torch.equal again, no tolerance anywhere.

Frames are random planes (0 and 255 in each) inside buffers whose padding -- the row tails past W or 2 W, the gap in front of the chroma plane, the
frame's tail -- is poisoned with a byte of its own; the operator writes into a canary-filled buffer whose bytes around the outputs must stay
untouched."""
import ctypes as C

import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model, timed_launches as _launches
from serving_cases import SENSOR_ARGS, SENSOR_H, SENSOR_W
import yuv_cases as Y_

pytestmark = pytest.mark.gpu
POISON = 0xEE


def _layout(fmt, H, W):
    """a layout with a padded pitch, (nv12) a gap in front of the chroma plane, and a tail behind the last byte"""
    if fmt == "nv12":
        pitch = W + 10
        uv = pitch * H + 6
        return spec.YuvLayout.nv12(H, W, pitch, uv, uv + pitch * (H // 2) + 4)
    pitch = 2 * W + 12
    return spec.YuvLayout.yuyv(H, W, pitch, pitch * H + 8)


def _at_minimum_alignment(host, layout):
    """the frames on the device at the smallest address offset the format allows (2 for nv12, 4 for yuyv) inside a larger, poisoned buffer"""
    a = layout.base_alignment
    store = torch.full((host.numel() + 16,), POISON, dtype=torch.uint8, device="cuda")
    dev = store[a:a + host.numel()].view(host.shape).copy_(host)
    assert dev.data_ptr() % (2 * a) == a and dev.is_contiguous()
    return dev


def _rects(H, W):
    """(left, right) rectangle pairs: odd origins and odd sizes, a single pixel in the far corner and inside, one row, the full frame"""
    return [(None, (1, 1, W - 1, H - 1)),
            ((W - 1, H - 1, 1, 1), (0, 1, W - 1, H - 2)),
            ((1, 0, max(1, W // 2), H - 1), (W - W // 2 - 1, 1, W // 2 + 1, 1)),
            ((0, 0, W, H), (W // 2, H // 2, 1, 1))]


MIRRORS = [(0, 1), (1, 0), (1, 1), (0, 0)]
OPERATOR = [(38, 54, 64), (96, 80, 128), (6, 4, 64), (130, 258, 260)]          # 6 x 4: an upscale; S0 = 260: the table loop's second pass


def _run_between_canaries(l8, r8, B, layout, colour, rect_l, rect_r, mirror_l, mirror_r, S0):
    n, pad, canary = B * S0 * S0 * 3, 1024, 0xA5
    flat = torch.full((2 * (n + pad) + pad,), canary, dtype=torch.uint8, device="cuda")
    out_l, out_r = flat[pad:pad + n], flat[2 * pad + n:2 * pad + 2 * n]          # canaries in front of, between and behind the outputs
    assert out_l.data_ptr() % 4 == 0 and out_r.data_ptr() % 4 == 0
    rl = (C.c_int * 4)(*spec.check_resize_rect("t", rect_l, layout.H, layout.W))
    rr = (C.c_int * 4)(*spec.check_resize_rect("t", rect_r, layout.H, layout.W))
    L.check(L.load().egotap_yuv_u8_resize(L.ptr(l8), L.ptr(r8), B, C.byref(L.yuv_source(layout, colour)), rl, rr, mirror_l, mirror_r, S0, L.ptr(out_l),
                                          L.ptr(out_r), L.stream()))
    torch.cuda.synchronize()
    for lo, hi in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, flat.numel())):
        assert bool((flat[lo:hi] == canary).all()), (lo, hi)
    return out_l.view(B, S0, S0, 3), out_r.view(B, S0, S0, 3)


# ------------------------------------------------------------------------------------------------------------ 1. the operator
@pytest.mark.parametrize("H,W,S0", OPERATOR)
@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_operator_equals_the_integer_restatement_and_stays_inside_its_outputs(fmt, H, W, S0):
    B = 3
    layout = _layout(fmt, H, W)
    lh, rh = Y_.frames(100 + H, B, layout, POISON), Y_.frames(200 + W, B, layout, POISON)
    assert bool(Y_.padding_mask(layout).any())
    l8, r8 = _at_minimum_alignment(lh, layout), _at_minimum_alignment(rh, layout)
    for colour, (rect_l, rect_r), (mirror_l, mirror_r) in zip(Y_.COLOURS, _rects(H, W), MIRRORS):
        got_l, got_r = _run_between_canaries(l8, r8, B, layout, colour, rect_l, rect_r, mirror_l, mirror_r, S0)
        want_l = spec.yuv_resize_u8(lh, layout, colour, rect_l, bool(mirror_l), S0)
        want_r = spec.yuv_resize_u8(rh, layout, colour, rect_r, bool(mirror_r), S0)
        assert torch.equal(got_l.cpu(), want_l), (colour, rect_l, mirror_l, int((got_l.cpu() != want_l).sum()))
        assert torch.equal(got_r.cpu(), want_r), (colour, rect_r, mirror_r, int((got_r.cpu() != want_r).sum()))
    # the Python face: aligned frames, the default rectangle on the left, the same bytes
    colour, rect_r = Y_.COLOURS[1], _rects(H, W)[0][1]
    a, b = L.yuv_u8_resize(lh.cuda(), rh.cuda(), layout, colour, S0, rect_right=rect_r, mirror_right=True)
    assert torch.equal(a.cpu(), spec.yuv_resize_u8(lh, layout, colour, None, False, S0))
    assert torch.equal(b.cpu(), spec.yuv_resize_u8(rh, layout, colour, rect_r, True, S0))


@pytest.mark.parametrize("fmt", ["nv12", "yuyv"])
def test_grid_stride_loop_takes_a_second_turn(fmt):
    B, H, W, S0 = 3, 38, 54, 1024
    groups = B * S0 * (S0 // 4)
    assert groups > 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256          # more thread groups than the grid holds
    layout, colour = _layout(fmt, H, W), Y_.COLOURS[0]
    lh, rh = Y_.frames(31, B, layout, POISON), Y_.frames(32, B, layout, POISON)
    l8, r8 = _at_minimum_alignment(lh, layout), _at_minimum_alignment(rh, layout)
    rect_l, rect_r = (1, 1, 51, 35), (3, 0, 50, 37)
    got_l, got_r = _run_between_canaries(l8, r8, B, layout, colour, rect_l, rect_r, 0, 1, S0)
    # (the restatement in torch integers on the device's copy of the same bytes: exact wherever it runs, and quick at this size)
    assert torch.equal(got_l, spec.yuv_resize_u8(lh.cuda(), layout, colour, rect_l, False, S0))
    assert torch.equal(got_r, spec.yuv_resize_u8(rh.cuda(), layout, colour, rect_r, True, S0))


# ------------------------------------------------------------------------------------------------------------ 2. every triple
def test_every_triple_on_the_device_bt601_limited():
    frame, layout = Y_.all_triples_nv12()
    colour = spec.YuvColour("bt601", "limited")
    dev = frame.cuda()
    a, b = L.yuv_u8_resize(dev, dev, layout, colour, 4096)          # w = h = S0: an exact copy of the converted frame
    want = spec.yuv_to_rgb_u8(frame, layout, colour)
    assert torch.equal(a.cpu(), want) and torch.equal(b, a)


@pytest.mark.parametrize("colour", Y_.COLOURS[1:], ids=[f"{c.matrix}-{c.range}" for c in Y_.COLOURS[1:]])
def test_lattice_triples_on_the_device(colour):
    frame, layout = Y_.lattice_nv12()
    dev = frame.cuda()
    a, b = L.yuv_u8_resize(dev, dev, layout, colour, 512)
    want = spec.yuv_to_rgb_u8(frame, layout, colour)
    assert torch.equal(a.cpu(), want) and torch.equal(b, a)


# ------------------------------------------------------------------------------------------------------------ 3. one call
B, CHUNK = 3, 2          # one full piece and one ragged piece


def _clones(out):
    return tuple(t.clone() for t in out)


@pytest.mark.parametrize("hm,setting", [(32, "f32"), (64, "bf16_frozen")])
def test_one_call_equals_the_sensor_entry_on_the_converted_frames(hm, setting):
    m, p = _model("UnrealEgo", hm)
    layout = spec.YuvLayout.nv12(SENSOR_H, SENSOR_W, pitch=SENSOR_W + 16)
    colour = spec.YuvColour("bt601", "limited")
    lh, rh = Y_.frames(41, B, layout, POISON), Y_.frames(42, B, layout, POISON)
    rgb_l, rgb_r = spec.yuv_to_rgb_u8(lh, layout, colour).cuda(), spec.yuv_to_rgb_u8(rh, layout, colour).cuda()
    l8, r8 = lh.cuda(), rh.cuda()
    every = dict(return_heatmaps=True, return_keypoints=True, return_limbs=True)
    lean = dict(return_keypoints=True, return_limbs=True)          # no heatmaps asked for: the hand-off route where the setting has one
    try:
        m.set_precision(setting.split("_")[0])
        if setting.endswith("_frozen"):
            assert m.freeze_weights(batch=CHUNK) == {}
        m.opt.hm_chunk = CHUNK
        graphs = m._rgb_state(torch.device("cuda", torch.cuda.current_device())).graphs
        graphs.clear()
        want = _clones(m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, **every))
        want_lean = _clones(m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, **lean))
        want_form = m.rgb_form()
        assert want_form == ("handoff" if setting == "bf16_frozen" else "scratch")
        want_graphed = _clones(m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, graphed=True, **every))          # the sensor entry's own graph
        assert len(graphs) == 1 and all(torch.equal(a, b) for a, b in zip(want_graphed, want))
        for graphed in (False, True):
            got = m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, **SENSOR_ARGS, graphed=graphed, **every)
            torch.cuda.synchronize()
            assert len(got) == 4
            for name, a, b in zip(("pose", "heatmaps", "keypoints", "limbs"), got, want):
                assert torch.equal(a, b), (graphed, name, float((a - b).abs().max()))
            got = m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, **SENSOR_ARGS, graphed=graphed, **lean)
            torch.cuda.synchronize()
            assert len(got) == 3 and (graphed or m.rgb_form() == want_form)
            for name, a, b in zip(("pose", "keypoints", "limbs"), got, want_lean):
                assert torch.equal(a, b), (graphed, name, float((a - b).abs().max()))
        assert len(graphs) == 3 and sum("sensor_yuv" in k for k in graphs) == 2 and sum("sensor" in k for k in graphs) == 1
        # another colour is another graph: the key holds the layout and the colour
        m.predict_pose_from_sensor_yuv(l8, r8, layout, spec.YuvColour("bt709", "full"), **SENSOR_ARGS, graphed=True, **every)
        assert len(graphs) == 4
        # the existing entry afterwards: its earlier bits, on the graph it already had
        again = m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, graphed=True, **every)
        torch.cuda.synchronize()
        assert len(graphs) == 4 and all(torch.equal(a, b) for a, b in zip(again, want))
        eager = m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, **every)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, want))
        # the timing hook: one conversion-and-resize launch per piece, no RGB resize; everything else is what the sensor entry launches
        yuv = _launches(m, lambda: m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, **SENSOR_ARGS, **lean))
        rgb = _launches(m, lambda: m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, **lean))
        assert [x for x in yuv if "resize" in x[0] or "resize" in x[1]] == [("yuv_u8_resize", "yuv_u8_resize_kernel", 2)], yuv
        assert [x for x in rgb if "resize" in x[0]] == [("rgb_u8_resize", "rgb_u8_resize_kernel", 2)], rgb
        assert sorted(x for x in yuv if "resize" not in x[0]) == sorted(x for x in rgb if "resize" not in x[0])
    finally:
        m._rgb["graphs"].clear()
        m.unfreeze_weights()
        m.set_precision("f32")
        m.opt.hm_chunk = 256


def test_a_full_frame_at_the_output_size_still_converts():
    """no identity request: H = W = 4S with the full rectangle and no mirror launches the kernel (an exact copy of the converted frame)"""
    m, p = _model("UnrealEgo", 32)
    layout, colour = spec.YuvLayout.yuyv(128, 128), spec.YuvColour("bt709", "limited")
    lh, rh = Y_.frames(51, 2, layout), Y_.frames(52, 2, layout)
    want = m.predict_pose_from_camera(spec.yuv_to_rgb_u8(lh, layout, colour).cuda(), spec.yuv_to_rgb_u8(rh, layout, colour).cuda()).clone()
    l8, r8 = lh.cuda(), rh.cuda()
    got = m.predict_pose_from_sensor_yuv(l8, r8, layout, colour)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    launches = _launches(m, lambda: m.predict_pose_from_sensor_yuv(l8, r8, layout, colour))
    assert [x for x in launches if "resize" in x[0]] == [("yuv_u8_resize", "yuv_u8_resize_kernel", 1)], launches


def test_mixed_precisions_run_the_module_route_by_name():
    """networks in different precisions cannot share one handle: lib.yuv_u8_resize, the converter and the module forwards run -- the bits of the
    sensor entry's module route on the converted frames; graphed is refused by name"""
    m, p = _model("UnrealEgo", 64)
    layout, colour = spec.YuvLayout.yuyv(SENSOR_H, SENSOR_W, pitch=2 * SENSOR_W + 8), spec.YuvColour("bt709", "full")
    lh, rh = Y_.frames(61, 2, layout, POISON), Y_.frames(62, 2, layout, POISON)
    rgb_l, rgb_r = spec.yuv_to_rgb_u8(lh, layout, colour).cuda(), spec.yuv_to_rgb_u8(rh, layout, colour).cuda()
    l8, r8 = lh.cuda(), rh.cuda()
    every = dict(return_heatmaps=True, return_keypoints=True, return_limbs=True)
    try:
        m.net_HeatMap.set_precision("bf16")
        m.net_RotHeatMap.set_precision("bf16")                      # the head stays fp32
        assert "different precisions" in m._rgb_one_call_refusal()
        want = _clones(m.predict_pose_from_sensor(rgb_l, rgb_r, **SENSOR_ARGS, **every))
        got = m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, **SENSOR_ARGS, **every)
        torch.cuda.synchronize()
        assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
        with pytest.raises(L.EgotapError, match=r"predict_pose_from_sensor_yuv\(graphed=True\).*the conversion and resize.*ungraphed"):
            m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, **SENSOR_ARGS, graphed=True)
    finally:
        m.eval()
        m.set_precision("f32")
