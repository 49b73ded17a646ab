"""The sensor's own frames on the device: egotap_rgb_u8_resize (rgb_u8_resize_kernel) and EgoTAPAutoEncoderModel.predict_pose_from_sensor
(egotap_predict_pose_sensor_u8).

The expected value of the operator is spec.resize_u8, the integer restatement of the same arithmetic, computed on the host: the comparison is
torch.equal.  The expected value of the one call is predict_pose_from_camera on those host-resized bytes: torch.equal again, no tolerance anywhere.

Frames are random bytes in which 0 and 255 both occur, with a two-pixel border of byte 0 in some cases and 255 in others, so a clamped or wrapped
edge fails; the operator writes into a canary-filled buffer whose bytes around the outputs must stay untouched."""
import ctypes as C

import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model, timed_launches as _launches

pytestmark = pytest.mark.gpu


def _frames8(seed, B, H, W, edge):
    """stereo sensor frames uint8 [B, H, W, 3] x 2 on the host: random bytes, a 0 and a 255 inside every image, a two-pixel border of byte `edge`"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + H + W + edge)
    out = []
    for _ in range(2):
        x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        x[:, H // 2, W // 2, :] = 0
        x[:, H // 3, W // 3, :] = 255
        for sl in (slice(0, 2), slice(-2, None)):
            x[:, sl, :, :] = edge
            x[:, :, sl, :] = edge
        assert bool((x == 0).any()) and bool((x == 255).any())
        out.append(x)
    return out


# ------------------------------------------------------------------------------------------------------------ 1. the operator
def _rects(H, W):
    """(left, right) rectangle pairs: the full frame, rectangles touching each edge, one pixel wide / high"""
    return [(None, (0, 0, W, H)),
            ((0, 0, W // 2 + 1, H - 3), (W - W // 2, 3, W // 2, H - 3)),          # left / top edge | right / bottom edge
            ((W - 1, 0, 1, H), (0, H - 1, W, 1)),                                # the last column, one pixel wide | the last row, one pixel high
            ((0, 1, 1, 1), (3, 2, W - 5, H - 4))]                                # a single pixel | an interior rectangle


# (37, 53, 260): more columns than a workgroup has threads, so the tap table is built in two passes; the odd W puts rows at every byte alignment
OPERATOR = [(37, 53, 64), (96, 120, 64), (130, 258, 64), (512, 640, 256), (37, 53, 260)]


def _at_odd_addresses(lh, rh):
    """the frames on the device at an odd byte address inside a larger allocation: source rows start at any byte"""
    store = [torch.empty(t.numel() + 8, dtype=torch.uint8, device="cuda") for t in (lh, rh)]
    return store[0][1:1 + lh.numel()].view(lh.shape).copy_(lh), store[1][3:3 + rh.numel()].view(rh.shape).copy_(rh)


def _run_between_canaries(l8, r8, rect_l, rect_r, mirror_l, mirror_r, S0):
    """egotap_rgb_u8_resize into a canary-filled buffer -> (left, right) uint8 [B, S0, S0, 3] on the device; the bytes in front of, between and
    behind the outputs must stay untouched"""
    B, H, W = l8.shape[:3]
    n, pad, canary = B * S0 * S0 * 3, 1024, 0xA5
    flat = torch.full((2 * (n + pad) + pad,), canary, dtype=torch.uint8, device="cuda")
    out_l, out_r = flat[pad:pad + n], flat[2 * pad + n:2 * pad + 2 * n]
    assert out_l.data_ptr() % 4 == 0 and out_r.data_ptr() % 4 == 0
    rl = (C.c_int * 4)(*spec.check_resize_rect("t", rect_l, H, W))
    rr = (C.c_int * 4)(*spec.check_resize_rect("t", rect_r, H, W))
    L.check(L.load().egotap_rgb_u8_resize(L.ptr(l8), L.ptr(r8), B, H, W, rl, rr, mirror_l, mirror_r, S0, L.ptr(out_l), L.ptr(out_r), L.stream()))
    torch.cuda.synchronize()
    for lo, hi in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, flat.numel())):
        assert bool((flat[lo:hi] == canary).all()), (lo, hi)
    return out_l.view(B, S0, S0, 3), out_r.view(B, S0, S0, 3)


@pytest.mark.parametrize("H,W,S0", OPERATOR)
@pytest.mark.parametrize("B", [1, 3])
def test_operator_equals_the_integer_restatement_and_stays_inside_its_outputs(H, W, S0, B):
    lh, rh = _frames8(1, B, H, W, 255 if B == 1 else 0)
    l8, r8 = _at_odd_addresses(lh, rh)
    for k, (rect_l, rect_r) in enumerate(_rects(H, W)):
        for mirror_l, mirror_r in ((0, 0), (0, 1)) if k % 2 else ((1, 0), (0, 0)):
            got_l, got_r = (t.cpu() for t in _run_between_canaries(l8, r8, rect_l, rect_r, mirror_l, mirror_r, S0))
            want_l, want_r = spec.resize_u8(lh, rect_l, bool(mirror_l), S0), spec.resize_u8(rh, rect_r, bool(mirror_r), S0)
            assert torch.equal(got_l, want_l), (rect_l, mirror_l, int((got_l != want_l).sum()))
            assert torch.equal(got_r, want_r), (rect_r, mirror_r, int((got_r != want_r).sum()))
    # the Python face: aligned frames, the same bytes
    a, b = L.rgb_u8_resize(lh.cuda(), rh.cuda(), S0, rect_right=_rects(H, W)[1][1], mirror_right=True)
    assert torch.equal(a.cpu(), spec.resize_u8(lh, None, False, S0)) and torch.equal(b.cpu(), spec.resize_u8(rh, _rects(H, W)[1][1], True, S0))


def test_grid_stride_loop_takes_a_second_turn():
    H, W, S0 = 7, 9, 64
    B = 2 * torch.cuda.get_device_properties(0).multi_processor_count + 1          # the smallest batch with more thread groups than the grid holds
    assert B * S0 * (S0 // 4) > 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256 >= (B - 1) * S0 * (S0 // 4)
    lh, rh = _frames8(9, B, H, W, 255)
    l8, r8 = _at_odd_addresses(lh, rh)
    rect_l, rect_r = (1, 0, 7, 6), None
    for mirror_l, mirror_r in ((0, 1), (1, 0)):
        got_l, got_r = _run_between_canaries(l8, r8, rect_l, rect_r, mirror_l, mirror_r, S0)
        # (the restatement in torch integers on the device's copy of the same bytes: exact wherever it runs, and quick at this size)
        assert torch.equal(got_l, spec.resize_u8(lh.cuda(), rect_l, bool(mirror_l), S0))
        assert torch.equal(got_r, spec.resize_u8(rh.cuda(), rect_r, bool(mirror_r), S0))


def test_operator_copies_exactly_when_the_rectangle_has_the_output_size():
    lh, rh = _frames8(2, 2, 96, 120, 0)
    a, b = L.rgb_u8_resize(lh.cuda(), rh.cuda(), 64, rect_left=(56, 32, 64, 64), rect_right=(0, 0, 64, 64), mirror_right=True)
    assert torch.equal(a.cpu(), lh[:, 32:96, 56:120]) and torch.equal(b.cpu(), rh[:, :64, :64].flip(2))


# ------------------------------------------------------------------------------------------------------------ 2. one call
CROP, CROP_R = (8, 0, 112, 96), (0, 2, 110, 94)          # of 96 x 120 sensor frames


def _host_resized(lh, rh, S0, crop=CROP, crop_r=CROP_R, mirror_r=True):
    return spec.resize_u8(lh, crop, False, S0).cuda(), spec.resize_u8(rh, crop_r, mirror_r, S0).cuda()


def _check_one_call(m, B, chunk, edge, S0=256, seed=3):
    m.opt.hm_chunk = chunk
    lh, rh = _frames8(seed, B, 96, 120, edge)
    c8l, c8r = _host_resized(lh, rh, S0)
    want_pose, want_cat = (t.clone() for t in m.predict_pose_from_camera(c8l, c8r, return_heatmaps=True))
    want_only = m.predict_pose_from_camera(c8l, c8r).clone()
    want_form = m.rgb_form()
    l8, r8 = lh.cuda(), rh.cuda()
    pose, cat = m.predict_pose_from_sensor(l8, r8, crop=CROP, crop_right=CROP_R, mirror_right=True, return_heatmaps=True)
    torch.cuda.synchronize()
    assert torch.equal(cat, want_cat), (B, chunk, float((cat - want_cat).abs().max()))
    assert torch.equal(pose, want_pose), (B, chunk)
    only = m.predict_pose_from_sensor(l8, r8, crop=CROP, crop_right=CROP_R, mirror_right=True)
    torch.cuda.synchronize()
    assert m.rgb_form() == want_form
    assert torch.equal(only, want_only), (B, chunk)


def test_predict_pose_from_sensor_equals_the_camera_entry_on_host_resized_bytes_f32():
    m, p = _model()
    _check_one_call(m, 2, 256, 0)


def test_predict_pose_from_sensor_bf16_frozen_with_a_ragged_last_piece():
    m, p = _model()
    try:
        m.set_precision("bf16")
        assert m.freeze_weights(batch=2) == {}
        _check_one_call(m, 5, 2, 255)                                # hm_chunk = 2 at B = 5: pieces of 2, 2 and 1 frames
        assert m.rgb_form() == "handoff"                            # conv_heatmap wrote the head's operand, as for the camera entry
        assert all(n.weights_frozen for n in (m.net_HeatMap, m.net_RotHeatMap, m.net_AutoEncoder))
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")


def test_other_side_resizes_and_converts_inside_the_call():
    m, p = _model("UnrealEgo", 32)                                  # no stem reads bytes at this side: resize, then the converter
    _check_one_call(m, 2, 256, 255, S0=128, seed=4)


def test_identity_request_equals_the_camera_entry_on_the_same_tensor():
    m, p = _model()
    l8, r8 = (t.cuda() for t in _frames8(5, 2, 256, 256, 0))
    want_pose, want_cat = (t.clone() for t in m.predict_pose_from_camera(l8, r8, return_heatmaps=True))
    pose, cat = m.predict_pose_from_sensor(l8, r8, return_heatmaps=True)
    torch.cuda.synchronize()
    assert torch.equal(pose, want_pose) and torch.equal(cat, want_cat)
    # the full rectangle spelt out is the same request; with the mirror flag it is not the identity and goes through the kernel (an exact, mirrored copy)
    pose2 = m.predict_pose_from_sensor(l8, r8, crop=(0, 0, 256, 256))
    mirrored = m.predict_pose_from_sensor(l8, r8, mirror_right=True)
    want_m = m.predict_pose_from_camera(l8, r8.flip(2).contiguous())
    torch.cuda.synchronize()
    assert torch.equal(pose2, want_pose) and torch.equal(mirrored, want_m)


# ------------------------------------------------------------------------------------------------------------ 3. graphed
def test_graphed_replays_with_fresh_bytes_on_a_graph_of_its_own():
    m, p = _model()
    try:
        m._rgb_state(torch.device("cuda", torch.cuda.current_device())).graphs.clear()
        for k in range(2):                                          # the second call replays: other bytes copied into the static inputs
            lh, rh = _frames8(6 + k, 2, 96, 120, 255 * k)
            want = m.predict_pose_from_sensor(lh.cuda(), rh.cuda(), crop=CROP, crop_right=CROP_R, mirror_right=True).clone()
            c8l, c8r = _host_resized(lh, rh, 256)
            assert torch.equal(want, m.predict_pose_from_camera(c8l, c8r))
            got = m.predict_pose_from_sensor(lh.cuda(), rh.cuda(), crop=CROP, crop_right=CROP_R, mirror_right=True, graphed=True)
            torch.cuda.synchronize()
            assert torch.equal(got, want), k
        keys = list(m._rgb["graphs"])
        assert len(keys) == 1 and "sensor" in keys[0] and "u8" not in keys[0]          # one capture, keyed by the source kind
        m.predict_pose_from_camera(c8l, c8r, graphed=True)
        keys = list(m._rgb["graphs"])
        assert len(keys) == 2 and sum("sensor" in k for k in keys) == 1                 # the camera entry's graph is another one
        m.predict_pose_from_sensor(lh.cuda(), rh.cuda(), crop=CROP, crop_right=CROP_R, mirror_right=False, graphed=True)
        assert len(m._rgb["graphs"]) == 3                                               # ... and so is another mirror flag's
    finally:
        m._rgb["graphs"].clear()


# ------------------------------------------------------------------------------------------------------------ 4. the timing hook
@pytest.mark.parametrize("hm,B,chunk,pieces", [(64, 5, 2, 3), (32, 2, 256, 1)])
def test_one_resize_launch_per_piece_and_none_in_the_existing_entries(hm, B, chunk, pieces):
    m, p = _model("UnrealEgo", hm)
    m.opt.hm_chunk = chunk
    lh, rh = _frames8(8, B, 96, 120, 0)
    l8, r8 = lh.cuda(), rh.cuda()
    c8l, c8r = _host_resized(lh, rh, 4 * hm, None, None, False)
    table = m.camera_table(l8.device)
    lf = torch.stack([table[c][c8l.long()[..., c]] for c in range(3)], dim=1).contiguous()
    rf = torch.stack([table[c][c8r.long()[..., c]] for c in range(3)], dim=1).contiguous()
    m.predict_pose_from_camera(c8l, c8r)                             # (the serving handle exists from here on)
    camera = _launches(m, lambda: m.predict_pose_from_camera(c8l, c8r))
    floats = _launches(m, lambda: m.predict_pose_from_rgb(lf, rf))
    sensor = _launches(m, lambda: m.predict_pose_from_sensor(l8, r8))
    identity = _launches(m, lambda: m.predict_pose_from_sensor(c8l, c8r))
    for existing in (camera, floats, identity):
        assert existing and not [x for x in existing if "resize" in x[0] or "resize" in x[1]], existing
    assert identity == camera                                        # read in place: the camera entry's launches, no more
    new = [x for x in sensor if "resize" in x[0]]
    assert new == [("rgb_u8_resize", "rgb_u8_resize_kernel", pieces)], new
    # everything else is what the camera entry launches (at the side without byte stems the converter runs once per piece in both)
    assert sorted(x for x in sensor if x not in new) == sorted(camera)
