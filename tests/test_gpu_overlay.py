"""Heatmaps, keypoints and bones drawn onto the frames on the device: egotap_heat_u8 (heat_u8_kernel), egotap_overlay_u8 (overlay_u8_kernel) and
``Overlay.draw`` behind a serving call.

Both operators are defined in integers or single float32 roundings (spec.heat_u8, spec.overlay_taps, spec.overlay_u8), so every comparison here is
in bytes: no tolerance anywhere.  The raw entries write into views with canary bytes in front of and behind them."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
CANARY, PAD = 0xA5, 64


def _between_canaries(shape, dtype=torch.uint8):
    """(flat, view): a tensor of `shape` inside a flat buffer with PAD canary bytes on either side (PAD keeps the view 16-byte aligned)"""
    n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    flat = torch.full((n + 2 * PAD,), CANARY, dtype=torch.uint8, device="cuda")
    return flat, flat[PAD:PAD + n].view(dtype).view(shape)


def _canaries_intact(flat):
    return bool((flat[:PAD] == CANARY).all()) and bool((flat[-PAD:] == CANARY).all())


# ------------------------------------------------------------------------------------------------------------ 1. heat_u8
def _maps(B, Cn, S, bf16, seed):
    """values around the clamps with negatives, values above 1, NaNs and infinities; for bf16 every value is a bf16 value"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, Cn, S, S), generator=g) * 0.25 + 0.04
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:24]
    flat[idx[:8]], flat[idx[8:16]], flat[idx[16:20]], flat[idx[20:]] = float("nan"), 3.0, float("inf"), float("-inf")
    return x.bfloat16().float() if bf16 else x


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("n,G", [(1, 1), (15, 1), (30, 2), (64, 1)])
@pytest.mark.parametrize("S", [16, 48, 64])
def test_heat_u8_equals_the_spec_in_every_byte(S, n, G, bf16):
    for B in (1, 3):
        c0, Cn = 2, n + 3                                             # a channel slice c0 .. c0 + n - 1 of a wider tensor
        host = _maps(B, Cn + 2, S, bf16, 100 * S + n + B)
        big = host.cuda().bfloat16() if bf16 else host.cuda()
        bits = torch.int16 if bf16 else torch.int32
        before = big.view(bits).clone()
        sl = big[:, 1:1 + Cn]                                         # ... which is itself a dim-1 slice: image stride (Cn + 2) S*S
        want = spec.heat_u8(host[:, 1:1 + Cn].numpy(), c0, n, G)
        flat, out = _between_canaries((B, G, S, S))
        L.check(L.load().egotap_heat_u8(L.ptr(sl), L.BF16 if bf16 else L.F32, B, Cn, S, sl.stride(0), c0, n, G, L.ptr(out), L.stream()))
        torch.cuda.synchronize()
        assert _canaries_intact(flat)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert torch.equal(L.heat_u8(sl, c0, n, G), out)              # the Python face: the same launch
        assert torch.equal(big.view(bits), before)                    # the input is unchanged, in bits (it holds NaNs)


# ------------------------------------------------------------------------------------------------------------ 2. overlay_u8
def _palette(n, seed):
    g = np.random.default_rng(seed)
    return tuple(tuple(int(v) for v in row) for row in np.concatenate([g.integers(0, 256, (n, 3)), g.integers(40, 256, (n, 1))], axis=1))


def _canvases(B, Hc, Wc, E, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (B, Hc, Wc, 3), generator=g, dtype=torch.uint8) for _ in range(E)]


def _random_marks(B, E, M, Hc, Wc, seed):
    """marks on pixel centres, on Q4 ties (16 x = k + 0.5), at random sixteenths, partly and wholly off the canvas; what is not drawn -- NaN, inf, a low
    score, out of range -- in the first and the last lane"""
    g = np.random.default_rng(seed)
    m = np.zeros((B, E, M, 4), np.float32)
    m[..., 0] = g.integers(-3 * 16, (Wc + 3) * 16, (B, E, M)) / 16.0
    m[..., 1] = g.integers(-3 * 16, (Hc + 3) * 16, (B, E, M)) / 16.0
    m[..., 2] = g.uniform(0.5, 1.0, (B, E, M))
    m[..., 3] = g.integers(0, 4096, (B, E, M))
    kinds = np.arange(M) % 5
    m[..., 0] = np.where(kinds == 1, np.floor(m[..., 0]) + 0.5, m[..., 0])                 # on a pixel centre
    m[..., 1] = np.where(kinds == 1, np.floor(m[..., 1]) + 0.5, m[..., 1])
    m[..., 0] = np.where(kinds == 2, m[..., 0] + 1 / 32, m[..., 0])                        # rint's tie, both parities of 16 x
    m[..., 1] = np.where(kinds == 2, m[..., 1] - 1 / 32, m[..., 1])
    m[..., 0] = np.where(kinds == 3, -100.0 - m[..., 0], m[..., 0])                        # wholly off the canvas
    bad = [(np.nan, 1.0, 0.9), (np.inf, 2.0, 0.9), (3.0, 3.0, 0.25), (40000.0, 1.0, 0.9), (1.0, -32768.0, 0.9), (2.0, 2.0, np.nan)]
    for b in range(B):
        for e in range(E):
            for lane in {0, M - 1}:
                if (b + e + lane) % 2 == 0 or M == 1 and b == 0:
                    m[b, e, lane, :3] = bad[(b + 2 * e + lane) % len(bad)]
    if M == 1:
        m[-1, -1, 0, :3] = (1.5, 2.5, 0.9)                                                   # at least one frame draws its only mark
    return m


def _run(canvases, style, marks=None, heat8=None, taps=None, in_place=False):
    """the raw entry between canaries -> the outputs as numpy; checks the canaries and that every input kept its bytes"""
    E = len(canvases)
    B, Hc, Wc, _ = canvases[0].shape
    dev = [c.cuda() for c in canvases]
    bufs = [_between_canaries((B, Hc, Wc, 3)) for _ in range(E)]
    if in_place:
        for (_, view), c in zip(bufs, dev):
            view.copy_(c)
        ins = [view for _, view in bufs]
    else:
        ins = dev
    mk = None if marks is None else torch.from_numpy(marks).cuda()
    h8 = None if heat8 is None else torch.from_numpy(heat8).cuda()
    tp = [(None, None)] * 2 if taps is None else [tuple(torch.from_numpy(t).cuda() for t in pair) for pair in taps] + [(None, None)] * (2 - E)
    prm = L.overlay_style_struct(style)
    L.check(L.load().egotap_overlay_u8(L.ptr(ins[0]), L.ptr(ins[1]) if E == 2 else None, B, Hc, Wc, L.ptr(h8), 0 if heat8 is None else heat8.shape[2],
                                       L.ptr(tp[0][0]), L.ptr(tp[0][1]), L.ptr(tp[1][0]), L.ptr(tp[1][1]), L.ptr(mk), C.byref(prm), L.ptr(bufs[0][1]),
                                       L.ptr(bufs[1][1]) if E == 2 else None, L.stream()))
    torch.cuda.synchronize()
    assert all(_canaries_intact(flat) for flat, _ in bufs)
    if not in_place:
        assert all(torch.equal(d.cpu(), c) for d, c in zip(dev, canvases))
    if mk is not None:
        assert np.array_equal(mk.cpu().numpy().view(np.int32), marks.view(np.int32))
    if h8 is not None:
        assert np.array_equal(h8.cpu().numpy(), heat8) and all(np.array_equal(t.cpu().numpy(), w) for pair, want in zip(tp, taps) for t, w in zip(pair, want))
    return [view.cpu().numpy() for _, view in bufs]


def _check(canvases, style, marks=None, heat8=None, taps=None):
    want = spec.overlay_u8(canvases[0].numpy(), canvases[1].numpy() if len(canvases) == 2 else None, style, marks=marks, heat8=heat8, taps=taps)
    got = _run(canvases, style, marks, heat8, taps)
    for e, g in enumerate(got):
        assert np.array_equal(g, want[e]), (e, np.argwhere(g != want[e])[:8])
    again = _run(canvases, style, marks, heat8, taps, in_place=True)                           # in place equals out of place
    assert all(np.array_equal(a, g) for a, g in zip(again, got))
    return got


@pytest.mark.parametrize("M", [1, 17, 64])
@pytest.mark.parametrize("E", [1, 2])
@pytest.mark.parametrize("Hc,Wc", [(4, 4), (5, 8), (48, 100), (64, 64)])
def test_marks_and_bones_equal_the_spec_in_every_byte(Hc, Wc, E, M):
    B, seed = 2, 1000 * Hc + 10 * M + E
    g = np.random.default_rng(seed)
    Lb = min(64, 2 * M)
    bones = tuple((int(i), int(j)) for i, j in g.integers(0, M, (Lb, 2)))                      # (i, i) among them: bones of length zero
    style = spec.OverlayStyle(bones=bones, mark_rgba=_palette(M, seed), bone_rgba=_palette(Lb, seed + 1), r16=int(g.integers(0, 60)), w16=int(g.integers(0, 40)))
    marks = _random_marks(B, E, M, Hc, Wc, seed)
    got = _check(_canvases(B, Hc, Wc, E, seed), style, marks)
    if M > 1 and Hc >= 48:
        assert any((g != c.numpy()).any() for g, c in zip(got, _canvases(B, Hc, Wc, E, seed)))      # something was drawn


def test_bones_of_every_kind():
    """zero length, horizontal, vertical, steep, one end not drawn, both ends off the canvas and the bone crossing it -- on a 48 x 100 canvas"""
    pts = [(20.5, 10.5), (20.5, 10.5), (80.5, 10.5), (20.5, 40.5), (23.25, 45.0), (np.nan, 5.0), (-30.0, 24.0), (140.0, 30.0), (50.0, -20.0), (52.0, 70.0),
           (5.0, 5.0), (95.03125, 43.96875)]
    marks = np.zeros((1, 1, len(pts), 4), np.float32)
    marks[0, 0, :, :2] = pts
    marks[0, 0, :, 2] = 1.0
    marks[0, 0, 10, 2] = 0.1                                                                   # a low score
    bones = ((0, 0), (0, 1), (0, 2), (0, 3), (3, 4), (0, 5), (2, 10), (6, 7), (8, 9), (10, 11), (3, 11))
    for w16 in (0, 8, 24, 200):
        style = spec.OverlayStyle(bones=bones, mark_rgba=((0, 0, 0, 0),) * len(pts), bone_rgba=_palette(len(bones), w16), w16=w16)
        canvases = _canvases(1, 48, 100, 1, 5)
        got = _check(canvases, style, marks)
        base = canvases[0].numpy()
        assert (got[0][0, 26, 40] != base[0, 26, 40]).any() or w16 == 0                        # bone (6, 7) crosses the canvas from outside
        assert (got[0][0, 20:30, 50:53] != base[0, 20:30, 50:53]).any() or w16 == 0            # bone (8, 9), steep, as well


def _heat_case(B, E, S, seed):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (B, E, S, S)).astype(np.uint8)


@pytest.mark.parametrize("name,S,Hc,Wc,affines", [
    ("x4", 16, 64, 64, [(4.0, 0.0, 4.0, 0.0), (4.0, 0.0, 4.0, 0.0)]),
    ("mirrored", 16, 64, 64, [(4.0, 0.0, 4.0, 0.0), (-4.0, 64.0, 4.0, 0.0)]),
    ("partly outside", 16, 64, 64, [(3.5, 9.25, 2.75, -6.5), (-5.0, 50.0, 4.0, 30.0)]),
    ("S = Wc", 64, 64, 64, [(1.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0)]),
    ("sensor", 48, 48, 100, [tuple(float(v) for v in spec.sensor_keypoint_affine((8, 0, 88, 44), False, 48)),
                             tuple(float(v) for v in spec.sensor_keypoint_affine((0, 2, 96, 40), True, 48))]),
])
def test_heat_layer_equals_the_spec_in_every_byte(name, S, Hc, Wc, affines):
    for E in (1, 2):
        B = 2
        heat8 = _heat_case(B, E, S, 7 + E)
        taps = [(spec.overlay_taps(ax, bx, S, Wc), spec.overlay_taps(ay, by, S, Hc)) for ax, bx, ay, by in affines[:E]]
        if name == "partly outside":
            assert all((t == -1).any() and (t >= 0).any() for pair in taps for t in pair)
        style = spec.OverlayStyle(heat_rgba=(255, 64, 0, 200))
        got = _check(_canvases(B, Hc, Wc, E, 3), style, heat8=heat8, taps=taps)
        if name == "S = Wc":                                                                   # every tap weight is 0: A is the map's own byte
            c = _canvases(B, Hc, Wc, E, 3)[0].numpy().astype(np.int64)
            t = heat8[:, 0].astype(np.int64)[..., None] * 200
            assert np.array_equal(got[0], ((c * (65536 - t) + np.array([255, 64, 0]) * t + 32768) >> 16).astype(np.uint8))
        # all three layers at once, in their order
        M = 17
        full = spec.OverlayStyle(bones=tuple((j, j + 1) for j in range(M - 1)), mark_rgba=_palette(M, 1), bone_rgba=_palette(M - 1, 2), heat_rgba=(0, 255, 64, 255))
        _check(_canvases(B, Hc, Wc, E, 4), full, _random_marks(B, E, M, Hc, Wc, 11), heat8, taps)


def test_more_store_groups_than_one_pass_of_the_grid():
    """The grid STRIDES: blockIdx.x runs over min(ceil(groups / 256), max(1, 8 CUs / (B E))) workgroups of 256 threads per frame and eye, each thread
    taking store groups 256 gridDim.x apart.  B is chosen so that a 160 x 256 canvas (10240 groups of four pixels) needs more than one pass."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    E, Hc, Wc = 2, 160, 256
    B = max(1, math.ceil(8 * cus / (E * 32)))
    cap = max(1, 8 * cus // (B * E))
    assert Hc * Wc // 4 > 256 * cap, (cus, B, cap)
    marks = np.zeros((B, E, 3, 4), np.float32)
    g = np.random.default_rng(9)
    marks[..., 0], marks[..., 1], marks[..., 2] = g.uniform(0, Wc, (B, E, 3)), g.uniform(0, Hc, (B, E, 3)), 1.0
    style = spec.OverlayStyle(bones=((0, 1), (1, 2)), mark_rgba=_palette(3, 1), bone_rgba=_palette(2, 2), r16=100, w16=30)
    canvases = _canvases(B, Hc, Wc, E, 21)
    want = spec.overlay_u8(canvases[0].numpy(), canvases[1].numpy(), style, marks=marks)
    got = _run(canvases, style, marks)
    assert all(np.array_equal(g_, w) for g_, w in zip(got, want))


def test_python_face_draws_in_place_and_out_of_place():
    B, Hc, Wc, M = 2, 48, 100, 17
    style = spec.OverlayStyle(bones=((0, 1), (2, 3)), mark_rgba=_palette(M, 5), bone_rgba=_palette(2, 6))
    marks = _random_marks(B, 2, M, Hc, Wc, 77)
    canvases = _canvases(B, Hc, Wc, 2, 8)
    want = spec.overlay_u8(canvases[0].numpy(), canvases[1].numpy(), style, marks=marks)
    l8, r8 = (c.cuda() for c in canvases)
    mk = torch.from_numpy(marks).cuda()
    out_l, out_r = L.overlay_u8(l8, r8, style, marks=mk)
    assert np.array_equal(out_l.cpu().numpy(), want[0]) and np.array_equal(out_r.cpu().numpy(), want[1])
    assert torch.equal(l8.cpu(), canvases[0]) and torch.equal(r8.cpu(), canvases[1])
    one, none = L.overlay_u8(l8, None, style, marks=mk[:, :1].contiguous())
    assert none is None and np.array_equal(one.cpu().numpy(), want[0])
    L.overlay_u8(l8, r8, style, marks=mk, out=(l8, r8))
    assert np.array_equal(l8.cpu().numpy(), want[0]) and np.array_equal(r8.cpu().numpy(), want[1])


# ------------------------------------------------------------------------------------------------------------ 3. behind the serving call
def test_overlay_draw_behind_the_serving_call():
    m, p = _model()
    J, S, B = p.n_joints_hm, p.hm_size, 2
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(11)
    l8, r8 = (torch.randint(0, 256, (B, 4 * S, 4 * S, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2))
    flags = dict(return_keypoints=True, return_heatmaps=True)
    pose0, hm0, kp0 = (t.clone() for t in m.predict_pose_from_camera(l8, r8, **flags))
    ov = m.new_overlay()
    pose, hm, kp = m.predict_pose_from_camera(l8, r8, **flags)
    out_l, out_r = ov.draw(l8, r8, keypoints=kp, heatmaps=hm)
    torch.cuda.synchronize()
    assert torch.equal(pose, pose0) and torch.equal(hm, hm0) and torch.equal(kp, kp0)       # the call's bits are as without the overlay
    heat8 = spec.heat_u8(hm.cpu().numpy(), 0, 2 * J, 2)
    taps = [(spec.overlay_taps(4.0, 0.0, S, 4 * S), spec.overlay_taps(4.0, 0.0, S, 4 * S))] * 2
    want = spec.overlay_u8(l8.cpu().numpy(), r8.cpu().numpy(), ov.style_for(True, False), marks=kp.cpu().numpy(), heat8=heat8, taps=taps)
    assert np.array_equal(out_l.cpu().numpy(), want[0]) and np.array_equal(out_r.cpu().numpy(), want[1])
    assert (want[0] != l8.cpu().numpy()).any()
    # the limbs as well, and the left eye alone
    pose, hm, kp, lb = m.predict_pose_from_camera(l8, r8, return_limbs=True, **flags)
    out_l, none = ov.draw(l8, None, keypoints=kp, heatmaps=hm, limbs=lb)
    marks = ov.marks(kp, lb, eyes=1)
    assert none is None and tuple(marks.shape) == (B, 1, 3 * J, 4)
    want = spec.overlay_u8(l8.cpu().numpy(), None, ov.style_for(True, True), marks=marks.cpu().numpy(), heat8=spec.heat_u8(hm.cpu().numpy(), 0, J, 1), taps=taps[:1])
    assert np.array_equal(out_l.cpu().numpy(), want[0])
    # the timing hook shows the two launches under their names
    lib, h = L.load(), m._rgb_state(dev).handle.h
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        ov.draw(l8, r8, keypoints=kp, heatmaps=hm)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 2 and '"role": "heat_u8"' in detail and '"role": "overlay_u8"' in detail and "overlay_u8_kernel" in detail, detail
    pose1, hm1, kp1 = m.predict_pose_from_camera(l8, r8, **flags)
    assert torch.equal(pose1, pose0) and torch.equal(kp1, kp0)
