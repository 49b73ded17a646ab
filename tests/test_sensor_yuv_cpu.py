"""Host side of the NV12 / YUYV sensor entries (egotap_yuv_u8_resize, egotap_predict_pose_sensor_yuv / _kp / _kpl) and of the integer arithmetic they
compute (spec.YuvLayout, spec.YuvColour, spec.yuv_to_rgb_u8, spec.yuv_resize_u8): gated against the clipped float64 formula by the DERIVED bound
0.5 + (max |Y - y_off| + sum of max |C - 128| over the channel's chroma terms) * 2^-15, cross-checked against PIL within one byte, exported, declared
and refusing by name -- no kernel is launched here (every refusal comes before the first launch; the pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
import yuv_cases as Y_
from test_sensor_resize_cpu import _handle, _ints, _refused

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NEW = ("egotap_yuv_u8_resize", "egotap_predict_pose_sensor_yuv", "egotap_predict_pose_sensor_yuv_kp", "egotap_predict_pose_sensor_yuv_kpl")
# of a 38 x 54 frame
BAD_RECTS = [((0, 0, 0, 10), b"empty source rectangle"), ((0, 0, 10, 0), b"empty source rectangle"), ((0, 0, 10, -3), b"empty source rectangle"),
             ((-1, 0, 10, 10), b"outside the frame"), ((0, -1, 10, 10), b"outside the frame"), ((45, 0, 10, 10), b"outside the frame"),
             ((0, 29, 10, 10), b"outside the frame"), ((0, 0, 55, 38), b"outside the frame"), ((0, 0, 54, 39), b"outside the frame")]
COLOUR_IDS = [f"{c.matrix}-{c.range}" for c in Y_.COLOURS]


@pytest.fixture(scope="module")
def triples():
    """every (Y, U, V) once: the all-triples NV12 frame and, independently of the layout code, the full-resolution planes it was built from"""
    frame, layout = Y_.all_triples_nv12()
    ys, xs = torch.arange(4096).view(4096, 1), torch.arange(4096).view(1, 4096)
    k = (ys >> 1) * 2048 + (xs >> 1)
    Y = 4 * (k & 63) + 2 * (ys & 1) + (xs & 1)
    U, V = k >> 14, (k >> 6) & 255
    code = (Y << 16 | U << 8 | V).flatten()
    assert torch.equal(torch.sort(code).values, torch.arange(1 << 24))          # each triple exactly once
    return frame, layout, Y.to(torch.uint8).numpy(), U.to(torch.uint8).numpy(), V.to(torch.uint8).numpy()


# ------------------------------------------------------------------------------------------------------------ 1. the arithmetic
def test_coefficients_are_derived_and_stay_below_2_24():
    assert spec.YuvColour("bt601", "limited").coefficients() == (19077, 26149, 6419, 13320, 33050, 16)          # the issue's orientation values
    assert spec.YuvColour() == spec.YuvColour("bt601", "limited")
    for c in Y_.COLOURS:
        cy, rv, gu, gv, bu, y_off = c.coefficients()
        real = c.real_coefficients()
        assert all(abs(q / 16384.0 - r) <= 2.0 ** -15 for q, r in zip((cy, rv, gu, gv, bu), real[:5])), c
        assert y_off == (16 if c.range == "limited" else 0)
        lum = cy * max(255 - y_off, y_off)
        assert max(lum + rv * 128, lum + (gu + gv) * 128, lum + bu * 128) + (1 << 13) < 1 << 24, c
    with pytest.raises(ValueError, match="unknown matrix"):
        spec.YuvColour("bt2020", "full")
    with pytest.raises(ValueError, match="unknown range"):
        spec.YuvColour("bt709", "video")


@pytest.mark.parametrize("colour", Y_.COLOURS, ids=COLOUR_IDS)
def test_every_triple_is_within_the_derived_bound_of_the_float64_formula(triples, colour):
    frame, layout, Y, U, V = triples
    got = spec.yuv_to_rgb_u8(frame, layout, colour)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, 4096, 4096, 3)
    got = got[0].numpy()
    cy, rv, gu, gv, bu, y_off = colour.real_coefficients()
    lum_max = max(255 - y_off, y_off)                                # max |Y - y_off| over the bytes
    lum = cy * (Y.astype(np.float64) - y_off)
    u, v = U.astype(np.float64) - 128.0, V.astype(np.float64) - 128.0
    for ch, (name, real, terms) in enumerate((("R", lum + rv * v, 1), ("G", lum - gu * u - gv * v, 2), ("B", lum + bu * u, 1))):
        # each integer coefficient is within 2^-15 of the real one; the one rounding adds 0.5; clipping moves nothing apart
        bound = 0.5 + (lum_max + terms * 128) * 2.0 ** -15
        err = float(np.abs(got[..., ch].astype(np.float64) - np.clip(real, 0.0, 255.0)).max())
        print(f"{colour.matrix} {colour.range} {name}: max |byte - real| = {err:.4f} (bound {bound:.4f})")
        assert err <= bound + 1e-9, (name, err, bound)


@pytest.mark.parametrize("colour", Y_.COLOURS, ids=COLOUR_IDS)
def test_grey_axis(colour):
    y = torch.arange(256, dtype=torch.int32)
    mid = torch.full_like(y, 128)
    r, g, b = spec.yuv_rgb_bytes(y, mid, mid, colour)
    assert torch.equal(r, g) and torch.equal(g, b)
    if colour.range == "full":
        assert torch.equal(r, y)
    else:
        assert int(r[16]) == 0 and int(r[235]) == 255
        assert not r[:16].any() and bool((r[235:] == 255).all())                  # below 16 and above 235 clip
        assert int(r[17]) == 1 and int(r[234]) == 254 and bool((r[1:] >= r[:-1]).all())


def test_pil_full_range_bt601_is_within_one_byte(triples):
    Image = pytest.importorskip("PIL.Image")
    frame, layout, Y, U, V = triples
    ours = spec.yuv_to_rgb_u8(frame, layout, spec.YuvColour("bt601", "full"))[0].numpy()
    packed = np.stack([Y, U, V], axis=-1)
    theirs = np.asarray(Image.frombytes("YCbCr", (4096, 4096), packed.tobytes()).convert("RGB"))
    diff = np.abs(ours.astype(np.int16) - theirs.astype(np.int16))
    print(f"PIL YCbCr -> RGB: max difference {int(diff.max())}, bytes that differ {100.0 * float((diff != 0).mean()):.1f} %")
    assert int(diff.max()) <= 1


# ------------------------------------------------------------------------------------------------------------ 2. layouts
LAYOUTS = [spec.YuvLayout.nv12(6, 8), spec.YuvLayout.nv12(6, 8, pitch=12), spec.YuvLayout.nv12(6, 8, pitch=12, uv_offset=12 * 6 + 10),
           spec.YuvLayout.nv12(6, 8, pitch=12, uv_offset=12 * 6 + 10, frame_stride=12 * 6 + 10 + 12 * 3 + 6),
           spec.YuvLayout.nv12(2, 2, pitch=6),                          # uv_offset + W < pitch * H: the Y rows do not fill their pitch
           spec.YuvLayout.yuyv(5, 8), spec.YuvLayout.yuyv(5, 8, pitch=24), spec.YuvLayout.yuyv(5, 8, pitch=24, frame_stride=24 * 5 + 8)]


def test_tight_defaults():
    a = spec.YuvLayout.nv12(6, 8)
    assert (a.format, a.pitch, a.uv_offset, a.frame_stride, a.base_alignment) == ("nv12", 8, 48, 72, 2)
    b = spec.YuvLayout.yuyv(5, 8)
    assert (b.format, b.pitch, b.uv_offset, b.frame_stride, b.base_alignment) == ("yuyv", 16, 0, 80, 4)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.format}-{l.pitch}-{l.uv_offset}-{l.frame_stride}")
@pytest.mark.parametrize("colour", [Y_.COLOURS[0], Y_.COLOURS[3]], ids=[COLOUR_IDS[0], COLOUR_IDS[3]])
def test_hand_built_frames_and_padding(layout, colour):
    Yp, Up, Vp = Y_.planes(11, 2, layout)
    want = Y_.rgb_by_hand(Yp, Up, Vp, layout, colour)                 # chroma of (y, x) picked as (y >> 1, x >> 1) / (y, x >> 1) by index arithmetic
    a = Y_.pack(Yp, Up, Vp, layout, fill=0)
    got = spec.yuv_to_rgb_u8(a, layout, colour)
    assert torch.equal(got, want)
    pad = Y_.padding_mask(layout)
    tight = layout in (spec.YuvLayout.nv12(6, 8), spec.YuvLayout.yuyv(5, 8))
    assert bool(pad.any()) != tight
    b = Y_.pack(Yp, Up, Vp, layout, fill=0xEE)
    assert torch.equal(a[:, ~pad], b[:, ~pad]) and (tight or not torch.equal(a, b))
    assert torch.equal(spec.yuv_to_rgb_u8(b, layout, colour), want)            # no padding byte reaches an output byte
    for k in torch.nonzero(pad).flatten().tolist():                              # ... one at a time
        c = a.clone()
        c[:, k] ^= 0xFF
        assert torch.equal(spec.yuv_to_rgb_u8(c, layout, colour), want), k
    for k in torch.nonzero(~pad).flatten().tolist()[::7]:                        # ... while a plane byte does
        c = a.clone()
        c[:, k] ^= 0xFF
        assert not torch.equal(spec.yuv_to_rgb_u8(c, layout, colour), want), k
    as_np = spec.yuv_to_rgb_u8(a.numpy(), layout, colour)                        # the numpy face gives the same bytes; so does any [n, ...] shape
    assert isinstance(as_np, np.ndarray) and np.array_equal(as_np, want.numpy())
    assert torch.equal(spec.yuv_to_rgb_u8(a.view(2, layout.frame_stride // 2, 2), layout, colour), want)
    with pytest.raises(ValueError, match="frame_stride"):
        spec.yuv_to_rgb_u8(a[:, :-2], layout, colour)
    with pytest.raises(ValueError, match="uint8"):
        spec.yuv_to_rgb_u8(a.float(), layout, colour)


@pytest.mark.parametrize("layout", [spec.YuvLayout.nv12(10, 12, pitch=14), spec.YuvLayout.yuyv(9, 12, pitch=28)], ids=["nv12", "yuyv"])
def test_odd_rectangles_pick_the_chroma_of_their_block(layout):
    colour = Y_.COLOURS[0]
    Yp, Up, Vp = Y_.planes(12, 1, layout)
    a = Y_.pack(Yp, Up, Vp, layout, fill=0x5A)
    rgb = Y_.rgb_by_hand(Yp, Up, Vp, layout, colour)
    S0 = 4
    for rect in ((1, 1, 4, 4), (3, 1, 4, 4), (1, 3, 4, 4), (5, 5, 4, 4)):          # w = h = S0: an exact copy of the rectangle, odd origins
        x0, y0, w, h = rect
        got = spec.yuv_resize_u8(a, layout, colour, rect, False, S0)
        assert torch.equal(got, rgb[:, y0:y0 + h, x0:x0 + w]), rect
        assert torch.equal(spec.yuv_resize_u8(a, layout, colour, rect, True, S0), got.flip(2)), rect
    for rect in ((1, 1, 3, 5), (2, 3, 7, 3), (11, 8, 1, 1), (0, 0, 12, layout.H)):      # odd sizes, one pixel, the full frame: the composition by definition
        assert torch.equal(spec.yuv_resize_u8(a, layout, colour, rect, False, 8), spec.resize_u8(rgb, rect, False, 8)), rect
    # the single pixel (8, 11) takes the chroma of block (8 >> 1, 11 >> 1) (nv12) or pair 11 >> 1 of row 8 (yuyv): move that block's U and only then
    cy = 4 if layout.format == "nv12" else 8
    one = spec.yuv_resize_u8(a, layout, colour, (11, 8, 1, 1), False, 4)
    for (by, bx), moves in (((cy, 5), True), ((cy, 4), False), ((cy - 1, 5), False)):
        U2 = Up.clone()
        U2[:, by, bx] ^= 0x80
        other = spec.yuv_resize_u8(Y_.pack(Yp, U2, Vp, layout, fill=0x5A), layout, colour, (11, 8, 1, 1), False, 4)
        assert torch.equal(other, one) != moves, (by, bx)


BAD_NV12 = [(dict(H=5, W=8), "H and W must be even"), (dict(H=6, W=7), "H and W must be even"), (dict(H=0, W=8), "between 1 and 16384"),
            (dict(H=6, W=16386), "between 1 and 16384"), (dict(H=6, W=8, pitch=6), "pitch 6 is smaller than W"),
            (dict(H=6, W=8, pitch=10, uv_offset=56), "planes overlap"), (dict(H=6, W=8, uv_offset=46), "planes overlap"),
            (dict(H=6, W=8, frame_stride=70), "past frame_stride"), (dict(H=6, W=8, pitch=10, frame_stride=60 + 20 + 6), "past frame_stride"),
            (dict(H=6, W=8, pitch=9, uv_offset=54, frame_stride=90), "must be even"), (dict(H=6, W=8, uv_offset=49, frame_stride=74), "must be even"),
            (dict(H=6, W=8, frame_stride=73), "must be even")]
BAD_YUYV = [(dict(H=5, W=7), "W must be even"), (dict(H=0, W=8), "between 1 and 16384"), (dict(H=5, W=8, pitch=12), "smaller than 2 W"),
            (dict(H=5, W=8, frame_stride=76), "past frame_stride"), (dict(H=5, W=8, pitch=20, frame_stride=92), "past frame_stride"),
            (dict(H=5, W=8, pitch=18, frame_stride=92), "multiples of 4"), (dict(H=5, W=8, frame_stride=82), "multiples of 4")]


def test_layout_constructors_refuse_by_name():
    for kw, word in BAD_NV12:
        with pytest.raises(ValueError, match="YuvLayout.nv12: .*" + word):
            spec.YuvLayout.nv12(**kw)
    for kw, word in BAD_YUYV:
        with pytest.raises(ValueError, match="YuvLayout.yuyv: .*" + word):
            spec.YuvLayout.yuyv(**kw)
    with pytest.raises(ValueError, match="unknown format"):
        spec.YuvLayout("i420", 6, 8, 8, 48, 72)
    with pytest.raises(ValueError, match="no chroma plane"):
        spec.YuvLayout("yuyv", 5, 8, 16, 2, 80)
    assert spec.YuvLayout.nv12(16384, 16384).frame_stride == 16384 * 16384 * 3 // 2          # the largest frame is accepted


# ------------------------------------------------------------------------------------------------------------ 3. symbols
def test_new_symbols_are_declared_and_exported():
    import subprocess
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egotap.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", L._build.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(egotap_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert hasattr(lib, name) and name in L.exported_symbols() and name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert lib.egotap_abi_version() == 2               # additive: the version stays
    assert "egotap_predict_pose_sensor_yuv_workspace_bytes" not in exported          # the sensor entry's query serves: there is no new one
    assert C.sizeof(L.EgotapYuvSource) == 48 and L.EgotapYuvSource.uv_offset.offset == 32 and re.search(r"}\s*egotap_yuv_source\s*;", header)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def _desc(fmt="nv12", matrix=0, range_=0, **kw):
    """a descriptor, valid unless a field is overridden: nv12 38 x 54 (pitch 64, a padded Y plane) or yuyv 37 x 54 (pitch 112)"""
    if fmt == "nv12":
        f = dict(struct_size=C.sizeof(L.EgotapYuvSource), format=0, matrix=matrix, range=range_, H=38, W=54, pitch=64, uv_offset=64 * 38 + 32,
                 frame_stride=64 * 38 + 32 + 64 * 19 + 16)
    else:
        f = dict(struct_size=C.sizeof(L.EgotapYuvSource), format=1, matrix=matrix, range=range_, H=37, W=54, pitch=112, uv_offset=0, frame_stride=112 * 37 + 8)
    f.update(kw)
    return L.EgotapYuvSource(*(f[n] for n, _ in L.EgotapYuvSource._fields_))


BAD_DESCS = [(dict(struct_size=44), b"struct_size"), (dict(struct_size=0), b"struct_size"), (dict(format=2), b"unknown format"), (dict(format=-1), b"unknown format"),
             (dict(matrix=2), b"unknown matrix"), (dict(range_=2), b"unknown range"), (dict(range_=-1), b"unknown range"),
             (dict(H=0), b"height and width"), (dict(W=16386), b"height and width"),
             (dict(H=37), b"even H and W"), (dict(W=53), b"even H and W"), (dict(pitch=52), b"pitch is too small"),
             (dict(uv_offset=64 * 37 + 52), b"planes overlap"), (dict(frame_stride=64 * 38 + 32 + 64 * 18 + 52), b"past frame_stride"),
             (dict(pitch=63), b"even pitch"), (dict(uv_offset=64 * 38 + 33), b"even pitch"), (dict(frame_stride=64 * 38 + 32 + 64 * 19 + 17), b"even pitch"),
             (dict(fmt="yuyv", W=53), b"even W"), (dict(fmt="yuyv", pitch=104), b"pitch is too small"), (dict(fmt="yuyv", frame_stride=112 * 36 + 104), b"past frame_stride"),
             (dict(fmt="yuyv", pitch=110), b"multiples of 4"), (dict(fmt="yuyv", frame_stride=112 * 37 + 6), b"multiples of 4")]


def test_descriptors_mirror_the_layout_constructors():
    for fmt, layout in (("nv12", spec.YuvLayout.nv12(38, 54, 64, 64 * 38 + 32, 64 * 38 + 32 + 64 * 19 + 16)), ("yuyv", spec.YuvLayout.yuyv(37, 54, 112, 112 * 37 + 8))):
        a, b = _desc(fmt, 1, 1), L.yuv_source(layout, spec.YuvColour("bt709", "full"))
        assert bytes(a) == bytes(b), fmt


def test_operator_refusals():
    lib = L.load()
    f, who = lib.egotap_yuv_u8_resize, b"egotap_yuv_u8_resize"
    l8, r8, ol, orr = (C.c_void_p(a) for a in (0x200002, 0x300006, 0x500000, 0x600000))          # NV12 frames may sit at any even address
    full = _ints(0, 0, 54, 38)
    d = C.byref(_desc())
    _refused(lib, f, who, l8, r8, 0, d, full, full, 0, 0, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, None, r8, 2, d, full, full, 0, 0, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, None, 2, d, full, full, 0, 0, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, r8, 2, None, full, full, 0, 0, 64, ol, orr, None, word=b"null source descriptor")
    _refused(lib, f, who, l8, r8, 2, d, None, full, 0, 0, 64, ol, orr, None, word=b"null rectangle")
    _refused(lib, f, who, l8, r8, 2, d, full, None, 0, 0, 64, ol, orr, None, word=b"null rectangle")
    _refused(lib, f, who, l8, r8, 2, d, full, full, 0, 0, 64, None, orr, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 2, d, full, full, 0, 0, 64, ol, C.c_void_p(0x600002), None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, r8, 2, d, full, full, 0, 0, 62, ol, orr, None, word=b"multiple of 4")
    _refused(lib, f, who, l8, r8, 2, d, full, full, 0, 0, 4100, ol, orr, None, word=b"multiple of 4")
    _refused(lib, f, who, C.c_void_p(0x200001), r8, 2, d, full, full, 0, 0, 64, ol, orr, None, word=b"2-byte aligned")
    _refused(lib, f, who, l8, C.c_void_p(0x300003), 2, d, full, full, 0, 0, 64, ol, orr, None, word=b"2-byte aligned")
    dy = C.byref(_desc("yuyv"))
    fully = _ints(0, 0, 54, 37)
    _refused(lib, f, who, l8, C.c_void_p(0x300004), 2, dy, fully, fully, 0, 0, 64, ol, orr, None, word=b"4-byte aligned (YUYV")
    _refused(lib, f, who, C.c_void_p(0x200004), r8, 2, dy, fully, fully, 0, 0, 64, ol, orr, None, word=b"4-byte aligned (YUYV")
    for kw, word in BAD_DESCS:
        rect = fully if kw.get("fmt") == "yuyv" else full
        _refused(lib, f, who, l8, r8, 2, C.byref(_desc(**kw)), rect, rect, 0, 0, 64, ol, orr, None, word=word)
    for rect, word in BAD_RECTS:
        _refused(lib, f, who, l8, r8, 2, d, _ints(*rect), full, 0, 0, 64, ol, orr, None, word=word)
        _refused(lib, f, who, l8, r8, 2, d, full, _ints(*rect), 1, 1, 64, ol, orr, None, word=word)


@pytest.mark.parametrize("suffix", ["", "_kp", "_kpl"])
@pytest.mark.parametrize("hm", [64, 32])
def test_one_call_refusals(hm, suffix):
    lib, h = _handle(hm=hm)
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 38, 54, 0, C.byref(need)) == 0          # the sensor entry's query IS the size
        name = "egotap_predict_pose_sensor_yuv" + suffix
        fn, who = getattr(lib, name), name.encode()
        kp, lb = C.c_void_p(0x4000000), C.c_void_p(0x5000000)          # (clear of the fake heatmaps)
        extra = {"": (), "_kp": (kp,), "_kpl": (kp, lb)}[suffix]

        def f(*a):
            return fn(*a, *extra)
        l8, r8, tab, pose, hmp, ws = (C.c_void_p(a) for a in (0x200002, 0x300002, 0x400000, 0x500000, 0x600000, 0x700000))
        rects, mir, d = _ints(0, 0, 54, 38, 3, 5, 11, 9), _ints(0, 1), C.byref(_desc())
        ok = (4, d, rects, mir, tab, pose, hmp, 0, ws, need.value, None)
        _refused(lib, f, who, None, l8, r8, *ok, word=b"null handle")
        _refused(lib, f, who, h, None, r8, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, None, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, r8, 4, None, rects, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"null source descriptor")
        _refused(lib, f, who, h, l8, r8, 4, d, None, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"null rectangles")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, None, tab, pose, hmp, 0, ws, need.value, None, word=b"mirror flags")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, None, pose, hmp, 0, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, None, hmp, 0, ws, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, hmp, 0, None, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 0, d, rects, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, hmp, -1, ws, need.value, None, word=b"chunk")
        for kw, word in BAD_DESCS:
            r = _ints(0, 0, 54, 37, 0, 0, 54, 37) if kw.get("fmt") == "yuyv" else rects
            _refused(lib, f, who, h, l8, r8, 4, C.byref(_desc(**kw)), r, mir, tab, pose, hmp, 0, ws, need.value, None, word=word)
        for rect, word in BAD_RECTS:
            _refused(lib, f, who, h, l8, r8, 4, d, _ints(*rect, 0, 0, 54, 38), mir, tab, pose, hmp, 0, ws, need.value, None, word=word)
            _refused(lib, f, who, h, l8, r8, 4, d, _ints(0, 0, 54, 38, *rect), mir, tab, pose, hmp, 0, ws, need.value, None, word=word)
        _refused(lib, f, who, h, C.c_void_p(0x200001), r8, *ok, word=b"2-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, C.byref(_desc("yuyv")), _ints(0, 0, 54, 37, 0, 0, 54, 37), mir, tab, pose, hmp, 0, ws, need.value, None,
                 word=b"4-byte aligned (YUYV")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, C.c_void_p(0x400004), pose, hmp, 0, ws, need.value, None, word=b"16-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, C.c_void_p(0x600008), 0, ws, need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, hmp, 0, C.c_void_p(0x700010), need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, hmp, 0, ws, need.value - 1, None, word=b"workspace too small")
        u8 = C.c_size_t()          # the byte entry's size is short by the slice: a YUV source always converts into it
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, 0, C.byref(u8)) == 0
        _refused(lib, f, who, h, l8, r8, 4, d, rects, mir, tab, pose, hmp, 0, ws, u8.value, None, word=b"workspace too small")
        if suffix == "_kp":
            assert fn(h, l8, r8, *ok, None) == INVALID and b"null keypoints" in lib.egotap_last_error()
            assert fn(h, l8, r8, *ok, C.c_void_p(0x4000008)) == INVALID and b"16-byte aligned" in lib.egotap_last_error()
        if suffix == "_kpl":
            assert fn(h, l8, r8, *ok, kp, C.c_void_p(0x5000008)) == INVALID and b"limbs must be 16-byte aligned" in lib.egotap_last_error()
            assert fn(h, l8, r8, *ok, kp, kp) == INVALID and b"overlaps" in lib.egotap_last_error()
        form = C.c_int(-1)
        assert lib.egotap_debug_predict_pose_rgb_form(h, C.byref(form)) == 0 and form.value == 0          # nothing ran
    finally:
        lib.egotap_destroy(h)


def test_unbound_network_is_refused_by_key():
    lib, h = _handle(bind=(L.NET_LIFT, L.NET_HM_POS))
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 2, 38, 54, 0, C.byref(need)) == 0
        l8, r8, tab, pose, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x700000))
        rc = lib.egotap_predict_pose_sensor_yuv(h, l8, r8, 2, C.byref(_desc()), _ints(0, 0, 54, 38, 0, 0, 54, 38), _ints(0, 0), tab, pose, None, 0, ws, need.value, None)
        msg = lib.egotap_last_error()
        assert rc == INVALID and b"egotap_predict_pose_sensor_yuv" in msg and b"unbound parameter" in msg and b"limb estimator" in msg, msg
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 5. the Python faces
def test_check_yuv_frames_wording():
    from egotap_amd import models
    from egotap_amd.options import preset_defaults
    layout = spec.YuvLayout.nv12(38, 54, pitch=64)
    fs = layout.frame_stride
    cpu8 = torch.zeros(2, fs, dtype=torch.uint8)
    m = types.SimpleNamespace(opt=preset_defaults("UnrealEgo", 64), net_AutoEncoder=types.SimpleNamespace(preset=spec.lift_preset("UnrealEgo", 64)))
    m.predict_pose_from_sensor_yuv = types.MethodType(models.EgoTAPAutoEncoderModel.predict_pose_from_sensor_yuv, m)
    with pytest.raises(L.EgotapError, match="predict_pose_from_sensor_yuv runs on the GPU only"):
        m.predict_pose_from_sensor_yuv(cpu8, cpu8, layout)
    with pytest.raises(ValueError, match="layout is a spec.YuvLayout"):
        m.predict_pose_from_sensor_yuv(cpu8, cpu8, (38, 54))
    with pytest.raises(L.EgotapError, match="yuv_u8_resize runs on the GPU only"):
        L.yuv_u8_resize(cpu8, cpu8, layout, Y_.COLOURS[0], 64)

    class OnGpu(torch.Tensor):          # dtype and shape are looked at once the frames are on a GPU: a stand-in for "is on the GPU"
        is_cuda = True
    g = lambda t: t.as_subclass(OnGpu)      # noqa: E731
    who = "predict_pose_from_sensor_yuv"
    assert L.check_yuv_frames(who, g(cpu8), g(cpu8), layout) == 2
    assert L.check_yuv_frames(who, g(cpu8.view(2, fs // 2, 2)), g(cpu8.view(2, fs // 2, 2)), layout) == 2
    assert L.check_yuv_frames(who, g(cpu8[:0]), g(cpu8[:0]), layout) == 0
    with pytest.raises(L.EgotapError, match="dtype uint8"):
        L.check_yuv_frames(who, g(cpu8.float()), g(cpu8.float()), layout)
    with pytest.raises(ValueError, match=f"frame_stride = {fs} bytes each"):
        L.check_yuv_frames(who, g(cpu8[:, :-2]), g(cpu8[:, :-2]), layout)
    with pytest.raises(ValueError, match="of one shape"):
        L.check_yuv_frames(who, g(cpu8), g(cpu8[:1]), layout)
    with pytest.raises(L.EgotapError, match="contiguous"):
        nc = torch.zeros(fs, 2, dtype=torch.uint8).t()
        L.check_yuv_frames(who, g(nc), g(nc), layout)
    big = torch.zeros(2 * fs + 8, dtype=torch.uint8)
    odd = big[big.data_ptr() % 2 + 1:][:2 * fs].view(2, fs)          # an odd address
    with pytest.raises(L.EgotapError, match="multiple of 2 bytes"):
        L.check_yuv_frames(who, g(odd), g(odd), layout)
    # the sensor entry keeps its signature
    import inspect
    assert list(inspect.signature(models.EgoTAPAutoEncoderModel.predict_pose_from_sensor).parameters)[:6] == ["self", "left8", "right8", "crop", "crop_right", "mirror_right"]
