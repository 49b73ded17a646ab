"""Heatmaps, keypoints and bones drawn onto the frames, on the host: the restatements spec.heat_u8 / spec.overlay_taps / spec.overlay_u8 held against
the reference's own picture of a heatmap stack (tests/golden/visuals_heat.npz, tools/make_golden.py --only visuals) and against closed forms that do
not use the restatement, then every refusal of the two entries with fake pointers (nothing launches) and the Python faces.  No GPU."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from egotap_amd import lib as L
from egotap_amd import spec

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visuals_heat.npz")
GREY = 100


def _canvas(Hc, Wc, value=GREY):
    return np.full((1, Hc, Wc, 3), value, np.uint8)


def _mark_style(r16, rgba=(255, 255, 255, 255), **kw):
    return spec.OverlayStyle(mark_rgba=(rgba,), r16=r16, **kw)


def _marks(*pts, score=1.0):
    m = np.zeros((1, 1, len(pts), 4), np.float32)
    m[0, 0, :, :2], m[0, 0, :, 2] = pts, score
    return m


def _coverage(out, base=GREY, colour=255, alpha=255):
    """coverage of every pixel of a one-layer picture on a flat canvas, by inverting the blend for each of its seventeen possible values (0, 16 .. 256):
    a closed form of the layer rule, not the restatement's code path"""
    table = {}
    for cov in range(0, 257, 16):
        t = cov * alpha
        table[(base * (65536 - t) + colour * t + 32768) >> 16] = cov
    assert len(table) == 17
    return np.vectorize(table.__getitem__)(out[0, :, :, 0].astype(np.int64))


# ------------------------------------------------------------------------------------------------ heat_u8
def test_heat_u8_equals_the_reference_picture_in_every_pixel():
    z = np.load(GOLD)
    x = z["hm_q"].astype(np.float32) / np.float32(1024)
    got = spec.heat_u8(x, 0, 15, 1)
    assert got.shape == (2, 1, 32, 32) and got.dtype == np.uint8
    assert np.array_equal(got[:, 0], z["out"][..., 0])                                          # every pixel: the dyadic inputs have one sum in any order
    assert (z["out"] == 0).sum() > 100 and (z["out"] == 255).sum() > 100 and ((z["out"] > 0) & (z["out"] < 255)).sum() > 100
    # two groups are the two halves' own pictures; a slice is the slice's picture
    two = spec.heat_u8(x[:, :14], 0, 14, 2)
    assert np.array_equal(two[:, 0], spec.heat_u8(x[:, :7], 0, 7, 1)[:, 0]) and np.array_equal(two[:, 1], spec.heat_u8(x, 7, 7, 1)[:, 0])


def test_heat_u8_value_rules():
    inf, nan = np.inf, np.nan
    col = np.array([0.0, -0.0, -1.0, 0.5, 1.0, 1.5, 254.9 / 255, 1 / 255, 0.999 / 255, nan, inf, -inf, 2.0 ** -130, 100.0, 0.25, 0.75], np.float32)
    x = np.zeros((1, 2, 16, 16), np.float32)
    x[0, 0, 0], x[0, 0, 1], x[0, 1, 1] = col, col, 0.25
    x[0, 0, 2], x[0, 1, 2] = inf, -inf                                                          # inf - inf = NaN
    out = spec.heat_u8(x, 0, 2, 1)[0, 0]
    assert out[0].tolist() == [0, 0, 0, 127, 255, 255, 254, 1, 0, 0, 255, 0, 0, 255, 63, 191]  # truncation, not rounding
    assert out[1].tolist() == [63, 63, 0, 191, 255, 255, 255, 64, 64, 0, 255, 0, 63, 255, 127, 255]
    assert (out[2] == 0).all()
    with pytest.raises(ValueError, match="heat_u8"):
        spec.heat_u8(x, 0, 2, 3)
    with pytest.raises(ValueError, match="heat_u8"):
        spec.heat_u8(x, 1, 2, 1)


# ------------------------------------------------------------------------------------------------ overlay_taps
def test_overlay_taps_identity_x4_mirror_and_partial_extent():
    assert spec.overlay_taps(1.0, 0.0, 16, 16).tolist() == list(range(16))                     # the identity: tap X, weight 0
    for S, k in ((16, 4), (64, 4), (48, 2)):
        i0, i1, w1 = spec.resize_taps(S, k * S)
        t = spec.overlay_taps(float(k), 0.0, S, k * S)
        assert t.dtype == np.int32 and np.array_equal(t, i0 | (w1 << 16))
        m = spec.overlay_taps(-float(k), float(k * S), S, k * S)                               # a mirror: column X takes the taps of column L - 1 - X
        assert np.array_equal(m, t[::-1])
    part = spec.overlay_taps(4.0, 8.0, 16, 64)                                                 # the map covers canvas 8 .. 72: columns 0 .. 7 lie outside
    assert (part[:8] == -1).all() and (part[8:] >= 0).all() and np.array_equal(part[8:], spec.overlay_taps(4.0, 0.0, 16, 64)[:56])
    right = spec.overlay_taps(2.0, 0.0, 16, 64)                                                # ... and 0 .. 32: columns 32 .. 63 outside
    assert (right[:32] >= 0).all() and (right[32:] == -1).all()
    assert (spec.overlay_taps(1.0, 1000.0, 16, 64) == -1).all()
    for bad in ((0.0, 0.0), (math.nan, 0.0), (1.0, math.inf)):
        with pytest.raises(ValueError, match="overlay_taps"):
            spec.overlay_taps(*bad, 16, 64)


# ------------------------------------------------------------------------------------------------ closed forms of the marks and the bones
def test_alpha_zero_leaves_the_canvas_in_bits():
    g = np.random.default_rng(1)
    c = g.integers(0, 256, (2, 24, 32, 3)).astype(np.uint8)
    style = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((255, 0, 0, 0), (0, 255, 0, 0)), bone_rgba=((0, 0, 255, 0),), heat_rgba=(255, 255, 255, 0))
    marks = np.tile(_marks((8.0, 8.0), (20.0, 15.0)), (2, 2, 1, 1))
    heat8 = g.integers(0, 256, (2, 2, 8, 8)).astype(np.uint8)
    taps = [(spec.overlay_taps(4.0, 0.0, 8, 32), spec.overlay_taps(3.0, 0.0, 8, 24))] * 2
    out_l, out_r = spec.overlay_u8(c, c[::-1].copy(), style, marks=marks, heat8=heat8, taps=taps)
    assert np.array_equal(out_l, c) and np.array_equal(out_r, c[::-1])


@pytest.mark.parametrize("r16", [0, 8, 40, 100, 163])
def test_a_disc_on_a_pixel_centre_is_symmetric_and_has_the_area_of_a_circle(r16):
    n = 41
    out, none = spec.overlay_u8(_canvas(n, n), None, _mark_style(r16), marks=_marks((20.5, 20.5)))
    assert none is None
    cov = _coverage(out)
    for sym in (cov[::-1], cov[:, ::-1], cov.T, cov[::-1, ::-1], cov.T[::-1], cov.T[:, ::-1], cov.T[::-1, ::-1]):      # with the identity: the eight reflections
        assert np.array_equal(sym, cov)
    assert cov[20, 20] == min(r16 + 8, 16) * 16 and cov[0, 0] == 0
    # coverage falls from 1 to 0 over one pixel centred on the circle of radius r: the area is that of the circle to within the pixels the edge
    # passes through (at most one per unit of perimeter and its neighbour)
    r = r16 / 16.0
    perimeter_pixels = int(((cov > 0) & (cov < 256)).sum()) + 1
    assert abs(cov.sum() / 256.0 - math.pi * r * r) <= perimeter_pixels, (cov.sum() / 256.0, math.pi * r * r, perimeter_pixels)
    if r16 >= 40:
        assert abs(cov.sum() / 256.0 - math.pi * r * r) <= 0.02 * math.pi * r * r + 1.0


def test_mark_coverage_along_a_row_is_the_ramp():
    """a mark on a pixel centre, r16 = 40: pixel k columns away has d = 16 k, coverage clamp(48 - 16 k, 0, 16) * 16"""
    out, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(40), marks=_marks((4.5, 4.5)))
    assert _coverage(out)[4].tolist() == [0, 0, 256, 256, 256, 256, 256, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    out, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(44), marks=_marks((4.5, 4.5)))
    assert _coverage(out)[4, 4:9].tolist() == [256, 256, 256, 64, 0] and _coverage(out)[4, 0:5].tolist() == [0, 64, 256, 256, 256]
    # a Q4 tie: 16 x = 72.5 rounds to the even 72, 16 x = 73.5 to 74
    a, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(40), marks=_marks((72.5 / 16, 4.5)))
    b, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(40), marks=_marks((72.0 / 16, 4.5)))
    c, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(40), marks=_marks((73.5 / 16, 4.5)))
    d, _ = spec.overlay_u8(_canvas(9, 16), None, _mark_style(40), marks=_marks((74.0 / 16, 4.5)))
    assert np.array_equal(a, b) and np.array_equal(c, d) and not np.array_equal(a, c)


def test_what_is_not_eligible_is_not_drawn():
    base = _canvas(16, 16)
    for pt, score in (((np.nan, 4.0), 1.0), ((4.0, np.inf), 1.0), ((4.0, 4.0), 0.49), ((4.0, 4.0), np.nan), ((32768.0, 4.0), 1.0), ((4.0, -32768.0), 1.0)):
        out, _ = spec.overlay_u8(base, None, _mark_style(40), marks=_marks(pt, score=score))
        assert np.array_equal(out, base), (pt, score)
    out, _ = spec.overlay_u8(base, None, _mark_style(40), marks=_marks((4.0, 4.0), score=0.5))
    assert not np.array_equal(out, base)
    assert spec.overlay_eligible(_marks((32767.9, -32767.9)), 0.5).all()
    # a bone with one end not drawn is not drawn
    style = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((0, 0, 0, 0),) * 2, bone_rgba=((255, 255, 255, 255),), w16=16)
    m = _marks((2.0, 8.0), (14.0, 8.0))
    assert not np.array_equal(spec.overlay_u8(base, None, style, marks=m)[0], base)
    m[0, 0, 1, 2] = 0.1
    assert np.array_equal(spec.overlay_u8(base, None, style, marks=m)[0], base)


@pytest.mark.parametrize("w16", [0, 8, 16, 40])
def test_a_horizontal_bone_covers_rows_symmetrically(w16):
    style = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((0, 0, 0, 0),) * 2, bone_rgba=((255, 255, 255, 255),), w16=w16)
    out, _ = spec.overlay_u8(_canvas(21, 40), None, style, marks=_marks((8.5, 10.5), (31.5, 10.5)))
    cov = _coverage(out)
    assert np.array_equal(cov, cov[::-1]) and np.array_equal(cov, cov[:, ::-1])               # about the bone's row and about its middle column
    inner = cov[:, 9:31]                                                                       # between the ends: d = 16 |row - 10| exactly
    want = [min(max(w16 + 8 - 16 * abs(y - 10), 0), 16) * 16 for y in range(21)]
    assert all(inner[y].tolist() == [want[y]] * 22 for y in range(21))


def test_a_vertical_bone_is_the_horizontal_one_transposed():
    style = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((0, 0, 0, 0),) * 2, bone_rgba=((255, 255, 255, 255),), w16=24)
    h, _ = spec.overlay_u8(_canvas(24, 24), None, style, marks=_marks((4.25, 10.5), (19.0, 10.5)))
    v, _ = spec.overlay_u8(_canvas(24, 24), None, style, marks=_marks((10.5, 4.25), (10.5, 19.0)))
    assert np.array_equal(_coverage(h), _coverage(v).T)


@pytest.mark.parametrize("w16", [0, 24, 100])
def test_a_bone_of_length_zero_is_the_disc_of_its_half_width(w16):
    pt = (12.3125, 9.75)
    bone = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((0, 0, 0, 0),) * 2, bone_rgba=((9, 200, 77, 255),), w16=w16, r16=3)
    disc = spec.OverlayStyle(mark_rgba=((9, 200, 77, 255),), r16=w16, w16=5)
    g = np.random.default_rng(3)
    c = g.integers(0, 256, (1, 24, 28, 3)).astype(np.uint8)
    assert np.array_equal(spec.overlay_u8(c, None, bone, marks=_marks(pt, pt))[0], spec.overlay_u8(c, None, disc, marks=_marks(pt))[0])
    same = spec.OverlayStyle(bones=((0, 0),), mark_rgba=((0, 0, 0, 0),), bone_rgba=((9, 200, 77, 255),), w16=w16)
    assert np.array_equal(spec.overlay_u8(c, None, same, marks=_marks(pt))[0], spec.overlay_u8(c, None, disc, marks=_marks(pt))[0])


def test_isqrt_is_the_floor_for_every_size_the_kernel_meets():
    g = np.random.default_rng(5)
    r = np.concatenate([np.arange(0, 3000), g.integers(0, 1 << 21, 20000)]).astype(np.int64)
    for n in (r * r, r * r + 1, r * r - 1 + (r == 0), r * r + 2 * r):
        got = spec.overlay_isqrt(n)
        assert (got * got <= n).all() and ((got + 1) * (got + 1) > n).all()
    assert [int(spec.overlay_isqrt(n)) for n in (0, 1, 2, 3, 4, (1 << 42) - 1)] == [0, 1, 1, 1, 2, (1 << 21) - 1]


def test_the_layers_lie_in_their_order():
    """full alpha everywhere: where a mark, a bone and the heat overlap the mark shows, where only bone and heat do the bone shows"""
    heat8 = np.full((1, 1, 16, 16), 255, np.uint8)
    taps = [(spec.overlay_taps(1.0, 0.0, 16, 16), spec.overlay_taps(1.0, 0.0, 16, 16))]
    style = spec.OverlayStyle(bones=((0, 1),), mark_rgba=((255, 0, 0, 255), (255, 0, 0, 255)), bone_rgba=((0, 255, 0, 255),), r16=24, w16=24, heat_rgba=(0, 0, 255, 255))
    out, _ = spec.overlay_u8(_canvas(16, 16, 0), None, style, marks=_marks((3.5, 8.5), (12.5, 8.5)), heat8=heat8, taps=taps)
    px = out[0]
    assert px[8, 3].tolist() == [254, 1, 0]                      # the mark: t = 256 * 255, so 255 / 256 of its colour and 1 / 256 of the bone's 254 below
    assert px[8, 8].tolist() == [0, 254, 1]                      # the bone between the marks, over the heat's 253
    assert px[1, 1].tolist() == [0, 0, 253]                      # the heat alone: A = 255, t = 255 * 255
    # a second bone of a higher index lies over the first
    two = spec.OverlayStyle(bones=((0, 1), (2, 3)), mark_rgba=((0, 0, 0, 0),) * 4, bone_rgba=((0, 255, 0, 255), (255, 255, 0, 255)), w16=24)
    out, _ = spec.overlay_u8(_canvas(16, 16, 0), None, two, marks=_marks((2.5, 8.5), (13.5, 8.5), (8.5, 2.5), (8.5, 13.5)))
    assert out[0, 8, 8].tolist() == [254, 255, 0] and out[0, 8, 4].tolist() == [0, 254, 0] and out[0, 4, 8].tolist() == [254, 254, 0]


def test_heat_layer_identity_taps_blend_the_maps_own_byte():
    g = np.random.default_rng(8)
    heat8 = g.integers(0, 256, (1, 1, 16, 16)).astype(np.uint8)
    taps = [(spec.overlay_taps(1.0, 0.0, 16, 16), spec.overlay_taps(1.0, 0.0, 16, 16))]
    out, _ = spec.overlay_u8(_canvas(16, 16, 10), None, spec.OverlayStyle(heat_rgba=(210, 210, 210, 255)), heat8=heat8, taps=taps)
    t = heat8[0, 0].astype(np.int64) * 255
    assert np.array_equal(out[0, :, :, 1], ((10 * (65536 - t) + 210 * t + 32768) >> 16).astype(np.uint8))
    # x 2 on a constant map is that constant; outside the extent the canvas is left alone
    flat = np.full((1, 1, 16, 16), 77, np.uint8)
    taps = [(spec.overlay_taps(2.0, 4.0, 16, 40), spec.overlay_taps(2.0, 0.0, 16, 32))]
    out, _ = spec.overlay_u8(_canvas(32, 40, 10), None, spec.OverlayStyle(heat_rgba=(210, 210, 210, 255)), heat8=flat, taps=taps)
    inside = (10 * (65536 - 77 * 255) + 210 * 77 * 255 + 32768) >> 16
    assert (out[0, :, 4:36] == inside).all() and (out[0, :, :4] == 10).all() and (out[0, :, 36:] == 10).all()


# ------------------------------------------------------------------------------------------------ styles
def test_overlay_style_of_the_presets():
    for preset, J in (("UnrealEgo", 15), ("EgoCap", 17)):
        s = spec.overlay_style(preset)
        par, row0 = spec.skeleton_parents(preset), spec.stereo_pose_row0(spec.lift_preset(preset))
        assert len(s.mark_rgba) == J and len(s.bones) == len(s.bone_rgba) == sum(1 for r in range(row0, row0 + J) if par[r] >= row0)
        assert all(par[j + row0] - row0 == i for i, j in s.bones) and s.min_score == spec.STEREO_MIN_SCORE
        mir = spec.SKELETON_MIRROR[preset]
        for j, c in enumerate(s.mark_rgba):
            r = j + row0
            assert c == (spec.OVERLAY_CENTRE_RGBA if mir[r] < 0 else spec.OVERLAY_LEFT_RGBA if r < mir[r] else spec.OVERLAY_RIGHT_RGBA)
        assert {spec.OVERLAY_LEFT_RGBA, spec.OVERLAY_RIGHT_RGBA, spec.OVERLAY_CENTRE_RGBA} == set(s.mark_rgba)
    with pytest.raises(ValueError):
        spec.overlay_style("Nobody")
    for kw in (dict(bones=((0, 1),), mark_rgba=((1, 2, 3, 4),), bone_rgba=((1, 2, 3, 4),)), dict(mark_rgba=((1, 2, 3),)), dict(mark_rgba=((1, 2, 3, 256),)),
               dict(bones=((0, 0),), mark_rgba=((1, 2, 3, 4),)), dict(r16=-1), dict(w16=16385), dict(min_score=math.nan), dict(mark_rgba=((0, 0, 0, 0),) * 65)):
        with pytest.raises(ValueError, match="OverlayStyle"):
            spec.OverlayStyle(**kw)


# ------------------------------------------------------------------------------------------------ the ABI and the Python faces
def test_the_entries_are_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    for name in ("egotap_heat_u8", "egotap_overlay_u8"):
        assert name in L.exported_symbols() and hasattr(lib, name) and f"int {name}(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert C.sizeof(L.EgotapOverlayStyle) == 664
    o = L.overlay_style_struct(spec.overlay_style("UnrealEgo"))
    assert (o.n_marks, o.n_bones, o.r16, o.w16, o.min_score) == (15, 14, 40, 16, 0.5) and tuple(o.heat_rgba) == (255, 255, 255, 160)
    assert tuple(o.bones[0]) == spec.overlay_style("UnrealEgo").bones[0] and tuple(o.mark_rgba[14]) == spec.overlay_style("UnrealEgo").mark_rgba[14]
    for name in ("heat_u8", "overlay_u8", "overlay_tap_tables", "overlay_style_struct"):
        assert callable(getattr(L, name))
    for name in ("heat_u8", "overlay_taps", "overlay_u8", "overlay_style", "OverlayStyle", "overlay_isqrt", "overlay_blend", "overlay_eligible"):
        assert hasattr(spec, name)


def test_heat_u8_refuses_by_name_before_any_launch():
    lib, P = L.load(), C.c_void_p
    hm, out = 0x100000, 0x900000
    ok = dict(hm=P(hm), dtype=L.F32, B=2, C=30, S=64, stride=30 * 4096, c0=0, n=30, G=2, out=P(out))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_heat_u8(a["hm"], a["dtype"], a["B"], a["C"], a["S"], a["stride"], a["c0"], a["n"], a["G"], a["out"], None)
        return rc, lib.egotap_last_error().decode()
    in_bytes = (30 * 4096 + 30 * 4096) * 4
    cases = [(dict(hm=None), "null"), (dict(out=None), "null"), (dict(dtype=L.I64), "unknown dtype"), (dict(B=0), "batch"), (dict(n=0), "at least 1"),
             (dict(n=-2), "at least 1"), (dict(G=4), "multiple of groups"), (dict(G=0), "multiple of groups"), (dict(c0=-1), "not inside"),
             (dict(c0=1), "not inside"), (dict(n=32, G=2), "not inside"), (dict(S=0), "multiple of 16"), (dict(S=40), "multiple of 16"),
             (dict(S=-16), "multiple of 16"), (dict(S=4112), "multiple of 16"), (dict(stride=30 * 4096 - 4), "image_stride"),
             (dict(stride=30 * 4096 + 2), "multiple of 16 bytes"), (dict(dtype=L.BF16, stride=30 * 4096 + 4), "multiple of 16 bytes"),
             (dict(hm=P(hm + 8)), "16-byte aligned"), (dict(out=P(out + 4)), "8-byte aligned"),
             (dict(out=P(hm)), "heat8 overlaps hm"), (dict(out=P(hm + in_bytes - 8)), "heat8 overlaps hm"), (dict(out=P(hm - 8)), "heat8 overlaps hm")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_heat_u8:") and word in msg, (kw, rc, msg)


def test_overlay_u8_refuses_by_name_before_any_launch():
    lib, P = L.load(), C.c_void_p
    B, Hc, Wc, S, M = 2, 48, 100, 16, 17
    canvas = B * Hc * Wc * 3
    l8, r8, ol, orr, h8, txl, tyl, txr, tyr, mk = (0x1000000 * (k + 1) for k in range(10))

    def sty(**kw):
        o = L.overlay_style_struct(spec.OverlayStyle(bones=((0, 1), (1, 16)), mark_rgba=((1, 2, 3, 4),) * M, bone_rgba=((5, 6, 7, 8),) * 2))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def bad_bone():
        o = sty()
        o.bones[1][1] = 17
        return o
    ok = dict(l8=P(l8), r8=P(r8), B=B, Hc=Hc, Wc=Wc, h8=P(h8), S=S, txl=P(txl), tyl=P(tyl), txr=P(txr), tyr=P(tyr), mk=P(mk), st=sty(), ol=P(ol), orr=P(orr))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_overlay_u8(a["l8"], a["r8"], a["B"], a["Hc"], a["Wc"], a["h8"], a["S"], a["txl"], a["tyl"], a["txr"], a["tyr"], a["mk"],
                                   C.byref(a["st"]) if a["st"] is not None else None, a["ol"], a["orr"], None)
        return rc, lib.egotap_last_error().decode()
    nan = float("nan")
    cases = [(dict(l8=None), "null"), (dict(ol=None), "null"), (dict(st=None), "null"), (dict(r8=None), "both given or both NULL"),
             (dict(orr=None), "both given or both NULL"), (dict(B=0), "batch"), (dict(B=65536), "batch"), (dict(Hc=0), "canvas"), (dict(Wc=0), "canvas"),
             (dict(Wc=102), "canvas"), (dict(Wc=16388), "canvas"), (dict(Hc=16385), "canvas"),
             (dict(l8=P(l8 + 2)), "4-byte aligned"), (dict(r8=P(r8 + 1)), "4-byte aligned"), (dict(ol=P(ol + 2)), "4-byte aligned"), (dict(orr=P(orr + 3)), "4-byte aligned"),
             (dict(S=0), "heat side"), (dict(S=4097), "heat side"), (dict(txl=None), "tap tables"), (dict(tyl=None), "tap tables"), (dict(txr=None), "tap tables"),
             (dict(tyr=None), "tap tables"), (dict(txl=P(txl + 4)), "16-byte aligned"), (dict(txr=P(txr + 8)), "16-byte aligned"), (dict(tyl=P(tyl + 2)), "4-byte aligned"),
             (dict(tyr=P(tyr + 1)), "4-byte aligned"), (dict(mk=P(mk + 8)), "marks must be 16-byte aligned"),
             (dict(st=sty(n_marks=0)), "n_marks"), (dict(st=sty(n_marks=65)), "n_marks"), (dict(st=sty(n_bones=-1)), "n_bones"), (dict(st=sty(n_bones=65)), "n_bones"),
             (dict(st=bad_bone()), "bone 1 joins marks 1 and 17"), (dict(st=sty(n_marks=16)), "bone 1 joins marks 1 and 16"),
             (dict(st=sty(r16=-1)), "r16 and w16"), (dict(st=sty(r16=16385)), "r16 and w16"), (dict(st=sty(w16=-1)), "r16 and w16"), (dict(st=sty(w16=16385)), "r16 and w16"),
             (dict(st=sty(min_score=nan)), "min_score"),
             # out == in exactly is the one permitted overlap
             (dict(ol=P(l8 + 4)), "out_left8 overlaps left8"), (dict(ol=P(l8 - 4)), "out_left8 overlaps left8"), (dict(orr=P(r8 + canvas - 4)), "out_right8 overlaps right8"),
             (dict(ol=P(r8)), "out_left8 overlaps right8"), (dict(orr=P(l8)), "out_right8 overlaps left8"), (dict(r8=P(l8)), "right8 overlaps left8"),
             (dict(orr=P(ol)), "out_right8 overlaps out_left8"), (dict(ol=P(l8), orr=P(l8), r8=P(r8)), "out_right8 overlaps left8"),
             (dict(h8=P(l8 + 8)), "heat8 overlaps left8"), (dict(ol=P(h8)), "heat8 overlaps out_left8"), (dict(txl=P(orr + 16)), "tx_left overlaps out_right8"),
             (dict(tyl=P(txl + 16)), "ty_left overlaps tx_left"), (dict(txr=P(txl)), "tx_right overlaps tx_left"), (dict(tyr=P(tyl)), "ty_right overlaps ty_left"),
             (dict(tyr=P(h8 + 4)), "ty_right overlaps heat8"), (dict(mk=P(l8 + 16)), "marks overlaps left8"), (dict(mk=P(ol + canvas - 16)), "marks overlaps out_left8"),
             (dict(mk=P(h8)), "marks overlaps heat8"), (dict(mk=P(txr)), "marks overlaps tx_right"), (dict(ol=P(mk)), "marks overlaps out_left8")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_overlay_u8:") and word in msg, (kw, rc, msg)


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch
    from egotap_amd import models as M
    style = spec.overlay_style("UnrealEgo")
    c = torch.zeros(2, 48, 100, 3, dtype=torch.uint8)
    kp, lb, hm = torch.zeros(2, 2, 15, 4), torch.zeros(2, 2, 15, 8), torch.zeros(2, 90, 16, 16)
    with pytest.raises(L.EgotapError, match="float32 or bfloat16"):
        L.heat_u8(hm.double())
    with pytest.raises(ValueError, match=r"\[B, C, S, S\]"):
        L.heat_u8(hm[0])
    with pytest.raises(ValueError, match="equal groups"):
        L.heat_u8(hm, 0, 30, 4)
    with pytest.raises(ValueError, match="equal groups"):
        L.heat_u8(hm, 80, 30, 2)
    with pytest.raises(L.EgotapError, match="contiguous per image"):
        L.heat_u8(hm[:, :, ::2, ::2])
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.heat_u8(hm, 0, 30, 2)
    with pytest.raises(ValueError, match="OverlayStyle"):
        L.overlay_u8(c, c, None)
    with pytest.raises(ValueError, match="canvases"):
        L.overlay_u8(c.float(), c, style, marks=kp)
    with pytest.raises(ValueError, match="canvases"):
        L.overlay_u8(c, c[:1], style, marks=kp)
    with pytest.raises(ValueError, match="multiple of 4"):
        L.overlay_u8(c[:, :, :98], c[:, :, :98], style, marks=kp)
    with pytest.raises(ValueError, match="no marks are given"):
        L.overlay_u8(c, c, style)
    with pytest.raises(ValueError, match=r"marks are a tensor \[B, E, M, 4\]"):
        L.overlay_u8(c, None, style, marks=kp)
    with pytest.raises(ValueError, match="heat8"):
        L.overlay_u8(c, c, style, marks=kp, heat8=torch.zeros(2, 1, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="taps"):
        L.overlay_u8(c, c, style, marks=kp, heat8=torch.zeros(2, 2, 16, 16, dtype=torch.uint8))
    with pytest.raises(ValueError, match="out is"):
        L.overlay_u8(c, c, style, marks=kp, out=(c.float(), c))
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.overlay_u8(c, c, style, marks=kp)
    tx, ty = L.overlay_tap_tables((4.0, 0.0, 4.0, 0.0), 16, 48, 100, "cpu")
    assert tx.dtype == torch.int32 and tuple(tx.shape) == (100,) and tuple(ty.shape) == (48,) and int(tx[99]) == -1 and int(ty[47]) >= 0
    # the helper on the model
    model = M.EgoTAPAutoEncoderModel.__new__(M.EgoTAPAutoEncoderModel)
    torch.nn.Module.__init__(model)
    ov = M.Overlay(15, style)
    assert ov.style_for(True, False) is style or ov.style_for(True, False) == style
    both = ov.style_for(True, True)
    assert len(both.mark_rgba) == 45 and len(both.bones) == 14 + 15 and both.bones[14] == (15, 16) and both.mark_rgba[15][3] == 0
    assert len(ov.style_for(False, True).mark_rgba) == 30 and ov.style_for(False, False).mark_rgba == ()
    lb[..., 2], lb[..., 3], lb[..., 4], lb[..., 5], lb[..., 6] = 10.0, 20.0, math.pi / 2, 8.0, 0.75
    m = ov.marks(kp, lb, eyes=1)
    assert tuple(m.shape) == (2, 1, 45, 4)
    assert torch.allclose(m[0, 0, 15], torch.tensor([10.0, 16.0, 0.75, 0.0]), atol=1e-5) and torch.allclose(m[0, 0, 16], torch.tensor([10.0, 24.0, 0.75, 0.0]), atol=1e-5)
    assert ov.marks() is None
    taps = ov.taps(None, 16, 64, 64, "cpu")
    assert ov.taps(None, 16, 64, 64, "cpu") is taps and len(taps) == 2 and taps[0][0].data_ptr() != taps[1][0].data_ptr()
    assert np.array_equal(taps[0][0].numpy(), spec.overlay_taps(4.0, 0.0, 16, 64))
    assert np.array_equal(ov.taps("identity", 64, 64, 64, "cpu", eyes=1)[0][1].numpy(), np.arange(64))
    with pytest.raises(ValueError, match="affine"):
        ov.taps("mirror", 16, 64, 64, "cpu")
    with pytest.raises(ValueError, match="keypoints"):
        ov.draw(c, c, keypoints=kp[:, :, :14])
    with pytest.raises(ValueError, match="limbs"):
        ov.draw(c, c, limbs=lb[..., :4])
    with pytest.raises(ValueError, match="heatmaps"):
        ov.draw(c, c, heatmaps=hm[:, :20])
    with pytest.raises(L.EgotapError, match="GPU only"):
        ov.draw(c, c, keypoints=kp)
    with pytest.raises(ValueError, match="one mark per heatmap joint"):
        M.Overlay(17, style)
