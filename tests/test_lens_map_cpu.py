"""Host side of the lens entries (egotap_lens_remap, egotap_predict_pose_lens / _kp / _kpl) and of the map they gather through (spec.LensMap,
spec.lens_map, spec.lens_taps, spec.lens_remap_u8, spec.lens_map_points).

The anchor: with the same calibration as model camera and sensor and no rotation the map is the identity lens, and spec.lens_remap_u8 must equal
spec.resize_u8 -- the reference-pinned resize -- bit for bit on every pixel inside the image circle.  The closed forms use helper models whose
rays and projections are written out here, not the functions under test.  No kernel is launched: every refusal comes before the first launch and
the pointers below are never dereferenced."""
import ctypes as C
import dataclasses
import os
import re
import types

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
import ocam_inputs as OI
from test_sensor_resize_cpu import _handle, _ints, _refused

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NEW = ("egotap_lens_remap", "egotap_predict_pose_lens_workspace_bytes", "egotap_predict_pose_lens", "egotap_predict_pose_lens_kp",
       "egotap_predict_pose_lens_kpl")
ONE = 2048


@pytest.fixture(scope="module")
def anchor_frames():
    return np.random.default_rng(5).integers(0, 256, (2, 1024, 1024, 3), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------ 1. the anchor
@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("S0", [64, 128, 192, 256, 384])
def test_identity_lens_equals_the_resize_bit_for_bit_inside_the_circle(anchor_frames, S0, mirror):
    cam = OI.calibration(0)
    assert cam.size == (1024, 1024) and cam.radius == 500.0
    m = spec.lens_map(cam, cam, S0, mirror=mirror)
    assert (m.S0, m.H, m.W, m.model_size, m.mirror) == (S0, 1024, 1024, (1024, 1024), mirror)
    got = spec.lens_remap_u8(anchor_frames, m)
    want = spec.resize_u8(anchor_frames, (0, 0, 1024, 1024), mirror, S0)
    ok = m.valid
    share = float(ok.mean())
    differing = int((got[:, ok] != want[:, ok]).sum())
    print(f"S0 {S0} mirror {mirror}: valid share {share:.4f}, differing bytes on valid pixels {differing}")
    assert 0.74 <= share <= 0.76          # the circle is pi 500^2 / 1024^2 = 0.749 of the frame
    assert differing == 0
    assert not got[:, ~ok].any()          # the default fill


# ------------------------------------------------------------------------------------------------------------ 2. closed forms
def _helper(f, xc, yc, size, radius=0.0, name="helper"):
    """cam2world((u, v)) = (u', v', f) / |.| with (u', v') = (u - xc, v - yc); world2cam of a ray whose lateral part has length n and height z lands
    f * atan(z / n) from the centre, along the lateral direction"""
    return dataclasses.replace(OI.pinhole(f, name), xc=xc, yc=yc, size=size, radius=radius)


def _closed(model, sensor, f, f2, S0, a=0.0, mirror=False):
    """(u, v, xs, ys) of every output pixel by the closed forms: the ray of (u', v') is (u', v', f) / |.|, rotated about z by a; the sensor puts it
    f2 * atan(f / r) from its centre along the rotated direction, r = hypot(u', v')"""
    X, Y = np.meshgrid(np.arange(S0, dtype=np.float64), np.arange(S0, dtype=np.float64))
    if mirror:
        X = S0 - 1 - X
    u = (X + 0.5) * model.size[1] / S0 - 0.5
    v = (Y + 0.5) * model.size[0] / S0 - 0.5
    up, vp = u - model.xc, v - model.yc
    r = np.hypot(up, vp)
    rho = f2 * np.arctan(f / r)
    ca, sa = np.cos(a), np.sin(a)
    return u, v, sensor.xc + (ca * up - sa * vp) / r * rho, sensor.yc + (sa * up + ca * vp) / r * rho


@pytest.mark.parametrize("a", [0.0, 0.3, -1.1])
@pytest.mark.parametrize("mirror", [False, True])
def test_entries_follow_the_closed_form_of_two_helper_lenses(a, mirror):
    f, f2, S0 = 300.0, 40.0, 32
    model = _helper(f, 31.25, 23.75, (48, 64))           # no pixel centre sits on the axis: r > 0 everywhere
    sensor = _helper(f2, 100.0, 90.0, (200, 220))
    # the model's rays by the closed form, against the function the map calls
    uv = np.stack(np.meshgrid(np.arange(64.0), np.arange(48.0)), axis=-1)
    want = np.concatenate([uv - (31.25, 23.75), np.full(uv.shape[:2] + (1,), f)], axis=-1)
    want /= np.linalg.norm(want, axis=-1, keepdims=True)
    assert np.abs(spec.ocam_cam2world_ref(uv, model) - want).max() < 1e-14
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    m = spec.lens_map(model, sensor, S0, R=None if a == 0.0 else R, mirror=mirror)
    u, v, xs, ys = _closed(model, sensor, f, f2, S0, a, mirror)
    inside = (xs >= 0) & (xs <= 219) & (ys >= 0) & (ys <= 199)
    assert inside.all() and m.valid.all()                 # f2 * pi / 2 = 63 pixels from the centre at most: the whole map lands inside the frame
    # float64 error is far below 2^-11, so only a tie of the rounding can move an entry, by one
    want_fx, want_fy = np.floor(xs * ONE + 0.5), np.floor(ys * ONE + 0.5)
    assert np.abs(m.taps[..., 0] - want_fx).max() <= 1 and np.abs(m.taps[..., 1] - want_fy).max() <= 1
    assert (m.taps[..., 0] != want_fx).mean() < 0.01 and (m.taps[..., 1] != want_fy).mean() < 0.01
    # the pixel offsets rotate by a: against the unrotated map's real coordinates
    _, _, x0, y0 = _closed(model, sensor, f, f2, S0, 0.0, mirror)
    dx, dy = x0 - sensor.xc, y0 - sensor.yc
    assert np.abs((xs - sensor.xc) - (np.cos(a) * dx - np.sin(a) * dy)).max() < 1e-11
    assert np.abs(m.taps[..., 1] / ONE - sensor.yc - (np.sin(a) * dx + np.cos(a) * dy)).max() <= 2.0 ** -11
    # lens_map_points agrees with the entries at pixel centres
    pts = spec.lens_map_points(np.stack([u, v], axis=-1), model, sensor, R=None if a == 0.0 else R)
    assert np.abs(pts - m.taps / ONE).max() <= 2.0 ** -11


def test_frame_size_scales_calibration_pixels_per_axis():
    f, f2, S0 = 300.0, 40.0, 16
    model, sensor = _helper(f, 31.25, 23.75, (48, 64)), _helper(f2, 100.0, 90.0, (200, 220))
    _, _, xs, ys = _closed(model, sensor, f, f2, S0)
    m = spec.lens_map(model, sensor, S0, frame_size=(100, 330))
    assert (m.H, m.W) == (100, 330)
    want = np.stack([(xs + 0.5) * 1.5 - 0.5, (ys + 0.5) * 0.5 - 0.5], axis=-1)
    assert m.valid.all() and np.abs(m.taps / ONE - want).max() <= 2.0 ** -11
    pts = spec.lens_map_points([[31.25, 23.75]], model, sensor, frame_size=(100, 330))          # the axis lands on the centre, scaled
    assert np.allclose(pts, [[100.5 * 1.5 - 0.5, 90.5 * 0.5 - 0.5]], atol=1e-12)
    frames = np.zeros((1, 200, 220, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match=r"built for 100 x 330 frames, got 200 x 220"):          # a frame of another size is refused
        spec.lens_remap_u8(frames, m)
    with pytest.raises(ValueError, match="between 1 and 16384"):
        spec.lens_map(model, sensor, S0, frame_size=(0, 330))
    with pytest.raises(ValueError, match="R is 3 x 3"):
        spec.lens_map(model, sensor, S0, R=np.eye(2))


# ------------------------------------------------------------------------------------------------------------ 3. validity
def test_entries_outside_either_circle_the_frame_or_from_a_nan_pixel_are_invalid():
    f, f2, S0 = 300.0, 40.0, 32
    # the model's circle: the test is on (u, v), which this test computes itself
    model = _helper(f, 31.25, 23.75, (48, 64), radius=20.3)
    sensor = _helper(f2, 100.0, 90.0, (200, 220))
    u, v, xs, ys = _closed(model, sensor, f, f2, S0)
    rm = np.hypot(u - model.xc, v - model.yc)
    assert abs(rm - 20.3).min() > 1e-9
    m = spec.lens_map(model, sensor, S0)
    assert np.array_equal(m.valid, rm <= 20.3) and 0.2 < m.valid.mean() < 0.8
    assert (m.taps[~m.valid] == -1).all()
    # the sensor's circle: the test is on the sensor's calibration pixel, here from the closed form
    sensor = _helper(f2, 100.0, 90.0, (200, 220), radius=60.0)
    m = spec.lens_map(_helper(f, 31.25, 23.75, (48, 64)), sensor, S0)
    rs = np.hypot(xs - 100.0, ys - 90.0)
    assert abs(rs - 60.0).min() > 1e-9 and np.array_equal(m.valid, rs <= 60.0) and 0.2 < m.valid.mean() < 0.8
    # the frame: a sensor whose centre sits near a corner sees a quarter of the map
    sensor = _helper(f2, 3.0, 5.0, (60, 70))
    _, _, xs, ys = _closed(model, sensor, f, f2, S0)
    inside = (xs >= 0) & (xs <= 69) & (ys >= 0) & (ys <= 59)
    m = spec.lens_map(_helper(f, 31.25, 23.75, (48, 64)), sensor, S0)
    assert np.array_equal(m.valid, inside) and 0.05 < inside.mean() < 0.5
    # a sensor polynomial that overflows to inf - inf for steep rays gives a NaN calibration pixel there (and -inf a little further out): invalid,
    # not an exception and not an entry
    near = _helper(20.0, 31.25, 23.75, (48, 64))
    wild = spec.OcamModel(name="wild", pol=[f2], invpol=[0.0, f2, 0.0, 1e308, -1e308], xc=100.0, yc=90.0, size=(200, 220))
    with np.errstate(all="ignore"):
        pix = spec.ocam_world2cam_ref(spec.ocam_cam2world_ref(np.stack([u, v], axis=-1), near), wild)
    bad = np.isnan(pix).any(axis=-1)
    assert 0.02 < bad.mean() < 0.5
    m = spec.lens_map(near, wild, S0)
    assert not m.valid[bad].any() and not m.valid.any()            # (where the polynomial stays finite it is of the order 1e306: outside the frame)


def test_the_last_pixel_exactly_is_valid_and_its_second_tap_is_itself():
    # the ray of the model's centre pixel is the axis, which every sensor puts on its centre EXACTLY: a sensor whose centre is its last pixel
    model = _helper(300.0, 4.0, 4.0, (8, 8))
    sensor = _helper(40.0, 6.0, 4.0, (5, 7))
    m = spec.lens_map(model, sensor, 8)                  # S0 = the model's size: u = X exactly
    assert tuple(m.taps[4, 4]) == (6 * ONE, 4 * ONE) and m.valid[4, 4]
    ok, ix0, ix1, wx1, iy0, iy1, wy1 = spec.lens_taps(m)
    assert (ix0[4, 4], ix1[4, 4], wx1[4, 4], iy0[4, 4], iy1[4, 4], wy1[4, 4]) == (6, 6, 0, 4, 4, 0)
    frames = np.random.default_rng(1).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    assert np.array_equal(spec.lens_remap_u8(frames, m)[:, 4, 4], frames[:, 4, 6])
    # one step further is outside
    beyond = spec.lens_map(model, dataclasses.replace(sensor, xc=6.0 + 2.0 ** -20), 8)
    assert not beyond.valid[4, 4]


def _tap_extents(m):
    ok, ix0, ix1, wx1, iy0, iy1, wy1 = spec.lens_taps(m)
    assert ok.any() and ix0[ok].min() >= 0 and iy0[ok].min() >= 0 and ix1[ok].max() == m.W - 1 and iy1[ok].max() == m.H - 1      # the last row and column are hit
    assert (ix1 >= ix0).all() and (iy1 >= iy0).all() and (wx1 < ONE).all() and (wy1 < ONE).all()
    return [(y[ok], x[ok]) for y in (iy0, iy1) for x in (ix0, ix1)]


def test_every_tap_the_restatement_reads_lies_inside_the_frame():
    model = _helper(20.0, 31.25, 23.75, (48, 64))           # a short focal length: the map covers a disc of radius f2 * pi / 2, not a thin ring
    for H, W, f2 in ((38, 54, 40.0), (6, 8, 4.0)):
        sensor = _helper(f2, W - 1.5 - 0.5 * f2, H - 1.25 - 0.5 * f2, (H, W))          # ... which runs over the frame's far edges
        m = spec.lens_map(model, sensor, 64)
        assert 0.0 < m.valid.mean() < 1.0
        taps = _tap_extents(m)
        nv12 = spec.YuvLayout.nv12(H, W, pitch=W + 10, uv_offset=(W + 10) * H + 6)
        yuyv = spec.YuvLayout.yuyv(H, W, pitch=2 * W + 12)
        for y, x in taps:
            assert (3 * (y * W + x) + 2).max() < 3 * H * W                                                     # packed RGB: the pixel's last byte
            assert (y * nv12.pitch + x).max() < nv12.uv_offset                                                 # NV12: the luma byte, in its plane
            assert (nv12.uv_offset + (y >> 1) * nv12.pitch + 2 * (x >> 1) + 1).max() < nv12.frame_stride       # ... and the chroma pair's last byte
            assert ((y >> 1).max(), (2 * (x >> 1) + 1).max()) == (H // 2 - 1, W - 1)
            assert (y * yuyv.pitch + 4 * (x >> 1) + 3).max() < yuyv.frame_stride                               # YUYV: the pair's last byte
            assert (4 * (x >> 1) + 3).max() == 2 * W - 1                                                       # ... inside the row's 2 W bytes


def test_mirroring_flips_the_output_columns():
    cam, other = OI.rig_models(True)
    a = spec.lens_map(cam, other, 64, OI.SMALL_R, frame_size=(480, 640))
    b = spec.lens_map(cam, other, 64, OI.SMALL_R, frame_size=(480, 640), mirror=True)
    assert b.mirror and not a.mirror and np.array_equal(b.taps, a.taps[:, ::-1])
    assert 0.6 < a.valid.mean() < 0.7
    frames = np.random.default_rng(2).integers(0, 256, (1, 480, 640, 3), dtype=np.uint8)
    assert np.array_equal(spec.lens_remap_u8(frames, b, (1, 2, 3)), spec.lens_remap_u8(frames, a, (1, 2, 3))[:, :, ::-1])


def test_restatement_by_hand_and_its_faces():
    taps = np.full((4, 4, 2), -1, dtype=np.int32)
    taps[0, 0] = (0, 0)
    taps[0, 1] = (6 * ONE, 4 * ONE)                       # the far corner of a 5 x 7 frame
    taps[1, 2] = (2 * ONE + 512, 1 * ONE + 1536)          # a quarter along x, three quarters along y
    m = spec.LensMap(taps, 4, 5, 7, (8, 8))
    frames = np.random.default_rng(3).integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    got = spec.lens_remap_u8(frames, m, fill=(9, 8, 7))
    assert got.shape == (2, 4, 4, 3) and got.dtype == np.uint8
    assert np.array_equal(got[:, 0, 0], frames[:, 0, 0]) and np.array_equal(got[:, 0, 1], frames[:, 4, 6])
    p = frames.astype(np.int64)
    want = (512 * (1536 * p[:, 1, 2] + 512 * p[:, 1, 3]) + 1536 * (1536 * p[:, 2, 2] + 512 * p[:, 2, 3]) + (1 << 21)) >> 22
    assert np.array_equal(got[:, 1, 2], want)
    rest = np.ones((4, 4), dtype=bool)
    rest[0, 0] = rest[0, 1] = rest[1, 2] = False
    assert (got[:, rest] == (9, 8, 7)).all()
    as_torch = spec.lens_remap_u8(torch.from_numpy(frames), m, fill=(9, 8, 7))
    assert torch.is_tensor(as_torch) and np.array_equal(as_torch.numpy(), got)
    with pytest.raises(ValueError, match="uint8"):
        spec.lens_remap_u8(frames.astype(np.float32), m)
    with pytest.raises(ValueError, match="three bytes"):
        spec.lens_remap_u8(frames, m, fill=(0, 0, 256))
    with pytest.raises(ValueError, match="spec.LensMap"):
        spec.lens_remap_u8(frames, taps)
    with pytest.raises(ValueError):
        m.taps[0, 0, 0] = 5                               # a map is read-only
    with pytest.raises(ValueError, match="int32"):
        spec.LensMap(taps.astype(np.int64), 4, 5, 7, (8, 8))
    bad = taps.copy()
    bad[2, 2] = (7 * ONE, 0)
    with pytest.raises(ValueError, match="outside the 5 x 7 frame"):
        spec.LensMap(bad, 4, 5, 7, (8, 8))
    bad[2, 2] = (3, -1)
    with pytest.raises(ValueError, match=r"valid in both halves or \(-1, -1\)"):
        spec.LensMap(bad, 4, 5, 7, (8, 8))


# ------------------------------------------------------------------------------------------------------------ 4. symbols
def test_new_symbols_are_declared_and_exported():
    import subprocess
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egotap.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", L._build.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(egotap_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert hasattr(lib, name) and name in L.exported_symbols() and name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2          # additive: the version stays
    assert re.search(r"}\s*egotap_lens_source\s*;", header)
    S = L.EgotapLensSource
    assert (C.sizeof(S), S.mirror.offset, S.map_left.offset, S.map_right.offset, S.fill.offset, S.yuv.offset) == (104, 24, 32, 40, 48, 56)
    assert (L.LENS_FORMATS["rgb8"], L.LENS_FORMATS["nv12"], L.LENS_FORMATS["yuyv"]) == (0, 1, 2)
    for name, value in (("EGOTAP_LENS_RGB8", 0), ("EGOTAP_LENS_NV12", 1), ("EGOTAP_LENS_YUYV", 2)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", header), name


# ------------------------------------------------------------------------------------------------------------ 5. refusals
MAP_L, MAP_R = 0x800000, 0x900010


def _yuv(fmt, **kw):
    if fmt == "nv12":
        f = dict(struct_size=C.sizeof(L.EgotapYuvSource), format=0, matrix=0, range=0, H=38, W=54, pitch=64, uv_offset=64 * 38 + 32,
                 frame_stride=64 * 38 + 32 + 64 * 19 + 16)
    else:
        f = dict(struct_size=C.sizeof(L.EgotapYuvSource), format=1, matrix=0, range=0, H=38, W=54, pitch=112, uv_offset=0, frame_stride=112 * 38 + 8)
    f.update(kw)
    return L.EgotapYuvSource(*(f[n] for n, _ in L.EgotapYuvSource._fields_))


def _desc(fmt="rgb8", yuv=None, **kw):
    """a descriptor, valid unless a field is overridden: 38 x 54 frames, a 1024 x 1024 model camera, the right eye mirrored"""
    d = L.EgotapLensSource()
    d.struct_size, d.format, d.H, d.W, d.model_h, d.model_w = C.sizeof(L.EgotapLensSource), L.LENS_FORMATS[fmt], 38, 54, 1024, 1024
    d.mirror[1] = 1
    d.map_left, d.map_right = MAP_L, MAP_R
    if fmt != "rgb8":
        d.yuv = _yuv(fmt, **(yuv or {}))
    for k, v in kw.items():
        setattr(d, k, v)
    return d


BAD_DESCS = [(dict(struct_size=100), b"struct_size"), (dict(struct_size=0), b"struct_size"), (dict(format=3), b"unknown format"), (dict(format=-1), b"unknown format"),
             (dict(H=0), b"height and width"), (dict(W=16385), b"height and width"), (dict(H=-3), b"height and width"),
             (dict(map_left=None), b"null lens map"), (dict(map_right=None), b"null lens map"),
             (dict(map_left=MAP_L + 8), b"16-byte aligned"), (dict(map_right=MAP_R + 4), b"16-byte aligned"),
             (dict(fmt="nv12", yuv=dict(format=1)), b"another format"), (dict(fmt="yuyv", yuv=dict(format=0)), b"another format"),
             (dict(fmt="nv12", yuv=dict(H=40)), b"another H or W"), (dict(fmt="yuyv", W=56), b"another H or W"),
             (dict(fmt="nv12", yuv=dict(struct_size=44)), b"struct_size"), (dict(fmt="nv12", yuv=dict(matrix=2)), b"unknown matrix"),
             (dict(fmt="nv12", yuv=dict(range=2)), b"unknown range"), (dict(fmt="nv12", yuv=dict(pitch=52)), b"pitch is too small"),
             (dict(fmt="nv12", yuv=dict(pitch=63)), b"even pitch"), (dict(fmt="nv12", H=37, yuv=dict(H=37)), b"even H and W"),
             (dict(fmt="nv12", H=0, yuv=dict(H=0)), b"height and width"),
             (dict(fmt="yuyv", W=53, yuv=dict(W=53)), b"even W"), (dict(fmt="yuyv", yuv=dict(pitch=110)), b"multiples of 4"),
             (dict(fmt="yuyv", yuv=dict(frame_stride=112 * 37 + 104)), b"past frame_stride")]


def test_operator_refusals():
    lib = L.load()
    f, who = lib.egotap_lens_remap, b"egotap_lens_remap"
    l8, r8, ol, orr = (C.c_void_p(a) for a in (0x200001, 0x300003, 0x500000, 0x600000))          # RGB8 frames may sit at any address
    d = C.byref(_desc())
    _refused(lib, f, who, l8, r8, 0, d, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, l8, r8, -1, d, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, None, r8, 2, d, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, None, 2, d, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, r8, 2, None, 64, ol, orr, None, word=b"null source descriptor")
    _refused(lib, f, who, l8, r8, 2, d, 64, None, orr, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 2, d, 64, ol, None, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 2, d, 64, C.c_void_p(0x500002), orr, None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, r8, 2, d, 64, ol, C.c_void_p(0x600001), None, word=b"4-byte aligned")
    for S0 in (0, -4, 62, 4100, 8192):
        _refused(lib, f, who, l8, r8, 2, d, S0, ol, orr, None, word=b"multiple of 4")
    even = (C.c_void_p(0x200002), C.c_void_p(0x300006))
    quad = (C.c_void_p(0x200004), C.c_void_p(0x300008))
    for kw, word in BAD_DESCS:
        a, b = quad if kw.get("fmt") == "yuyv" else even
        _refused(lib, f, who, a, b, 2, C.byref(_desc(**kw)), 64, ol, orr, None, word=word)
    _refused(lib, f, who, C.c_void_p(0x200001), even[1], 2, C.byref(_desc("nv12")), 64, ol, orr, None, word=b"2-byte aligned")
    _refused(lib, f, who, even[0], C.c_void_p(0x300003), 2, C.byref(_desc("nv12")), 64, ol, orr, None, word=b"2-byte aligned")
    _refused(lib, f, who, quad[0], even[1], 2, C.byref(_desc("yuyv")), 64, ol, orr, None, word=b"4-byte aligned (YUYV")
    _refused(lib, f, who, None, even[1], 2, C.byref(_desc("yuyv")), 64, ol, orr, None, word=b"null frames")


@pytest.mark.parametrize("suffix", ["", "_kp", "_kpl"])
@pytest.mark.parametrize("hm", [64, 32])
def test_one_call_refusals(hm, suffix):
    lib, h = _handle(hm=hm)
    try:
        need, sensor = C.c_size_t(), C.c_size_t()
        assert lib.egotap_predict_pose_lens_workspace_bytes(h, 4, 0, C.byref(need)) == 0
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 38, 54, 0, C.byref(sensor)) == 0 and need.value == sensor.value      # the sensor entry's size
        assert lib.egotap_predict_pose_lens_workspace_bytes(h, 4, 3, C.byref(need)) == 0
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 1000, 2000, 3, C.byref(sensor)) == 0 and need.value == sensor.value
        assert lib.egotap_predict_pose_lens_workspace_bytes(h, 4, 0, C.byref(need)) == 0
        q, who = lib.egotap_predict_pose_lens_workspace_bytes, b"egotap_predict_pose_lens_workspace_bytes"
        _refused(lib, q, who, None, 4, 0, C.byref(need), word=b"null argument")
        _refused(lib, q, who, h, 4, 0, None, word=b"null argument")
        _refused(lib, q, who, h, -1, 0, C.byref(need), word=b"negative")
        _refused(lib, q, who, h, 4, -1, C.byref(need), word=b"negative")
        name = "egotap_predict_pose_lens" + suffix
        fn, who = getattr(lib, name), name.encode()
        kp, lb = C.c_void_p(0x4000000), C.c_void_p(0x5000000)          # (clear of the fake heatmaps)
        extra = {"": (), "_kp": (kp,), "_kpl": (kp, lb)}[suffix]

        def f(*a):
            return fn(*a, *extra)
        l8, r8, tab, pose, hmp, ws = (C.c_void_p(a) for a in (0x200002, 0x300002, 0x400000, 0x500000, 0x600000, 0x700000))
        d = C.byref(_desc())
        ok = (4, d, tab, pose, hmp, 0, ws, need.value, None)
        _refused(lib, f, who, None, l8, r8, *ok, word=b"null handle")
        _refused(lib, f, who, h, None, r8, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, None, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, r8, 4, None, tab, pose, hmp, 0, ws, need.value, None, word=b"null source descriptor")
        _refused(lib, f, who, h, l8, r8, 4, d, None, pose, hmp, 0, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, None, hmp, 0, ws, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, hmp, 0, None, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 0, d, tab, pose, hmp, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, hmp, -1, ws, need.value, None, word=b"chunk")
        quad = (C.c_void_p(0x200004), C.c_void_p(0x300008))
        for kw, word in BAD_DESCS:
            a, b = quad if kw.get("fmt") == "yuyv" else (l8, r8)
            _refused(lib, f, who, h, a, b, 4, C.byref(_desc(**kw)), tab, pose, hmp, 0, ws, need.value, None, word=word)
        for kw in (dict(model_h=0), dict(model_w=-1), dict(model_w=16385)):
            _refused(lib, f, who, h, l8, r8, 4, C.byref(_desc(**kw)), tab, pose, hmp, 0, ws, need.value, None, word=b"model camera's calibration image")
        _refused(lib, f, who, h, C.c_void_p(0x200001), r8, 4, C.byref(_desc("nv12")), tab, pose, hmp, 0, ws, need.value, None, word=b"2-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, C.byref(_desc("yuyv")), tab, pose, hmp, 0, ws, need.value, None, word=b"4-byte aligned (YUYV")
        _refused(lib, f, who, h, l8, r8, 4, d, C.c_void_p(0x400004), pose, hmp, 0, ws, need.value, None, word=b"16-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, C.c_void_p(0x600008), 0, ws, need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, hmp, 0, C.c_void_p(0x700010), need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, hmp, 0, ws, need.value - 1, None, word=b"workspace too small")
        u8 = C.c_size_t()          # the byte entry's size is short by the slice: a lens source always gathers into it
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, 0, C.byref(u8)) == 0
        _refused(lib, f, who, h, l8, r8, 4, d, tab, pose, hmp, 0, ws, u8.value, None, word=b"workspace too small")
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
        assert lib.egotap_predict_pose_lens_workspace_bytes(h, 2, 0, C.byref(need)) == 0
        l8, r8, tab, pose, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x700000))
        rc = lib.egotap_predict_pose_lens(h, l8, r8, 2, C.byref(_desc()), tab, pose, None, 0, ws, need.value, None)
        msg = lib.egotap_last_error()
        assert rc == INVALID and b"egotap_predict_pose_lens" in msg and b"unbound parameter" in msg and b"limb estimator" in msg, msg
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 6. the Python faces
class _OnGpu(torch.Tensor):          # dtype and shape are looked at once the frames are on a GPU: a stand-in for "is on the GPU"
    is_cuda = True


def _fake_maps(S0=256, H=38, W=54, model=(1024, 1024), fill=((0, 0, 0), (0, 0, 0)), mirror_right=True):
    """a lib.LensMaps whose device tensors are host tensors: what the faces check before anything touches a GPU"""
    taps = np.full((S0, S0, 2), -1, dtype=np.int32)
    left, right = spec.LensMap(taps, S0, H, W, model), spec.LensMap(taps, S0, H, W, model, mirror_right)
    t = torch.zeros(S0 * S0, 2, dtype=torch.int32)
    return L.LensMaps(left, right, t, t.clone(), fill)


def test_python_faces_check_on_the_host():
    from egotap_amd import models
    from egotap_amd.options import preset_defaults
    taps = np.full((256, 256, 2), -1, dtype=np.int32)
    a = spec.LensMap(taps, 256, 38, 54, (1024, 1024))
    with pytest.raises(ValueError, match="spec.LensMap"):
        L.lens_maps(a, taps)
    with pytest.raises(ValueError, match="one output side"):
        L.lens_maps(a, spec.LensMap(taps[:128, :128], 128, 38, 54, (1024, 1024)))
    with pytest.raises(ValueError, match="one frame size"):
        L.lens_maps(a, spec.LensMap(taps, 256, 38, 56, (1024, 1024)))
    with pytest.raises(ValueError, match="calibration size"):
        L.lens_maps(a, spec.LensMap(taps, 256, 38, 54, (960, 1280)))
    with pytest.raises(ValueError, match="multiple of 4"):
        L.lens_maps(spec.LensMap(taps[:6, :6], 6, 38, 54, (8, 8)), spec.LensMap(taps[:6, :6], 6, 38, 54, (8, 8)))
    for fill in ((0, 0), (0, 0, 256), ((1, 2, 3),), ((1, 2, 3), (4, 5))):
        with pytest.raises(ValueError, match="fill is three bytes"):
            L.lens_maps(a, a, fill=fill)
    with pytest.raises(L.EgotapError, match="live on the GPU"):
        L.lens_maps(a, a, device="cpu")

    m = types.SimpleNamespace(opt=preset_defaults("UnrealEgo", 64), net_AutoEncoder=types.SimpleNamespace(preset=spec.lift_preset("UnrealEgo", 64)))
    m.lens_maps = types.MethodType(models.EgoTAPAutoEncoderModel.lens_maps, m)
    m.predict_pose_from_lens = types.MethodType(models.EgoTAPAutoEncoderModel.predict_pose_from_lens, m)
    small = spec.LensMap(taps[:128, :128], 128, 38, 54, (1024, 1024))
    with pytest.raises(ValueError, match=r"read 256 x 256 frames \(4 \* hm_size\), the map was built for S0 = 128"):
        m.lens_maps(small, small)

    maps = _fake_maps()
    assert maps.mirrors == (0, 1) and (maps.S0, maps.H, maps.W, maps.model_size) == (256, 38, 54, (1024, 1024))
    d = L.lens_source(maps)
    assert (d.struct_size, d.format, d.H, d.W, d.model_h, d.model_w, tuple(d.mirror)) == (104, 0, 38, 54, 1024, 1024, (0, 1))
    assert (d.map_left, d.map_right) == (maps.map_left.data_ptr(), maps.map_right.data_ptr())
    layout, colour = spec.YuvLayout.nv12(38, 54, pitch=64), spec.YuvColour("bt709", "full")
    d = L.lens_source(_fake_maps(fill=((1, 2, 3), (4, 5, 6))), layout, colour)
    assert d.format == 1 and bytes(d.yuv) == bytes(L.yuv_source(layout, colour)) and [list(f) for f in d.fill] == [[1, 2, 3], [4, 5, 6]]
    assert L.lens_source(maps, spec.YuvLayout.yuyv(38, 54), colour).format == 2

    cpu8 = torch.zeros(2, 38, 54, 3, dtype=torch.uint8)
    g = lambda t: t.as_subclass(_OnGpu)      # noqa: E731
    who = "predict_pose_from_lens"
    with pytest.raises(L.EgotapError, match="predict_pose_from_lens runs on the GPU only"):
        m.predict_pose_from_lens(cpu8, cpu8, maps)
    with pytest.raises(L.EgotapError, match="lens_remap runs on the GPU only"):
        L.lens_remap(cpu8, cpu8, maps, 256)
    with pytest.raises(ValueError, match="what lens_maps returns"):
        m.predict_pose_from_lens(g(cpu8), g(cpu8), (a, a))
    assert L.check_lens_frames(who, g(cpu8), g(cpu8), maps) == 2
    with pytest.raises(ValueError, match=r"built for 38 x 54 frames, got 38 x 56"):
        L.check_lens_frames(who, g(torch.zeros(2, 38, 56, 3, dtype=torch.uint8)), g(torch.zeros(2, 38, 56, 3, dtype=torch.uint8)), maps)
    with pytest.raises(L.EgotapError, match="dtype uint8"):
        L.check_lens_frames(who, g(cpu8.float()), g(cpu8.float()), maps)
    with pytest.raises(ValueError, match="layout is a spec.YuvLayout"):
        L.check_lens_frames(who, g(cpu8), g(cpu8), maps, (38, 54), colour)
    yuv8 = torch.zeros(2, layout.frame_stride, dtype=torch.uint8)
    assert L.check_lens_frames(who, g(yuv8), g(yuv8), maps, layout, colour) == 2
    with pytest.raises(ValueError, match="frame_stride"):
        L.check_lens_frames(who, g(yuv8[:, :-2]), g(yuv8[:, :-2]), maps, layout, colour)
    other = spec.YuvLayout.nv12(40, 54)
    with pytest.raises(ValueError, match=r"built for 38 x 54 frames, got 40 x 54"):
        L.check_lens_frames(who, g(torch.zeros(2, other.frame_stride, dtype=torch.uint8)), g(torch.zeros(2, other.frame_stride, dtype=torch.uint8)), maps, other, colour)
    with pytest.raises(ValueError, match=r"maps were built for S0 = 128"):
        m.predict_pose_from_lens(g(cpu8), g(cpu8), _fake_maps(S0=128))
    with pytest.raises(ValueError, match=r"built for S0 = 256, got S0 = 128"):
        L.lens_remap(g(cpu8), g(cpu8), maps, 128)
    # the sensor entries keep their signatures
    import inspect
    assert list(inspect.signature(models.EgoTAPAutoEncoderModel.predict_pose_from_lens).parameters)[:6] == ["self", "left8", "right8", "maps", "layout", "colour"]
    assert list(inspect.signature(models.EgoTAPAutoEncoderModel.predict_pose_from_sensor).parameters)[:6] == ["self", "left8", "right8", "crop", "crop_right", "mirror_right"]
