"""CPU-side checks of the heatmap-peaks feature (egotap.h: egotap_heatmap_peaks and the three _kp serving entries): the exports, every host-side
refusal (fake pointers: nothing is launched), and the definition itself -- spec.heatmap_peaks_ref -- against the reference's own rendering of the
ground-truth maps and against the resize whose map the sensor affine inverts."""
import ctypes as C

import numpy as np
import pytest

from egotap_amd import lib as L
from egotap_amd import spec
from oracle import heatmap_synth_ref as R

NEW = ("egotap_heatmap_peaks", "egotap_predict_pose_rgb_kp", "egotap_predict_pose_rgb_u8_kp", "egotap_predict_pose_sensor_u8_kp")


def test_the_new_entries_are_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name) and f"int {name}(" in text
    assert lib.egotap_abi_version() == 2 and L.BF16 == 2 and "EGOTAP_BF16 = 2" in text


def test_heatmap_peaks_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    ok = dict(hm=P(0x10000), dtype=L.F32, B=3, S=64, stride=90 * 4096, c0=2, n=6, groups=2, affine=None, peaks=P(0x20000))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_heatmap_peaks(a["hm"], a["dtype"], a["B"], a["S"], a["stride"], a["c0"], a["n"], a["groups"], a["affine"], a["peaks"], None)
        return rc, lib.egotap_last_error().decode()
    cases = [(dict(hm=None), "null"), (dict(peaks=None), "null"), (dict(B=0), "must be positive"), (dict(n=0), "must be positive"),
             (dict(groups=0), "groups must be"), (dict(groups=4), "multiple of groups"), (dict(c0=-1), "negative first channel"),
             (dict(stride=8 * 4096 - 4), "image_stride"), (dict(c0=85), "image_stride"), (dict(S=60), "multiple of 16"), (dict(S=8), "multiple of 16"),
             (dict(S=144, stride=90 * 144 * 144), "multiple of 16"), (dict(hm=P(0x10004)), "16-byte aligned"), (dict(peaks=P(0x20008)), "16-byte aligned"),
             (dict(dtype=L.I64), "unknown dtype"), (dict(dtype=7), "unknown dtype"),
             (dict(dtype=L.BF16, stride=90 * 4096 + 4), "multiple of 16 bytes"), (dict(stride=90 * 4096 + 2), "multiple of 16 bytes")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_heatmap_peaks:") and word in msg, (kw, rc, msg)


def _cfg():
    return L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, 64, 128, 1024, 8, 3, 16, 512)


def test_kp_entries_refuse_their_extra_output_before_any_launch():
    """the handle has nothing bound: a call that passes the keypoint checks ends at 'unbound parameter', still before any launch"""
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.egotap_create(C.byref(_cfg()), C.byref(h)))
    P = C.c_void_p
    B, J, S = 2, 15, 64
    left, right, table, ws = P(0x100000), P(0x200000), P(0x300000), P(0x1000000)
    pose, hm, kp = 0x400000, 0x500000, 0x4000000
    pose_bytes, hm_bytes, kp_bytes = B * 16 * 3 * 4, B * 6 * J * S * S * 4, B * 2 * J * 16
    rects, flags = (C.c_int * 8)(10, 20, 300, 200, 10, 20, 300, 200), (C.c_int * 2)(0, 1)
    entries = {
        "egotap_predict_pose_rgb_kp": lambda po, hmo, k: lib.egotap_predict_pose_rgb_kp(h, left, right, B, P(po), P(hmo), 0, ws, 1 << 40, None, P(k)),
        "egotap_predict_pose_rgb_u8_kp": lambda po, hmo, k: lib.egotap_predict_pose_rgb_u8_kp(h, left, right, B, table, P(po), P(hmo), 0, ws, 1 << 40, None, P(k)),
        "egotap_predict_pose_sensor_u8_kp": lambda po, hmo, k: lib.egotap_predict_pose_sensor_u8_kp(h, left, right, B, 480, 640, rects, flags, table, P(po), P(hmo), 0,
                                                                                              ws, 1 << 40, None, P(k)),
    }
    try:
        for name, fn in entries.items():
            cases = [((pose, hm, None), "null keypoints"), ((pose, hm, kp + 8), "keypoints must be 16-byte aligned"),
                     ((pose, hm, pose), "overlaps"), ((pose, hm, pose + pose_bytes - 16), "overlaps"), ((pose, hm, pose - kp_bytes + 16), "overlaps"),
                     ((pose, hm, hm + hm_bytes - 16), "overlaps"), ((pose, hm, hm + 4096), "overlaps"),
                     # directly behind pose / in front of the heatmaps is no overlap; without heatmaps their extent is nobody's
                     ((pose, hm, pose + pose_bytes), "unbound parameter"), ((pose, hm, hm - kp_bytes), "unbound parameter"),
                     ((pose, None, hm + 4096), "unbound parameter"), ((pose, hm, kp), "unbound parameter")]
            for args, word in cases:
                rc = fn(*args)
                msg = lib.egotap_last_error().decode()
                assert rc == 1 and msg.startswith(name + ":") and word in msg, (name, args, rc, msg)
    finally:
        lib.egotap_destroy(h)


# joints in the reference's 1024-pixel frame, as fractions of the frame: (x, y, in view?)
_JOINTS = [(0.31, 0.42, True), (0.312, 0.421, True),          # two joints in one pixel (at sides 32, 64 and 128: 0.31 S and 0.312 S share an integer part)
           (0.001, 0.5, True), (0.999, 0.5, True), (0.5, 0.001, True), (0.5, 0.999, True),      # a peak on each of the four edges
           (0.0, 0.0, True), (0.9999, 0.9999, True),                                                # corners
           (0.77, 0.13, True),
           (1.2, 0.5, False), (0.5, 1.3, False), (-0.3, 0.5, False), (0.5, -0.4, False), (1.0, 0.5, False)]      # out of view: the reference renders nothing


@pytest.mark.parametrize("S", [32, 64, 128])
def test_round_trip_against_the_reference_rendering(S):
    coords = np.array([(fx * 1024.0, fy * 1024.0) for fx, fy, _ in _JOINTS], dtype=np.float64)
    hm = R.coord2d_to_heatmap(coords, res=S)                                  # [n, S, S] float32
    rec = spec.heatmap_peaks_ref(hm[None])[0]
    seen = {}
    for i, (fx, fy, inside) in enumerate(_JOINTS):
        x, y = coords[i] / 1024.0 * S
        px, py, score, index = (rec[i, k] for k in range(4))
        if not inside:
            assert not hm[i].any() and score == 0 and index == 0, (i, rec[i])
            continue
        ix, iy = int(x), int(y)
        assert index == iy * S + ix, (i, rec[i], ix, iy)
        assert score.tobytes() == hm[i].max().tobytes() and score > 0.9
        # half a pixel plus at most a quarter; no neighbour on one side: no step on that axis
        assert abs(px - (ix + 0.5)) <= 0.25 and abs(py - (iy + 0.5)) <= 0.25
        if ix in (0, S - 1):
            assert px == ix + 0.5
        if iy in (0, S - 1):
            assert py == iy + 0.5
        assert abs(px - x) <= 0.75 and abs(py - y) <= 0.75
        seen.setdefault(int(index), []).append(i)
    assert [0, 1] in seen.values()                                            # the two joints of one pixel read out the same record
    assert np.array_equal(rec[0], rec[1])
    edges = {(int(c[0] / 1024.0 * S), int(c[1] / 1024.0 * S)) for c, j in zip(coords, _JOINTS) if j[2]}
    assert {(0, S // 2), (S - 1, S // 2), (S // 2, 0), (S // 2, S - 1), (0, 0), (S - 1, S - 1)} <= edges


def test_the_definition_ties_nans_and_negative_maps():
    S = 16
    h = np.zeros((1, 6, S, S), dtype=np.float32)
    h[0, 0, 3, 5] = h[0, 0, 9, 2] = 2.0                                      # equal maxima: the first in scan order
    h[0, 1] = -3.0
    h[0, 1, 7, 7] = -1.0                                                      # all negative
    h[0, 2] = np.nan                                                          # only NaNs
    h[0, 3, 4, 4], h[0, 3, 4, 5], h[0, 3, 0, 0] = 1.0, np.nan, np.nan        # a NaN never wins, and a NaN neighbour gives no step
    h[0, 4, 6, 6], h[0, 4, 6, 7], h[0, 4, 5, 6] = 1.0, 0.5, 0.25             # steps towards the higher neighbours
    h[0, 5, 2, 3] = np.inf
    r = spec.heatmap_peaks_ref(h)[0]
    assert r[0].tolist() == [5.5, 3.5, 2.0, 3 * S + 5]
    assert r[1].tolist() == [7.5, 7.5, -1.0, 7 * S + 7]
    assert r[2, 3] == 0 and np.isnan(r[2, 2]) and r[2, 0] == 0.5 and r[2, 1] == 0.5
    assert r[3].tolist() == [4.5, 4.5, 1.0, 4 * S + 4]
    assert r[4].tolist() == [6.75, 6.25, 1.0, 6 * S + 6]
    assert r[5].tolist() == [3.5, 2.5, np.inf, 2 * S + 3]
    # the affine is ONE rounding: a case where float64 multiply-add rounded to float32 differs from the fused result
    a = spec._fma_f32(np.array([1 + 2.0 ** -23], np.float32), np.array([1 - 2.0 ** -23], np.float32), np.array([2.0 ** 24 + 2], np.float32))
    assert a[0] == 2.0 ** 24 + 2
    g = spec.heatmap_peaks_ref(h, groups=2, affine=[(4, 0, 4, 0), (-4.6875, 310, 3.125, 20)])[0]
    assert g[0].tolist() == [22.0, 14.0, 2.0, 3 * S + 5] and g[4].tolist() == [310 - 4.6875 * 6.75, 20 + 3.125 * 6.25, 1.0, 6 * S + 6]


@pytest.mark.parametrize("mirror", [False, True])
def test_sensor_affine_inverts_the_resize_map(mirror):
    """Joints at known sensor coordinates, seen through a crop that is neither square nor at the origin, rendered at side S and read out with the
    affine: within half a heatmap pixel of quantisation plus the quarter-pixel step, 0.75 w / S and 0.75 h / S sensor pixels.  With the eye
    mirrored the rendered x is flipped.  The direction itself is taken from spec.resize_u8: a bright patch of the sensor frame is resized, and
    the affine maps the place where it lands back onto the patch."""
    S, (x0, y0, w, h) = 64, (70, 30, 300, 200)
    rect = (x0, y0, w, h)
    rng = np.random.default_rng(5)
    truth = np.stack([x0 + rng.uniform(0, w, 12), y0 + rng.uniform(0, h, 12)], axis=1)
    u = (truth[:, 0] - x0) / w * S
    v = (truth[:, 1] - y0) / h * S
    if mirror:
        u = S - u
    hm = R.coord2d_to_heatmap(np.stack([u, v], axis=1) / S * 1024.0, res=S)
    aff = spec.sensor_keypoint_affine(rect, mirror, S)
    assert all(isinstance(t, np.float32) for t in aff)
    rec = spec.heatmap_peaks_ref(hm[None], groups=1, affine=[aff])[0]
    assert (rec[:, 2] > 0.9).all()
    assert (np.abs(rec[:, 0] - truth[:, 0]) <= 0.75 * w / S).all(), np.abs(rec[:, 0] - truth[:, 0]).max()
    assert (np.abs(rec[:, 1] - truth[:, 1]) <= 0.75 * h / S).all(), np.abs(rec[:, 1] - truth[:, 1]).max()
    # the direction, from the resize: a patch left of the crop's centre lands right of the output's centre exactly when the eye is mirrored
    S0, (X, Y), r = 4 * S, (x0 + 40, y0 + 150), 2
    frame = np.zeros((1, 260, 400, 3), dtype=np.uint8)
    frame[0, Y - r:Y + r + 1, X - r:X + r + 1] = 255
    out = spec.resize_u8(frame, rect, mirror, S0)[0, :, :, 0].astype(np.float64)
    assert out.sum() > 0
    cu = (out.sum(axis=0) * (np.arange(S0) + 0.5)).sum() / out.sum()           # the patch's centre in output pixels (centres at i + 0.5)
    cv = (out.sum(axis=1) * (np.arange(S0) + 0.5)).sum() / out.sum()
    bx = float(aff[0]) * (cu / 4) + float(aff[1])
    by = float(aff[2]) * (cv / 4) + float(aff[3])
    # one output pixel of the resize (w / S0, h / S0 sensor pixels) bounds what two-tap sampling of a symmetric patch can move its centre
    assert abs(bx - (X + 0.5)) <= w / S0 and abs(by - (Y + 0.5)) <= h / S0, (bx, by)
    assert (cu > S0 / 2) == mirror
