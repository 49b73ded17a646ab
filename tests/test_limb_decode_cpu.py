"""CPU-side checks of the limb-decode feature (egotap.h: egotap_limb_decode and the three _kpl serving entries): the exports, every host-side
refusal (fake pointers: nothing is launched), the definition itself -- spec.limb_decode_ref -- on hand cases and on the reference's own target maps,
and that the inputs of tests/test_gpu_limb_decode.py stay inside the conditioning gates' caps."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import limb_decode_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from egotap_amd.synthetic import synth_input
from oracle import heatmap_synth_ref as R

NEW = ("egotap_limb_decode", "egotap_predict_pose_rgb_kpl", "egotap_predict_pose_rgb_u8_kpl", "egotap_predict_pose_sensor_u8_kpl")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "heatmap_synth.npz"))


def test_the_new_entries_are_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name) and f"int {name}(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2


def test_limb_decode_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    ok = dict(hm=P(0x10000), dtype=L.F32, B=3, S=64, stride=92 * 4096, c0=30, n=15, eyes=2, affine=None, limbs=P(0x20000))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_limb_decode(a["hm"], a["dtype"], a["B"], a["S"], a["stride"], a["c0"], a["n"], a["eyes"], a["affine"], a["limbs"], None)
        return rc, lib.egotap_last_error().decode()
    cases = [(dict(hm=None), "null"), (dict(limbs=None), "null"), (dict(B=0), "must be positive"), (dict(n=0), "must be positive"),
             (dict(eyes=0), "eyes must be"), (dict(eyes=33, stride=1 << 30), "eyes must be"), (dict(c0=-1), "negative first channel"),
             (dict(stride=90 * 4096 - 4), "image_stride"), (dict(c0=33), "image_stride"), (dict(eyes=3), "image_stride"), (dict(n=16), "image_stride"),
             (dict(S=60), "multiple of 16"), (dict(S=8), "multiple of 16"), (dict(S=144, stride=92 * 144 * 144), "multiple of 16"),
             (dict(hm=P(0x10004)), "16-byte aligned"), (dict(limbs=P(0x20008)), "16-byte aligned"),
             (dict(dtype=L.I64), "unknown dtype"), (dict(dtype=7), "unknown dtype"),
             (dict(dtype=L.BF16, stride=92 * 4096 + 4), "multiple of 16 bytes"), (dict(stride=92 * 4096 + 2), "multiple of 16 bytes")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_limb_decode:") and word in msg, (kw, rc, msg)


def test_the_python_face_checks_its_arguments_before_it_asks_for_a_gpu():
    hm = torch.zeros((2, 62, 16, 16))
    cases = [(dict(hm=np.zeros((2, 62, 16, 16), np.float32)), L.EgotapError, "torch tensor"),
             (dict(hm=hm.double()), L.EgotapError, "float32 or bfloat16"), (dict(hm=hm[0]), ValueError, "[B, C, S, S]"),
             (dict(hm=torch.zeros((2, 62, 16, 32))), ValueError, "[B, C, S, S]"), (dict(c0=-1), ValueError, "not inside"), (dict(c0=3), ValueError, "not inside"),
             (dict(n_limbs=0), ValueError, "not inside"), (dict(eyes=3), ValueError, "not inside"), (dict(eyes=0), ValueError, "not inside"),
             (dict(hm=hm.permute(0, 1, 3, 2)), L.EgotapError, "contiguous per image"), (dict(hm=hm[:, ::2], n_limbs=7), L.EgotapError, "contiguous per image"),
             (dict(affine=[(1, 0, 1, 0)]), ValueError, "[eyes, 4]"), (dict(), L.EgotapError, "on the GPU only")]
    for kw, exc, word in cases:
        a = dict(dict(hm=hm, c0=2, n_limbs=15, eyes=2, affine=None), **kw)
        with pytest.raises(exc) as e:
            L.limb_decode(a["hm"], a["c0"], a["n_limbs"], a["eyes"], a["affine"])
        assert "limb_decode" in str(e.value) and word in str(e.value), (kw, str(e.value))


def _cfg():
    return L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, 64, 128, 1024, 8, 3, 16, 512)


def test_kpl_entries_refuse_their_extra_outputs_before_any_launch():
    """the handle has nothing bound: a call that passes the output checks ends at 'unbound parameter', still before any launch"""
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.egotap_create(C.byref(_cfg()), C.byref(h)))
    P = C.c_void_p
    B, J, S = 2, 15, 64
    left, right, table, ws = P(0x100000), P(0x200000), P(0x300000), P(0x1000000)
    pose, hm, kp, lb = 0x400000, 0x500000, 0x4000000, 0x5000000
    pose_bytes, hm_bytes, kp_bytes, lb_bytes = B * 16 * 3 * 4, B * 6 * J * S * S * 4, B * 2 * J * 16, B * 2 * J * 32
    rects, flags = (C.c_int * 8)(10, 20, 300, 200, 10, 20, 300, 200), (C.c_int * 2)(0, 1)
    entries = {
        "egotap_predict_pose_rgb_kpl": lambda po, hmo, k, l: lib.egotap_predict_pose_rgb_kpl(h, left, right, B, P(po), P(hmo), 0, ws, 1 << 40, None, P(k), P(l)),
        "egotap_predict_pose_rgb_u8_kpl": lambda po, hmo, k, l: lib.egotap_predict_pose_rgb_u8_kpl(h, left, right, B, table, P(po), P(hmo), 0, ws, 1 << 40, None,
                                                                                               P(k), P(l)),
        "egotap_predict_pose_sensor_u8_kpl": lambda po, hmo, k, l: lib.egotap_predict_pose_sensor_u8_kpl(h, left, right, B, 480, 640, rects, flags, table, P(po),
                                                                                                     P(hmo), 0, ws, 1 << 40, None, P(k), P(l)),
    }
    try:
        for name, fn in entries.items():
            cases = [((pose, hm, kp, lb + 8), "limbs must be 16-byte aligned"), ((pose, hm, kp + 8, lb), "keypoints must be 16-byte aligned"),
                     ((pose, hm, pose, lb), "keypoints overlaps"),
                     ((pose, hm, kp, pose), "limbs overlaps"), ((pose, hm, kp, pose + pose_bytes - 16), "limbs overlaps"),
                     ((pose, hm, kp, pose - lb_bytes + 16), "limbs overlaps"), ((pose, hm, kp, hm + hm_bytes - 16), "limbs overlaps"),
                     ((pose, hm, kp, hm + 4096), "limbs overlaps"), ((pose, hm, kp, kp), "limbs overlaps"), ((pose, hm, kp, kp + kp_bytes - 16), "limbs overlaps"),
                     ((pose, hm, kp, kp - lb_bytes + 16), "limbs overlaps"),
                     # directly behind / in front of another output is no overlap; an output that is not asked for has no extent; either extra
                     # output may be NULL, and with both NULL the call is the parent
                     ((pose, hm, kp, kp + kp_bytes), "unbound parameter"), ((pose, hm, kp, kp - lb_bytes), "unbound parameter"),
                     ((pose, hm, kp, pose + pose_bytes), "unbound parameter"), ((pose, None, kp, hm + 4096), "unbound parameter"),
                     ((pose, hm, None, kp), "unbound parameter"), ((pose, hm, kp, None), "unbound parameter"), ((pose, hm, None, None), "unbound parameter"),
                     ((pose, hm, kp, lb), "unbound parameter")]
            for args, word in cases:
                rc = fn(*args)
                msg = lib.egotap_last_error().decode()
                assert rc == 1 and msg.startswith(name + ":") and word in msg, (name, args, rc, msg)
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ the definition, by hand
def _pair(S, pixels):
    """[1, 2, S, S]: one eye, one limb; pixels: (ix, iy, c, s)"""
    h = np.zeros((1, 2, S, S), dtype=np.float32)
    for ix, iy, c, s in pixels:
        h[0, 0, iy, ix], h[0, 1, iy, ix] = c, s
    return h


def test_an_all_zero_pair_and_a_nan_pixel_give_the_empty_record():
    S = 32
    r = spec.limb_decode_ref(_pair(S, []), 0, 1, 1)[0, 0, 0]
    assert r.tolist() == [0, 0, S / 2, S / 2, 0, 0, 0, 0]
    aff = spec.sensor_keypoint_affine((70, 30, 320, 320), True, S)                 # a mirrored sensor eye: x = 70 + 320 - 10 x
    r = spec.limb_decode_ref(_pair(S, []), 0, 1, 1, affine=[aff])[0, 0, 0]
    assert r.tolist() == [0, 0, 70 + 320 - 10 * S / 2, 30 + 10 * S / 2, 0, 0, 0, 0]
    for bad in (np.nan, np.inf):
        r = spec.limb_decode_ref(_pair(S, [(3, 4, 1.0, 2.0), (9, 9, bad, 0.0)]), 0, 1, 1)[0, 0, 0]
        assert r[[0, 1, 4, 5]].tolist() == [0, 0, 0, 0] and r[2] == S / 2 and r[3] == S / 2
        assert (np.isnan(r[7]) if np.isnan(bad) else r[7] == np.inf)
        assert r[6] == (np.float32(math.sqrt(5.0)) if np.isnan(bad) else np.inf)    # the peak as computed: a NaN never wins


def test_a_single_pixel():
    S, ix, iy = 16, 11, 4
    r = spec.limb_decode_ref(_pair(S, [(ix, iy, 3.0, 4.0)]), 0, 1, 1)[0, 0, 0]
    assert r[0] == np.float32(math.atan2(4, 3)) and r[1] == 1 and r[2] == ix + 0.5 and r[3] == iy + 0.5
    assert abs(r[5]) <= 1e-5 and r[6] == 5 and r[7] == 5                            # (phi: the orientation of a round mass is not defined)


def test_runs_and_the_mirror():
    S, k = 32, 7
    runs = {"h": [(5 + i, 9, 0.5, -1.0) for i in range(k)], "v": [(9, 5 + i, 0.5, -1.0) for i in range(k)], "d": [(5 + i, 8 + i, 0.5, -1.0) for i in range(k)]}
    rec = {name: spec.limb_decode_ref(_pair(S, px), 0, 1, 1)[0, 0, 0].astype(np.float64) for name, px in runs.items()}
    for name, (phi, l2, x, y) in {"h": (0.0, k * k - 1, 5 + k / 2, 9.5), "v": (math.pi / 2, k * k - 1, 9.5, 5 + k / 2),
                                  "d": (math.pi / 4, 2 * (k * k - 1), 5 + k / 2, 8 + k / 2)}.items():
        r = rec[name]
        assert abs(r[4] - phi) <= 1e-6, (name, r)
        assert abs(r[5] ** 2 - l2) <= 1e-5 * l2, (name, r)                          # the discrete uniform variance (k^2 - 1) / 12 along the run
        assert r[0] == np.float32(math.atan2(-1.0, 0.5)) and abs(r[1] - 1) <= 1e-7 and r[2] == x and r[3] == y
    # under ax < 0 the diagonal flips, the vertical run stays at +pi/2 (the range is (-pi/2, pi/2]), theta does not move
    for aff in ([(-1.0, float(S), 1.0, 0.0)], [spec.sensor_keypoint_affine((0, 0, S, S), True, S)]):
        r = spec.limb_decode_ref(_pair(S, runs["d"]), 0, 1, 1, affine=aff)[0, 0, 0].astype(np.float64)
        assert abs(r[4] + math.pi / 4) <= 1e-6 and r[2] == S - (5 + k / 2) and r[0] == np.float32(math.atan2(-1.0, 0.5))
        r = spec.limb_decode_ref(_pair(S, runs["v"]), 0, 1, 1, affine=aff)[0, 0, 0].astype(np.float64)
        assert abs(r[4] - math.pi / 2) <= 1e-6
    # a scale: the segment in output units
    r = spec.limb_decode_ref(_pair(S, runs["d"]), 0, 1, 1, affine=[(4.0, 0.0, 4.0, 0.0)])[0, 0, 0].astype(np.float64)
    assert abs(r[5] ** 2 - 16 * 2 * (k * k - 1)) <= 1e-3 and abs(r[4] - math.pi / 4) <= 1e-6


@pytest.mark.parametrize("mirror", [False, True])
def test_the_mirror_direction_is_the_resize_s(mirror):
    """a diagonal that descends to the right in the sensor frame, seen through spec.resize_u8 with and without the mirror, decoded with
    spec.sensor_keypoint_affine: the segment comes back where and how it lies in the SENSOR frame either way"""
    S, rect = 64, (40, 20, 256, 256)
    frame = np.zeros((1, 300, 340, 3), dtype=np.uint8)
    for i in range(120):
        frame[0, 60 + i - 2:60 + i + 3, 90 + i - 2:90 + i + 3] = 255                # from (90, 60) to (210, 180): phi = +pi/4 in sensor pixels
    seen = spec.resize_u8(frame, rect, mirror, 4 * S)[0, :, :, 0].astype(np.float32).reshape(S, 4, S, 4).mean(axis=(1, 3)) / 255
    hm = np.stack([seen * 0.6, seen * 0.8])[None]
    r = spec.limb_decode_ref(hm, 0, 1, 1, affine=[spec.sensor_keypoint_affine(rect, mirror, S)])[0, 0, 0].astype(np.float64)
    plain = spec.limb_decode_ref(hm, 0, 1, 1)[0, 0, 0].astype(np.float64)
    assert abs(r[4] - math.pi / 4) <= 0.02 and abs(plain[4] - (-1 if mirror else 1) * math.pi / 4) <= 0.02, (r, plain)
    assert abs(r[2] - 150) <= 1.0 and abs(r[3] - 120) <= 1.0 and abs(r[0] - math.atan2(0.8, 0.6)) <= 1e-6, r
    assert abs(r[5] - 120 * math.sqrt(2)) <= 4.0, r                                 # (the 5-pixel square brush adds its own extent)


# ------------------------------------------------------------------------------------------------------------ the reference's own targets
def _fixture_joints(preset, n):
    p2l = synth_input(f"synth_p2l_{preset}", (3, n, 2), -60.0, 1080.0).astype(np.float64)
    p2r = synth_input(f"synth_p2r_{preset}", (3, n, 2), -60.0, 1080.0).astype(np.float64)
    p2l[0, 1] = [512.0, 256.0]
    p2l[0, 2] = [-100.0, 500.0]
    p3 = synth_input(f"synth_p3_{preset}", (3, n, 3), -40.0, 40.0).astype(np.float64)
    return p2l, p2r, p3


@pytest.mark.parametrize("preset,n", [("UnrealEgo", 16), ("EgoCap", 18)])
@pytest.mark.parametrize("res", [16, 48, 64, 128])
def test_round_trip_on_the_reference_targets(preset, n, res):
    """theta is exact in real arithmetic (the maps are fp32 products, relative error about 2^-24 each): 1e-5 rad against the fixture's theta, coherence
    >= 1 - 1e-6; a limb out of view gives the empty record (sides 16 and 48 have one; theta does not depend on the side, so they are held against the
    fixture's theta of side 64).  How far (x, y) lies from the drawn segment's midpoint and length from its pixel length is
    MEASURED and printed, not asserted (the anti-aliased line is not symmetric; clipped limbs lose part of their segment): DESIGN 3.21 has the maxima."""
    p2l, p2r, p3 = _fixture_joints(preset, n)
    J, par = n - 1, R.KINEMATIC_PARENTS[preset]
    seen = empty = 0
    dmid = dlen = dmid_in = dlen_in = 0.0
    for b in range(3):
        cat, _, theta = R.process_frame(p2l[b], p2r[b], p3[b], preset, res)
        theta = GOLD[f"{preset}_{res if res in (64, 128) else 64}_{b}_theta"]
        rec = spec.limb_decode_ref(cat[None], 2 * J, J, 2)[0]
        for eye, pts in enumerate((p2l[b], p2r[b])):
            for l in range(J):
                r = rec[eye, l]
                if not (cat[2 * J + eye * 2 * J + l].any() or cat[2 * J + eye * 2 * J + J + l].any()):
                    assert r.tolist() == [0, 0, res / 2, res / 2, 0, 0, 0, 0]
                    empty += 1
                    continue
                seen += 1
                assert abs(float(r[0]) - float(theta[l])) <= 1e-5, (b, eye, l, r, theta[l])
                assert r[1] >= 1 - 1e-6 and r[1] <= 1 + 1e-6 and r[6] > 0 and r[7] > 0
                pi, ci = np.rint(pts[par[l + 1]] * res / 1024.0), np.rint(pts[l + 1] * res / 1024.0)      # the pixels the line is drawn between
                mid = (pi + ci) / 2 + 0.5
                d1, d2 = math.hypot(r[2] - mid[0], r[3] - mid[1]), abs(float(r[5]) - float(np.linalg.norm(pi - ci)))
                dmid, dlen = max(dmid, d1), max(dlen, d2)
                if all(0 <= v <= res - 1 for v in (*pi, *ci)):
                    dmid_in, dlen_in = max(dmid_in, d1), max(dlen_in, d2)
    print(f"{preset} {res}: {seen} limbs seen, {empty} empty; |(x, y) - midpoint| <= {dmid:.3f} px, |length - pixel length| <= {dlen:.3f} px; "
          f"both ends inside the map: {dmid_in:.3f} px, {dlen_in:.3f} px")
    assert seen > 0 and seen + empty == 3 * 2 * J and (preset != "UnrealEgo" or res > 48 or empty > 0)


# ------------------------------------------------------------------------------------------------------------ the GPU test's inputs
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("J", [15, 17])
@pytest.mark.parametrize("S", [16, 48, 64, 128])
def test_the_gpu_tests_inputs_stay_inside_the_gates_caps(S, J, bf16):
    """with the reference definition alone: the conditioning gates exclude nothing on the target, single-mass and run inputs (a single mass has no
    orientation: only its theta gate is meant) and at most 5 % of the noisy records, for the seeds tests/limb_decode_inputs.py fixes"""
    for affine in (None, I.MIRROR):
        want = I.reference(J, S, bf16, affine)
        I.check_gates(I.excluded(want, J, affine))
        cat = I.category(J)
        empty = ~((want[..., 7] > 0) & np.isfinite(want[..., 7]))
        assert empty[np.isin(cat, I.EMPTY)].all() and not empty[cat == "target"].all()
        I.compare(want, want, J, affine, out=lambda s: None)                        # the comparison accepts the reference itself
