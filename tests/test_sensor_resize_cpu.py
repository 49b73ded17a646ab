"""Host side of the sensor entries (egotap_rgb_u8_resize, egotap_predict_pose_sensor_u8) and of the integer arithmetic they compute
(spec.resize_taps, spec.resize_u8): gated against float64 bilinear interpolation by the DERIVED bound 0.5 + 510 / 4096 (+ 1e-6), pinned against the
reference's own crop_resize_images within one byte, exported, declared, sized and refusing by name -- no kernel is launched here (every refusal
comes before the first launch; the pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from egotap_amd import lib as L
from egotap_amd import spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
GATE = 0.5 + 510.0 / 4096.0 + 1e-6          # = 0.6246: each weight is off by at most 2^-12 per axis (2 * 255 / 4096), the one rounding adds 0.5
NEW = ("egotap_rgb_u8_resize", "egotap_predict_pose_sensor_u8", "egotap_predict_pose_sensor_u8_workspace_bytes")


def _frames(seed, n, H, W):
    """random bytes with 0 and 255 present and a two-pixel border of 255 (so an edge that is clamped or wrapped wrongly moves the result)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    x[:, H // 2, W // 2, :] = 0
    x[:, H // 3, W // 3, :] = 255
    for sl in (slice(0, 2), slice(-2, None)):
        x[:, sl, :, :] = 255
        x[:, :, sl, :] = 255
    return x


def _exact(x, rect, S0):
    """float64 bilinear interpolation of the cropped frame, NHWC: the issue's reference expression"""
    x0, y0, w, h = rect
    crop = x[:, y0:y0 + h, x0:x0 + w, :].permute(0, 3, 1, 2).double()
    return F.interpolate(crop, size=(S0, S0), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------ 1. the arithmetic
@pytest.mark.parametrize("L_,S0", [(37, 64), (53, 64), (48, 64), (64, 64), (120, 64), (640, 256), (1024, 256), (1, 64), (2, 8)])
def test_taps_are_the_stated_integers_and_near_the_real_weights(L_, S0):
    i0, i1, w1 = spec.resize_taps(L_, S0)
    assert i0.dtype == np.int64 and i0.shape == (S0,)
    for X in range(S0):                                          # the stated expression, in Python integers
        n = max((2 * X + 1) * L_ - S0, 0)
        a, r = divmod(n, 2 * S0)
        assert (i0[X], i1[X], w1[X]) == (a, min(a + 1, L_ - 1), (r * 2048 + S0) // (2 * S0))
    assert i0.min() >= 0 and i1.max() <= L_ - 1 and w1.min() >= 0 and w1.max() <= 2048
    src = np.maximum((np.arange(S0) + 0.5) * L_ / S0 - 0.5, 0.0)          # align_corners=False
    assert np.array_equal(i0, np.floor(src).astype(np.int64))
    assert np.abs(w1 / 2048.0 - (src - np.floor(src))).max() <= 2.0 ** -12 + 1e-12
    if L_ == S0:
        assert np.array_equal(i0, np.arange(S0)) and not w1.any()        # an exact copy


CASES = [((37, 53), 64, None), ((37, 53), 256, None), ((96, 120), 64, None), ((96, 120), 256, (11, 0, 109, 96)),
         ((512, 640), 64, (64, 0, 512, 512)), ((512, 640), 256, None), ((1024, 1024), 64, None), ((1024, 1024), 256, None),
         ((96, 120), 64, (0, 0, 48, 48)),                               # an upscale, 48 -> 64, touching the top-left corner
         ((96, 120), 64, (72, 48, 48, 48)),                             # ... and the bottom-right corner
         ((37, 53), 64, (0, 5, 1, 30)), ((37, 53), 64, (52, 0, 1, 37)),  # one pixel wide, on the left and on the right edge
         ((37, 53), 64, (3, 36, 40, 1))]                                 # one pixel high, on the bottom edge


@pytest.mark.parametrize("hw,S0,rect", CASES)
def test_integer_resize_is_within_the_derived_bound_of_float64_bilinear(hw, S0, rect):
    H, W = hw
    x = _frames(H * 1000 + W + S0, 2 if H <= 512 else 1, H, W)
    r = spec.check_resize_rect("test", rect, H, W)
    got = spec.resize_u8(x, rect, False, S0)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], S0, S0, 3)
    err = float((got.double() - _exact(x, r, S0)).abs().max())
    print(f"{hw} -> {S0} rect {r}: max |byte - E| = {err:.4f} (gate {GATE:.4f})")
    assert err <= GATE, err
    mirrored = spec.resize_u8(x, rect, True, S0)
    assert torch.equal(mirrored, got.flip(-2))                   # the mirror is flip(-2) of the unmirrored result, bit for bit
    as_np = spec.resize_u8(x.numpy(), rect, False, S0)            # the numpy face gives the same bytes
    assert isinstance(as_np, np.ndarray) and np.array_equal(as_np, got.numpy())


def test_identity_is_an_exact_copy_and_mirror_of_flip_then_crop():
    x = _frames(5, 2, 64, 64)
    assert torch.equal(spec.resize_u8(x, None, False, 64), x)
    assert torch.equal(spec.resize_u8(x, (0, 0, 64, 64), True, 64), x.flip(2))
    big = _frames(6, 1, 96, 120)
    assert torch.equal(spec.resize_u8(big, (56, 32, 64, 64), False, 64), big[:, 32:96, 56:120])
    # the reference flips the frame, then crops at x0' (flipped coordinates): x0 = W - x0' - w here, with the mirror flag
    x0f, w = 7, 80
    ref_way = spec.resize_u8(big.flip(2).contiguous(), (x0f, 3, w, 90), False, 64)
    assert torch.equal(spec.resize_u8(big, (120 - x0f - w, 3, w, 90), True, 64), ref_way)


def test_rectangles_are_checked_by_name():
    assert spec.check_resize_rect("who", None, 37, 53) == (0, 0, 53, 37)
    for bad in ((0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (50, 0, 4, 5), (0, 33, 5, 5), (0, 0, 54, 37)):
        with pytest.raises(ValueError, match="who: rectangle .* empty or outside the 37 x 53 frame"):
            spec.check_resize_rect("who", bad, 37, 53)
    with pytest.raises(ValueError, match=r"\(x0, y0, w, h\)"):
        spec.check_resize_rect("who", (1, 2, 3), 37, 53)
    with pytest.raises(ValueError, match="uint8"):
        spec.resize_u8(torch.zeros(1, 8, 8, 3), None, False, 4)


# ------------------------------------------------------------------------------------------------------------ 2. the reference pin
def _golden_input():
    """the fixture's input, regenerated from its seed (tools/make_golden.py gen_sensor_resize): uint8 [1, 512, 640, 3]"""
    g = torch.Generator().manual_seed(20261018)
    return torch.randint(0, 256, (1, 512, 640, 3), generator=g, dtype=torch.uint8)


def test_reference_crop_resize_is_within_one_byte():
    """tests/golden/sensor_resize_ref.npz holds only the OUTPUT bytes of the reference's crop_resize_images(do_crop=False) on the seeded 512 x 640
    frame (its uint8 F.interpolate is a two-pass fixed-point scheme: bit-equality with it is not the goal).  The reference must stay within 1.0 of
    float64 on this frame (asserted when the fixture is made and here); with the derived bound that puts every byte within 1 of ours."""
    gold = np.load(os.path.join(REPO, "tests", "golden", "sensor_resize_ref.npz"))
    ref = torch.from_numpy(gold["out"])                          # uint8 [1, 3, 256, 256], the reference's layout
    assert ref.dtype == torch.uint8 and tuple(ref.shape) == (1, 3, 256, 256)
    x = _golden_input()
    ref = ref.permute(0, 2, 3, 1)
    exact = _exact(x, (0, 0, 640, 512), 256)
    ref_err = float((ref.double() - exact).abs().max())
    assert ref_err <= 1.0, ref_err
    ours = spec.resize_u8(x, None, False, 256)
    diff = (ours.to(torch.int16) - ref.to(torch.int16)).abs()
    print(f"reference vs float64: {ref_err:.4f}; ours vs reference: max {int(diff.max())}, bytes that differ {int((diff != 0).sum())} of {diff.numel()}")
    assert int(diff.max()) <= 1


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


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def _handle(bind=(L.NET_LIFT, L.NET_HM_POS, L.NET_HM_ROT), hm=64):
    lib = L.load()
    cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, hm, 128, 1024, 8, 3, 16, 512)
    h = C.c_void_p()
    assert lib.egotap_create(C.byref(cfg), C.byref(h)) == 0
    fake = C.c_void_p(0x100000)
    specs = {L.NET_LIFT: [(k, s) for k, s in spec.lift_state_spec(spec.lift_preset("UnrealEgo", hm))],
             L.NET_HM_POS: [(k, s) for k, s, _ in spec.hm_state_spec(15)], L.NET_HM_ROT: [(k, s) for k, s, _ in spec.hm_state_spec(30)]}
    for net in bind:
        for key, shape in specs[net]:
            dt = L.I64 if key.endswith("num_batches_tracked") else L.F32
            assert lib.egotap_bind_param(h, net, key.encode(), fake, int(np.prod(shape, dtype=np.int64)), dt) == 0, key
    return lib, h


def _refused(lib, f, who, *args, word):
    assert f(*args) == INVALID, args
    msg = lib.egotap_last_error()
    assert who in msg and word in msg, msg


def _ints(*v):
    return (C.c_int * len(v))(*v)


BAD_RECTS = [((0, 0, 0, 10), b"empty source rectangle"), ((0, 0, 10, 0), b"empty source rectangle"), ((0, 0, 10, -3), b"empty source rectangle"),
             ((-1, 0, 10, 10), b"outside the frame"), ((0, -1, 10, 10), b"outside the frame"), ((44, 0, 10, 10), b"outside the frame"),
             ((0, 28, 10, 10), b"outside the frame"), ((0, 0, 54, 37), b"outside the frame"), ((0, 0, 53, 38), b"outside the frame")]


def test_operator_refusals():
    lib = L.load()
    f, who = lib.egotap_rgb_u8_resize, b"egotap_rgb_u8_resize"
    l8, r8, ol, orr = (C.c_void_p(a) for a in (0x200001, 0x300003, 0x500000, 0x600000))          # the SOURCE may sit at any address
    full = _ints(0, 0, 53, 37)
    _refused(lib, f, who, l8, r8, 0, 37, 53, full, full, 0, 0, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, l8, r8, -2, 37, 53, full, full, 0, 0, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, None, r8, 2, 37, 53, full, full, 0, 0, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, None, 2, 37, 53, full, full, 0, 0, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, r8, 2, 37, 53, None, full, 0, 0, 64, ol, orr, None, word=b"null rectangle")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, None, 0, 0, 64, ol, orr, None, word=b"null rectangle")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 64, None, orr, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 64, ol, None, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 64, C.c_void_p(0x500002), orr, None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 64, ol, C.c_void_p(0x600001), None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 62, ol, orr, None, word=b"multiple of 4")
    _refused(lib, f, who, l8, r8, 2, 37, 53, full, full, 0, 0, 0, ol, orr, None, word=b"multiple of 4")
    _refused(lib, f, who, l8, r8, 2, 0, 53, full, full, 0, 0, 64, ol, orr, None, word=b"height and width")
    _refused(lib, f, who, l8, r8, 2, 37, 20000, full, full, 0, 0, 64, ol, orr, None, word=b"height and width")
    for rect, word in BAD_RECTS:
        _refused(lib, f, who, l8, r8, 2, 37, 53, _ints(*rect), full, 0, 0, 64, ol, orr, None, word=word)
        _refused(lib, f, who, l8, r8, 2, 37, 53, full, _ints(*rect), 1, 1, 64, ol, orr, None, word=word)


@pytest.mark.parametrize("hm", [64, 32])
def test_one_call_from_sensor_refusals(hm):
    lib, h = _handle(hm=hm)
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 37, 53, 0, C.byref(need)) == 0
        f, who = lib.egotap_predict_pose_sensor_u8, b"egotap_predict_pose_sensor_u8"
        l8, r8, tab, pose, hmp, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000))
        rects, mir = _ints(0, 0, 53, 37, 3, 4, 10, 10), _ints(0, 1)
        ok = (4, 37, 53, rects, mir, tab, pose, hmp, 0, ws, need.value, None)
        _refused(lib, f, who, None, l8, r8, *ok, word=b"null handle")
        _refused(lib, f, who, h, None, r8, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, None, *ok, word=b"null frames")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, None, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"null rectangles")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, None, tab, pose, hmp, 0, ws, need.value, None, word=b"mirror flags")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, None, pose, hmp, 0, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, None, hmp, 0, ws, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, hmp, 0, None, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 0, 37, 53, rects, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, -3, 37, 53, rects, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, hmp, -1, ws, need.value, None, word=b"chunk")
        _refused(lib, f, who, h, l8, r8, 4, 0, 53, rects, mir, tab, pose, hmp, 0, ws, need.value, None, word=b"height and width")
        for rect, word in BAD_RECTS:
            _refused(lib, f, who, h, l8, r8, 4, 37, 53, _ints(*rect, 0, 0, 53, 37), mir, tab, pose, hmp, 0, ws, need.value, None, word=word)
            _refused(lib, f, who, h, l8, r8, 4, 37, 53, _ints(0, 0, 53, 37, *rect), mir, tab, pose, hmp, 0, ws, need.value, None, word=word)
        _refused(lib, f, who, h, C.c_void_p(0x200001), r8, *ok, word=b"4-byte aligned")
        _refused(lib, f, who, h, l8, C.c_void_p(0x300002), *ok, word=b"4-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, C.c_void_p(0x400004), pose, hmp, 0, ws, need.value, None, word=b"16-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, C.c_void_p(0x600008), 0, ws, need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, hmp, 0, C.c_void_p(0x700010), need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, hmp, 0, ws, need.value - 1, None, word=b"workspace too small")
        # the byte entry's size is short by the slice, also for the identity request (which reads in place but keeps one sizing rule)
        u8 = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, 0, C.byref(u8)) == 0
        _refused(lib, f, who, h, l8, r8, 4, 37, 53, rects, mir, tab, pose, hmp, 0, ws, u8.value, None, word=b"workspace too small")
        S0 = 4 * hm
        _refused(lib, f, who, h, l8, r8, 4, S0, S0, _ints(0, 0, S0, S0, 0, 0, S0, S0), _ints(0, 0), tab, pose, hmp, 0, ws, u8.value, None, word=b"workspace too small")
        form = C.c_int(-1)
        assert lib.egotap_debug_predict_pose_rgb_form(h, C.byref(form)) == 0 and form.value == 0          # nothing ran
    finally:
        lib.egotap_destroy(h)


@pytest.mark.parametrize("missing,word", [(L.NET_LIFT, b"lifting head"), (L.NET_HM_POS, b"position estimator"), (L.NET_HM_ROT, b"limb estimator")])
def test_unbound_network_is_refused_by_key(missing, word):
    lib, h = _handle(bind=[n for n in (L.NET_LIFT, L.NET_HM_POS, L.NET_HM_ROT) if n != missing])
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 2, 37, 53, 0, C.byref(need)) == 0
        l8, r8, tab, pose, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x700000))
        assert lib.egotap_predict_pose_sensor_u8(h, l8, r8, 2, 37, 53, _ints(0, 0, 53, 37, 0, 0, 53, 37), _ints(0, 0), tab, pose, None, 0, ws, need.value, None) == INVALID
        msg = lib.egotap_last_error()
        assert b"egotap_predict_pose_sensor_u8" in msg and b"unbound parameter" in msg and word in msg and b"not bound" in msg, msg
    finally:
        lib.egotap_destroy(h)


@pytest.mark.parametrize("hm", [64, 128, 32])
def test_workspace_is_the_byte_entrys_plus_exactly_the_slice(hm):
    lib, h = _handle(bind=(), hm=hm)
    try:
        def q(fn, *a):
            v = C.c_size_t()
            assert fn(h, *a, C.byref(v)) == 0
            return v.value
        S0 = 4 * hm
        for B, chunk in ((1, 0), (3, 0), (3, 2), (37, 16), (300, 64), (5, 1000)):
            c = B if chunk == 0 or chunk > B else chunk
            for H, W in ((37, 53), (512, 640), (1024, 1024), (S0, S0)):          # the slice holds output frames: H and W do not enter
                assert q(lib.egotap_predict_pose_sensor_u8_workspace_bytes, B, H, W, chunk) == \
                    q(lib.egotap_predict_pose_rgb_u8_workspace_bytes, B, chunk) + c * 2 * 3 * S0 * S0
        bad = C.c_size_t()
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, -1, 37, 53, 0, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 37, 53, -1, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 0, 53, 0, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(h, 4, 37, 53, 0, None) == INVALID
        assert lib.egotap_predict_pose_sensor_u8_workspace_bytes(None, 4, 37, 53, 0, C.byref(bad)) == INVALID
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 5. the Python faces
def test_check_sensor_frames_wording():
    from egotap_amd import models
    from egotap_amd.options import preset_defaults
    cpu8 = torch.zeros(1, 37, 53, 3, dtype=torch.uint8)
    m = types.SimpleNamespace(opt=preset_defaults("UnrealEgo", 64), net_AutoEncoder=types.SimpleNamespace(preset=spec.lift_preset("UnrealEgo", 64)))
    m.predict_pose_from_sensor = types.MethodType(models.EgoTAPAutoEncoderModel.predict_pose_from_sensor, m)
    with pytest.raises(L.EgotapError, match="predict_pose_from_sensor runs on the GPU only"):
        m.predict_pose_from_sensor(cpu8, cpu8)
    with pytest.raises(L.EgotapError, match="rgb_u8_resize runs on the GPU only"):
        L.rgb_u8_resize(cpu8, cpu8, 64)

    class OnGpu(torch.Tensor):          # dtype and shape are looked at once the frames are on a GPU: a stand-in for "is on the GPU"
        is_cuda = True
    g = lambda t: t.as_subclass(OnGpu)      # noqa: E731
    who = "predict_pose_from_sensor"
    assert L.check_sensor_frames(who, g(cpu8), g(cpu8)) == (1, 37, 53)
    assert L.check_sensor_frames(who, g(torch.zeros(0, 8, 9, 3, dtype=torch.uint8)), g(torch.zeros(0, 8, 9, 3, dtype=torch.uint8))) == (0, 8, 9)
    with pytest.raises(L.EgotapError, match="dtype uint8"):
        L.check_sensor_frames(who, g(cpu8.float()), g(cpu8.float()))
    with pytest.raises(ValueError, match=r"expected left8 / right8 \[B, H, W, 3\]"):
        L.check_sensor_frames(who, g(torch.zeros(1, 3, 37, 53, dtype=torch.uint8)), g(torch.zeros(1, 3, 37, 53, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="one H and W for both eyes"):
        L.check_sensor_frames(who, g(cpu8), g(torch.zeros(1, 37, 54, 3, dtype=torch.uint8)))
    with pytest.raises(ValueError, match=r"expected left8 / right8 \[B, H, W, 3\]"):
        L.check_sensor_frames(who, g(torch.zeros(37, 53, 3, dtype=torch.uint8)), g(torch.zeros(37, 53, 3, dtype=torch.uint8)))
    with pytest.raises(L.EgotapError, match="contiguous"):
        nc = torch.zeros(1, 53, 37, 3, dtype=torch.uint8).permute(0, 2, 1, 3)
        L.check_sensor_frames(who, g(nc), g(nc))
    # the camera entry's checker is what it was: it still refuses any other shape by name
    with pytest.raises(ValueError, match=r"expected left8 / right8 \[B, 256, 256, 3\]"):
        L.check_camera_frames("predict_pose_from_camera", g(cpu8), g(cpu8), 256)
