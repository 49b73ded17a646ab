"""Host side of the camera-byte entries (egotap_rgb_u8_to_f32, egotap_hm_forward_u8, egotap_predict_pose_rgb_u8) and of the value table they
read: pinned against the reference's own arithmetic, exported, declared, sized and refusing by name -- no kernel is launched here (every refusal
comes before the first launch; the pointers below are never dereferenced)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
NEW = ("egotap_rgb_u8_to_f32", "egotap_hm_forward_u8", "egotap_hm_forward_u8_workspace_bytes", "egotap_predict_pose_rgb_u8",
       "egotap_predict_pose_rgb_u8_workspace_bytes")


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


# ------------------------------------------------------------------------------------------------------------ 1. the value table
def test_table_equals_the_reference_fixture_bit_for_bit():
    """tests/golden/rgb_u8_norm.npz is the reference's normalize_ImageNet on the 256 byte values / 255 per channel, .float() last
    (tools/make_golden.py --only rgb_u8)"""
    gold = np.load(os.path.join(REPO, "tests", "golden", "rgb_u8_norm.npz"))["table"]
    t = spec.rgb_u8_table()
    assert t.dtype == np.float32 and t.shape == (3, 256) and gold.dtype == np.float32 and gold.shape == (3, 256)
    assert np.array_equal(t.view(np.int32), gold.view(np.int32))
    assert np.array_equal(spec.rgb_u8_table(types.SimpleNamespace()).view(np.int32), gold.view(np.int32))      # an opt without overrides
    # the stated expression, per element, in Python floats (float64) around numpy's float32 division
    for c, v in ((0, 0), (1, 1), (2, 127), (0, 254), (2, 255)):
        x = float(np.float32(v) / np.float32(255))
        assert t[c, v] == np.float32((x - spec.RGB_MEAN[c]) / spec.RGB_STD[c])
    assert t[0, 0] < -2.0 and t[2, 255] > 2.6                   # byte 0 is NOT zero after normalisation: padding must not come from the table


def test_opt_overrides_move_the_table():
    base = spec.rgb_u8_table()
    opt = types.SimpleNamespace(rgb_mean=[0.5, 0.5, 0.5], rgb_std=[0.25, 0.5, 1.0])
    t = spec.rgb_u8_table(opt)
    assert not np.array_equal(t, base)
    x = (np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255)).astype(np.float64)
    for c, sd in enumerate((0.25, 0.5, 1.0)):
        assert np.array_equal(t[c], ((x - 0.5) / sd).astype(np.float32))
    only_mean = spec.rgb_u8_table(types.SimpleNamespace(rgb_mean=[0.0, 0.0, 0.0], rgb_std=None))
    assert np.array_equal(only_mean[1], (x / spec.RGB_STD[1]).astype(np.float32))
    with pytest.raises(ValueError):
        spec.rgb_u8_table(types.SimpleNamespace(rgb_mean=[0.5, 0.5], rgb_std=None))
    with pytest.raises(ValueError):
        spec.rgb_u8_table(types.SimpleNamespace(rgb_mean=None, rgb_std=[1.0, 0.0, 1.0]))


# ------------------------------------------------------------------------------------------------------------ 2. symbols
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


# ------------------------------------------------------------------------------------------------------------ 3. refusals
def _refused(lib, f, who, *args, word):
    assert f(*args) == INVALID, args
    msg = lib.egotap_last_error()
    assert who in msg and word in msg, msg


def test_converter_refusals():
    lib = L.load()
    f, who = lib.egotap_rgb_u8_to_f32, b"egotap_rgb_u8_to_f32"
    l8, r8, tab, lo, ro = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000))
    assert f(None, None, 0, 256, None, None, None, None) == 0                                  # batch 0: a no-op, nothing is looked at
    _refused(lib, f, who, l8, r8, -1, 256, tab, lo, ro, None, word=b"negative batch")
    _refused(lib, f, who, None, r8, 2, 256, tab, lo, ro, None, word=b"null frames")
    _refused(lib, f, who, l8, None, 2, 256, tab, lo, ro, None, word=b"null frames")
    _refused(lib, f, who, l8, r8, 2, 256, None, lo, ro, None, word=b"null table")
    _refused(lib, f, who, l8, r8, 2, 256, tab, None, ro, None, word=b"null output")
    _refused(lib, f, who, C.c_void_p(0x200001), r8, 2, 256, tab, lo, ro, None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, C.c_void_p(0x300002), 2, 256, tab, lo, ro, None, word=b"4-byte aligned")
    _refused(lib, f, who, l8, r8, 2, 256, tab, C.c_void_p(0x500008), ro, None, word=b"16-byte aligned")
    _refused(lib, f, who, l8, r8, 2, 254, tab, lo, ro, None, word=b"multiple of 4")


@pytest.mark.parametrize("hm", [64, 32])
def test_estimator_from_bytes_refusals(hm):
    lib, h = _handle(hm=hm)
    try:
        need = C.c_size_t()
        assert lib.egotap_hm_forward_u8_workspace_bytes(h, 4, C.byref(need)) == 0
        f, who = lib.egotap_hm_forward_u8, b"egotap_hm_forward_u8"
        l8, r8, tab, out, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000))
        stride = 30 * hm * hm
        _refused(lib, f, who, None, 1, l8, r8, 4, tab, out, stride, ws, need.value, None, word=b"null handle")
        _refused(lib, f, who, h, 0, l8, r8, 4, tab, out, stride, ws, need.value, None, word=b"net must be")
        _refused(lib, f, who, h, 1, None, r8, 4, tab, out, stride, ws, need.value, None, word=b"null frames")
        _refused(lib, f, who, h, 1, l8, r8, 4, None, out, stride, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, 1, l8, r8, 0, tab, out, stride, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, 1, l8, r8, -2, tab, out, stride, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, 1, C.c_void_p(0x200001), r8, 4, tab, out, stride, ws, need.value, None, word=b"4-byte aligned")
        _refused(lib, f, who, h, 1, l8, C.c_void_p(0x300002), 4, tab, out, stride, ws, need.value, None, word=b"4-byte aligned")
        _refused(lib, f, who, h, 1, l8, r8, 4, tab, None, stride, ws, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, 1, l8, r8, 4, tab, out, stride, ws, need.value - 1, None, word=b"workspace too small")
        if hm == 32:        # the float entry's size is short by the converter slice here
            base = C.c_size_t()
            assert lib.egotap_hm_workspace_bytes(h, 4, C.byref(base)) == 0
            _refused(lib, f, who, h, 1, l8, r8, 4, tab, out, stride, ws, base.value, None, word=b"workspace too small")
    finally:
        lib.egotap_destroy(h)


def test_one_call_from_bytes_refusals():
    lib, h = _handle()
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, 0, C.byref(need)) == 0
        f, who = lib.egotap_predict_pose_rgb_u8, b"egotap_predict_pose_rgb_u8"
        l8, r8, tab, pose, hm, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000))
        _refused(lib, f, who, None, l8, r8, 4, tab, pose, hm, 0, ws, need.value, None, word=b"null handle")
        _refused(lib, f, who, h, None, r8, 4, tab, pose, hm, 0, ws, need.value, None, word=b"null frames")
        _refused(lib, f, who, h, l8, None, 4, tab, pose, hm, 0, ws, need.value, None, word=b"null frames")
        _refused(lib, f, who, h, l8, r8, 4, None, pose, hm, 0, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, l8, r8, 4, tab, None, hm, 0, ws, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, hm, 0, None, need.value, None, word=b"null argument")
        _refused(lib, f, who, h, l8, r8, 0, tab, pose, hm, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, -3, tab, pose, hm, 0, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, hm, -1, ws, need.value, None, word=b"chunk")
        _refused(lib, f, who, h, C.c_void_p(0x200001), r8, 4, tab, pose, hm, 0, ws, need.value, None, word=b"4-byte aligned")
        _refused(lib, f, who, h, C.c_void_p(0x200002), r8, 4, tab, pose, hm, 0, ws, need.value, None, word=b"4-byte aligned")
        _refused(lib, f, who, h, l8, C.c_void_p(0x300002), 4, tab, pose, hm, 0, ws, need.value, None, word=b"4-byte aligned")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, C.c_void_p(0x600008), 0, ws, need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, hm, 0, C.c_void_p(0x700010), need.value, None, word=b"aligned")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, hm, 0, ws, need.value - 1, None, word=b"workspace too small")
        _refused(lib, f, who, h, l8, r8, 4, tab, pose, None, 0, ws, 0, None, word=b"workspace too small")
        form = C.c_int(-1)
        assert lib.egotap_debug_predict_pose_rgb_form(h, C.byref(form)) == 0 and form.value == 0          # nothing ran
    finally:
        lib.egotap_destroy(h)


@pytest.mark.parametrize("missing,word", [(L.NET_LIFT, b"lifting head"), (L.NET_HM_POS, b"position estimator"), (L.NET_HM_ROT, b"limb estimator")])
def test_unbound_network_is_refused_by_key(missing, word):
    lib, h = _handle(bind=[n for n in (L.NET_LIFT, L.NET_HM_POS, L.NET_HM_ROT) if n != missing])
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 2, 0, C.byref(need)) == 0
        l8, r8, tab, pose, out, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000))
        assert lib.egotap_predict_pose_rgb_u8(h, l8, r8, 2, tab, pose, None, 0, ws, need.value, None) == INVALID
        msg = lib.egotap_last_error()
        assert b"egotap_predict_pose_rgb_u8" in msg and b"unbound parameter" in msg and word in msg and b"not bound" in msg, msg
        if missing != L.NET_LIFT:
            assert lib.egotap_hm_forward_u8(h, missing, l8, r8, 2, tab, out, 90 * 4096, ws, need.value, None) == INVALID
            msg = lib.egotap_last_error()
            assert b"egotap_hm_forward_u8" in msg and b"unbound parameter" in msg and word in msg and b"not bound" in msg, msg
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 4. workspace sizes
@pytest.mark.parametrize("hm", [64, 128, 32])
def test_workspace_bytes_against_the_float_entries(hm):
    """sides 64 / 128: the stems read the bytes themselves, the sizes are the float entries'; elsewhere larger by exactly the converter slice
    of one chunk: chunk x 2 eyes x 3 x S0^2 fp32"""
    lib, h = _handle(bind=(), hm=hm)
    try:
        def q(fn, *a):
            v = C.c_size_t()
            assert fn(h, *a, C.byref(v)) == 0
            return v.value
        S0 = 4 * hm
        for B, chunk in ((1, 0), (3, 0), (3, 2), (37, 16), (300, 64), (5, 1000)):
            c = B if chunk == 0 or chunk > B else chunk
            extra = 0 if hm in (64, 128) else c * 2 * 3 * S0 * S0 * 4
            assert q(lib.egotap_predict_pose_rgb_u8_workspace_bytes, B, chunk) == q(lib.egotap_predict_pose_rgb_workspace_bytes, B, chunk) + extra
        for B in (1, 2, 3, 37):
            extra = 0 if hm in (64, 128) else B * 2 * 3 * S0 * S0 * 4
            assert q(lib.egotap_hm_forward_u8_workspace_bytes, B) == q(lib.egotap_hm_workspace_bytes, B) + extra
        bad = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, -1, 0, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, -1, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_rgb_u8_workspace_bytes(h, 4, 0, None) == INVALID
        assert lib.egotap_hm_forward_u8_workspace_bytes(None, 4, C.byref(bad)) == INVALID
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ 5. the Python faces
def _faces(**opt_kw):
    """the two Python faces without a GPU: the wrapper's methods on a stand-in that has what they read before anything touches the device (the
    wrapper itself moves its networks to the GPU when it is built), and a real estimator module on the CPU"""
    from egotap_amd import models, networks
    from egotap_amd.options import preset_defaults
    opt = preset_defaults("UnrealEgo", 64)
    for k, v in opt_kw.items():
        setattr(opt, k, v)
    m = types.SimpleNamespace(opt=opt, net_AutoEncoder=types.SimpleNamespace(preset=spec.lift_preset("UnrealEgo", 64)))
    m.predict_pose_from_camera = types.MethodType(models.EgoTAPAutoEncoderModel.predict_pose_from_camera, m)
    m.camera_table = types.MethodType(models.EgoTAPAutoEncoderModel.camera_table, m)
    pos_opt = preset_defaults("UnrealEgo", 64)
    pos_opt.num_rot_heatmap = 0
    for k, v in opt_kw.items():
        setattr(pos_opt, k, v)
    return m, networks.HeatMap_UnrealEgo_Shared(pos_opt, "resnet18", 2).eval()


def test_python_refusals_are_worded_like_the_float_entry():
    m, net = _faces()
    cpu8 = torch.zeros(1, 256, 256, 3, dtype=torch.uint8)
    for f in (m.predict_pose_from_camera, net.forward_from_camera):
        with pytest.raises(L.EgotapError, match="GPU only"):
            f(cpu8, cpu8)
    # dtype and shape are looked at once the frames are on a GPU: the checker itself, with a stand-in for "is on the GPU"
    class OnGpu(torch.Tensor):
        is_cuda = True
    as_gpu = lambda t: t.as_subclass(OnGpu)      # noqa: E731
    with pytest.raises(L.EgotapError, match="uint8"):
        L.check_camera_frames("predict_pose_from_camera", as_gpu(torch.zeros(1, 256, 256, 3)), as_gpu(torch.zeros(1, 256, 256, 3)), 256)
    with pytest.raises(ValueError, match=r"expected left8 / right8 \[B, 256, 256, 3\]"):
        L.check_camera_frames("predict_pose_from_camera", as_gpu(torch.zeros(1, 3, 256, 256, dtype=torch.uint8)),
                              as_gpu(torch.zeros(1, 3, 256, 256, dtype=torch.uint8)), 256)
    with pytest.raises(L.EgotapError, match="contiguous"):
        nc = torch.zeros(1, 256, 3, 256, dtype=torch.uint8).permute(0, 1, 3, 2)
        L.check_camera_frames("predict_pose_from_camera", as_gpu(nc), as_gpu(nc), 256)
    assert L.check_camera_frames("x", as_gpu(cpu8), as_gpu(cpu8), 256) == 1
    net.train()
    with pytest.raises(NotImplementedError, match="eval-mode"):
        net.forward_from_camera(cpu8, cpu8)
    # the tables the two faces hand to the library are spec's, and opt.rgb_mean / rgb_std reach them
    cpu = torch.device("cpu")
    assert np.array_equal(m.camera_table(cpu).numpy(), spec.rgb_u8_table()) and np.array_equal(net.camera_table(cpu).numpy(), spec.rgb_u8_table())
    m.opt.rgb_mean = [0.25, 0.25, 0.25]                          # the model's table follows its opt between calls
    assert np.array_equal(m.camera_table(cpu).numpy(), spec.rgb_u8_table(m.opt)) and not np.array_equal(m.camera_table(cpu).numpy(), spec.rgb_u8_table())
    m.opt.rgb_mean = None
    assert np.array_equal(m.camera_table(cpu).numpy(), spec.rgb_u8_table())
    m2, net2 = _faces(rgb_mean=[0.5, 0.5, 0.5], rgb_std=[0.25, 0.25, 0.25])
    for t in (m2.camera_table(cpu), net2.camera_table(cpu)):
        assert t.dtype == torch.float32 and tuple(t.shape) == (3, 256)
        assert np.array_equal(t.numpy(), spec.rgb_u8_table(m2.opt)) and not np.array_equal(t.numpy(), spec.rgb_u8_table())
