"""Frozen-weight serving, host side: the six C entries are exported and answer without a device where they can, and the module methods
refuse by name where there is nothing to freeze (no kernel is launched here)."""
import ctypes as C
import re
import subprocess

import pytest

from egotap_amd import lib as L

SIX = ["egotap_lift_frozen_bytes", "egotap_lift_freeze", "egotap_lift_unfreeze", "egotap_hm_frozen_bytes", "egotap_hm_freeze", "egotap_hm_unfreeze"]


def _cfg(hm_size=64, n_joints_hm=15, estimate_head=1):
    return L.EgotapConfig(C.sizeof(L.EgotapConfig), n_joints_hm, estimate_head, hm_size, 128, 1024, 8, 3, 16, 512)


def test_the_six_entries_are_declared_bound_and_exported():
    lib = L.load()
    out = subprocess.run(["nm", "-D", "--defined-only", L._build.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(egotap_[a-z0-9_]+)$", out, flags=re.M))
    for n in SIX:
        assert n in exported and n in L.exported_symbols() and hasattr(lib, n), n
    assert lib.egotap_abi_version() == 2          # symbols were only added


def _lift_formula(hm, layers=3, D=1024):
    """bytes of the lifting head's arena from the layer shapes: bf16 copies of the patch projection [D, 256], per ViT block q | k | v [3D, D],
    o [D, D], up [4D, D], down [D, 4D], the two fc1 [2048, (hm / 16)^2 D] and [2048, 2 hm^2]; per block the fused fp32 q | k | v bias [3D]"""
    k1 = (hm // 16) ** 2 * D
    return 2 * (D * 256 + layers * 12 * D * D + 2048 * k1 + 2048 * 2 * hm * hm) + layers * 3 * D * 4


@pytest.mark.parametrize("hm,joints,head", [(64, 15, 1), (128, 17, 0)])
def test_lift_frozen_bytes_without_a_device(hm, joints, head):
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.egotap_create(C.byref(_cfg(hm, joints, head)), C.byref(h)))
    try:
        n = C.c_size_t(123)
        L.check(lib.egotap_lift_frozen_bytes(h, C.byref(n)))
        assert n.value == 0                                        # fp32 (the default mode) prepares nothing
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["bf16x3"]))
        L.check(lib.egotap_lift_frozen_bytes(h, C.byref(n)))
        assert n.value == 0
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["bf16"]))
        L.check(lib.egotap_lift_frozen_bytes(h, C.byref(n)))
        assert n.value == _lift_formula(hm)
        # freeze refuses by name before any launch: wrong mode, then a missing arena
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["f32"]))
        assert lib.egotap_lift_freeze(h, C.c_void_p(0x10000), 1 << 40, None) == 1
        assert b"precision" in lib.egotap_last_error()
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["bf16"]))
        assert lib.egotap_lift_freeze(h, None, 1 << 40, None) == 1
        assert b"arena" in lib.egotap_last_error()
        assert lib.egotap_lift_freeze(h, C.c_void_p(0x10000), 1 << 40, None) == 3      # parameters not bound: refused before the launch
        L.check(lib.egotap_lift_unfreeze(h))
    finally:
        lib.egotap_destroy(h)


def test_ragged_sequence_and_other_sides_have_nothing_to_freeze():
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.egotap_create(C.byref(_cfg(96)), C.byref(h)))      # 1296 tokens: not a multiple of 32; estimator side 96: exact-fp32 path
    try:
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["bf16"]))
        n = C.c_size_t(123)
        L.check(lib.egotap_lift_frozen_bytes(h, C.byref(n)))
        assert n.value == 0
        assert lib.egotap_lift_freeze(h, C.c_void_p(0x10000), 1 << 40, None) == 1
        assert b"multiple of 32" in lib.egotap_last_error()
        for net in (L.NET_HM_POS, L.NET_HM_ROT):
            L.check(lib.egotap_hm_frozen_bytes(h, net, 1, C.byref(n)))
            assert n.value == 0
            assert lib.egotap_hm_freeze(h, net, 1, C.c_void_p(0x10000), 1 << 40, None) == 1
            assert b"64 and 128" in lib.egotap_last_error()
    finally:
        lib.egotap_destroy(h)


def test_hm_frozen_bytes_without_a_device():
    lib = L.load()
    h = C.c_void_p()
    L.check(lib.egotap_create(C.byref(_cfg()), C.byref(h)))
    try:
        n = C.c_size_t(123)
        L.check(lib.egotap_hm_frozen_bytes(h, L.NET_HM_POS, 1, C.byref(n)))
        assert n.value == 0                                        # fp32
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["bf16"]))
        L.check(lib.egotap_hm_frozen_bytes(h, L.NET_HM_POS, 1, C.byref(n)))
        # resnet18: the packed bf16 weights alone are 2 bytes x (backbone 11.2 M + decoder 1x1 1.4 M + 3x3 (padded concat) 24.3 M) ~ 74 MB
        assert 70e6 < n.value < 90e6 and n.value % 256 == 0
        one = n.value
        L.check(lib.egotap_hm_frozen_bytes(h, L.NET_HM_ROT, 8, C.byref(n)))
        assert n.value == one                                      # the slices' sizes do not depend on the batch or the net
        assert lib.egotap_hm_frozen_bytes(h, L.NET_LIFT, 1, C.byref(n)) == 1
        assert lib.egotap_hm_frozen_bytes(h, L.NET_HM_POS, 0, C.byref(n)) == 1
        L.check(lib.egotap_hm_unfreeze(h, L.NET_HM_POS))
    finally:
        lib.egotap_destroy(h)


def _opt(preset="UnrealEgo", hm=64):
    from egotap_amd.options import preset_defaults
    return preset_defaults(preset, hm)


def test_freeze_weights_on_a_cpu_module_raises_by_name():
    from egotap_amd import networks
    net = networks.EgoTAPAutoEncoder(_opt(), input_channel_scale=2).eval()
    assert not net.weights_frozen
    with pytest.raises(L.EgotapError, match="CPU"):
        net.freeze_weights()
    with pytest.raises(L.EgotapError, match="not frozen"):
        net.refresh_frozen_weights()
    net.unfreeze_weights()                                         # a no-op on a module that is not frozen
    assert not net.weights_frozen
    opt = _opt()
    opt.num_rot_heatmap = 0
    hm = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", 2).eval()
    with pytest.raises(L.EgotapError, match="CPU"):
        hm.freeze_weights()
    assert not hm.weights_frozen
    bott = networks.HeatMap_UnrealEgo_Shared(opt, "resnet50", 2).eval()
    with pytest.raises(L.EgotapError, match="resnet50"):
        bott.freeze_weights()


def test_frozen_tensor_lists_match_what_the_library_keeps():
    """the Python staleness check watches exactly the tensors whose prepared copies the arena holds (egotap_abi.hip frozen_key)"""
    from egotap_amd import networks
    net = networks.EgoTAPAutoEncoder(_opt(), input_channel_scale=2)
    ts = net._frozen_tensors()
    assert len(ts) == 1 + 3 * 9 + 2                                # patch projection, 3 blocks x (6 weights + q, k, v bias), two fc1
    assert sum(t.numel() for t in ts if t.dim() >= 2) * 2 + 3 * 3 * 1024 * 4 == _lift_formula(64)
    opt = _opt()
    opt.num_rot_heatmap = 0
    hm = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", 2)
    sd = hm.state_dict(keep_vars=True)
    ids = {id(t) for t in hm._frozen_tensors()}
    bb = "backbone.backbone.backbone."
    assert id(sd[bb + "layer1.0.conv1.weight"]) in ids and id(sd[bb + "layer1.0.bn1.running_var"]) in ids
    assert id(sd["after_backbone.conv_heatmap.bias"]) in ids
    assert id(sd[bb + "conv1.weight"]) not in ids and id(sd[bb + "bn1.running_var"]) not in ids      # the stem is read live
    assert len(ids) == 19 * 5 + 8 * 2                              # 19 convolutions with BatchNorm (weight + 4) and 8 decoder convolutions (weight, bias)
