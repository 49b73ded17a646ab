"""egotap_lift_train_bytes (host only, no kernel is launched): the saved-activation and backward-workspace sizes of the one-call
training step are pinned for both presets, every precision mode and small to large batches, so that a change of the plans'
layout cannot pass unnoticed."""
import ctypes as C

import pytest

from egotap_amd import lib as L
from egotap_amd import spec

# (preset, precision, B): (saved bytes, workspace bytes); f32 and bf16x3 share the fp32-tensor plans, bf16 is the bf16-storage step
EXPECTED = {
    ("UnrealEgo", "f32", 1): (120110080, 1287445760),
    ("UnrealEgo", "f32", 3): (360243200, 1336317184),
    ("UnrealEgo", "f32", 256): (30737082880, 7518552320),
    ("UnrealEgo", "f32", 1024): (122948200960, 26285179136),
    ("UnrealEgo", "bf16x3", 1): (120110080, 1287445760),
    ("UnrealEgo", "bf16x3", 3): (360243200, 1336317184),
    ("UnrealEgo", "bf16x3", 256): (30737082880, 7518552320),
    ("UnrealEgo", "bf16x3", 1024): (122948200960, 26285179136),
    ("UnrealEgo", "bf16", 1): (388926464, 340446464),
    ("UnrealEgo", "bf16", 3): (529084416, 365970688),
    ("UnrealEgo", "bf16", 256): (18259065344, 3594785024),
    ("UnrealEgo", "bf16", 1024): (72079718912, 13421252864),
    ("EgoCap", "f32", 1): (120378368, 1287554304),
    ("EgoCap", "f32", 3): (361048064, 1336642816),
    ("EgoCap", "f32", 256): (30805764608, 7546339584),
    ("EgoCap", "f32", 1024): (123222927872, 26396328192),
    ("EgoCap", "bf16x3", 1): (120378368, 1287554304),
    ("EgoCap", "bf16x3", 3): (361048064, 1336642816),
    ("EgoCap", "bf16x3", 256): (30805764608, 7546339584),
    ("EgoCap", "bf16x3", 1024): (123222927872, 26396328192),
    ("EgoCap", "bf16", 1): (389293056, 340571392),
    ("EgoCap", "bf16", 3): (530184192, 366345472),
    ("EgoCap", "bf16", 256): (18352912896, 3626766592),
    ("EgoCap", "bf16", 1024): (72455109120, 13549179136),
}


@pytest.mark.parametrize("preset", ["UnrealEgo", "EgoCap"])
@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_lift_train_bytes_pinned(preset, mode):
    lib = L.load()
    p = spec.lift_preset(preset, 64)
    cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), p.n_joints_hm, int(p.estimate_head), p.hm_size, p.hidden, p.vit_dim, p.vit_heads,
                         p.vit_layers, p.patch, p.pu_hidden)
    h = C.c_void_p()
    assert lib.egotap_create(C.byref(cfg), C.byref(h)) == 0
    assert lib.egotap_set_precision(h, L.PRECISIONS[mode]) == 0
    for B in (1, 3, 256, 1024):
        sb, wb = C.c_size_t(), C.c_size_t()
        assert lib.egotap_lift_train_bytes(h, B, C.byref(sb), C.byref(wb)) == 0
        assert (sb.value, wb.value) == EXPECTED[(preset, mode, B)], (preset, mode, B)
    lib.egotap_destroy(h)
