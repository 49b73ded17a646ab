"""The pose-only entry (egotap_lift_predict_pose): the same pose bits as the full forward at every batch size and geometry, eager and
graphed, and at a batch that fills the chip the last ViT layer really runs on the live rows only."""
import ctypes as C
import json

import pytest
import torch

pytestmark = pytest.mark.gpu


def _hm(p, B, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand((B, p.in_channels, p.hm_size, p.hm_size), generator=g, device="cuda", dtype=torch.float32)


def _timed_roles(net, fn):
    from egotap_amd import lib as L
    lib, h = L.load(), net._ensure_handle()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        fn()
        torch.cuda.synchronize()
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        return {d["role"]: d for d in json.loads(lib.egotap_timing_detail(h).decode())}
    finally:
        L.check(lib.egotap_timing_enable(h, 0))


@pytest.mark.parametrize("preset,hm,B", [("UnrealEgo", 64, 1), ("UnrealEgo", 64, 2), ("UnrealEgo", 64, 3), ("UnrealEgo", 64, 8),
                                         ("UnrealEgo", 64, 64), ("UnrealEgo", 64, 256), ("EgoCap", 64, 1), ("EgoCap", 64, 256),
                                         ("EgoCap", 128, 2), ("EgoCap", 128, 32), ("UnrealEgo", 48, 256)])
def test_predict_pose_equals_forward(preset, hm, B):
    from gpu_util import lift_net
    net, _, p = lift_net(preset, hm)
    x = _hm(p, B, 1000 + B + hm)
    full = net(x)[0].clone()
    pose = net.predict_pose(x)
    torch.cuda.synchronize()
    assert torch.equal(pose, full)


@pytest.mark.parametrize("preset,hm,B", [("UnrealEgo", 64, 2), ("UnrealEgo", 64, 256)])
def test_predict_pose_graphed_equals_forward(preset, hm, B):
    from gpu_util import lift_net
    net, _, p = lift_net(preset, hm)
    x = _hm(p, B, 7 + B)
    full = net(x)[0].clone()
    assert torch.equal(net.predict_pose_graphed(x), full)
    net.__dict__.get("_graphs", {}).clear()


def test_pruned_launches_run_at_b256():
    """no silent fallback: at B = 256 the last layer's products run compact, with the FLOPs of the live rows"""
    from gpu_util import lift_net
    net, _, p = lift_net("UnrealEgo", 64)
    B = 256
    x = _hm(p, B, 3)
    net.predict_pose(x)                      # warm: handle, binding, workspace
    roles = _timed_roles(net, lambda: net.predict_pose(x))
    D, Mc, M = 1024, B * p.tokens * 16, B * 576
    for r in ("kv", "q_live", "attn_out_live", "mlp_up_live", "mlp_down_live"):    # (whole rounds of 256 x 256 tiles + the rows past them)
        assert roles[r]["launches"] in (1, 2), r
    assert roles["attn_out_live"]["flops"] == pytest.approx(2.0 * Mc * D * D, rel=1e-5)
    assert roles["mlp_down_live"]["flops"] == pytest.approx(2.0 * Mc * D * 4 * D, rel=1e-5)
    exact = lambda v: pytest.approx(v, rel=1e-5)          # (the detail prints 7 significant digits)
    assert roles["q_live"]["flops"] == exact(2.0 * Mc * D * D)
    assert roles["kv"]["flops"] == exact(2.0 * M * 2 * D * D)
    assert roles["mlp_up_live"]["flops"] == exact(2.0 * Mc * 4 * D * D)
    NL = p.vit_layers                        # the layers before the last run on every row
    assert roles["qkv"]["launches"] == NL - 1 and roles["mlp_up"]["launches"] == NL - 1
    full = _timed_roles(net, lambda: net(x))
    assert "q_live" not in full and full["qkv"]["launches"] == NL
