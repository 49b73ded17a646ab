"""Layer 0 of the pose-only forward projects the frame-invariant tokens (the grid's dummy cells: mask token + position embedding, the
contiguous tail of every image for UnrealEgo at 64 x 64 heatmaps) once per call: the live rows of every image as one compact product, image 0's
tail as a second one, and an attention that reads the tail's q | k | v from image 0.  Same bits as the full forward; rows (b > 0, n >= n0) of
the q | k | v buffer are neither written nor read."""
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


@pytest.mark.parametrize("B,N,heads,shared_from", [(2, 64, 1, 32), (3, 96, 2, 32)])
def test_shared_tail_attention(B, N, heads, shared_from):
    """one private + one shared tile, then two shared tiles (shared query blocks included): bit-equal to the plain attention on a tensor whose
    tail rows are equal in every image, also when the tail rows of the images behind the first hold NaN (they are not read)"""
    from egotap_amd import lib as L
    D = heads * 128
    g = torch.Generator(device="cuda").manual_seed(11 * B + N)
    qkv = torch.randn((B, N, 3 * D), generator=g, device="cuda", dtype=torch.float32)
    qkv[1:, shared_from:] = qkv[0, shared_from:]
    ref = L.attention(qkv.view(B * N, 3 * D), B, N, heads)
    assert torch.equal(L.attention_f32_shared(qkv.view(B * N, 3 * D), B, N, heads, N), ref)
    assert torch.equal(L.attention_f32_shared(qkv.view(B * N, 3 * D), B, N, heads, shared_from), ref)
    poisoned = qkv.clone()
    poisoned[1:, shared_from:] = float("nan")
    out = L.attention_f32_shared(poisoned.view(B * N, 3 * D), B, N, heads, shared_from)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def _smallest_shared_batch(net, p):
    for B in range(16, 65):
        x = _hm(p, B, 50 + B)
        if "qkv_shared" in _timed_roles(net, lambda: net.predict_pose(x)):
            return B
    pytest.fail("no batch in 16 .. 64 takes the shared layer-0 route")


@pytest.mark.parametrize("which", ["smallest", 64])
def test_forward_with_poisoned_workspace(which):
    """the rows layer 0 leaves unwritten are never read: the workspace filled with 0xFF bytes (NaN) between two calls changes nothing"""
    from gpu_util import lift_net
    net, _, p = lift_net("UnrealEgo", 64)
    B = _smallest_shared_batch(net, p) if which == "smallest" else which
    print("batch", B)
    x1, x2 = _hm(p, B, 21), _hm(p, B, 22)
    net.predict_pose(x1)                     # warm: handle, binding, workspace
    net.predict_pose(x1)
    assert "qkv_shared" in _timed_roles(net, lambda: net.predict_pose(x1))
    net._ws.fill_(0xFF)
    pose = net.predict_pose(x2).clone()
    full = net(x2)[0]
    torch.cuda.synchronize()
    assert torch.equal(pose, full)


def test_shared_launches_run_at_b256():
    """no silent fallback: at B = 256 layer 0's q | k | v is the live product (one launch, under the role of the other layers' products) plus
    one launch over the shared tail"""
    from gpu_util import lift_net
    net, _, p = lift_net("UnrealEgo", 64)
    B, D, NL = 256, 1024, p.vit_layers
    x = _hm(p, B, 5)
    net.predict_pose(x)
    roles = _timed_roles(net, lambda: net.predict_pose(x))
    assert roles["qkv_shared"]["launches"] == 1
    assert roles["qkv_shared"]["flops"] == pytest.approx(2.0 * 96 * 3 * D * D, rel=1e-5)
    assert roles["qkv"]["launches"] == NL - 1
    assert roles["qkv"]["flops"] == pytest.approx(2.0 * (B * 480 + (NL - 2) * B * 576) * 3 * D * D, rel=1e-5)
    assert "qkv_shared" not in _timed_roles(net, lambda: net(x))


@pytest.mark.parametrize("preset,hm,B", [("EgoCap", 64, 64), ("UnrealEgo", 48, 64)])
def test_predicate_stays_false(preset, hm, B):
    """dummy cells that are no whole grid row (EgoCap: T = 34), a sequence that is no whole number of attention tiles (48 x 48 heatmaps: 324
    tokens): layer 0 as in the full forward, same pose"""
    from gpu_util import lift_net
    net, _, p = lift_net(preset, hm)
    x = _hm(p, B, 31)
    full = net(x)[0].clone()
    roles = _timed_roles(net, lambda: net.predict_pose(x))
    assert "qkv_shared" not in roles and roles["qkv"]["launches"] >= 1
    pose = net.predict_pose(x)
    torch.cuda.synchronize()
    assert torch.equal(pose, full)
