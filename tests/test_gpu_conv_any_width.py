"""conv_f32_any_kernel (conv_f32.h): the exact-fp32 convolution at map widths without a power-of-two instantiation, reached through
egotap_hm_conv_bn_fwd (BatchNorm) and egotap_hmtrain_conv_fwd (bias), against float64 torch conv2d on the CPU."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WIDTHS = [2, 4, 6, 10, 12, 20, 24, 48, 96]
SHAPES = [(9, 1), (9, 2), (1, 1), (1, 2)]        # (taps, stride)
CANARY = 7.25


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _handle():
    from gpu_util import hm_net
    net, _ = hm_net("pos")
    return net._ensure_handle()


def _case(taps, stride, W, N, Cin, Cout, seed):
    k = 3 if taps == 9 else 1
    x = _rand((N, Cin, W * stride, W * stride), seed)
    w = _rand((Cout, Cin, k, k), seed + 1, -0.2, 0.2)
    return x, w, k


def _ref(x, w, k, stride, scale, shift, res, relu):
    y = F.conv2d(x.double(), w.double(), stride=stride, padding=(k - 1) // 2)
    y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    if res is not None:
        y = y + res.double()
    return y.clamp_min(0.0) if relu else y


def _check(got, ref):
    err = (got.cpu().double() - ref).abs().max().item()
    assert err <= 1e-4 * max(1.0, ref.abs().max().item()), f"max err {err:.3e} (max |ref| {ref.abs().max().item():.3e})"


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("taps,stride", SHAPES)
def test_conv_any_width_bn_residual_relu_into_channel_slice(taps, stride, W):
    """BatchNorm(eval) + residual + ReLU; Cin = 20 (not a multiple of the 32-deep k slab nor of the power-of-two kernels' channel slabs),
    Cout = 72 (a partial 64-channel tile); the output is a channel slice of a canary-filled buffer, the residual one of another"""
    from egotap_amd import hm_ops as H
    h = _handle()
    N, Cin, Cout, c0, Ctot = 3, 20, 72, 5, 80
    x, w, k = _case(taps, stride, W, N, Cin, Cout, 10 * W + taps + stride)
    gamma, beta = _rand((Cout,), 1, 0.5, 1.5), _rand((Cout,), 2)
    mean, var = _rand((Cout,), 3), _rand((Cout,), 4, 0.5, 2.0)
    res_full = _rand((N, Cout + 3, W, W), 5)
    res = res_full[:, 3:]
    xc = x.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((N, Ctot, W, W), CANARY, device="cuda")
        H.conv_bn_fwd(h, xc, w.cuda(), tuple(t.cuda() for t in (gamma, beta, mean, var)), H.View(out, c0, Cout),
                      res=H.View(res_full.cuda(), 3, Cout), taps=taps, stride=stride, relu=True)
        outs.append(out)
    torch.cuda.synchronize()
    sc = gamma.double() / torch.sqrt(var.double() + 1e-5)
    ref = _ref(x, w, k, stride, sc, beta.double() - mean.double() * sc, res, True)
    _check(outs[0][:, c0:c0 + Cout], ref)
    assert float((outs[0][:, :c0] - CANARY).abs().max()) == 0.0 and float((outs[0][:, c0 + Cout:] - CANARY).abs().max()) == 0.0
    assert torch.equal(outs[0], outs[1])                  # run to run, bit for bit


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("taps,stride", SHAPES)
def test_conv_any_width_bias_no_residual_no_relu(taps, stride, W):
    """bias, no residual, no ReLU; Cin = 36, Cout = 130 (two 128-channel tiles, the second nearly empty)"""
    from egotap_amd import hm_ops as H
    h = _handle()
    N, Cin, Cout = 2, 36, 130
    x, w, k = _case(taps, stride, W, N, Cin, Cout, 1000 + 10 * W + taps + stride)
    bias = _rand((Cout,), 6)
    out = torch.full((N, Cout, W, W), CANARY, device="cuda")
    H.conv_fwd(h, x.cuda(), w.cuda(), out, bias=bias.cuda(), taps=taps, stride=stride, relu=False)
    again = torch.full_like(out, -CANARY)
    H.conv_fwd(h, x.cuda(), w.cuda(), again, bias=bias.cuda(), taps=taps, stride=stride, relu=False)
    torch.cuda.synchronize()
    _check(out, _ref(x, w, k, stride, torch.ones(Cout), bias, None, False))
    assert torch.equal(out, again)


def test_conv_any_width_frame_does_not_depend_on_batch():
    """one workgroup sums a pixel's whole K in a fixed order whatever tile shape the grid size picks (one 96 x 96 frame: 64 x 64 tiles; eight:
    128 x 256 tiles), so a frame's output is the same bits in any batch and at any position in it"""
    from egotap_amd import hm_ops as H
    h = _handle()
    W, Cin, Cout = 96, 16, 128
    x, w, _ = _case(9, 1, W, 8, Cin, Cout, 77)
    bias = _rand((Cout,), 8)
    one = torch.empty((1, Cout, W, W), device="cuda")
    eight = torch.empty((8, Cout, W, W), device="cuda")
    H.conv_fwd(h, x[5:6].cuda(), w.cuda(), one, bias=bias.cuda(), taps=9, relu=True)
    H.conv_fwd(h, x.cuda(), w.cuda(), eight, bias=bias.cuda(), taps=9, relu=True)
    torch.cuda.synchronize()
    assert torch.equal(one[0], eight[5])


@pytest.mark.parametrize("Cout", [130, 64])
@pytest.mark.parametrize("taps,stride", SHAPES)
def test_conv_any_width_large_grid_tiles(taps, stride, Cout):
    """enough pixels for the 256-pixel tiles (8 frames of 96 x 96: 128-channel tiles for Cout = 130, 64-channel ones for Cout = 64), BatchNorm +
    ReLU into a channel slice of a canary-filled buffer"""
    from egotap_amd import hm_ops as H
    h = _handle()
    N, W, Cin, c0 = 8, 96, 12, 3
    x, w, k = _case(taps, stride, W, N, Cin, Cout, 500 + Cout + taps + stride)
    gamma, beta = _rand((Cout,), 11, 0.5, 1.5), _rand((Cout,), 12)
    mean, var = _rand((Cout,), 13), _rand((Cout,), 14, 0.5, 2.0)
    out = torch.full((N, Cout + 4, W, W), CANARY, device="cuda")
    H.conv_bn_fwd(h, x.cuda(), w.cuda(), tuple(t.cuda() for t in (gamma, beta, mean, var)), H.View(out, c0, Cout), taps=taps, stride=stride,
                  relu=True)
    torch.cuda.synchronize()
    sc = gamma.double() / torch.sqrt(var.double() + 1e-5)
    _check(out[:, c0:c0 + Cout], _ref(x, w, k, stride, sc, beta.double() - mean.double() * sc, None, True))
    assert float((out[:, :c0] - CANARY).abs().max()) == 0.0 and float((out[:, c0 + Cout:] - CANARY).abs().max()) == 0.0
