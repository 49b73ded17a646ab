"""GPU parity of the heatmap-estimator training operators (C ABI egotap_hmtrain_*) against float64 torch autograd on the CPU."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _close(got, ref64, atol, rtol=1e-4, msg=""):
    got = got.detach().cpu().double()
    err = (got - ref64).abs()
    tol = atol + rtol * ref64.abs()
    assert bool((err <= tol).all()), f"{msg} max err {err.max().item():.3e} (max ref {ref64.abs().max().item():.3e})"


def _handle():
    from gpu_util import hm_net
    net, _ = hm_net("pos")
    return net._ensure_handle()


CONVS = [  # (ks, stride, Cin, Cout, Wout, N)
    (3, 1, 64, 64, 64, 2), (3, 1, 128, 128, 32, 3), (3, 1, 100, 200, 16, 4), (3, 1, 512, 512, 8, 2),
    (3, 2, 64, 128, 32, 2), (3, 2, 128, 256, 16, 3), (3, 2, 256, 512, 8, 2),
    (1, 1, 128, 128, 64, 2), (1, 1, 256, 260, 32, 2), (1, 1, 512, 516, 16, 3), (1, 1, 1024, 1024, 8, 2),
    (1, 2, 64, 128, 32, 2), (1, 2, 128, 256, 16, 2), (1, 2, 256, 512, 8, 2),
    # [r3] the 2 x 2 wave layout of the layers with at most 64 output channels (ragged on both sides), odd image counts for the row splits,
    # the stem
    (3, 1, 70, 50, 64, 3), (1, 1, 512, 30, 64, 3), (1, 1, 100, 64, 64, 1), (3, 1, 640, 512, 64, 1), (7, 2, 3, 64, 128, 3),
]


@pytest.mark.parametrize("ks,stride,Cin,Cout,W,N", CONVS)
def test_conv_wgrad_and_dgrad(ks, stride, Cin, Cout, W, N):
    """weight gradient (implicit GEMM over pixels, split over images) and input gradient (forward kernels on flipped weights,
    stride 2 through zero-upsampled dY) against autograd of F.conv2d; ragged channel counts; accumulate mode"""
    from egotap_amd import hm_ops as H
    h = _handle()
    x, w = _rand((N, Cin, W * stride, W * stride), 1), _rand((Cout, Cin, ks, ks), 2, -0.1, 0.1)
    dy = _rand((N, Cout, W, W), 3)
    xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(xr, wr, None, stride, (ks - 1) // 2).backward(dy.double())
    dw = torch.full((Cout, Cin, ks, ks), 3.0, device="cuda")
    H.conv_wgrad(dy.cuda(), x.cuda(), dw, ks=ks, stride=stride)
    scale = float(wr.grad.abs().mean())
    _close(dw, wr.grad, atol=2e-4 * scale + 1e-5, msg="dw")
    first = dw.clone()
    H.conv_wgrad(dy.cuda(), x.cuda(), dw, ks=ks, stride=stride, accumulate=True)
    _close(dw, 2 * wr.grad, atol=4e-4 * scale + 2e-5, msg="dw accumulate")
    again = torch.empty_like(dw)
    H.conv_wgrad(dy.cuda(), x.cuda(), again, ks=ks, stride=stride)
    assert torch.equal(first, again)
    if ks == 7:
        return                                     # the stem has no input gradient (the images are data)
    dx = torch.full((N, Cin, W * stride, W * stride), 7.0, device="cuda")
    H.conv_dgrad(h, dy.cuda(), w.cuda(), dx, taps=ks * ks, stride=stride)
    _close(dx, xr.grad, atol=2e-4 * float(xr.grad.abs().mean()) + 1e-5, msg="dx")


def test_stem_raw_and_wgrad():
    from egotap_amd import hm_ops as H
    B, S0 = 2, 256
    l, r, w = _rand((B, 3, S0, S0), 1), _rand((B, 3, S0, S0), 2), _rand((64, 3, 7, 7), 3, -0.1, 0.1)
    x = torch.stack([l, r], 1).reshape(2 * B, 3, S0, S0)
    z = torch.empty((2 * B, 64, S0 // 2, S0 // 2), device="cuda")
    H.stem_fwd(l.cuda(), r.cuda(), w.cuda(), z)
    wr = w.double().requires_grad_(True)
    ref = F.conv2d(x.double(), wr, None, 2, 3)
    _close(z, ref.detach(), 2e-5)
    dy = _rand(tuple(z.shape), 4)
    ref.backward(dy.double())
    dw = torch.empty((64, 3, 7, 7), device="cuda")
    H.conv_wgrad(dy.cuda(), x.cuda(), dw, ks=7, stride=2)
    _close(dw, wr.grad, atol=2e-4 * float(wr.grad.abs().mean()), msg="stem dw")


@pytest.mark.parametrize("N,C,Hs,relu,with_res", [(4, 64, 32, True, False), (6, 128, 16, True, True), (2, 516, 8, False, False), (3, 64, 64, True, True)])
def test_bn2d_fwd_bwd(N, C, Hs, relu, with_res):
    from egotap_amd import hm_ops as H
    z, res = _rand((N, C, Hs, Hs), 1, -2, 2), _rand((N, C, Hs, Hs), 2)
    g, b = _rand((C,), 3, 0.5, 1.5), _rand((C,), 4)
    rm, rv = _rand((C,), 5), _rand((C,), 6, 0.5, 2.0)
    dy = _rand((N, C, Hs, Hs), 7)
    zr, gr, br, rr = (t.double().requires_grad_(True) for t in (z, g, b, res))
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    y = F.batch_norm(zr, rm64, rv64, gr, br, True, 0.1, 1e-5)
    if with_res:
        y = y + rr
    if relu:
        y = F.relu(y)
    y.backward(dy.double())
    yd = torch.empty_like(z, device="cuda")
    rmd, rvd = rm.cuda(), rv.cuda()
    mean, rstd = H.bn2d_fwd(z.cuda(), yd, g.cuda(), b.cuda(), rmd, rvd, res=res.cuda() if with_res else None, relu=relu)
    _close(yd, y.detach(), 2e-5)
    _close(rmd, rm64, 1e-6)
    _close(rvd, rv64, 1e-5)
    dz, dres = torch.empty_like(yd), (torch.empty_like(yd) if with_res else None)
    dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    H.bn2d_bwd(z.cuda(), yd, dy.cuda(), g.cuda(), mean, rstd, dz, dg, db, dres=dres, relu=relu)
    _close(dz, zr.grad, 2e-5, rtol=1e-3)
    _close(dg, gr.grad, 2e-3, rtol=1e-4)
    _close(db, br.grad, 2e-3, rtol=1e-4)
    if with_res:
        _close(dres, rr.grad, 1e-6)


def test_pointwise_backward_ops():
    from egotap_amd import hm_ops as H
    # max-pool 3/2/1 (ties broken like torch: first maximum in the window scan)
    x = _rand((2, 8, 32, 32), 1)
    x[0, 0, 4:8, 4:8] = 0.5                       # plateau: ties
    xr = x.double().requires_grad_(True)
    dy = _rand((2, 8, 16, 16), 2)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.double())
    dx = torch.empty_like(x, device="cuda")
    H.maxpool_bwd(x.cuda(), dy.cuda(), dx)
    _close(dx, xr.grad, 1e-6)
    # [r3] strip kernel: a last strip that is not full (24 rows = 16 + 8), the training size (128) and one plane row per strip element
    for side, seed in ((24, 5), (128, 6), (8, 7)):
        x = _rand((3, 5, side, side), seed)
        x[1, 2, 2:7, 1:6] = 0.25
        xr = x.double().requires_grad_(True)
        dy = _rand((3, 5, side // 2, side // 2), seed + 10)
        F.max_pool2d(xr, 3, 2, 1).backward(dy.double())
        dx = torch.full_like(x, 9.0, device="cuda")
        H.maxpool_bwd(x.cuda(), dy.cuda(), dx)
        torch.cuda.synchronize()
        _close(dx, xr.grad, 1e-6, msg=f"maxpool backward, side {side}")
    # bilinear x2 upsample, align_corners=True, into / out of channel slices of wider buffers
    src = _rand((3, 6, 8, 8), 3).double().requires_grad_(True)
    dup = _rand((3, 10, 16, 16), 4)
    F.interpolate(src, scale_factor=2, mode="bilinear", align_corners=True).backward(dup[:, 2:8].double())
    dsrc = torch.zeros((3, 9, 8, 8), device="cuda")
    H.upsample_bwd(H.View(dup.cuda(), 2, 6), H.View(dsrc, 1, 6))
    _close(dsrc[:, 1:7], src.grad, 1e-5)
    assert float(dsrc[:, 0].abs().max()) == 0 and float(dsrc[:, 7:].abs().max()) == 0
    # ReLU mask and per-channel sums on slices
    y, d = _rand((2, 12, 16, 16), 5), _rand((2, 12, 16, 16), 6)
    dz = torch.zeros((2, 20, 16, 16), device="cuda")
    H.relu_bwd(H.View(y.cuda(), 4, 8), H.View(d.cuda(), 4, 8), H.View(dz, 10, 8))
    _close(dz[:, 10:18], (d[:, 4:12] * (y[:, 4:12] > 0)).double(), 0)
    out = torch.full((8,), 2.0, device="cuda")
    H.chansum(H.View(d.cuda(), 4, 8), out)
    _close(out, d[:, 4:12].double().sum((0, 2, 3)), 1e-4)
    H.chansum(H.View(d.cuda(), 4, 8), out, accumulate=True)
    _close(out, 2 * d[:, 4:12].double().sum((0, 2, 3)), 2e-4)


@pytest.mark.parametrize("limb", [False, True])
def test_mse_loss(limb):
    """heatmap_shared_model.py:109-151: lambda * (MSE(left) + MSE(right)), limb maps divided by sqrt(gt_plength) first"""
    from egotap_amd import hm_ops as H
    B, Cn, S = 3, 30 if not limb else 60, 64
    pred, gt = _rand((B, Cn, S, S), 1), _rand((B, Cn, S, S), 2)
    plen = _rand((B, Cn), 3, 1.0, 40.0) if limb else None
    pr = pred.double().requires_grad_(True)
    lam = 10.0
    if limb:
        sq = torch.sqrt(plen.double())[..., None, None]
        loss = lam * (F.mse_loss(pr[:, :Cn // 2] / sq[:, :Cn // 2], gt.double()[:, :Cn // 2] / sq[:, :Cn // 2])
                      + F.mse_loss(pr[:, Cn // 2:] / sq[:, Cn // 2:], gt.double()[:, Cn // 2:] / sq[:, Cn // 2:]))
    else:
        loss = lam * (F.mse_loss(pr[:, :Cn // 2], gt.double()[:, :Cn // 2]) + F.mse_loss(pr[:, Cn // 2:], gt.double()[:, Cn // 2:]))
    loss.backward()
    l, dp = H.mse(pred.cuda(), gt.cuda(), plen.cuda() if limb else None, lam)
    np.testing.assert_allclose(float(l), float(loss.detach()), rtol=1e-5)
    _close(dp, pr.grad, 1e-9, rtol=1e-4)


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("Cin,Cout,W,N", [(64, 64, 64, 2), (128, 128, 32, 3), (100, 200, 16, 4), (640, 512, 64, 1), (1540, 1024, 16, 2)])
def test_conv_wgrad_bf16_modes(mode, Cin, Cout, W, N):
    """3x3 stride-1 weight gradient on the bf16 matrix cores: pre-shifted input rows (shuffled edge pixels, zero halos), ragged
    channel counts (Cin = 100, 1540), image split; bf16x3 against float64 with the 2^-16 error model, bf16 against the float64
    gradient of the rounded operands"""
    from egotap_amd import hm_ops as H
    x, dy = _rand((N, Cin, W, W), 1), _rand((N, Cout, W, W), 3)
    w = torch.zeros((Cout, Cin, 3, 3), dtype=torch.float64, requires_grad=True)
    xs, ds = (x.double(), dy.double()) if mode == "bf16x3" else (x.bfloat16().double(), dy.bfloat16().double())
    F.conv2d(xs, w, None, 1, 1).backward(ds)
    dw = torch.full((Cout, Cin, 3, 3), 3.0, device="cuda")
    H.conv_wgrad(dy.cuda(), x.cuda(), dw, ks=3, stride=1, precision=mode)
    scale = float(w.grad.abs().mean())
    _close(dw, w.grad, atol=(3e-4 if mode == "bf16x3" else 2e-4) * scale + 1e-5, msg="dw " + mode)
    again = torch.empty_like(dw)
    H.conv_wgrad(dy.cuda(), x.cuda(), again, ks=3, stride=1, precision=mode)
    assert torch.equal(dw, again)


# ---------------------------------------------------------------------------------------------------------------------------------
# The operators as the training step of hm_training.py calls them: on a handle in a bf16 precision mode WITH the repacked-weight scratch
# bound (gpu_util.hm_handle; without it conv_any takes the fp32 kernels in every mode and a test of the mode tests nothing), on channel
# slices of wider buffers, accumulating, per eye, and at width 128.  Every case runs twice for equal bits.
CANARY = -777.0


def _rb(t):
    return t.float().bfloat16().double()


def _bf_kernel(mode, taps, stride, cout, w):
    """does conv_any (abi_conv_routing.inc) route this forward-form convolution to conv_bf16_kernel?"""
    return mode != "f32" and taps == 9 and stride == 1 and ((cout >= 128 and w in (64, 32, 16, 8)) or (cout == 64 and w == 64)
                                                           or (mode == "bf16" and cout == 64 and w == 128))


def _conv_gate(mode, routed, ref):
    return ((3e-4 if mode == "bf16x3" else 2e-4) if routed else 2e-4) * float(ref.abs().mean()) + 1e-5


def _twice(fn, out):
    """run fn (which writes `out` from scratch or on top of what `restore` puts back) twice: equal bits"""
    fn()
    first = out.clone()
    fn()
    torch.cuda.synchronize()
    assert torch.equal(first, out), "two runs differ"
    return first


DGRADS = [  # (Cout, Cin, W of dy, N, stride): dx has Cin channels -- the output channels of the kernel that computes it
    (132, 20, 64, 2, 1), (132, 20, 32, 2, 1), (132, 20, 16, 2, 1), (132, 20, 8, 2, 1),          # fp32 kernels on a bf16-mode handle (20 < 128)
    (20, 132, 64, 2, 1), (20, 132, 32, 2, 1), (20, 132, 16, 2, 1), (20, 132, 8, 2, 1),          # conv_bf16_kernel, ragged 128 + 4 channel tiles
    (64, 64, 64, 2, 1),                                                                         # the 64-channel tile (layer1)
    (128, 64, 16, 2, 2), (128, 64, 32, 2, 2),                # stride 2 through the zero-upsampled dY: dx at width 32 (fp32) and 64 (layer2.0: bf16)
    (1024, 1540, 16, 1, 1),                                  # conv_up3: 1540 output channels, the pack buffer filled to 99.2 %
]


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("Cout,Cin,W,N,stride", DGRADS)
def test_conv_dgrad_bf16_modes(mode, Cout, Cin, W, N, stride):
    """input gradient under the bf16 modes against float64 autograd of F.conv2d (mode bf16: of the operands rounded to bf16): plain,
    accumulate=True on a canary-filled dx (res aliases y in the kernel), and dx as a channel slice of a wider canary buffer"""
    from gpu_util import conv_kernels_of, hm_handle
    from egotap_amd import hm_ops as H
    h = hm_handle(mode)
    Wx = W * stride
    w, dy = _rand((Cout, Cin, 3, 3), 2, -0.1, 0.1), _rand((N, Cout, W, W), 3)
    routed = _bf_kernel(mode, 9, 1, Cin, Wx)
    x = torch.zeros((N, Cin, Wx, Wx), dtype=torch.float64, requires_grad=True)
    w64, dy64 = (_rb(w), _rb(dy)) if routed and mode == "bf16" else (w.double(), dy.double())
    F.conv2d(x, w64, None, stride, 1).backward(dy64)
    ref = x.grad
    atol = _conv_gate(mode, routed, ref)
    wd, dyd = w.cuda(), dy.cuda()
    dx = torch.full((N, Cin, Wx, Wx), 7.0, device="cuda")
    kern = conv_kernels_of(h, lambda: H.conv_dgrad(h, dyd, wd, dx, taps=9, stride=stride))
    assert len(kern) == 1 and kern[0][1] == 1, kern
    assert kern[0][0].startswith("conv_bf16_kernel<") == routed and (not routed or kern[0][0].endswith(f"W{Wx},{mode}>")), kern
    _twice(lambda: H.conv_dgrad(h, dyd, wd, dx, taps=9, stride=stride), dx)
    _close(dx, ref, atol=atol, rtol=0.0, msg=f"dx {mode}")
    # accumulate on top of a canary (small: the sum is rounded to fp32 once more, 2^-24 of its magnitude)
    def acc():
        dx.fill_(5.0)
        H.conv_dgrad(h, dyd, wd, dx, taps=9, stride=stride, accumulate=True)
    _twice(acc, dx)
    _close(dx, ref + 5.0, atol=atol + 2.0 ** -24 * (5.0 + float(ref.abs().max())), rtol=0.0, msg=f"dx accumulate {mode}")
    # into channels [3, 3 + Cin) of a wider buffer
    wide = torch.full((N, Cin + 8, Wx, Wx), CANARY, device="cuda")
    _twice(lambda: H.conv_dgrad(h, dyd, wd, H.View(wide, 3, Cin), taps=9, stride=stride), wide)
    assert torch.equal(wide[:, 3:3 + Cin], _twice(lambda: H.conv_dgrad(h, dyd, wd, dx, taps=9, stride=stride), dx))
    assert bool((wide[:, :3] == CANARY).all()) and bool((wide[:, 3 + Cin:] == CANARY).all())


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("Cin,Cout,W,N", [(20, 132, 32, 2), (72, 64, 64, 2)])
def test_conv_fwd_bf16_modes_on_slices(mode, Cin, Cout, W, N):
    """the decoder's use of the forward kernel: bias + ReLU into a channel slice of a concat buffer, input read from a channel slice"""
    from gpu_util import conv_kernels_of, hm_handle
    from egotap_amd import hm_ops as H
    h = hm_handle(mode)
    xw, w, b = _rand((N, Cin + 9, W, W), 1), _rand((Cout, Cin, 3, 3), 2, -0.1, 0.1), _rand((Cout,), 4)
    x = xw[:, 5:5 + Cin]
    xs, ws = (_rb(x), _rb(w)) if mode == "bf16" else (x.double(), w.double())
    ref = F.relu(F.conv2d(xs, ws, b.double(), 1, 1))
    xd, wd, bd = xw.cuda(), w.cuda(), b.cuda()
    wide = torch.full((N, Cout + 11, W, W), CANARY, device="cuda")
    run = lambda: H.conv_fwd(h, H.View(xd, 5, Cin), wd, H.View(wide, 4, Cout), bias=bd, taps=9, relu=True)     # noqa: E731
    kern = conv_kernels_of(h, run)
    assert kern == [(f"conv_bf16_kernel<3x3,s1,W{W},{mode}>", 1)], kern
    _twice(run, wide)
    _close(wide[:, 4:4 + Cout], ref, atol=_conv_gate(mode, True, ref), rtol=0.0, msg=f"conv_fwd {mode}")
    assert float(ref.mean()) > 0 and bool((ref == 0).any())                       # the ReLU cuts
    assert bool((wide[:, :4] == CANARY).all()) and bool((wide[:, 4 + Cout:] == CANARY).all())


def test_conv_bf16_modes_without_a_pack_buffer_run_fp32():
    """what the helper is for: set_precision alone leaves conv_any on the fp32 kernels"""
    from gpu_util import conv_kernels_of
    from egotap_amd import hm_ops as H
    from egotap_amd import networks
    from gpu_util import make_opt
    opt = make_opt()
    opt.num_rot_heatmap = 0
    net = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", input_channel_scale=2).cuda()
    net.set_precision("bf16")
    h = net._ensure_handle()
    x, w, y = _rand((1, 16, 16, 16), 1).cuda(), _rand((128, 16, 3, 3), 2).cuda(), torch.empty((1, 128, 16, 16), device="cuda")
    kern = conv_kernels_of(h, lambda: H.conv_fwd(h, x, w, y, taps=9))
    assert len(kern) == 1 and kern[0][0].startswith("conv_f32_kernel<"), kern


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, False)])
def test_bn2d_per_eye_slices_accumulate(relu, with_res):
    """bn2d_fwd / bn2d_bwd as hm_training._bn_fwd / _bn_bwd call them: once per eye on the two channel-slice views of a [B, 2C, s, s]
    buffer (image stride = twice the slice), dgamma / dbeta written by eye 0 and accumulated by eye 1; against float64 per-eye BatchNorm.
    relu=False, y=None is the downsample branch."""
    from egotap_amd import hm_ops as H
    B, C_, s = 3, 64, 32
    z, res, dy = _rand((B, 2 * C_, s, s), 1, -2, 2), _rand((B, 2 * C_, s, s), 2), _rand((B, 2 * C_, s, s), 7)
    g, b = _rand((C_,), 3, 0.5, 1.5), _rand((C_,), 4)
    rm, rv = _rand((C_,), 5), _rand((C_,), 6, 0.5, 2.0)
    gr, br = g.double().requires_grad_(True), b.double().requires_grad_(True)
    rm64, rv64 = rm.double().clone(), rv.double().clone()
    refs = []
    for e in range(2):
        sl = slice(e * C_, (e + 1) * C_)
        zr, rr = z[:, sl].double().requires_grad_(True), res[:, sl].double().requires_grad_(True)
        y = F.batch_norm(zr, rm64, rv64, gr, br, True, 0.1, 1e-5)
        if with_res:
            y = y + rr
        if relu:
            y = F.relu(y)
        y.backward(dy[:, sl].double())
        refs.append((y.detach(), zr.grad, rr.grad, gr.grad.clone(), br.grad.clone(), rm64.clone(), rv64.clone()))
    zd, resd, dyd, gd, bd = z.cuda(), res.cuda(), dy.cuda(), g.cuda(), b.cuda()
    yd = torch.full_like(zd, CANARY)
    dz, dres = torch.full_like(zd, CANARY), torch.full_like(zd, CANARY)
    dg, db = torch.full((C_,), CANARY, device="cuda"), torch.full((C_,), CANARY, device="cuda")
    for rep in range(2):
        rmd, rvd = rm.cuda(), rv.cuda()
        stats = []
        for e in range(2):
            stats.append(H.bn2d_fwd(H.View(zd, e * C_, C_), H.View(yd, e * C_, C_), gd, bd, rmd, rvd, res=H.View(resd, e * C_, C_) if with_res else None, relu=relu))
            if e == 0:
                assert bool((yd[:, C_:] == CANARY).all()) or rep == 1                   # eye 0 leaves eye 1's channels alone
            _close(rmd, refs[e][5], 1e-6)
            _close(rvd, refs[e][6], 1e-5)
        for e in range(2):
            H.bn2d_bwd(H.View(zd, e * C_, C_), H.View(yd, e * C_, C_) if relu else None, H.View(dyd, e * C_, C_), gd, stats[e][0], stats[e][1],
                       H.View(dz, e * C_, C_), dg, db, dres=H.View(dres, e * C_, C_) if with_res else None, relu=relu, accumulate=e == 1)
            _close(dg, refs[e][3], 2e-3, rtol=1e-4, msg=f"dgamma after eye {e}")             # (autograd accumulates over the eyes as well)
            _close(db, refs[e][4], 2e-3, rtol=1e-4, msg=f"dbeta after eye {e}")
        if rep == 0:
            first = [t.clone() for t in (yd, dz, dres, dg, db, rmd, rvd)]
        else:
            assert all(torch.equal(a, c) for a, c in zip(first, (yd, dz, dres, dg, db, rmd, rvd)))
    for e in range(2):
        sl = slice(e * C_, (e + 1) * C_)
        _close(yd[:, sl], refs[e][0], 2e-5, msg=f"y eye {e}")
        _close(dz[:, sl], refs[e][1], 2e-5, rtol=1e-3, msg=f"dz eye {e}")
        if with_res:
            _close(dres[:, sl], refs[e][2], 1e-6, msg=f"dres eye {e}")
    if not with_res:
        assert bool((dres == CANARY).all())


def test_width_128_operators():
    """what a stage-1 step at heatmap side 128 (512 x 512 RGB) would reach and nothing else does.  The 3x3 and 1x1 weight gradients at
    wout = 128 do not exist (hm_train.h: only the stem's 7x7 / 2 is instantiated at that width; a 128-wide double-buffered row tile of the
    others exceeds the LDS): the ABI says so by name and leaves dW alone, and hm_training.hm_train_forward refuses the side.  The 3x3 input
    gradient at wout = 128 and the max-pool backward at side 256 exist: against float64 autograd."""
    from gpu_util import hm_handle
    from egotap_amd import hm_ops as H
    from egotap_amd import lib as L
    h = hm_handle("f32")
    N, Cin, Cout, W = 2, 20, 72, 128
    x, dy = _rand((N, Cin, W, W), 1), _rand((N, Cout, W, W), 3)
    for ks in (3, 1):
        dw = torch.full((Cout, Cin, ks, ks), 3.0, device="cuda")
        with pytest.raises(L.EgotapError, match=f"egotap_hmtrain_conv_wgrad: unsupported ks={ks} stride=1 wout=128"):
            H.conv_wgrad(dy.cuda(), x.cuda(), dw, ks=ks, stride=1)
        torch.cuda.synchronize()
        assert bool((dw == 3.0).all())
    w, dy = _rand((64, Cin, 3, 3), 2, -0.1, 0.1), _rand((N, 64, W, W), 4)
    xr = torch.zeros((N, Cin, W, W), dtype=torch.float64, requires_grad=True)
    F.conv2d(xr, w.double(), None, 1, 1).backward(dy.double())
    dx = torch.full((N, Cin, W, W), 7.0, device="cuda")
    _twice(lambda: H.conv_dgrad(h, dy.cuda(), w.cuda(), dx, taps=9), dx)
    _close(dx, xr.grad, atol=2e-4 * float(xr.grad.abs().mean()) + 1e-5, rtol=0.0, msg="dx at width 128")
    x = _rand((2, 3, 256, 256), 5)
    x[1, 2, 2:7, 251:256] = 0.25                                  # ties, at the right edge
    xr = x.double().requires_grad_(True)
    dy = _rand((2, 3, 128, 128), 6)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.double())
    dx = torch.full_like(x, 9.0, device="cuda")
    _twice(lambda: H.maxpool_bwd(x.cuda(), dy.cuda(), dx), dx)
    _close(dx, xr.grad, 1e-6, msg="maxpool backward, side 256")
