"""Every stage of the bf16 heatmap decoder (EGOTAP_PREC_BF16: conv_bf16s.h, egotap_abi.hip hm_bf16_decoder; net_architecture.py:139-173)
against float64 arithmetic on ITS OWN inputs as the GPU produced them.

End to end the bf16 estimator is gated at 2 % relative L2 against the float64 oracle (test_gpu_hm.py): about ten bf16 roundings deep, so a
stage error below that budget -- a few border pixels of a 3x3 convolution, a few channels of a concat slice, a systematic half-ulp bias --
passes it, and a failure there does not say which stage is wrong.  Here every stage is read back from the workspace
and recomputed in float64 from the bf16 tensors the stage before it stored and the weights rounded to bf16 (round to nearest even, as the
pack kernel rounds them).  What is left between the two is the fp32 accumulation and one bf16 rounding of the stored value:

* bf16 outputs: |got - ref| <= 2^-8 |ref| + 1.01 delta per element (half a bf16 spacing is at most 2^-8 of the value it rounds, and the
  value rounded is within delta of ref), AND at least 95 % of the elements whose correctly rounded value is not zero are bit-equal to
  bf16(ref): a stored value differs from it only where the fp32 sum lies on the other side of a rounding midpoint than the exact sum, and a
  typical fp32 error of a few u sum|t| is 1e-7 .. 1e-4 of the value against a bf16 spacing of 2^-8 .. 2^-7 of it -- a fraction of a percent
  of the elements.  A systematic error (a weight truncated instead of rounded, a bias added in bf16, a stale channel) moves far more.
* GEMM stages (1x1, 3x3, conv_heatmap): delta = 20 sqrt(n) u sum|t| over the n = K + 1 terms (products of bf16 operands, exact in fp32,
  and the bias) -- the probabilistic bound of fp32 summation in any order (Higham & Mary 2019: lambda sqrt(n) u sum|t| except with
  probability 2 n exp(-lambda^2 / 2)) at lambda = 10 with the unit roundoff u = 2^-24 doubled in case the matrix core's adds truncate.
* bilinear upsample (align_corners=True, fp32 arithmetic on four bf16 corners): delta = (8 h + 8) u max|v| over the (frame, channel) map
  of side h -- the source coordinate is computed in fp32 (at most 2 h u off per axis, moving a weight pair over a difference of at most
  2 max|v|), then four products and three sums.
* conv_heatmap stores fp32 NCHW: |got - ref| <= 1.01 delta.

Three routings: B = 2 (every 3x3 convolution split over K on the 32-deep kernel, the serving path), B = 37 (all three on the 64-deep kernel
with the scalar-origin operand addressing; ragged last row tile of the 8 x 8 level), EgoCap B = 1 (128 x 128 maps, conv_up1 unsplit on the
64-deep kernel, the others split; conv_heatmap on the 128-column tile)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from egotap_amd.synthetic import synth_input

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _rb(t):
    return t.float().bfloat16().double()


def _conv1(x, w, b):
    """1x1 convolution on channels-last x [n, s, s, Cin]: (value, sum of |terms|), float64"""
    xs = x.reshape(-1, x.shape[-1])
    v = xs @ w.reshape(w.shape[0], -1).T + b
    a = xs.abs() @ w.reshape(w.shape[0], -1).abs().T + b.abs()
    return v.reshape(*x.shape[:-1], -1), a.reshape(*x.shape[:-1], -1)


def _conv3(x, w, b):
    """3x3 convolution, zero padding 1 (F.conv2d's cross-correlation) on channels-last x [n, s, s, Cin], as nine shifted products"""
    n, s, _, cin = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    v = b.expand(n * s * s, -1).clone()
    a = b.abs().expand(n * s * s, -1).clone()
    for dy in range(3):
        for dx in range(3):
            xt = xp[:, dy:dy + s, dx:dx + s, :].reshape(-1, cin)
            wt = w[:, :, dy, dx]
            v += xt @ wt.T
            a += xt.abs() @ wt.abs().T
    return v.reshape(n, s, s, -1), a.reshape(n, s, s, -1)


def _up(t):
    """F.interpolate(scale_factor=2, bilinear, align_corners=True) on channels-last [n, h, h, C]"""
    return F.interpolate(t.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


@pytest.mark.parametrize("which,preset,hm,B,frames", [("rot", "UnrealEgo", 64, 2, (0, 1)), ("pos", "UnrealEgo", 64, 37, (0, 18, 36)),
                                                      ("rot", "EgoCap", 128, 1, (0,))])
def test_every_bf16_decoder_stage_against_float64_on_its_own_inputs(which, preset, hm, B, frames):
    from gpu_util import hm_net
    from egotap_amd import lib
    L = lib.load()
    net, sd_np = hm_net(which, preset=preset, hm=hm)
    S = 4 * hm
    nb = min(B, 4)          # distinct frames (the hash generator is slow): larger batches cycle through them with a per-frame scale
    left = torch.from_numpy(synth_input(f"rgbL_dec_{which}{hm}", (nb, 3, S, S), -2.0, 2.0)).cuda()
    right = torch.from_numpy(synth_input(f"rgbR_dec_{which}{hm}", (nb, 3, S, S), -2.0, 2.0)).cuda()
    if B > nb:
        idx = torch.arange(B, device="cuda") % nb
        gain = (1.0 + 0.01 * torch.arange(B, device="cuda", dtype=torch.float32)).view(B, 1, 1, 1)
        left, right = (left[idx] * gain).contiguous(), (right[idx] * gain).contiguous()
    fr = torch.tensor(frames, device="cuda")
    s64, s32, s16, s8 = hm, hm // 2, hm // 4, hm // 8

    def read(name, s, c):
        """bf16 channels-last [B, s, s, c] at the intermediate's offset (the bf16 map lives in the slot of the fp32 one)"""
        off, n = C.c_size_t(), C.c_int64()
        lib.check(L.egotap_hm_intermediate(net._ensure_handle(), B, name.encode(), C.byref(off), C.byref(n)))
        nbytes = B * s * s * c * 2
        assert nbytes <= 4 * n.value and off.value + nbytes <= net._ws.numel(), name
        return net._ws[off.value: off.value + nbytes].view(torch.bfloat16).view(B, s, s, c).clone()
    try:
        net.set_precision("bf16")
        y = net(left, right)
        torch.cuda.synchronize()
        lv = {i: read(f"layer{i}_bf16", s, 2 * c) for i, s, c in ((1, s64, 64), (2, s32, 128), (3, s16, 256), (4, s8, 512))}
        T4, C3, Y3 = read("u4", s8, 1024), read("cat3", s16, 1600), read("conv_up3", s16, 1024)
        C2, Y2 = read("cat2", s32, 1280), read("conv_up2", s32, 512)
        C1, Y1 = read("cat1", s64, 640), read("conv_up1", s64, 512)
        y = y.clone()
    finally:
        net.set_precision("f32")
    # channels 1540..1599 of the first concat pad conv_up3's K to a multiple of 64: zero in every frame (1540..1543 are the 1x1 kernel's guard
    # columns, zero weights and bias through the ReLU; the rest the forward clears)
    assert int(torch.count_nonzero(C3[..., 1540:])) == 0
    d = lambda t: t[fr].double()          # noqa: E731
    a = "after_backbone."
    wt = lambda k: _rb(torch.from_numpy(sd_np[a + k + ".weight"])).cuda()                # noqa: E731
    bs = lambda k: torch.from_numpy(sd_np[a + k + ".bias"]).double().cuda()              # noqa: E731
    stats = {}

    def gate_bf16(name, got, ref, delta):
        got = got.double()
        err = (got - ref).abs()
        tol = 2.0 ** -8 * ref.abs() + 1.01 * delta
        rr = _rb(ref)
        live = rr != 0
        n_live = int(live.sum())
        exact = float((got[live] == rr[live]).double().mean()) if n_live else 0.0
        rel = float((got - ref).norm() / ref.norm().clamp_min(1e-300))
        i = int((err - tol).argmax())
        stats[name] = f"err/tol {float((err / tol.clamp_min(1e-300)).max()):.3f}  exact {exact * 100:.2f} %  rel L2 {rel:.2e}  nonzero {n_live / ref.numel() * 100:.0f} %"
        print(f"{name:>26}: {stats[name]}")
        assert not bool((err > tol).any()), (name, int((err > tol).sum()), float(err.reshape(-1)[i]), float(tol.reshape(-1)[i]),
                                              float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]))
        assert n_live >= 0.01 * ref.numel(), (name, n_live)          # the stage carries real values, not a map the ReLU emptied
        assert exact >= 0.95, (name, exact)

    def gemm(x, k, taps):
        w, b = wt(k), bs(k)
        v, ab = (_conv3 if taps == 9 else _conv1)(x, w, b)
        n = taps * x.shape[-1] + 1
        return v, 20.0 * math.sqrt(n) * U * ab

    def up_stage(name, src, got):
        h = src.shape[1]
        delta = (8 * h + 8) * U * src.abs().amax(dim=(1, 2), keepdim=True)
        gate_bf16(name, got, _up(src), delta.expand_as(got))

    # E4: layer4_1x1 (on the two eyes' concatenated level 4), upsample into cat3[:1024], layer3_1x1 into cat3[1024:1540]
    v, dl = gemm(d(lv[4]), "layer4_1x1.0", 1)
    gate_bf16("layer4_1x1", d(T4), v.clamp_min(0.0), dl)
    up_stage("upsample -> cat3[:1024]", d(T4), d(C3)[..., :1024])
    v, dl = gemm(d(lv[3]), "layer3_1x1.0", 1)
    gate_bf16("layer3_1x1 -> cat3[1024:]", d(C3)[..., 1024:1540], v.clamp_min(0.0), dl)
    # E5: conv_up3 on cat3 (1540 channels), upsample into cat2[:1024], layer2_1x1 into cat2[1024:]
    v, dl = gemm(d(C3)[..., :1540], "conv_up3.0", 9)
    gate_bf16("conv_up3", d(Y3), v.clamp_min(0.0), dl)
    up_stage("upsample -> cat2[:1024]", d(Y3), d(C2)[..., :1024])
    v, dl = gemm(d(lv[2]), "layer2_1x1.0", 1)
    gate_bf16("layer2_1x1 -> cat2[1024:]", d(C2)[..., 1024:], v.clamp_min(0.0), dl)
    # E6: conv_up2, upsample into cat1[:512], layer1_1x1 into cat1[512:]
    v, dl = gemm(d(C2), "conv_up2.0", 9)
    gate_bf16("conv_up2", d(Y2), v.clamp_min(0.0), dl)
    up_stage("upsample -> cat1[:512]", d(Y2), d(C1)[..., :512])
    v, dl = gemm(d(lv[1]), "layer1_1x1.0", 1)
    gate_bf16("layer1_1x1 -> cat1[512:]", d(C1)[..., 512:], v.clamp_min(0.0), dl)
    # E7: conv_up1
    v, dl = gemm(d(C1), "conv_up1.0", 9)
    gate_bf16("conv_up1", d(Y1), v.clamp_min(0.0), dl)
    # E8: conv_heatmap, no ReLU, fp32 NCHW: the estimator's output itself
    v, dl = gemm(d(Y1), "conv_heatmap", 1)
    got = y[fr].double().permute(0, 2, 3, 1)
    assert got.shape == v.shape, (tuple(got.shape), tuple(v.shape))
    err = (got - v).abs()
    ratio = float((err / (1.01 * dl).clamp_min(1e-300)).max())
    print(f"{'conv_heatmap':>26}: err/tol {ratio:.3f}  rel L2 {float((got - v).norm() / v.norm()):.2e}")
    assert not bool((err > 1.01 * dl).any()), ("conv_heatmap", int((err > 1.01 * dl).sum()), float(err.max()))
