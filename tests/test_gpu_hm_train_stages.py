"""Every stage of one stage-1 training step of a heatmap estimator (egotap_amd/hm_training.py HmTrainFn: about 60 kernel launches chained
in Python) against float64 arithmetic on ITS OWN inputs as the GPU produced them.

End to end the step is gated at the fp32 oracle's own distance from float64 (test_gpu_hm_train_step.py: 1e-2 relative in the backbone,
5e-2 / 0.6 in the bf16 modes), so one wrong channel of 1540, a dropped pixel row, a channel offset into a concat buffer that is off by
one, or a per-eye sum that overwrites instead of accumulating passes there.  Here the module's ``_stage_trace`` keeps every tensor of the
step; each stage is recomputed in float64 on the CPU from the tensors the GPU fed it (ReLU masks from the GPU's own outputs, BatchNorm
backward from the GPU's saved mean / rstd) and compared under the gate of that operator's own test in test_gpu_hm_train_ops.py:

* convolutions (forward, input gradient, weight gradient) on the fp32 kernels: |err| <= 2e-4 mean|ref| + 1e-5;
  routed to the bf16 matrix cores in mode bf16x3: 3e-4 mean|ref| + 1e-5 (the 2^-16 error model of test_conv_wgrad_bf16_modes);
  in mode bf16: 2e-4 mean|ref| + 1e-5 against float64 on operands rounded to bf16 (only the fp32 accumulation is left);
* BatchNorm: y, mean, rstd, running statistics 2e-5 / 1e-6 / 1e-5 absolute (+ 1e-4 relative) as test_bn2d_fwd_bwd; dz 2e-5 + 1e-3 |ref|;
  dgamma / dbeta 2e-3 + 1e-4 |ref| after eye 0 and for the sum after eye 1; dres 1e-6;
* max-pool 1e-6, ReLU backward / pyramid add / identity copy / publication exact bits, bilinear upsample 1e-5 (+ 1e-4 relative),
  per-channel bias sums under the convolution gate.

The loss weight is chosen so that dpred = pred - gt (order one): with lambda = 1 the gradients are ~1e-6 and every absolute floor above
would pass anything.  A convolution whose float64 reference costs more than ~1 GFLOP is compared on a subset of output channels (exact:
dW[co] depends only on dy[:, co], dx[:, ci] only on w[:, ci]): channel 0, the last one, both ends of and one more channel from every 128-
(64-) channel tile, every channel of a ragged last tile; all images, all pixels.  Which kernel ran each convolution is read from the
library's timing hook after every launch: in the bf16 modes the 3x3 stride-1 stages must have run conv_bf16_kernel, in f32 none may."""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

from egotap_amd.synthetic import synth_input

pytestmark = pytest.mark.gpu
BB = "backbone.backbone.backbone."
AB = "after_backbone."


def _net(which, model_name, hm):
    from egotap_amd import networks
    from egotap_amd.options import preset_defaults
    from egotap_amd.synthetic import synth_hm_state_dict
    opt = preset_defaults("UnrealEgo", hm)
    if which == "pos":
        opt.num_rot_heatmap = 0
    else:
        opt.num_heatmap = 0
    net = networks.HeatMap_UnrealEgo_Shared(opt, model_name, input_channel_scale=2)
    sd_np = synth_hm_state_dict(net.num_heatmap, f"hm_{which}.", model_name)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    return net.cuda()


def d(t):
    return t.detach().double().cpu()


def rb(t):
    """round to bf16 (nearest even, as the pack and staging code of conv_bf16.h / the bf16 weight gradient round), back in float64"""
    return t.float().bfloat16().double()


def fwd_route(mode, taps, stride, cout, w):
    """precision of the kernel conv_any picks (abi_conv_routing.inc) for a forward-form convolution with `cout` output channels at width w"""
    if mode == "f32" or taps != 9 or stride != 1:
        return "f32"
    if (cout >= 128 and w in (64, 32, 16, 8)) or (cout == 64 and w == 64) or (mode == "bf16" and cout == 64 and w == 128):
        return mode
    return "f32"


def wgrad_route(mode, ks, stride, w):
    """... and of egotap_hmtrain_conv_wgrad"""
    return mode if mode != "f32" and ks == 3 and stride == 1 and w in (64, 32, 16) else "f32"


CONV_COEF = {"f32": 2e-4, "bf16x3": 3e-4, "bf16": 2e-4}


def subset(c, flops):
    """output channels a convolution is compared on (module docstring); every channel while the reference is cheap"""
    if flops <= 1e9:
        return list(range(c))
    tile = 64 if c <= 64 else 128
    s = {0, c - 1}
    for t0 in range(0, c, tile):
        n = min(tile, c - t0)
        s.update((t0, t0 + n - 1, t0 + (37 * (t0 // tile) + 11) % n))
        if n < tile:
            s.update(range(t0, c))
    return sorted(s)


class Gate:
    """collects (stage, worst error / tolerance); the test fails at the end with every stage that missed its gate"""

    def __init__(self, label):
        self.label, self.rows, self.bad = label, [], []

    def close(self, name, got, ref, atol, rtol=0.0, kind=""):
        got = d(got)
        assert got.shape == ref.shape, (name, tuple(got.shape), tuple(ref.shape))
        err = (got - ref).abs()
        tol = atol + rtol * ref.abs()
        ratio = float((err / tol).max()) if err.numel() else 0.0
        if not bool(torch.isfinite(got).all()):
            ratio = float("inf")
        self.rows.append((name, kind, ratio, float(err.max()), float(ref.abs().mean())))
        if not ratio <= 1.0:
            self.bad.append(f"{name} [{kind}]: err/tol {ratio:.3f}, max err {float(err.max()):.3e}, mean|ref| {float(ref.abs().mean()):.3e}")

    def conv(self, name, got, ref, route):
        self.close(name, got, ref, CONV_COEF[route] * float(ref.abs().mean()) + 1e-5, kind="conv " + route)

    def exact(self, name, got, ref):
        same = torch.equal(got.detach().cpu(), ref.detach().cpu())
        self.rows.append((name, "exact", 0.0 if same else float("inf"), 0.0, float(ref.detach().abs().double().mean())))
        if not same:
            self.bad.append(f"{name}: bits differ")

    def report(self):
        worst = {}
        for name, kind, ratio, err, mean in self.rows:
            if kind not in worst or ratio > worst[kind][0]:
                worst[kind] = (ratio, name, err, mean)
        print(f"--- {self.label}: {len(self.rows)} stage checks")
        for kind, (ratio, name, err, mean) in sorted(worst.items()):
            print(f"worst {kind:>12}: err/tol {ratio:.3f} at {name} (max err {err:.3e}, mean|ref| {mean:.3e})")
        for name, kind, ratio, err, mean in self.rows:
            if ratio > 0.5:
                print(f"   {name} [{kind}]: err/tol {ratio:.3f} (max err {err:.3e}, mean|ref| {mean:.3e})")
        assert not self.bad, f"{self.label}: {len(self.bad)} stages missed their gate:\n" + "\n".join(self.bad)


# ---------------------------------------------------------------------------------------------- float64 stages
def check_conv_fwd(g, name, mode, x, w, got, bias=None, relu=False, taps=9, stride=1):
    ks = 3 if taps == 9 else 7 if taps == 49 else 1
    cout, cin, wout = w.shape[0], w.shape[1], got.shape[3]
    route = fwd_route(mode, taps, stride, cout, wout)
    sub = subset(cout, 2.0 * cout * cin * ks * ks * got.shape[0] * wout * wout)
    x64, w64 = d(x), d(w)[sub]
    if route == "bf16":
        x64, w64 = rb(x64), rb(w64)
    ref = F.conv2d(x64, w64, d(bias)[sub] if bias is not None else None, stride, (ks - 1) // 2)
    if relu:
        ref = ref.clamp_min(0.0)
    g.conv(name, got[:, sub], ref, route)


def check_conv_dgrad(g, name, mode, dy, w, got, taps=9, stride=1, base=None):
    """got = [base +] d/dx conv(x, w) . dy: the forward kernel on flipped weights, `w.shape[1]` output channels at got's width"""
    ks = 3 if taps == 9 else 1
    cout, cin, win = w.shape[0], w.shape[1], got.shape[3]
    route = fwd_route(mode, taps, 1, cin, win)
    sub = subset(cin, 2.0 * cout * cin * taps * dy.shape[0] * dy.shape[3] ** 2)
    dy64, w64 = d(dy), d(w)[:, sub]
    if route == "bf16":
        dy64, w64 = rb(dy64), rb(w64)
    ref = torch.nn.grad.conv2d_input((got.shape[0], len(sub), win, win), w64, dy64, stride, (ks - 1) // 2)
    if base is not None:
        ref = ref + d(base[:, sub])
    g.conv(name, got[:, sub], ref, route)


def check_conv_wgrad(g, name, mode, dy, x, got, ks=3, stride=1):
    cout, cin, wout = got.shape[0], got.shape[1], dy.shape[3]
    route = wgrad_route(mode, ks, stride, wout)
    sub = subset(cout, 2.0 * cout * cin * ks * ks * dy.shape[0] * wout * wout)
    x64, dy64 = d(x), d(dy[:, sub])
    if route == "bf16":
        x64, dy64 = rb(x64), rb(dy64)
    ref = torch.nn.grad.conv2d_weight(x64, (len(sub), cin, ks, ks), dy64, stride, (ks - 1) // 2)
    g.conv(name, got[sub], ref, route)


def check_chansum(g, name, dy, got):
    ref = d(dy).sum((0, 2, 3))
    g.close(name, got, ref, 2e-4 * float(ref.abs().mean()) + 1e-5, kind="chansum")


def eyes(t, B):
    """[2B, C, s, s], image n = 2b + eye -> the two per-eye [B, C, s, s] tensors"""
    c = t.shape[1]
    v = t.reshape(B, 2 * c, t.shape[2], t.shape[3])
    return [v[:, e * c:(e + 1) * c] for e in range(2)]


def check_bn_fwd(g, name, B, z, y, gamma, beta, stats, run, res=None, relu=True):
    for e in range(2):
        z64 = d(eyes(z, B)[e])
        mean, var = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
        n = z64.numel() // z64.shape[1]
        ref = (z64 - mean[None, :, None, None]) / torch.sqrt(var + 1e-5)[None, :, None, None] * d(gamma)[None, :, None, None] + d(beta)[None, :, None, None]
        if res is not None:
            ref = ref + d(eyes(res, B)[e])
        if relu:
            ref = ref.clamp_min(0.0)
        g.close(f"{name} eye {e} y", eyes(y, B)[e], ref, 2e-5, 1e-4, kind="bn fwd")
        g.close(f"{name} eye {e} mean", stats[e][0], mean, 1e-6, 1e-4, kind="bn stats")
        g.close(f"{name} eye {e} rstd", stats[e][1], 1.0 / torch.sqrt(var + 1e-5), 1e-6, 1e-4, kind="bn stats")
        # the running statistics after this eye's update, from what the GPU held before it
        g.close(f"{name} eye {e} running_mean", run[e + 1][0], 0.9 * d(run[e][0]) + 0.1 * mean, 1e-6, 1e-4, kind="bn stats")
        g.close(f"{name} eye {e} running_var", run[e + 1][1], 0.9 * d(run[e][1]) + 0.1 * var * n / (n - 1), 1e-5, 1e-4, kind="bn stats")


def check_bn_bwd(g, name, B, z, y, dy, gamma, stats, dz, dg0, db0, dg, db, dres=None, relu=True):
    """per eye: dz, dres; dgamma / dbeta as eye 0 wrote them, then the sum eye 1 left (on top of the GPU's own eye-0 values)"""
    for e in range(2):
        z64, go = d(eyes(z, B)[e]), d(eyes(dy, B)[e])
        if relu:
            go = go * (d(eyes(y, B)[e]) > 0)
        mean, rstd = d(stats[e][0])[None, :, None, None], d(stats[e][1])[None, :, None, None]
        n = z64.numel() // z64.shape[1]
        xh = (z64 - mean) * rstd
        dbeta, dgamma = go.sum((0, 2, 3)), (go * xh).sum((0, 2, 3))
        ref = d(gamma)[None, :, None, None] * rstd * (go - dbeta[None, :, None, None] / n - xh * dgamma[None, :, None, None] / n)
        g.close(f"{name} eye {e} dz", eyes(dz, B)[e], ref, 2e-5, 1e-3, kind="bn dz")
        if dres is not None:
            g.close(f"{name} eye {e} dres", eyes(dres, B)[e], go, 1e-6, 1e-4, kind="bn dres")
        if e == 0:
            g.close(f"{name} eye 0 dgamma", dg0, dgamma, 2e-3, 1e-4, kind="bn dgamma/dbeta")
            g.close(f"{name} eye 0 dbeta", db0, dbeta, 2e-3, 1e-4, kind="bn dgamma/dbeta")
        else:
            g.close(f"{name} eye 0+1 dgamma", dg, d(dg0) + dgamma, 2e-3, 1e-4, kind="bn dgamma/dbeta")
            g.close(f"{name} eye 0+1 dbeta", db, d(db0) + dbeta, 2e-3, 1e-4, kind="bn dgamma/dbeta")


def up64(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)


def check_upsample_bwd(g, name, dy, got):
    src = torch.zeros(tuple(got.shape), dtype=torch.float64, requires_grad=True)
    up64(src).backward(d(dy))
    g.close(name, got, src.grad, 1e-5, 1e-4, kind="upsample")


# ---------------------------------------------------------------------------------------------- the traced step
def traced_step(which, model_name, mode, B, hm):
    """one real step with the stage trace on and the kernel of every conv_any launch recorded -> (net, trace, conv launches, pred)"""
    from egotap_amd import hm_ops as H
    from egotap_amd import lib as L
    net = _net(which, model_name, hm)
    net.train()
    net.set_precision(mode)
    net._stage_trace = tr = {}
    S0, n2 = 4 * hm, 2 * net.num_heatmap
    left = torch.from_numpy(synth_input(f"st_rgbL_{which}{hm}", (B, 3, S0, S0), -2.0, 2.0)).cuda()
    right = torch.from_numpy(synth_input(f"st_rgbR_{which}{hm}", (B, 3, S0, S0), -2.0, 2.0)).cuda()
    gt = torch.from_numpy(synth_input(f"st_gt_{which}{hm}", (B, n2, hm, hm), 0.0, 1.0)).cuda()
    plen = torch.from_numpy(synth_input(f"st_plen_{which}{hm}", (B, n2), 2.0, 40.0)).cuda() if which == "rot" else None
    lib, h = L.load(), net._ensure_handle()
    launches, orig = [], H.conv_fwd

    def conv_fwd(hh, x, w, y, bias=None, res=None, taps=9, stride=1, relu=False):
        orig(hh, x, w, y, bias=bias, res=res, taps=taps, stride=stride, relu=relu)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(hh, C.byref(n), C.byref(ms), C.byref(fl)))
        det = json.loads(lib.egotap_timing_detail(hh).decode())
        assert n.value == 1 and len(det) == 1, det
        launches.append(dict(taps=taps, stride=stride, cin=w.shape[1], cout=w.shape[0], w=H.V(y).W, accumulate=res is not None and H.V(res).t is H.V(y).t,
                             kernel=det[0]["kernel"]))

    L.check(lib.egotap_timing_enable(h, 1))
    H.conv_fwd = conv_fwd
    try:
        pred = net(left, right)
        # lambda such that dpred = pred - gt (position net; the limb net divides by the limb lengths on top): gradients of order one
        loss, dpred = H.mse(pred.detach().contiguous(), gt, plen, B * net.num_heatmap * hm * hm / 2.0)
        pred.backward(dpred)
        torch.cuda.synchronize()
    finally:
        H.conv_fwd = orig
        L.check(lib.egotap_timing_enable(h, 0))
        del net._stage_trace
    assert float(dpred.abs().mean()) > 1e-3
    return net, tr, launches, pred, dpred


def check_routes(mode, launches, hm):
    for c in launches:
        want = fwd_route(mode, c["taps"], c["stride"], c["cout"], c["w"])
        bf = c["kernel"].startswith("conv_bf16_kernel<")
        assert bf == (want != "f32"), (mode, c)
        if bf:
            assert c["kernel"] == f"conv_bf16_kernel<3x3,s1,W{c['w']},{mode}>", c
    ran = {(c["cin"], c["cout"], c["w"], c["accumulate"]) for c in launches if c["kernel"].startswith("conv_bf16_kernel<")}
    if mode == "f32":
        assert not ran
        return
    s = hm
    # input gradients of conv_up3 / conv_up2 / conv_up1 (ragged 1540, the pack buffer nearly full), of a stride-2 conv1 through the zero-
    # upsampled dY (layer2.0: 128 -> 64 channels at the input's width), the accumulating one of layer1, and the decoder's forward convolutions
    for shape in ((1024, 1540, s // 4, False), (512, 1280, s // 2, False), (512, 640, s, False), (128, 64, s, True), (64, 64, s, True),
                  (1540, 1024, s // 4, False), (1280, 512, s // 2, False), (640, 512, s, False)):
        assert shape in ran, (shape, sorted(ran))


def check_step(label, net, tr, mode, pred, dpred):
    from egotap_amd.hm_training import TRACE_CANARY
    g = Gate(label)
    P = dict(net.named_parameters())
    sv = tr["saved"]
    B = sv["B"]
    # ------------------------------------------------------------------ forward
    check_conv_fwd(g, "stem conv", mode, sv["x0"], P[BB + "conv1.weight"], sv["z0"], taps=49, stride=2)
    check_bn_fwd(g, "stem bn1", B, sv["z0"], sv["l0"], P[BB + "bn1.weight"], P[BB + "bn1.bias"], sv["m0"], tr["run:" + BB + "bn1"])
    g.close("maxpool", sv["p0"], F.max_pool2d(d(sv["l0"]), 3, 2, 1), 1e-6, kind="maxpool")
    blocks = sv["blocks"]
    assert len(blocks) == sum(net.blocks) and blocks[0]["xin"] is sv["p0"]
    for bi, r in enumerate(blocks):
        k = r["k"]
        if bi:
            assert r["xin"] is blocks[bi - 1]["y2"], k
        check_conv_fwd(g, k + "conv1", mode, r["xin"], P[k + "conv1.weight"], r["z1"], stride=r["stride"])
        check_bn_fwd(g, k + "bn1", B, r["z1"], r["y1"], P[k + "bn1.weight"], P[k + "bn1.bias"], r["m1"], tr["run:" + k + "bn1"])
        idt = r["xin"]
        assert ("zd" in r) == (k + "downsample.0.weight" in P), k
        if "zd" in r:
            check_conv_fwd(g, k + "downsample.0", mode, r["xin"], P[k + "downsample.0.weight"], r["zd"], taps=1, stride=r["stride"])
            check_bn_fwd(g, k + "downsample.1", B, r["zd"], r["yd"], P[k + "downsample.1.weight"], P[k + "downsample.1.bias"], r["md"],
                         tr["run:" + k + "downsample.1"], relu=False)
            idt = r["yd"]
        check_conv_fwd(g, k + "conv2", mode, r["y1"], P[k + "conv2.weight"], r["z2"])
        check_bn_fwd(g, k + "bn2", B, r["z2"], r["y2"], P[k + "bn2.weight"], P[k + "bn2.bias"], r["m2"], tr["run:" + k + "bn2"], res=idt)
    pyr = [r["y2"] for r in blocks if r["level"] is not None]
    L = sv["L"]
    assert len(pyr) == 4 and all(L[i].data_ptr() == pyr[i].data_ptr() and L[i].shape[1] == 2 * pyr[i].shape[1] for i in range(4))

    def dec(name, x, got, taps):
        check_conv_fwd(g, name, mode, x, P[AB + name + ".weight"], got, bias=P[AB + name + ".bias"], relu=name != "conv_heatmap", taps=taps)

    def concat(cat, src, n, skip, level):
        after, full = tr[cat + "_after_upsample"], sv[cat]
        g.close(f"upsample -> {cat}[:{n}]", after[:, :n], up64(d(src)), 1e-5, 1e-4, kind="upsample")
        g.exact(f"{cat}[{n}:] untouched by the upsample", after[:, n:], torch.full_like(after[:, n:], TRACE_CANARY))
        dec(skip, L[level], full[:, n:], 1)
        g.exact(f"{cat}[:{n}] untouched by {skip}", full[:, :n], after[:, :n])

    dec("layer4_1x1.0", L[3], sv["u4"], 1)
    concat("cat3", sv["u4"], 1024, "layer3_1x1.0", 2)
    dec("conv_up3.0", sv["cat3"], sv["x3"], 9)
    concat("cat2", sv["x3"], 1024, "layer2_1x1.0", 1)
    dec("conv_up2.0", sv["cat2"], sv["x2"], 9)
    concat("cat1", sv["x2"], 512, "layer1_1x1.0", 0)
    dec("conv_up1.0", sv["cat1"], sv["x1"], 9)
    dec("conv_heatmap", sv["x1"], tr["out"], 1)
    g.exact("the prediction is the traced output", pred, tr["out"])
    # ------------------------------------------------------------------ backward: decoder
    g.exact("dout is the loss gradient", tr["dout"], dpred)

    def bias_conv_bwd(name, dz, x, dx, taps):
        ks = 3 if taps == 9 else 1
        check_conv_wgrad(g, name + " wgrad", mode, dz, x, tr["g:" + AB + name + ".weight"], ks=ks)
        check_chansum(g, name + " bias", dz, tr["g:" + AB + name + ".bias"])
        check_conv_dgrad(g, name + " dgrad", mode, dz, P[AB + name + ".weight"], dx, taps=taps)

    def relu_bwd(name, y, dy, got):
        g.exact("relu_bwd " + name, got, dy * (y > 0))

    bias_conv_bwd("conv_heatmap", tr["dout"], sv["x1"], tr["dx1"], 1)
    prev = tr["dx1"]
    for up, x, cat, n, skip, level, dxn in (("conv_up1.0", "x1", "cat1", 512, "layer1_1x1.0", 0, "dx2"), ("conv_up2.0", "x2", "cat2", 1024, "layer2_1x1.0", 1, "dx3"),
                                           ("conv_up3.0", "x3", "cat3", 1024, "layer3_1x1.0", 2, "du4")):
        dcat = tr["d" + cat]
        relu_bwd(up, sv[x], prev, tr["dz:" + up])
        bias_conv_bwd(up, tr["dz:" + up], sv[cat], dcat, 9)
        relu_bwd(skip, sv[cat][:, n:], dcat[:, n:], tr["dz:" + skip])
        bias_conv_bwd(skip, tr["dz:" + skip], L[level], tr[f"dL{level}"], 1)
        check_upsample_bwd(g, f"upsample_bwd d{cat}[:{n}]", dcat[:, :n], tr[dxn])
        prev = tr[dxn]
    relu_bwd("layer4_1x1.0", sv["u4"], tr["du4"], tr["dz:layer4_1x1.0"])
    bias_conv_bwd("layer4_1x1.0", tr["dz:layer4_1x1.0"], L[3], tr["dL3"], 1)
    # ------------------------------------------------------------------ backward: backbone, last block first
    dy_next = None
    for bi in range(len(blocks) - 1, -1, -1):
        r = blocks[bi]
        k, stride = r["k"], r["stride"]
        dy = tr[k + "dy"]
        if r["level"] is not None:
            share = tr[f"dL{r['level']}"].view(dy.shape)
            if dy_next is None:
                g.exact(k + "dy is the decoder's share", dy, share)
            else:
                g.exact(k + "dy before the pyramid add", tr[k + "dy_before_add"], dy_next)
                g.exact(k + "pyramid add", dy, tr[k + "dy_before_add"].cpu() + share.cpu())
        else:
            assert k + "dy_before_add" not in tr
            g.exact(k + "dy is the next block's dxin", dy, dy_next)
        G = lambda n: tr["g:" + k + n]            # noqa: E731
        E0 = lambda n: tr["eye0:" + k + n]        # noqa: E731
        check_bn_bwd(g, k + "bn2 bwd", B, r["z2"], r["y2"], dy, P[k + "bn2.weight"], r["m2"], tr[k + "dz2"], E0("bn2.weight"), E0("bn2.bias"),
                     G("bn2.weight"), G("bn2.bias"), dres=tr[k + "dres"])
        check_conv_wgrad(g, k + "conv2 wgrad", mode, tr[k + "dz2"], r["y1"], G("conv2.weight"))
        check_conv_dgrad(g, k + "conv2 dgrad", mode, tr[k + "dz2"], P[k + "conv2.weight"], tr[k + "dy1"])
        check_bn_bwd(g, k + "bn1 bwd", B, r["z1"], r["y1"], tr[k + "dy1"], P[k + "bn1.weight"], r["m1"], tr[k + "dz1"], E0("bn1.weight"), E0("bn1.bias"),
                     G("bn1.weight"), G("bn1.bias"))
        check_conv_wgrad(g, k + "conv1 wgrad", mode, tr[k + "dz1"], r["xin"], G("conv1.weight"), stride=stride)
        if "zd" in r:
            check_bn_bwd(g, k + "downsample.1 bwd", B, r["zd"], None, tr[k + "dres"], P[k + "downsample.1.weight"], r["md"], tr[k + "dzd"],
                         E0("downsample.1.weight"), E0("downsample.1.bias"), G("downsample.1.weight"), G("downsample.1.bias"), relu=False)
            check_conv_wgrad(g, k + "downsample.0 wgrad", mode, tr[k + "dzd"], r["xin"], G("downsample.0.weight"), ks=1, stride=stride)
            check_conv_dgrad(g, k + "downsample.0 dgrad", mode, tr[k + "dzd"], P[k + "downsample.0.weight"], tr[k + "dxin_first"], taps=1, stride=stride)
        else:
            g.exact(k + "identity branch of dxin", tr[k + "dxin_first"], tr[k + "dres"])
        check_conv_dgrad(g, k + "conv1 dgrad (accumulating)", mode, tr[k + "dz1"], P[k + "conv1.weight"], tr[k + "dxin"], stride=stride, base=tr[k + "dxin_first"])
        dy_next = tr[k + "dxin"]
    # ------------------------------------------------------------------ backward: stem
    g.exact("dp0 is layer1.0's dxin", tr["dp0"], dy_next)
    l0 = d(sv["l0"]).requires_grad_(True)
    F.max_pool2d(l0, 3, 2, 1).backward(d(tr["dp0"]))
    g.close("maxpool_bwd", tr["dl0"], l0.grad, 1e-6, 1e-4, kind="maxpool")
    k = BB
    check_bn_bwd(g, "stem bn1 bwd", B, sv["z0"], sv["l0"], tr["dl0"], P[k + "bn1.weight"], sv["m0"], tr["dz0"], tr["eye0:" + k + "bn1.weight"],
                 tr["eye0:" + k + "bn1.bias"], tr["g:" + k + "bn1.weight"], tr["g:" + k + "bn1.bias"])
    check_conv_wgrad(g, "stem wgrad", mode, tr["dz0"], sv["x0"], tr["g:" + k + "conv1.weight"], ks=7, stride=2)
    # ------------------------------------------------------------------ publication
    # every parameter but the ResNet's classifier (backbone.fc.*: never read by the estimator, no gradient in the reference either)
    trained = sorted(n for n in P if not n.startswith(BB + "fc."))
    assert len(trained) == len(P) - 2
    assert sorted(n for n, p in P.items() if p.grad is not None) == trained
    assert sorted(n[2:] for n in tr if n.startswith("g:")) == trained
    for n in trained:
        g.exact(".grad of " + n, P[n].grad, tr["g:" + n])
    g.report()


@pytest.mark.parametrize("which,model_name,mode", [("rot", "resnet18", "f32"), ("rot", "resnet18", "bf16x3"), ("rot", "resnet18", "bf16"),
                                                   ("pos", "resnet34", "f32")])
def test_every_stage_of_a_training_step_against_float64_on_its_own_inputs(which, model_name, mode):
    """B = 2, 256 x 256 RGB.  resnet18 sin / cos net (60 output channels) in the three precision modes; resnet34 position net (30 output
    channels: conv_heatmap's input gradient pads the contracted channels to 32; blocks without a downsample branch, so the identity route
    of dres, at every block but the first of layers 2 - 4)"""
    net, tr, launches, pred, dpred = traced_step(which, model_name, mode, 2, 64)
    check_routes(mode, launches, 64)
    check_step(f"{model_name} {which} {mode} B=2 256x256", net, tr, mode, pred, dpred)


def test_a_training_step_at_heatmap_side_128_is_refused_by_name():
    """512 x 512 RGB: spec.HM_BATCH_STATS_SIDES admits 128 to the batch-statistics forward, but the step cannot finish there -- run as above it
    got through the forward and the decoder's input gradients and then failed in the first weight gradient ("egotap_hmtrain_conv_wgrad:
    unsupported ks=1 stride=1 wout=128"; the 3x3 one is missing too, test_gpu_hm_train_ops.py test_width_128_operators), with the running
    statistics already moved.  The differentiable forward now refuses the side by name before it launches anything."""
    net = _net("pos", "resnet18", 128)
    net.train()
    x = torch.zeros((1, 3, 512, 512), device="cuda")
    before = {k: v.clone() for k, v in net.named_buffers()}
    with pytest.raises(NotImplementedError, match="stage-1 training.* is built at heatmap side 64 only .*not 128"):
        net(x, x)
    assert all(torch.equal(v, before[k]) for k, v in net.named_buffers())
