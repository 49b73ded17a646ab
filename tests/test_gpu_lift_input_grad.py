"""The lifting head's gradient w.r.t. its input heatmaps in train mode (egotap_lift_backward_dhm, the scatter epilogues of the patch
embedding and of the rotation encoder's fc1): autograd reaches the head's input as it does through the reference's plain-PyTorch head,
so the heatmap estimators can be trained through the pose loss.  Checked against float64 autograd over the oracle
(oracle/lift_ref.lift_forward_train with hm.requires_grad_()) and against the reference's own hm.grad (tests/golden/train_dhm_ue_b2.npz,
tools/make_golden.py gen_train_dhm)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from egotap_amd.synthetic import synth_input, synth_state_dict

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LAM_M, LAM_C = 0.1, -0.01


def _net(preset="UnrealEgo", hm=64, mode="f32", one_call=True):
    from egotap_amd import networks, spec
    from egotap_amd.options import preset_defaults
    p = spec.lift_preset(preset, hm)
    net = networks.EgoTAPAutoEncoder(preset_defaults(preset, hm), input_channel_scale=2)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
    net = net.cuda().train()
    net.set_precision(mode)
    net.one_call_training = one_call
    return net, p


def _inputs(p, B, tag):
    hm = torch.from_numpy(synth_input(f"hm_{tag}", (B, p.in_channels, p.hm_size, p.hm_size)))
    gt = torch.from_numpy(synth_input(f"gt_{tag}", (B, p.out_joints, 3), -1.0, 1.0))
    return hm, gt


def _step(net, hm, gt, want_dhm=True):
    """train-mode forward, PoseLossFn, backward; returns (pose, {param: grad}, hm.grad)"""
    from egotap_amd.training import PoseLossFn
    x = hm.cuda().requires_grad_(want_dhm)
    net.zero_grad()
    pose = net(x)[0]
    PoseLossFn.apply(net, pose, gt.cuda(), LAM_M, LAM_C).sum().backward()
    torch.cuda.synchronize()
    grads = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    return pose.detach().clone(), grads, x.grad


def _oracle_dhm(hm, gt, p):
    """hm.grad of the loss O.train_step builds, float64 autograd over the oracle's train-mode forward"""
    from egotap_amd import spec
    from oracle import lift_ref as O
    x = hm.double().requires_grad_()
    sd = O.to_torch_sd(synth_state_dict(spec.lift_state_spec(p)), torch.float64)
    pose, _ = O.lift_forward_train(x, sd, p)
    loss = O.loss_mpjpe(pose, gt.double()) * LAM_M + O.loss_cos_sim(pose, gt.double(), p) * LAM_C * LAM_M
    (g,) = torch.autograd.grad(loss, x)
    return g


def _groups(p):
    J = p.n_joints_hm
    return {"position": slice(0, 2 * J), "rotation": slice(2 * J, 6 * J)}


def _fp32_gates(got, ref, p, stride=97, groups=("position", "rotation")):
    """per channel group, _check_against_golden's gates: sample error <= 5e-3 x the group's RMS magnitude, L2 norm within 1e-3"""
    for name, sl in _groups(p).items():
        if name not in groups:
            continue
        a, b = got[:, sl].double().cpu().reshape(-1), ref[:, sl].double().reshape(-1)
        scale = float(b.norm()) / np.sqrt(b.numel())
        err = float((a[::stride] - b[::stride]).abs().max())
        assert err <= 5e-3 * scale, f"{name}: sample err {err:.3e} vs typical magnitude {scale:.3e}"
        np.testing.assert_allclose(float(a.norm()), float(b.norm()), rtol=1e-3, err_msg=name)


def _bf16_gates(got, ref, p, cos_min=0.98, rel_max=0.2, groups=("position", "rotation")):
    """per channel group, the _grad_gates rule of the bf16 mode: cosine > 0.98, relative L2 < 0.2"""
    for name, sl in _groups(p).items():
        if name not in groups:
            continue
        a, b = got[:, sl].double().cpu().reshape(-1), ref[:, sl].double().reshape(-1)
        cos = float(a @ b / (a.norm() * b.norm()))
        rel = float((a - b).norm() / b.norm())
        assert cos > cos_min and rel < rel_max, f"{name}: cos {cos:.5f} rel {rel:.3e}"


def test_train_mode_head_returns_the_heatmap_gradient_of_the_reference():
    """UnrealEgo 64^2, B = 2, fp32: hm.grad exists after the pose loss's backward and matches the float64 oracle and the reference's
    own hm.grad (the fixture's inputs are gen_train's)"""
    net, p = _net()
    hm = torch.from_numpy(synth_input("hm_train", (2, 90, 64, 64)))
    gt = torch.from_numpy(synth_input("gt_train", (2, 16, 3), -1.0, 1.0))
    _, _, dhm = _step(net, hm, gt)
    assert dhm is not None and dhm.shape == hm.shape and dhm.dtype == torch.float32
    assert torch.isfinite(dhm).all()
    _fp32_gates(dhm, _oracle_dhm(hm, gt, p), p)
    g = np.load(os.path.join(GOLD, "train_dhm_ue_b2.npz"))
    st = int(g["dhm_stride"])
    got = dhm.double().cpu()
    norms = g["dhm_plane_norms"]                                                   # [B, C]
    flat_c = np.arange(got.numel())[::st] // (64 * 64) % 90                        # channel of each sample
    sample = got.reshape(-1)[::st].numpy()
    for name, sl in _groups(p).items():
        sel = (flat_c >= sl.start) & (flat_c < sl.stop)
        ref_norm = float(np.sqrt((norms[:, sl] ** 2).sum()))
        scale = ref_norm / np.sqrt(2 * (sl.stop - sl.start) * 64 * 64)
        err = float(np.abs(sample[sel] - g["dhm_sample"][sel]).max())
        assert err <= 5e-3 * scale, f"{name}: sample err {err:.3e} vs typical magnitude {scale:.3e} (reference golden)"
        np.testing.assert_allclose(float(got[:, sl].norm()), ref_norm, rtol=1e-3, err_msg=name)


@pytest.mark.parametrize("preset,hm_size,B,mode", [("UnrealEgo", 64, 2, "bf16x3"), ("UnrealEgo", 64, 2, "bf16"), ("EgoCap", 64, 3, "f32"),
                                                   ("UnrealEgo", 128, 1, "f32")])
def test_heatmap_gradient_against_float64_oracle(preset, hm_size, B, mode):
    """The rotation channels (one product behind the small FC layers) get the fp32 gates in fp32 and bf16x3.  The position channels sit
    behind the whole ViT backward, whose rounding reaches them element by element (the parameter gradients, sums over every token,
    average it out): at 64^2 in fp32 they get the fp32 gates; in bf16x3 (split-bf16 products) and at 128^2 (softmax over 2304 keys,
    B = 1) the gradient at the patch embedding's output is measured 2.6-2.7e-3 from float64 in relative L2 (3-5 % of the RMS at the
    worst sampled element) while the scatter product itself adds 2e-5 -- they get cosine > 0.9999, relative L2 < 1e-2.  bf16: the bf16
    gates on both."""
    net, p = _net(preset, hm_size, mode)
    hm, gt = _inputs(p, B, f"dhm_{preset}_{hm_size}")
    _, _, dhm = _step(net, hm, gt)
    assert dhm is not None and torch.isfinite(dhm).all()
    ref = _oracle_dhm(hm, gt, p)
    if mode == "bf16":
        _bf16_gates(dhm, ref, p)
    elif mode == "bf16x3" or hm_size == 128:
        _fp32_gates(dhm, ref, p, groups=("rotation",))
        _bf16_gates(dhm, ref, p, cos_min=0.9999, rel_max=1e-2, groups=("position",))
    else:
        _fp32_gates(dhm, ref, p)


def test_input_dtype_is_kept():
    net, p = _net()
    hm, gt = _inputs(p, 2, "dhm_dtype")
    _, _, d32 = _step(net, hm, gt)
    _, _, d64 = _step(net, hm.double(), gt)
    assert d64.dtype == torch.float64 and torch.equal(d64, d32.double())


@pytest.mark.parametrize("preset,B,mode", [("UnrealEgo", 3, "f32"), ("EgoCap", 2, "f32"), ("UnrealEgo", 3, "bf16"), ("EgoCap", 2, "bf16x3")])
def test_one_call_equals_composition_and_gradients_do_not_change(preset, B, mode):
    """the one-call ABI and the Python composition give the same hm.grad bit for bit (they run the same operators); every parameter
    gradient and the pose are the same bits whether hm requires a gradient or not"""
    out = {}
    for one_call, want in ((True, True), (False, True), (True, False)):
        net, p = _net(preset, 64, mode, one_call)
        hm, gt = _inputs(p, B, f"onecall_{preset}")
        out[(one_call, want)] = _step(net, hm, gt, want)
    pose_a, g_a, d_a = out[(True, True)]
    pose_b, g_b, d_b = out[(False, True)]
    pose_c, g_c, d_c = out[(True, False)]
    assert d_c is None and d_a is not None and torch.isfinite(d_a).all()
    assert torch.equal(d_a, d_b)
    assert torch.equal(pose_a, pose_b) and torch.equal(pose_a, pose_c)
    assert sorted(g_a) == sorted(g_b) == sorted(g_c) and len(g_a) > 50
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]) and torch.equal(g_a[k], g_c[k]), k


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "bf16"])
def test_abi_writes_every_element_once_and_null_dhm_is_the_plain_backward(mode):
    """egotap_lift_backward_dhm on a NaN-filled dhm leaves no NaN (every element written, nothing relies on a clear); two calls give
    the same bits; the gradient arena is the same bits as egotap_lift_backward's with dhm and with dhm == NULL"""
    from egotap_amd import lib as L
    from egotap_amd import train_ops as T
    from egotap_amd import training as TR
    net, p = _net(mode=mode)
    B = 2
    hm, _ = _inputs(p, B, "dhm_abi")
    hm = hm.cuda().contiguous()
    dpose = torch.from_numpy(synth_input("dpose_abi", (B, p.out_joints, 3), -1.0, 1.0)).cuda()
    lib, dev = L.load(), hm.device
    h = net._ensure_handle()
    net._bind(dev)
    net._act_scratch(B, dev)
    sb, wb = C.c_size_t(), C.c_size_t()
    L.check(lib.egotap_lift_train_bytes(h, B, C.byref(sb), C.byref(wb)))
    saved = torch.empty(sb.value, dtype=torch.uint8, device=dev)
    ws = torch.empty(wb.value, dtype=torch.uint8, device=dev)
    pose = torch.empty((B, p.out_joints, 3), dtype=torch.float32, device=dev)
    L.check(lib.egotap_lift_forward_train(h, T._p(hm), B, T._p(pose), T._p(saved), saved.numel(), T._p(ws), ws.numel(), T._s()))
    params = dict(net.named_parameters())
    P = {k: params[k] for k in TR._param_order(p)}
    ga, G = TR._grad_arena(net, P)
    TR._bind_grads(net, h, ga, G)

    def backward(entry, dhm=None):
        ga["flat"].fill_(-1.0)            # (not NaN: the arena's alignment gaps are never written, and NaN != NaN)
        args = (h, T._p(hm), T._p(dpose), B, T._p(saved), saved.numel(), T._p(ws), ws.numel(), None, 0, T._s())
        L.check(lib.egotap_lift_backward(*args) if entry == "plain" else lib.egotap_lift_backward_dhm(*args, T._p(dhm)))
        torch.cuda.synchronize()
        return ga["flat"].clone()

    plain = backward("plain")
    assert torch.equal(backward("dhm", None), plain)
    d1 = torch.full(hm.shape, float("nan"), device=dev)
    d2 = torch.full(hm.shape, float("nan"), device=dev)
    assert torch.equal(backward("dhm", d1), plain)
    assert torch.equal(backward("dhm", d2), plain)
    assert torch.isfinite(d1).all() and torch.equal(d1, d2)
    for name, sl in _groups(p).items():
        assert float(d1[:, sl].abs().max()) > 0, name


def test_large_batch_bf16_matches_small_batch_rows():
    """bf16 storage step at B = 1024 (the config 3 shape): dhm is finite, and the rows of frames 0-2 match a B = 3 run of the same three
    frames.  The large batch repeats those frames (frame i at every index = i mod 3), so its BatchNorm statistics are those of the three
    frames up to one extra copy of frame 0 in 1024; the pose gradient is given explicitly (the loss's 1 / B would differ)."""
    net, p = _net(mode="bf16")
    hm3, _ = _inputs(p, 3, "dhm_big")
    d3 = torch.from_numpy(synth_input("dpose_big", (3, p.out_joints, 3), -1.0, 1.0))
    out = []
    for B in (3, 1024):
        idx = torch.arange(B) % 3
        x = hm3[idx].cuda().requires_grad_()
        net.zero_grad()
        pose = net(x)[0]
        pose.backward(d3[idx].cuda())
        torch.cuda.synchronize()
        out.append(x.grad[:3].clone())
        assert torch.isfinite(x.grad).all()
        del x, pose
    from egotap_amd.training import release_scratch
    release_scratch(net)
    torch.cuda.empty_cache()
    _bf16_gates(out[1], out[0].cpu(), p)


def test_estimators_train_end_to_end_through_the_pose_loss():
    """RGB (256^2, B = 2) -> position and rotation estimators (resnet18, fp32, train mode) -> torch.cat -> head (train mode) -> pose loss:
    the estimators' parameters receive exactly (bitwise) what their own backward gives when fed the head's heatmap gradient"""
    from egotap_amd import networks
    from egotap_amd.options import preset_defaults
    from egotap_amd.synthetic import synth_hm_state_dict
    from egotap_amd.training import PoseLossFn

    def estimator(which):
        opt = preset_defaults("UnrealEgo")
        if which == "pos":
            opt.num_rot_heatmap = 0
        else:
            opt.num_heatmap = 0
        e = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", input_channel_scale=2)
        e.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(e.num_heatmap, f"hm_{which}.", "resnet18").items()}, strict=True)
        return e.cuda().train()

    pos, rot = estimator("pos"), estimator("rot")
    head, p = _net()
    left = torch.from_numpy(synth_input("e2e_rgbL", (2, 3, 256, 256), -2.0, 2.0)).cuda()
    right = torch.from_numpy(synth_input("e2e_rgbR", (2, 3, 256, 256), -2.0, 2.0)).cuda()
    gt = torch.from_numpy(synth_input("e2e_gt", (2, p.out_joints, 3), -1.0, 1.0)).cuda()
    bufs = {n: {k: v.clone() for k, v in e.named_buffers()} for n, e in (("pos", pos), ("rot", rot))}
    params = list(pos.parameters()) + list(rot.parameters()) + list(head.parameters())
    for q in params:
        q.grad = None
    hp, hr = pos(left, right), rot(left, right)
    hm = torch.cat((hp, hr), 1)
    assert hm.shape == (2, p.in_channels, 64, 64) and hm.requires_grad
    hm.retain_grad()
    pose = head(hm)[0]
    PoseLossFn.apply(head, pose, gt, LAM_M, LAM_C).sum().backward()
    torch.cuda.synchronize()
    dhm = hm.grad.clone()
    got = {(n, k): v.grad.clone() for n, e in (("pos", pos), ("rot", rot)) for k, v in e.named_parameters() if v.grad is not None}
    assert len(got) > 100
    assert all(float(g.abs().max()) > 0 for (n, k), g in got.items() if k.endswith("conv1.weight"))
    # the estimators' own backward, fed the head's dhm explicitly
    for n, e in (("pos", pos), ("rot", rot)):
        for k, v in e.named_buffers():
            v.copy_(bufs[n][k])
        e.zero_grad(set_to_none=True)
    hp2, hr2 = pos(left, right), rot(left, right)
    J2 = 2 * p.n_joints_hm
    torch.autograd.backward([hp2, hr2], [dhm[:, :J2], dhm[:, J2:]])
    torch.cuda.synchronize()
    for n, e in (("pos", pos), ("rot", rot)):
        for k, v in e.named_parameters():
            assert (v.grad is None) if (n, k) not in got else torch.equal(v.grad, got[(n, k)]), (n, k)
