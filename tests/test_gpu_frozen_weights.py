"""Frozen-weight serving in the "bf16" mode on the GPU: a frozen forward is the not-frozen forward bit for bit (the same GEMMs on the same bf16
bits), it really reads the arena (no weight preparation is launched), stale arenas are noticed, and training never sees any of it.
Every comparison is torch.equal."""
import ctypes as C
import os

import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import networks
from egotap_amd.synthetic import synth_input

pytestmark = pytest.mark.gpu

VIT_W = "pos_heatmap_encoder.vit.encoder.layer.1.intermediate.dense.weight"
FC1_W = "pos_heatmap_encoder.fc1.fc.weight"
PATCH_W = "pos_heatmap_encoder.vit.embeddings.patch_embeddings.projection.weight"
BB = "backbone.backbone.backbone."
CONV_W, BN_VAR = BB + "layer2.0.conv1.weight", BB + "layer3.1.bn2.running_var"


def _lift(preset="UnrealEgo", hm=64, prec="bf16", state=None):
    """a fresh lifting head (never the cached one of gpu_util: these tests change weights and freeze)"""
    from gpu_util import lift_net, make_opt
    _, sd_np, p = lift_net(preset, hm)
    net = networks.EgoTAPAutoEncoder(make_opt(preset, hm), input_channel_scale=2)
    net.load_state_dict(state if state is not None else {k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    net = net.cuda().eval()
    net.set_precision(prec)
    return net, p


def _twin(net, preset="UnrealEgo", hm=64):
    """a never-frozen network holding net's CURRENT weights"""
    t, _ = _lift(preset, hm, net.precision, state={k: v.detach().cpu() for k, v in net.state_dict().items()})
    assert not t.weights_frozen
    return t


def _hm_in(p, B, tag="fz"):
    x = torch.from_numpy(synth_input(f"hm_{tag}_{p.hm_size}", (min(B, 4), p.in_channels, p.hm_size, p.hm_size)))
    return x.repeat((B + x.shape[0] - 1) // x.shape[0], 1, 1, 1)[:B].contiguous().cuda()


def _lift_formula(hm, layers=3, D=1024):
    k1 = (hm // 16) ** 2 * D
    return 2 * (D * 256 + layers * 12 * D * D + 2048 * k1 + 2048 * 2 * hm * hm) + layers * 3 * D * 4


# ------------------------------------------------------------------------------------------------------------ 1. frozen = not frozen
@pytest.mark.parametrize("preset,hm", [("UnrealEgo", 64), ("EgoCap", 128)])
def test_frozen_forward_equals_not_frozen(preset, hm):
    net, p = _lift(preset, hm)
    xs = {B: _hm_in(p, B) for B in (1, 8, 40)}
    before = {B: (net.predict_pose(x).clone(), [t.clone() for t in net(x)]) for B, x in xs.items()}
    net.freeze_weights()
    assert net.weights_frozen
    n = C.c_size_t()
    L.check(L.load().egotap_lift_frozen_bytes(net._ensure_handle(), C.byref(n)))
    assert n.value == _lift_formula(hm) == net._frozen_arena.numel()
    for B, x in xs.items():
        pose = net.predict_pose(x)
        assert torch.equal(pose, before[B][0]), B
        outs = net(x)
        assert len(outs) == 4
        for a, b in zip(outs, before[B][1]):
            assert torch.equal(a, b), B
    assert torch.isfinite(before[1][0]).all() and float(before[1][0].abs().max()) > 0
    net.unfreeze_weights()
    assert not net.weights_frozen and net._frozen_arena is None
    assert torch.equal(net.predict_pose(xs[8]), before[8][0])


# ------------------------------------------------------------------------------------------------------------ 2. the forward reads the arena
def test_frozen_forward_reads_the_arena_not_the_parameters():
    net, p = _lift()
    x = _hm_in(p, 4)
    old = net.predict_pose(x).clone()
    net.freeze_weights()
    sd = dict(net.named_parameters())
    vers = [sd[k]._version for k in (VIT_W, FC1_W, PATCH_W)]
    for k in (VIT_W, FC1_W, PATCH_W):
        sd[k].data.zero_()                                         # through .data: no _version bump, nothing tells the module
    assert vers == [sd[k]._version for k in (VIT_W, FC1_W, PATCH_W)]
    assert torch.equal(net.predict_pose(x), old)                   # a per-call weight preparation would have read the zeros
    assert torch.equal(net(x)[0], old)
    twin = _twin(net)
    new = twin.predict_pose(x).clone()
    assert not torch.equal(new, old)
    net.refresh_frozen_weights()
    assert net.weights_frozen
    assert torch.equal(net.predict_pose(x), new)


# ------------------------------------------------------------------------------------------------------------ 3. staleness
def test_stale_arena_is_noticed_after_load_state_dict_optimizer_step_and_inplace_ops():
    from egotap_amd.training import EgotapAdamW
    net, p = _lift()
    x = _hm_in(p, 2)
    net.freeze_weights()
    arena = net._frozen_arena.data_ptr()
    first = net.predict_pose(x).clone()
    # (a) load_state_dict of other weights
    other = {k: (v.detach().cpu() * 0.75 if v.dtype == torch.float32 and v.dim() >= 2 else v.detach().cpu()) for k, v in net.state_dict().items()}
    net.load_state_dict(other)
    want = _twin(net).predict_pose(x).clone()
    assert not torch.equal(want, first)
    assert torch.equal(net.predict_pose(x), want) and net.weights_frozen
    # (b) one EgotapAdamW step (its kernels write the parameters through raw pointers)
    params = [q for q in net.parameters()]
    for i, q in enumerate(params):
        q.grad = torch.full_like(q, 1e-2 if i % 2 else -1e-2)
    EgotapAdamW(params, lr=1e-4, eps=1e-4, weight_decay=0.0).step()
    for q in params:
        q.grad = None
    want2 = _twin(net).predict_pose(x).clone()
    assert not torch.equal(want2, want)
    assert torch.equal(net.predict_pose(x), want2) and net.weights_frozen
    # (c) an in-place op under no_grad
    with torch.no_grad():
        for q in net.parameters():
            if q.dim() >= 2:
                q.mul_(1.01)
    want3 = _twin(net).predict_pose(x).clone()
    assert not torch.equal(want3, want2)
    assert torch.equal(net.predict_pose(x), want3)
    assert net.weights_frozen and net._frozen_arena.data_ptr() == arena      # every refresh went into the same arena


# ------------------------------------------------------------------------------------------------------------ 4. training is untouched
def test_training_step_after_a_freeze_equals_a_never_frozen_twins():
    from egotap_amd.training import EgotapAdamW, PoseLossFn
    net, p = _lift()
    twin = _twin(net)
    hm = _hm_in(p, 3, "fz_train")
    gt = torch.from_numpy(synth_input("gt_fz_train", (3, p.out_joints, 3), -1.0, 1.0)).cuda()
    net.freeze_weights()
    net.predict_pose(hm)
    out = []
    for n in (net, twin):
        n.train()
        assert not n.weights_frozen
        opt = EgotapAdamW(n.parameters(), lr=1e-3, eps=1e-4, weight_decay=0.0)
        opt.zero_grad()
        pose = n(hm)[0]
        loss = PoseLossFn.apply(n, pose, gt, 0.1, -0.01)
        loss.sum().backward()
        grads = {k: v.grad.clone() for k, v in n.named_parameters() if v.grad is not None}
        opt.step()
        out.append((loss.detach().clone(), grads, {k: v.clone() for k, v in n.named_buffers()}, {k: v.detach().clone() for k, v in n.named_parameters()}))
    (la, ga, ba, pa), (lb, gb, bb, pb) = out
    assert torch.equal(la, lb)
    assert sorted(ga) == sorted(gb) and len(ga) > 50
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    for k in ba:
        assert torch.equal(ba[k], bb[k]), k
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k
    net.eval()
    twin.eval()
    assert not net.weights_frozen                                  # back in eval mode the module is not frozen until asked again
    assert torch.equal(net.predict_pose(hm), twin.predict_pose(hm))
    net.freeze_weights()
    assert net.weights_frozen and torch.equal(net.predict_pose(hm), twin.predict_pose(hm))


def test_c_training_entries_ignore_a_frozen_handle():
    """egotap_lift_forward_train / egotap_lift_backward on a handle that IS frozen (below the module, which would unfreeze in .train()): stale arena,
    same training bits as a never-frozen twin"""
    from egotap_amd.training import PoseLossFn
    net, p = _lift()
    twin = _twin(net)
    hm = _hm_in(p, 2, "fz_ctrain")
    gt = torch.from_numpy(synth_input("gt_fz_ctrain", (2, p.out_joints, 3), -1.0, 1.0)).cuda()
    net.freeze_weights()
    dict(net.named_parameters())[VIT_W].data.mul_(0.5)             # the arena is stale now; training must read the live weights
    dict(twin.named_parameters())[VIT_W].data.mul_(0.5)
    torch.nn.Module.train(net, True)                               # the flag only: the handle stays frozen
    assert net.weights_frozen
    twin.train()
    res = []
    for n in (net, twin):
        n.zero_grad()
        pose = n(hm)[0]
        PoseLossFn.apply(n, pose, gt, 0.1, -0.01).sum().backward()
        res.append((pose.detach().clone(), {k: v.grad.clone() for k, v in n.named_parameters() if v.grad is not None}))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k


# ------------------------------------------------------------------------------------------------------------ 5. modes without prepared weights
def test_modes_without_prepared_weights_refuse_by_name_and_set_precision_unfreezes():
    net, p = _lift()
    x = _hm_in(p, 2)
    for mode in ("f32", "bf16x3"):
        net.set_precision(mode)
        with pytest.raises(L.EgotapError, match=mode):
            net.freeze_weights()
        assert not net.weights_frozen
    ragged, pr = _lift("UnrealEgo", 96)
    with pytest.raises(L.EgotapError, match="multiple of 32"):
        ragged.freeze_weights()
    assert not ragged.weights_frozen
    net.set_precision("bf16")
    net.freeze_weights()
    net.train()
    with pytest.raises(L.EgotapError, match="train mode"):
        net.freeze_weights()
    net.eval()
    net.freeze_weights()
    dict(net.named_parameters())[FC1_W].data.mul_(0.5)             # stale on purpose: a forward that still read the arena would show it
    for mode in ("bf16x3", "bf16", "f32"):
        net.set_precision(mode)
        assert not net.weights_frozen
        assert torch.equal(net.predict_pose(x), _twin(net).predict_pose(x)), mode
    # the library alone: egotap_set_precision on a frozen handle unfreezes it (the module is bypassed here)
    net.set_precision("bf16")
    net.freeze_weights()
    dict(net.named_parameters())[FC1_W].data.mul_(0.5)
    L.check(L.load().egotap_set_precision(net._ensure_handle(), L.PRECISIONS["bf16"]))
    twin = _twin(net)
    ws, B = net._workspace(2, x.device), 2
    pose = torch.empty((B, p.out_joints, 3), device="cuda")
    L.check(L.load().egotap_lift_predict_pose(net._ensure_handle(), C.c_void_p(x.data_ptr()), B, C.c_void_p(pose.data_ptr()), C.c_void_p(ws.data_ptr()),
                                              ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(pose, twin.predict_pose(x))


# ------------------------------------------------------------------------------------------------------------ 6. graph
@pytest.mark.parametrize("B", [1, 8])
def test_graphed_frozen_equals_eager_not_frozen(B):
    net, p = _lift()
    x = _hm_in(p, B)
    eager = net.predict_pose(x).clone()
    g0 = net.predict_pose_graphed(x).clone()                       # captured NOT frozen
    assert torch.equal(g0, eager)
    net.freeze_weights()
    assert torch.equal(net.predict_pose_graphed(x), eager)         # a new capture: the frozen state is part of the key
    assert len(net._graphs) == 2
    # freeze after a capture + changed weights (3a): neither the not-frozen graph's old result nor the frozen graph's stale arena
    other = {k: (v.detach().cpu() * 0.75 if v.dtype == torch.float32 and v.dim() >= 2 else v.detach().cpu()) for k, v in net.state_dict().items()}
    net.load_state_dict(other)
    want = _twin(net).predict_pose(x).clone()
    assert not torch.equal(want, eager)
    assert torch.equal(net.predict_pose_graphed(x), want)
    assert len(net._graphs) == 2                                   # the refresh went into the same arena: the captured frozen graph stayed valid
    net.unfreeze_weights()
    assert torch.equal(net.predict_pose_graphed(x), want)          # the not-frozen graph prepares from the live weights at every replay


# ------------------------------------------------------------------------------------------------------------ 7. estimators
def _est(which, model_name, hm, state=None):
    from gpu_util import hm_net, make_opt
    _, sd_np = hm_net(which, "cuda", "UnrealEgo", hm, model_name)
    opt = make_opt("UnrealEgo", hm)
    if which == "pos":
        opt.num_rot_heatmap = 0
    else:
        opt.num_heatmap = 0
    net = networks.HeatMap_UnrealEgo_Shared(opt, model_name, input_channel_scale=2)
    net.load_state_dict(state if state is not None else {k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
    net = net.cuda().eval()
    net.set_precision("bf16")
    return net


def _est_twin(net, which, model_name, hm):
    return _est(which, model_name, hm, state={k: v.detach().cpu() for k, v in net.state_dict().items()})


def _rgb(B, hm, tag="fz"):
    S = 4 * hm
    mk = lambda s: torch.from_numpy(synth_input(f"rgb_{s}_{tag}_{S}", (min(B, 2), 3, S, S), -2.0, 2.0))      # noqa: E731
    rep = lambda t: t.repeat((B + t.shape[0] - 1) // t.shape[0], 1, 1, 1)[:B].contiguous().cuda()              # noqa: E731
    return rep(mk("l")), rep(mk("r"))


def _run(net, l, r):
    out = torch.empty((l.shape[0], 2 * net.num_heatmap, net.hm_size, net.hm_size), device="cuda")
    return net.forward_into(l, r, out)


@pytest.mark.parametrize("which,model_name,hm", [("pos", "resnet18", 64), ("rot", "resnet34", 64), ("rot", "resnet18", 128), ("pos", "resnet34", 128)])
def test_estimator_frozen_equals_not_frozen(which, model_name, hm):
    net = _est(which, model_name, hm)
    FB, OB = (2, 9) if hm == 64 else (1, 3)                        # the frozen batch and another one
    ins = {B: _rgb(B, hm) for B in (FB, OB)}
    before = {B: _run(net, *ins[B]).clone() for B in ins}
    net.freeze_weights(FB)
    assert net.weights_frozen
    n = C.c_size_t()
    L.check(L.load().egotap_hm_frozen_bytes(net._ensure_handle(), net._net, FB, C.byref(n)))
    assert n.value == net._frozen_arena.numel() > 0
    for B in ins:
        assert torch.equal(_run(net, *ins[B]), before[B]), B
    assert torch.isfinite(before[FB]).all() and float(before[FB].abs().max()) > 0
    # batch statistics: never the arena (and afterwards the running statistics have moved, which the next frozen forward must see)
    twin = _est_twin(net, which, model_name, hm)
    lb, rb = _rgb(4, hm, "bn")
    a = torch.empty((4, 2 * net.num_heatmap, hm, hm), device="cuda")
    b = torch.empty_like(a)
    net.forward_bnbatch_into(lb, rb, a)
    twin.forward_bnbatch_into(lb, rb, b)
    assert torch.equal(a, b)
    for (k, u), (_, v) in zip(net.state_dict().items(), twin.state_dict().items()):
        assert torch.equal(u, v), k
    got = _run(net, *ins[FB])
    assert torch.equal(got, _run(twin, *ins[FB])) and not torch.equal(got, before[FB])


def test_estimator_reads_the_arena_and_notices_stale_weights():
    which, model_name, hm, B = "pos", "resnet18", 64, 2
    net = _est(which, model_name, hm)
    l, r = _rgb(B, hm)
    old = _run(net, l, r).clone()
    net.freeze_weights(B)
    sd = net.state_dict(keep_vars=True)
    # (2) through .data: the frozen forward keeps returning the old maps
    sd[CONV_W].data.mul_(0.5)
    sd[BN_VAR].data.mul_(4.0)
    assert torch.equal(_run(net, l, r), old)
    new = _run(_est_twin(net, which, model_name, hm), l, r).clone()
    assert not torch.equal(new, old)
    net.refresh_frozen_weights()
    assert torch.equal(_run(net, l, r), new)
    # (3a) load_state_dict of other weights, then running_var.copy_ alone (the fold is part of what is kept)
    other = {k: (v.detach().cpu() * 0.9 if v.dtype == torch.float32 and v.dim() == 4 else v.detach().cpu()) for k, v in net.state_dict().items()}
    net.load_state_dict(other)
    want = _run(_est_twin(net, which, model_name, hm), l, r).clone()
    assert not torch.equal(want, new)
    assert torch.equal(_run(net, l, r), want)
    with torch.no_grad():
        sd = net.state_dict(keep_vars=True)
        sd[BN_VAR].copy_(sd[BN_VAR] * 3.0)
    want2 = _run(_est_twin(net, which, model_name, hm), l, r).clone()
    assert not torch.equal(want2, want)
    assert torch.equal(_run(net, l, r), want2) and net.weights_frozen
    # train mode unfreezes; other sides have nothing to freeze
    net.train()
    assert not net.weights_frozen
    side96 = _est("pos", "resnet18", 96)
    with pytest.raises(L.EgotapError, match="64 and 128"):
        side96.freeze_weights()
    net.eval()
    net.set_precision("f32")
    with pytest.raises(L.EgotapError, match="f32"):
        net.freeze_weights()


# ------------------------------------------------------------------------------------------------------------ 8. wrapper
def _wrapper(tmp_path, **over):
    from egotap_amd import models, spec
    from egotap_amd.options import preset_defaults
    from egotap_amd.synthetic import synth_hm_state_dict, synth_state_dict
    if not os.path.exists(tmp_path / "hm_pos"):
        for sub, sd in (("hm_pos", synth_hm_state_dict(15, "hm_pos.")), ("hm_sin", synth_hm_state_dict(30, "hm_rot."))):
            os.makedirs(tmp_path / sub)
            torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, tmp_path / sub / "best_net_HeatMap.pth")
    opt = preset_defaults("UnrealEgo", 64)
    opt.isTrain, opt.use_gt_heatmap, opt.lr, opt.opt_eps, opt.weight_decay = True, False, 1e-3, 1e-4, 0.0
    opt.log_dir, opt.path_to_trained_heatmap = str(tmp_path), str(tmp_path / "hm" / "best_net_HeatMap.pth")
    for k, v in over.items():
        setattr(opt, k, v)
    m = models.create_model(opt)
    p = spec.lift_preset("UnrealEgo", 64)
    m.net_AutoEncoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
    return m


def test_wrapper_freeze_evaluate_and_training_step(tmp_path):
    class RunningAverageDict:                                      # what utils/evaluate.py hands evaluate(): only .update is used
        def __init__(self):
            self.rows = []

        def update(self, d):
            self.rows.append(d)

    B = 2
    data = {"input_rgb_left": torch.from_numpy(synth_input("rgb_l_fzw", (B, 3, 256, 256), -2.0, 2.0)),
            "input_rgb_right": torch.from_numpy(synth_input("rgb_r_fzw", (B, 3, 256, 256), -2.0, 2.0)),
            "gt_local_pose": torch.from_numpy(synth_input("gt_fzw", (B, 16, 3), -20.0, 20.0))}
    # serving in bf16 (no --use_amp: evaluate() keeps the caller's precision): evaluate() runs frozen and equals the not-frozen evaluate()
    s = _wrapper(tmp_path, use_amp=False)
    s.set_precision("bf16")
    s.eval()
    s.set_input(data)
    pose0, cat0, _ = s.evaluate(RunningAverageDict())
    pose0, cat0 = pose0.clone(), cat0.clone()
    assert s.freeze_weights(batch=B) == {}
    assert all(n.weights_frozen for n in (s.net_HeatMap, s.net_RotHeatMap, s.net_AutoEncoder))
    pose1, cat1, _ = s.evaluate(RunningAverageDict())
    assert torch.equal(pose1, pose0) and torch.equal(cat1, cat0)
    assert all(n.weights_frozen for n in (s.net_HeatMap, s.net_RotHeatMap, s.net_AutoEncoder))
    s.unfreeze_weights()
    assert not any(n.weights_frozen for n in (s.net_HeatMap, s.net_RotHeatMap, s.net_AutoEncoder))
    # --use_amp: freeze, evaluate() (fp32 there, as the reference disables autocast: the precision switch unfreezes), then a training step
    out = []
    for freeze in (True, False):
        m = _wrapper(tmp_path, use_amp=True, frozen_heatmap_bn_eval=True)
        m.set_precision("bf16")
        m.eval()
        m.set_input(data)
        if freeze:
            skipped = m.freeze_weights(batch=B)
            assert skipped == {} and m.net_AutoEncoder.weights_frozen
            m.net_RotHeatMap.train()
            assert "RotHeatMap" in m.freeze_weights(batch=B)       # a network that cannot freeze as it stands is skipped by name
            m.net_RotHeatMap.eval()
        pose, cat, _ = m.evaluate(RunningAverageDict())
        ev = (pose.clone(), cat.clone())
        m.train()
        m.optimize_parameters()
        assert not m.net_AutoEncoder.weights_frozen
        out.append((ev, m.loss_pose.detach().clone(), {k: v.detach().clone() for k, v in m.net_AutoEncoder.state_dict().items()}))
    (eva, la, sa), (evb, lb, sb) = out
    assert torch.equal(eva[0], evb[0]) and torch.equal(eva[1], evb[1])
    assert torch.equal(la, lb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
