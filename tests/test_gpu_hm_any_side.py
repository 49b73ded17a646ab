"""The heatmap estimators at heatmap sides other than 64 / 128 (any multiple of 16; RGB = 4 x the side, dataloader/data_loader.py:97-98):
eval-mode forward against the float64 oracle, batch independence, the precision modes (exact fp32 by name at these sides), the stage-2
wrapper's evaluate() from RGB, and the named refusals of the batch-statistics paths, which stay built at 64 / 128 only."""
import numpy as np
import pytest
import torch

from egotap_amd.synthetic import synth_hm_state_dict, synth_input, synth_state_dict

pytestmark = pytest.mark.gpu


def _rgb(name, B, hm):
    return torch.from_numpy(synth_input(name, (B, 3, 4 * hm, 4 * hm), -2.0, 2.0))


def _oracle_close(y, ref):
    err = (y.cpu().double() - ref).abs().max().item()
    assert err < 1e-4 * max(1.0, ref.abs().max().item()), f"max err {err:.3e} (max |ref| {ref.abs().max().item():.3e})"


@pytest.mark.parametrize("hm,which,B,model_name", [(16, "pos", 2, "resnet18"), (16, "rot", 1, "resnet18"), (32, "rot", 3, "resnet18"),
                                                   (32, "pos", 1, "resnet50"), (48, "pos", 2, "resnet34"), (48, "rot", 1, "resnet18"),
                                                   (96, "pos", 1, "resnet18")])
def test_hm_forward_any_side_matches_oracle(hm, which, B, model_name):
    from gpu_util import hm_net
    from oracle import hm_ref as H
    net, sd_np = hm_net(which, hm=hm, model_name=model_name)
    left, right = _rgb(f"rgbL_{which}_{hm}", B, hm), _rgb(f"rgbR_{which}_{hm}", B, hm)
    with torch.no_grad():
        ref = H.hm_forward(left.double(), right.double(), H.to_torch_sd(sd_np, torch.float64))
    y = net(left.cuda(), right.cuda())
    torch.cuda.synchronize()
    assert tuple(y.shape) == (B, 2 * net.num_heatmap, hm, hm)
    _oracle_close(y, ref)


def test_hm_forward_any_side_batch_independent_and_every_precision_exact():
    """hm 48: a frame inside a batch of 5, written into a channel slice of a canary-filled tensor, equals the frame alone (the power-of-two
    kernels at 24 / 12 ... split small batches over input channels: within 1e-5 of scale); the bf16x3 and bf16 modes run the exact-fp32
    path at this side and give its bits"""
    from gpu_util import hm_net
    net, _ = hm_net("pos", hm=48)
    left, right = _rgb("rgbL_b5_48", 1, 48).cuda(), _rgb("rgbR_b5_48", 1, 48).cuda()
    alone = net(left, right).clone()
    cat = torch.full((5, 40, 48, 48), 7.0, device="cuda")
    net.forward_into(left.repeat(5, 1, 1, 1), right.repeat(5, 1, 1, 1), cat, channel_offset=4)
    torch.cuda.synchronize()
    scale = float(alone.abs().max())
    assert float((cat[:, 4:34] - alone.expand(5, -1, -1, -1)).abs().max()) < 1e-5 * scale
    assert float((cat[:, :4] - 7.0).abs().max()) == 0.0 and float((cat[:, 34:] - 7.0).abs().max()) == 0.0
    two_l, two_r = _rgb("rgbL_prec_48", 2, 48).cuda(), _rgb("rgbR_prec_48", 2, 48).cuda()
    exact = net(two_l, two_r).clone()
    try:
        for mode in ("bf16x3", "bf16"):
            net.set_precision(mode)
            assert torch.equal(net(two_l, two_r), exact), mode
    finally:
        net.set_precision("f32")


class _Avg(dict):
    def update(self, d):
        for k, v in d.items():
            self.setdefault(k, []).append(float(v))


def _wrapper(hm):
    from egotap_amd import models, spec
    from egotap_amd.options import preset_defaults
    opt = preset_defaults("UnrealEgo", hm)
    assert opt.load_size_heatmap == [hm, hm]
    m = models.create_model(opt)
    p = spec.lift_preset("UnrealEgo", hm)
    sds = {"AutoEncoder": synth_state_dict(spec.lift_state_spec(p)),
           "HeatMap": synth_hm_state_dict(15, "hm_pos."), "RotHeatMap": synth_hm_state_dict(30, "hm_rot.")}
    for name, sd in sds.items():
        getattr(m, "net_" + name).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return m, sds, p


def _data(hm, B, tag):
    return {"input_rgb_left": _rgb(f"w_rgb_l_{tag}", B, hm), "input_rgb_right": _rgb(f"w_rgb_r_{tag}", B, hm),
            "gt_local_pose": torch.from_numpy(synth_input(f"w_gt_{tag}", (B, 16, 3), -1.0, 1.0))}


def _oracle_pose(data, sds, p):
    from oracle import hm_ref as H, lift_ref as O
    with torch.no_grad():
        pos = H.hm_forward(data["input_rgb_left"], data["input_rgb_right"], H.to_torch_sd(sds["HeatMap"]))
        rot = H.hm_forward(data["input_rgb_left"], data["input_rgb_right"], H.to_torch_sd(sds["RotHeatMap"]))
        return O.lift_forward(torch.cat([pos, rot], dim=1), O.to_torch_sd(sds["AutoEncoder"]), p)


@pytest.mark.parametrize("hm,B", [(32, 4), (96, 1)])
def test_wrapper_evaluate_from_rgb_at_any_side(hm, B):
    """test.py at --load_size_heatmap 32 / 96: model.eval() + set_eval_mode() (utils/evaluate.py:93-94), evaluate() from RGB through
    both estimators and the lifting head, against hm_ref + lift_ref; per-frame MPJPE as the reference computes it"""
    m, sds, p = _wrapper(hm)
    data = _data(hm, B, hm)
    m.set_input(data)
    m.eval()
    m.set_eval_mode()
    avg = _Avg()
    pose, hm_cat, avg = m.evaluate(avg)
    torch.cuda.synchronize()
    ref = _oracle_pose(data, sds, p)
    assert tuple(hm_cat.shape) == (B, 90, hm, hm)
    np.testing.assert_allclose(pose.cpu().numpy(), ref.numpy(), atol=1e-4, rtol=0)
    ref_mpjpe = [float(torch.linalg.norm(data["gt_local_pose"][i] - ref[i], dim=-1).mean() * 10) for i in range(B)]
    np.testing.assert_allclose(avg["mpjpe"], ref_mpjpe, rtol=1e-4)


def test_wrapper_evaluate_at_any_side_under_amp_runs_fp32():
    """a --use_amp model in a reduced mode: evaluate() switches the three networks to fp32 (forward(evaluate=True)) and back, so the pose
    has the fp32 run's bits and the mode survives"""
    hm, B = 32, 2
    m, sds, p = _wrapper(hm)
    data = _data(hm, B, "amp")
    m.set_input(data)
    m.eval()
    m.set_eval_mode()
    pose32 = m.evaluate(_Avg())[0].clone()
    m.use_amp = True                      # what create_model sets for isTrain + --use_amp
    m.set_precision("bf16")
    try:
        pose_amp = m.evaluate(_Avg())[0].clone()
        torch.cuda.synchronize()
        assert m.net_HeatMap.precision == "bf16" and m.net_RotHeatMap.precision == "bf16"
    finally:
        m.use_amp = False
        m.set_precision("f32")
    assert torch.equal(pose_amp, pose32)
    np.testing.assert_allclose(pose32.cpu().numpy(), _oracle_pose(data, sds, p).numpy(), atol=1e-4, rtol=0)


def test_batch_statistics_paths_refuse_other_sides_by_name():
    """hm 32: every estimator path with batch-statistics BatchNorm raises before it launches anything, naming the built sides"""
    from gpu_util import hm_net
    from egotap_amd import hm_training, models
    from egotap_amd.options import preset_defaults
    net, _ = hm_net("pos", hm=32)
    left, right = _rgb("rgbL_ref_32", 2, 32).cuda(), _rgb("rgbR_ref_32", 2, 32).cuda()
    out = torch.zeros((2, 30, 32, 32), device="cuda")
    try:
        net.set_precision("bf16")
        with pytest.raises(NotImplementedError, match="64 and 128"):
            net.forward_bnbatch_into(left, right, out)
    finally:
        net.set_precision("f32")
    with pytest.raises(NotImplementedError, match="64 and 128"):
        hm_training.hm_train_forward_nograd(net, left, right)
    assert not net.training
    # the stage-2 wrapper with net_RotHeatMap left in train mode (set_eval_mode() does not switch it, as in the reference)
    m, _, _ = _wrapper(32)
    m.set_input(_data(32, 2, "ref"))
    m.set_eval_mode()
    assert m.net_RotHeatMap.training
    with pytest.raises(NotImplementedError, match="64 and 128"):
        m.forward(evaluate=True)
    # stage-1 training
    opt = preset_defaults("UnrealEgo", 32)
    opt.model, opt.isTrain, opt.num_rot_heatmap = "heatmap_shared", True, 0
    s1 = models.create_model(opt)
    s1.set_input({"input_rgb_left": left.cpu(), "input_rgb_right": right.cpu(),
                  "gt_heatmap_left": torch.zeros((2, 15, 32, 32)), "gt_heatmap_right": torch.zeros((2, 15, 32, 32))})
    with pytest.raises(NotImplementedError, match="64 and 128"):
        s1.optimize_parameters()
    # side 128: the batch-statistics forward runs, the differentiable one is refused by name before it launches anything (the 3x3 / 1x1
    # weight-gradient kernels stop at map width 64; tests/test_gpu_hm_train_ops.py test_width_128_operators)
    net128, _ = hm_net("pos", hm=128)
    l128, r128 = _rgb("rgbL_ref_128", 1, 128).cuda(), _rgb("rgbR_ref_128", 1, 128).cuda()
    stats = {k: v.clone() for k, v in net128.named_buffers()}
    net128.train()
    try:
        with pytest.raises(NotImplementedError, match="side 64 only .*not 128"):
            net128(l128, r128)
        assert all(torch.equal(v, stats[k]) for k, v in net128.named_buffers())
    finally:
        net128.eval()
    y = hm_training.hm_train_forward_nograd(net128, l128, r128)
    assert tuple(y.shape) == (1, 30, 128, 128) and bool(torch.isfinite(y).all()) and not y.requires_grad
    for k, v in stats.items():                      # it ran on batch statistics: the running statistics moved; put them back (the net is shared)
        net128.state_dict()[k].copy_(v)
