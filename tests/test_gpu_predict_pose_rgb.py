"""EgoTAPAutoEncoderModel.predict_pose_from_rgb / egotap_predict_pose_rgb: stereo RGB -> pose in one call, without ground truth.

The one call composes the estimators' and the head's own internal forwards, so in fp32 it must reproduce set_input() + evaluate() bit for bit
(same kernels, same order; the pose-only head is bit-equal to the full forward).  In "bf16" without return_heatmaps, conv_heatmap
hands the head its bf16 operand directly: the head rounds every fp32 heatmap value to bf16 (round to nearest even) before its only uses of it, so
the pose must keep its bits there too."""
import os
import re

import numpy as np
import pytest
import torch

from egotap_amd.synthetic import synth_hm_state_dict, synth_input, synth_state_dict
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


class _Acc:
    def __init__(self):
        self.rows = []

    def update(self, d):
        self.rows.append(d)


def _frames(tag, B, hm):
    """B stereo frames [B, 3, 4 hm, 4 hm] x 2 on the GPU: four hash-RNG frames, repeated with a per-repeat gain past the fourth"""
    nb, S0 = min(B, 4), 4 * hm
    out = []
    for eye in "LR":
        x = torch.from_numpy(synth_input(f"rgb{eye}_{tag}_{hm}", (nb, 3, S0, S0), -2.0, 2.0)).cuda()
        if B > nb:
            idx = torch.arange(B, device="cuda")
            x = (x[idx % nb] * (1.0 + 0.03 * (idx // nb).float()).view(B, 1, 1, 1)).contiguous()
        out.append(x)
    return out


def _evaluate(m, p, left, right):
    """the existing route: set_input() with loader keys + evaluate()"""
    m.set_input({"input_rgb_left": left, "input_rgb_right": right, "gt_local_pose": torch.zeros(left.shape[0], p.out_joints, 3)})
    pose, cat, _ = m.evaluate(_Acc())
    return pose.clone(), cat.clone()


def _composed(m, p, left, right):
    """the parent's serving composition: chunked forward_into x 2 + predict_pose"""
    B = left.shape[0]
    chunk = min(B, int(m.opt.hm_chunk))
    cat = torch.empty((B, p.in_channels, p.hm_size, p.hm_size), device="cuda")
    for net, c0 in ((m.net_HeatMap, 0), (m.net_RotHeatMap, 2 * p.n_joints_hm)):
        ws = m.net_HeatMap._workspace(chunk, left.device)
        for lo in range(0, B, chunk):
            net.forward_into(left[lo:lo + chunk], right[lo:lo + chunk], cat[lo:lo + chunk], c0, workspace=ws)
    return m.net_AutoEncoder.predict_pose(cat).clone(), cat


# ------------------------------------------------------------------------------------------------------------ 1. fp32, bitwise
@pytest.mark.parametrize("preset,hm,B", [("UnrealEgo", 64, 1), ("UnrealEgo", 64, 3), ("UnrealEgo", 64, 37), ("UnrealEgo", 64, 300),
                                         ("EgoCap", 128, 1), ("EgoCap", 128, 3), ("EgoCap", 128, 37), ("EgoCap", 128, 300)])
def test_fp32_equals_set_input_plus_evaluate_bit_for_bit(preset, hm, B):
    m, p = _model(preset, hm)
    left, right = _frames("bitwise", B, hm)
    want_pose, want_cat = _evaluate(m, p, left, right)
    pose, cat = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
    torch.cuda.synchronize()
    assert m.rgb_form() == "heatmaps"
    assert tuple(pose.shape) == (B, p.out_joints, 3) and tuple(cat.shape) == (B, p.in_channels, hm, hm)
    assert torch.equal(cat, want_cat), float((cat - want_cat).abs().max())
    assert torch.equal(pose, want_pose), float((pose - want_pose).abs().max())
    only = m.predict_pose_from_rgb(left, right)                  # heatmaps kept inside the workspace: the same pose, the same heatmaps
    torch.cuda.synchronize()
    assert m.rgb_form() == "scratch"
    assert torch.equal(only, want_pose)
    assert torch.equal(m.rgb_intermediate("heatmaps", B), want_cat)
    del want_cat, cat
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ 2. against the reference
def test_pose_matches_the_reference_wrapper_fixture():
    """the reference wrapper's own evaluate() from RGB (tests/golden/wrapper_eval_ue_b4.npz), at the gate tests/test_gpu_wrapper_golden.py puts on it"""
    # "the gate of that file, not a new number": the gate is a literal inside that test and existing test files may not change, so it cannot
    # move to a shared constant -- it is read out of the source here, and this test fails loudly if that line is ever rewritten
    src = open(os.path.join(HERE, "test_gpu_wrapper_golden.py")).read()
    gate = re.search(r"tol = 1e-4 if use_gt else ([0-9.e-]+)", src)
    assert gate, "the wrapper golden test no longer states its from-RGB pose gate"
    tol = float(gate.group(1))
    m, p = _model("UnrealEgo", 64)
    g = np.load(os.path.join(GOLD, "wrapper_eval_ue_b4.npz"))
    left = torch.from_numpy(synth_input("wrap_rgbL_eval", (4, 3, 256, 256), -2.0, 2.0)).cuda()
    right = torch.from_numpy(synth_input("wrap_rgbR_eval", (4, 3, 256, 256), -2.0, 2.0)).cuda()
    pose, cat = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
    err = float(np.abs(pose.cpu().numpy() - g["rgb_pred_pose"]).max())
    print(f"pose from RGB: max |gpu - reference| = {err:.2e} (gate {tol:.0e})")
    assert err <= tol
    np.testing.assert_allclose(cat.reshape(-1)[::997].cpu().numpy(), g["rgb_heatmap_cat_sample"], atol=3e-4)      # which net fills which channels


# ------------------------------------------------------------------------------------------------------------ 3. no ground truth
def test_needs_no_ground_truth_and_no_set_input():
    m, p = _model("UnrealEgo", 64)
    left, right = _frames("nogt", 2, 64)
    for n in (m.net_AutoEncoder, m.net_HeatMap, m.net_RotHeatMap):
        assert not n.training
    flags = [(n.training, getattr(n, "precision", "f32")) for n in (m.net_AutoEncoder, m.net_HeatMap, m.net_RotHeatMap)]
    pose = m.predict_pose_from_rgb(left, right)
    torch.cuda.synchronize()
    assert tuple(pose.shape) == (2, p.out_joints, 3) and bool(torch.isfinite(pose).all()) and not pose.requires_grad
    assert flags == [(n.training, getattr(n, "precision", "f32")) for n in (m.net_AutoEncoder, m.net_HeatMap, m.net_RotHeatMap)]
    # the same RGB-only batch through the existing route: set_input takes it, evaluate() has no pose to compare with and raises, as before
    m.set_input({"input_rgb_left": left, "input_rgb_right": right})
    with pytest.raises((AttributeError, TypeError, ValueError, RuntimeError)):
        m.evaluate(_Acc())
    want, _ = _evaluate(m, p, left, right)
    assert torch.equal(pose, want)
    with pytest.raises(ValueError, match="expected left / right"):
        m.predict_pose_from_rgb(left[:, :, :128], right)
    with pytest.raises(Exception, match="GPU only"):
        m.predict_pose_from_rgb(left.cpu(), right.cpu())


# ------------------------------------------------------------------------------------------------------------ 4. precisions
def _oracle_pose(p, left, right):
    """float64 restatement of the whole pipeline on the CPU: both estimators, concat, lifting head"""
    from oracle import hm_ref as OH
    from oracle import lift_ref as OL
    from egotap_amd import spec
    J = p.n_joints_hm
    lift = OL.to_torch_sd(synth_state_dict(spec.lift_state_spec(p)), torch.float64)
    pos = OH.to_torch_sd(synth_hm_state_dict(J, "hm_pos."), torch.float64)
    rot = OH.to_torch_sd(synth_hm_state_dict(2 * J, "hm_rot."), torch.float64)
    with torch.no_grad():
        le, ri = left.double().cpu(), right.double().cpu()
        cat = torch.cat((OH.hm_forward(le, ri, pos), OH.hm_forward(le, ri, rot)), dim=1)
        return OL.lift_forward(cat, lift, p), cat


@pytest.mark.parametrize("preset,hm", [("UnrealEgo", 64)])
def test_reduced_precisions_against_the_float64_oracle_and_frozen_bits(preset, hm):
    m, p = _model(preset, hm)
    B = 2
    left, right = _frames("prec", B, hm)
    ref, _ = _oracle_pose(p, left, right)
    scale = float(ref.abs().max())
    exact = m.predict_pose_from_rgb(left, right)
    err = float((exact.double().cpu() - ref).abs().max())
    print(f"f32: max |gpu - float64 oracle| = {err:.2e} (max |ref| = {scale:.2f})")
    try:
        for mode, tol in (("bf16x3", 1e-4), ("bf16", 3e-2 * scale)):           # the gates of tests/test_gpu_lift.py
            m.set_precision(mode)
            low = m.predict_pose_from_rgb(left, right)
            err = float((low.double().cpu() - ref).abs().max())
            print(f"{mode}: max |gpu - float64 oracle| = {err:.2e} (gate {tol:.2e})")
            assert err < tol, (mode, err, tol)
        # bf16, frozen against not frozen: the same bits, with and without the heatmaps
        pose0, cat0 = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        pose0, cat0, only0 = pose0.clone(), cat0.clone(), m.predict_pose_from_rgb(left, right).clone()
        assert m.freeze_weights(batch=B) == {}
        assert all(n.weights_frozen for n in (m.net_HeatMap, m.net_RotHeatMap, m.net_AutoEncoder))
        pose1, cat1 = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        only1 = m.predict_pose_from_rgb(left, right)
        torch.cuda.synchronize()
        assert torch.equal(pose1, pose0) and torch.equal(cat1, cat0) and torch.equal(only1, only0)
        assert all(n.weights_frozen for n in (m.net_HeatMap, m.net_RotHeatMap, m.net_AutoEncoder))
        # and the frozen one call equals the frozen module forwards
        want, want_cat = _composed(m, p, left, right)
        assert torch.equal(pose1, want) and torch.equal(cat1, want_cat)
        m.unfreeze_weights()
        assert torch.equal(m.predict_pose_from_rgb(left, right), only0)
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")


# ------------------------------------------------------------------------------------------------------------ 5. the bf16 hand-off
@pytest.mark.parametrize("preset,hm,B", [("UnrealEgo", 64, 2), ("UnrealEgo", 64, 37), ("UnrealEgo", 64, 300),
                                         ("EgoCap", 128, 2), ("EgoCap", 128, 37), ("EgoCap", 128, 300)])
def test_bf16_hand_off_keeps_the_pose_bits(preset, hm, B):
    m, p = _model(preset, hm)
    left, right = _frames("handoff", B, hm)
    try:
        m.set_precision("bf16")
        with_pose, cat = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        torch.cuda.synchronize()
        assert m.rgb_form() == "heatmaps"
        with_pose = with_pose.clone()
        m._rgb["ws"].view(torch.int16).fill_(-1)                   # every 16-bit word of the workspace a bf16 NaN (0xFFFF), every float a NaN
        pose = m.predict_pose_from_rgb(left, right)
        torch.cuda.synchronize()
        assert m.rgb_form() == "handoff", m.rgb_form()             # conv_heatmap wrote the head's bf16 operand: no fp32 heatmaps
        assert bool(torch.isfinite(pose).all())
        assert torch.equal(pose, with_pose), float((pose - with_pose).abs().max())
        # the hand-off buffer, decoded on the CPU: bf16 [B, 6J, S, S], every element the bf16 rounding of the fp32 heatmap the other form returns
        # (one writer per element, nothing left of the NaN fill; all cells of the maps are live: dummy grid cells are not part of this tensor)
        got = m.rgb_intermediate("handoff", B).cpu()
        assert got.dtype == torch.bfloat16 and tuple(got.shape) == (B, p.in_channels, hm, hm)
        assert bool(torch.isfinite(got.float()).all())
        want = cat.cpu().to(torch.bfloat16)                        # torch rounds to nearest even
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), int((got.view(torch.int16) != want.view(torch.int16)).sum())
    finally:
        m.set_precision("f32")
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ 6. other heatmap sides
@pytest.mark.parametrize("hm", [32, 96])
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_other_sides_run_the_exact_fp32_routes_by_name(hm, mode):
    m, p = _model("UnrealEgo", hm)
    left, right = _frames("sides", 2, hm)
    try:
        m.set_precision(mode)
        want, want_cat = _composed(m, p, left, right)
        pose, cat = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        only = m.predict_pose_from_rgb(left, right)
        torch.cuda.synchronize()
        assert m.rgb_form() == "scratch"                           # no bf16 channels-last estimator at this side: never the hand-off
        assert torch.equal(cat, want_cat) and torch.equal(pose, want) and torch.equal(only, want)
        if mode == "bf16":                                         # the estimators ran the exact-fp32 path: the heatmaps are the fp32 mode's
            m.set_precision("f32")
            _, cat32 = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
            assert torch.equal(cat, cat32)
    finally:
        m.set_precision("f32")


def test_mixed_precisions_run_the_module_forwards_by_name():
    """networks in different precisions cannot share one handle: the module forwards + predict_pose run, same bits as composing them by hand;
    graphed is refused by name, and so is a network in train mode -- before either estimator runs"""
    from egotap_amd import lib as L
    m, p = _model("UnrealEgo", 64)
    left, right = _frames("mixed", 3, 64)
    try:
        m.net_HeatMap.set_precision("bf16")
        m.net_RotHeatMap.set_precision("bf16")                      # the head stays fp32
        assert "different precisions" in m._rgb_one_call_refusal()
        want, want_cat = _composed(m, p, left, right)
        pose, cat = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        only = m.predict_pose_from_rgb(left, right)
        torch.cuda.synchronize()
        assert torch.equal(pose, want) and torch.equal(cat, want_cat) and torch.equal(only, want)
        with pytest.raises(L.EgotapError, match="ungraphed"):
            m.predict_pose_from_rgb(left, right, graphed=True)
        m.net_AutoEncoder.train()
        with pytest.raises(L.EgotapError, match="eval mode"):
            m.predict_pose_from_rgb(left, right)
    finally:
        m.eval()
        m.set_precision("f32")


def test_rgb_intermediate_needs_an_ungraphed_call():
    from egotap_amd import lib as L, models
    from egotap_amd.options import preset_defaults
    opt = preset_defaults("UnrealEgo", 64)
    opt.model, opt.isTrain, opt.use_amp, opt.gpu_ids, opt.use_gt_heatmap = "egotap_autoencoder", False, False, [0], False
    fresh = models.create_model(opt)
    with pytest.raises(L.EgotapError, match="no ungraphed"):
        fresh.rgb_intermediate("heatmaps", 1)


# ------------------------------------------------------------------------------------------------------------ 7. graph
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graphed_replays_equal_eager(mode):
    m, p = _model("UnrealEgo", 64)
    try:
        m.set_precision(mode)
        if mode == "bf16":
            m.freeze_weights(batch=2)
        for ret in (False, True):
            for k, B in enumerate((2, 2, 3)):                      # two replays with fresh inputs, then a second batch size
                left, right = _frames(f"graph{k}", B, 64)
                eager = m.predict_pose_from_rgb(left, right, return_heatmaps=ret)
                eager = tuple(t.clone() for t in eager) if ret else (eager.clone(),)
                got = m.predict_pose_from_rgb(left, right, return_heatmaps=ret, graphed=True)
                got = got if ret else (got,)
                torch.cuda.synchronize()
                for a, b in zip(got, eager):
                    assert torch.equal(a, b), (mode, ret, k, float((a - b).abs().max()))
        keys = list(m._rgb["graphs"])
        assert len(keys) == 4 and {k[0] for k in keys} == {2, 3} and {k[1] for k in keys} == {False, True}      # one graph per (B, heatmaps wanted)
    finally:
        m._rgb["graphs"].clear()
        m.unfreeze_weights()
        m.set_precision("f32")


# ------------------------------------------------------------------------------------------------------------ 8. independence
def test_frames_are_independent_of_their_batch():
    """frame i of a B = 37 call against the same frame in a B = 3 call: small batches split their GEMMs over K by batch size, so to rounding
    (1e-5), as test_batch_rows_are_independent_and_deterministic states the property; two runs agree bit for bit"""
    m, p = _model("UnrealEgo", 64)
    left, right = _frames("indep", 37, 64)
    big = m.predict_pose_from_rgb(left, right).clone()
    again = m.predict_pose_from_rgb(left, right).clone()
    small = m.predict_pose_from_rgb(left[:3].contiguous(), right[:3].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(big, again)
    err = float((big[:3] - small).abs().max())
    print(f"frame in B = 37 against the same frame in B = 3: max |diff| = {err:.2e} (gate 1e-5)")
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------------------ 9. one session
def test_second_call_creates_and_binds_nothing(monkeypatch):
    """the host side of two consecutive calls (B = 2 in chunks of one frame, so the chunk loop runs twice): the serving entry creates ONE handle
    and binds on the first call only, the head's graphed entry captures once -- and both keep the bits of evaluate() / predict_pose"""
    from egotap_amd import lib as L
    m, p = _model("UnrealEgo", 64)
    m.opt.hm_chunk = 1
    m.__dict__.pop("_rgb", None)                                   # (the cached model may have served before: start without a serving handle)
    left, right = _frames("session", 2, 64)
    want, want_cat = _evaluate(m, p, left, right)
    lib, count = L.load(), {}
    for name in ("egotap_create", "egotap_bind_param", "egotap_predict_pose_rgb_workspace_bytes", "egotap_lift_workspace_bytes"):
        def counted(*args, _fn=getattr(lib, name), _name=name):
            count[_name] = count.get(_name, 0) + 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, counted)
    first = m.predict_pose_from_rgb(left, right).clone()
    assert count["egotap_create"] == 1 and count["egotap_bind_param"] > 0 and count["egotap_predict_pose_rgb_workspace_bytes"] == 1
    binds = count["egotap_bind_param"]
    second = m.predict_pose_from_rgb(left, right)
    torch.cuda.synchronize()
    assert count["egotap_create"] == 1 and count["egotap_bind_param"] == binds and count["egotap_predict_pose_rgb_workspace_bytes"] == 2
    assert torch.equal(first, want) and torch.equal(second, want)
    net = m.net_AutoEncoder
    net.__dict__.pop("_graphs", None)
    eager = net.predict_pose(want_cat).clone()
    count.clear()
    a = net.predict_pose_graphed(want_cat).clone()
    sized = count.get("egotap_lift_workspace_bytes", 0)            # the capture sizes the module's workspace (eager warm-up) and the graph's own
    b = net.predict_pose_graphed(want_cat)
    torch.cuda.synchronize()
    try:
        assert len(net._graphs) == 1 and "egotap_create" not in count and "egotap_bind_param" not in count
        assert sized == 2 and count["egotap_lift_workspace_bytes"] == sized      # a replay asks for nothing
        assert torch.equal(a, eager) and torch.equal(b, eager) and torch.equal(eager, want)
    finally:
        net._graphs.clear()
