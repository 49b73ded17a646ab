"""Camera bytes straight into the stems: egotap_rgb_u8_to_f32, HeatMap_UnrealEgo_Shared.forward_from_camera (egotap_hm_forward_u8) and
EgoTAPAutoEncoderModel.predict_pose_from_camera (egotap_predict_pose_rgb_u8).

The reference expression of every case is the host gather T(x8)[b, c, y, x] = table[c][x8[b, y, x, c]] fed to the existing float entry.  The byte
paths read the same values and keep every summation order, so EVERY comparison here is torch.equal: no tolerance is involved.

Frames are random bytes in which 0 and 255 both occur; the outermost two rows and columns of every image are byte 0 in some cases and byte 255 in
others, so a halo filled with table[c][0] (about -2.1) instead of 0.0, or a clamped edge, fails."""

import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import hm_net, serving_model as _model, timed_launches as _launches

pytestmark = pytest.mark.gpu


def _table():
    return torch.from_numpy(spec.rgb_u8_table()).cuda()


def _frames8(seed, B, S0, edge):
    """stereo frames uint8 [B, S0, S0, 3] x 2 on the GPU: random bytes, a 0 and a 255 inside every image, a two-pixel border of byte `edge`"""
    g = torch.Generator().manual_seed(1000 * seed + 7 * B + S0 + edge)
    out = []
    for _ in range(2):
        x = torch.randint(0, 256, (B, S0, S0, 3), generator=g, dtype=torch.uint8)
        x[:, 5, 7, :] = 0
        x[:, 6, 9, :] = 255
        for sl in (slice(0, 2), slice(S0 - 2, S0)):
            x[:, sl, :, :] = edge
            x[:, :, sl, :] = edge
        assert bool((x == 0).any()) and bool((x == 255).any())
        out.append(x.cuda())
    return out


def T(x8, table):
    """the reference expression: the host-side gather of the table, permuted to NCHW"""
    idx = x8.long()
    return torch.stack([table[c][idx[..., c]] for c in range(3)], dim=1).contiguous()


# ------------------------------------------------------------------------------------------------------------ 1. the converter
@pytest.mark.parametrize("S0", [64, 256])
@pytest.mark.parametrize("B", [1, 3])
def test_converter_equals_the_gather_and_stays_inside_its_outputs(S0, B):
    table = _table()
    l8, r8 = _frames8(1, B, S0, 255 if B == 1 else 0)
    n, pad, canary = B * 3 * S0 * S0, 1024, -12345.0
    flat = torch.full((2 * (n + pad) + pad,), canary, device="cuda")
    left, right = flat[pad:pad + n], flat[2 * pad + n:2 * pad + 2 * n]          # canaries in front of, between and behind the outputs
    assert left.data_ptr() % 16 == 0 and right.data_ptr() % 16 == 0
    L.check(L.load().egotap_rgb_u8_to_f32(L.ptr(l8), L.ptr(r8), B, S0, L.ptr(table), L.ptr(left), L.ptr(right), L.stream()))
    torch.cuda.synchronize()
    assert torch.equal(left.view(B, 3, S0, S0), T(l8, table)) and torch.equal(right.view(B, 3, S0, S0), T(r8, table))
    for lo, hi in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, flat.numel())):
        assert bool((flat[lo:hi] == canary).all()), (lo, hi)
    a, b = L.rgb_u8_to_f32(l8, r8, table)                                         # the Python face
    assert torch.equal(a, left.view(B, 3, S0, S0)) and torch.equal(b, right.view(B, 3, S0, S0))


# ------------------------------------------------------------------------------------------------------------ 2. one estimator
CASES = [(which, "resnet18", "UnrealEgo", 64, mode, B) for which in ("pos", "rot") for mode in ("f32", "bf16") for B in (2, 3)]
CASES += [("pos", "resnet34", "UnrealEgo", 64, "f32", 2),
          ("pos", "resnet18", "EgoCap", 128, "bf16", 1),       # 512 x 512 frames: several 64-column segments and row groups per image, the carry column
          ("pos", "resnet18", "UnrealEgo", 32, "f32", 2)]      # no stem reads bytes at this side: the converter route


@pytest.mark.parametrize("which,model_name,preset,hm,mode,B", CASES)
def test_forward_from_camera_equals_the_eval_forward_on_the_gather(which, model_name, preset, hm, mode, B):
    net, _ = hm_net(which, preset=preset, hm=hm, model_name=model_name)
    table = net.camera_table(torch.device("cuda", torch.cuda.current_device()))
    assert torch.equal(table, _table())
    l8, r8 = _frames8(2, B, 4 * hm, 0 if B == 2 else 255)
    try:
        net.set_precision(mode)
        want = net(T(l8, table), T(r8, table)).clone()
        got = net.forward_from_camera(l8, r8)
        torch.cuda.synchronize()
        assert tuple(got.shape) == tuple(want.shape) and bool(torch.isfinite(got).all())
        assert torch.equal(got, want), float((got - want).abs().max())
    finally:
        net.set_precision("f32")


# ------------------------------------------------------------------------------------------------------------ 3. one call
@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_predict_pose_from_camera_equals_the_float_entry_on_the_gather(mode):
    m, p = _model()
    table = m.camera_table(torch.device("cuda", torch.cuda.current_device()))
    try:
        m.set_precision(mode)
        for frozen in ((False, True) if mode == "bf16" else (False,)):
            if frozen:
                assert m.freeze_weights(batch=2) == {}
            for B, chunk, edge in ((2, 256, 0), (3, 2, 255)):           # hm_chunk = 2 at B = 3: a ragged last piece
                m.opt.hm_chunk = chunk
                l8, r8 = _frames8(3, B, 256, edge)
                lf, rf = T(l8, table), T(r8, table)
                want_pose, want_cat = (t.clone() for t in m.predict_pose_from_rgb(lf, rf, return_heatmaps=True))
                want_only = m.predict_pose_from_rgb(lf, rf).clone()
                want_form = m.rgb_form()
                pose, cat = m.predict_pose_from_camera(l8, r8, return_heatmaps=True)
                torch.cuda.synchronize()
                assert m.rgb_form() == "heatmaps"
                assert torch.equal(cat, want_cat), (mode, frozen, B, float((cat - want_cat).abs().max()))
                assert torch.equal(pose, want_pose), (mode, frozen, B)
                only = m.predict_pose_from_camera(l8, r8)
                torch.cuda.synchronize()
                assert m.rgb_form() == want_form == ("handoff" if mode == "bf16" else "scratch")      # bf16: conv_heatmap wrote the head's operand
                assert torch.equal(only, want_only), (mode, frozen, B)
            if frozen:
                assert all(n.weights_frozen for n in (m.net_HeatMap, m.net_RotHeatMap, m.net_AutoEncoder))
    finally:
        m.unfreeze_weights()
        m.set_precision("f32")


def test_other_side_runs_the_converter_inside_the_call():
    m, p = _model("UnrealEgo", 32)
    table = m.camera_table(torch.device("cuda", torch.cuda.current_device()))
    m.opt.hm_chunk = 2
    l8, r8 = _frames8(4, 3, 128, 255)
    want_pose, want_cat = (t.clone() for t in m.predict_pose_from_rgb(T(l8, table), T(r8, table), return_heatmaps=True))
    pose, cat = m.predict_pose_from_camera(l8, r8, return_heatmaps=True)
    torch.cuda.synchronize()
    assert torch.equal(cat, want_cat) and torch.equal(pose, want_pose)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_graphed_replays_with_fresh_bytes(mode):
    m, p = _model()
    table = m.camera_table(torch.device("cuda", torch.cuda.current_device()))
    try:
        m.set_precision(mode)
        if mode == "bf16":
            m.freeze_weights(batch=2)
        m._rgb_state(torch.device("cuda", torch.cuda.current_device())).graphs.clear()
        for k in range(2):                                          # the second call replays: other bytes copied into the static inputs
            l8, r8 = _frames8(5 + k, 2, 256, 255 * k)
            want = m.predict_pose_from_rgb(T(l8, table), T(r8, table)).clone()
            got = m.predict_pose_from_camera(l8, r8, graphed=True)
            torch.cuda.synchronize()
            assert torch.equal(got, want), (mode, k)
        keys = list(m._rgb["graphs"])
        assert len(keys) == 1 and "u8" in keys[0]                   # one capture, keyed by the source kind
        l8, r8 = _frames8(5, 2, 256, 0)
        m.predict_pose_from_rgb(T(l8, table), T(r8, table), graphed=True)
        assert len(m._rgb["graphs"]) == 2                           # the float entry's graph is another one
    finally:
        m._rgb["graphs"].clear()
        m.unfreeze_weights()
        m.set_precision("f32")


def test_second_call_creates_and_binds_nothing(monkeypatch):
    m, p = _model()
    m.__dict__.pop("_rgb", None)
    l8, r8 = _frames8(7, 2, 256, 0)
    lib, count = L.load(), {}
    for name in ("egotap_create", "egotap_bind_param", "egotap_predict_pose_rgb_u8_workspace_bytes"):
        def counted(*args, _fn=getattr(lib, name), _name=name):
            count[_name] = count.get(_name, 0) + 1
            return _fn(*args)
        monkeypatch.setattr(lib, name, counted)
    first = m.predict_pose_from_camera(l8, r8).clone()
    assert count["egotap_create"] == 1 and count["egotap_bind_param"] > 0 and count["egotap_predict_pose_rgb_u8_workspace_bytes"] == 1
    binds = count["egotap_bind_param"]
    second = m.predict_pose_from_camera(l8, r8)
    torch.cuda.synchronize()
    assert count["egotap_create"] == 1 and count["egotap_bind_param"] == binds and count["egotap_predict_pose_rgb_u8_workspace_bytes"] == 2
    assert torch.equal(first, second)
    # and the float entry afterwards shares that handle: still one, nothing bound again
    table = m.camera_table(l8.device)
    third = m.predict_pose_from_rgb(T(l8, table), T(r8, table))
    torch.cuda.synchronize()
    assert count["egotap_create"] == 1 and count["egotap_bind_param"] == binds and torch.equal(third, first)


# ------------------------------------------------------------------------------------------------------------ 4. the float path is untouched
@pytest.mark.parametrize("mode,hm", [("f32", 64), ("bf16", 64), ("f32", 32)])
def test_float_entry_launches_what_it_launched(mode, hm):
    """the byte call's timed launches are the float call's plus the byte-source stem (sides 64 / 128, one per estimator forward) or the converter
    (other sides, one per piece); the float call's list names no byte kernel"""
    m, p = _model("UnrealEgo", hm)
    table = m.camera_table(torch.device("cuda", torch.cuda.current_device()))
    l8, r8 = _frames8(8, 2, 4 * hm, 0)
    lf, rf = T(l8, table), T(r8, table)
    try:
        m.set_precision(mode)
        m.predict_pose_from_rgb(lf, rf)                              # (the serving handle exists from here on)
        floats = _launches(m, lambda: m.predict_pose_from_rgb(lf, rf))
        bytes_ = _launches(m, lambda: m.predict_pose_from_camera(l8, r8))
        assert floats and not [x for x in floats if "u8" in x[0] or "u8" in x[1]], floats
        new = [x for x in bytes_ if "u8" in x[1]]
        want = {("f32", 64): ("hm.stem_u8", "stem_conv7_mfma_u8_kernel"), ("bf16", 64): ("hm.stem_u8", "stem_pool_bf16s_u8_kernel"),
                ("f32", 32): ("rgb_u8_to_f32", "rgb_u8_to_f32_kernel")}[(mode, hm)]
        # sides 64 / 128: two estimator forwards, one byte-reading stem each; elsewhere the one piece is converted once and both estimators read it
        assert new == [want + (2 if hm == 64 else 1,)], new
        assert [x for x in bytes_ if x not in new] == floats
    finally:
        m.set_precision("f32")
