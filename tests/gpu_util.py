import types

import numpy as np
import torch

from egotap_amd import networks, spec
from egotap_amd.synthetic import synth_state_dict, synth_input


def make_opt(preset="UnrealEgo", hm=64):
    from egotap_amd.options import preset_defaults
    return preset_defaults(preset, hm)


_cache = {}


def lift_net(preset="UnrealEgo", hm=64, device="cuda"):
    """EgoTAPAutoEncoder with the hash-RNG weights, on the GPU, eval mode (cached per preset)."""
    key = (preset, hm, device)
    if key not in _cache:
        p = spec.lift_preset(preset, hm)
        net = networks.EgoTAPAutoEncoder(make_opt(preset, hm), input_channel_scale=2)
        sd_np = synth_state_dict(spec.lift_state_spec(p))
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
        net = net.to(device).eval()
        _cache[key] = (net, sd_np, p)
    return _cache[key]


def hm_net(which="pos", device="cuda", preset="UnrealEgo", hm=64, model_name="resnet18"):
    """HeatMap_UnrealEgo_Shared (position or sin/cos net) with hash-RNG weights on the GPU, eval mode."""
    from egotap_amd.synthetic import synth_hm_state_dict
    key = ("hm", which, device, preset, hm, model_name)
    if key not in _cache:
        opt = make_opt(preset, hm)
        if which == "pos":
            opt.num_rot_heatmap = 0
        else:
            opt.num_heatmap = 0
        net = networks.HeatMap_UnrealEgo_Shared(opt, model_name, input_channel_scale=2)
        sd_np = synth_hm_state_dict(net.num_heatmap, f"hm_{which}.", model_name)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=True)
        net = net.to(device).eval()
        _cache[key] = (net, sd_np)
    return _cache[key]


def hm_handle(precision="f32", device="cuda"):
    """C ABI handle of an estimator at `precision` with the repacked-weight scratch of the bf16 convolution kernels bound, the way
    hm_training.hm_train_forward binds it (without that buffer conv_any runs the fp32 kernels in every mode).  One module per precision,
    kept alive here: the handle and the buffer belong to it."""
    from egotap_amd import lib as L
    from egotap_amd.session import grown
    from egotap_amd.train_ops import _p
    key = ("hm_handle", precision, device)
    if key not in _cache:
        opt = make_opt()
        opt.num_rot_heatmap = 0
        net = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", input_channel_scale=2).to(device)
        net.set_precision(precision)
        _cache[key] = net
    net = _cache[key]
    h = net._ensure_handle()
    if precision != "f32":
        pack = grown(net, "_pack", L.load().egotap_hmtrain_pack_bytes(), next(net.parameters()).device)
        L.check(L.load().egotap_hmtrain_set_pack_buffer(h, _p(pack), pack.numel()))
    return h


def conv_kernels_of(h, fn):
    """kernel names of the convolution launches `fn` makes on handle `h`, in order (the event-timing hook of egotap_debug.h, read after
    every launch would aggregate by role: so fn is expected to make ONE conv_any launch per call of this function)"""
    import ctypes as C
    import json
    from egotap_amd import lib as L
    lib = L.load()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        fn()
        torch.cuda.synchronize()
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        return [(d["kernel"], d["launches"]) for d in json.loads(lib.egotap_timing_detail(h).decode())]
    finally:
        L.check(lib.egotap_timing_enable(h, 0))


def serving_model(preset="UnrealEgo", hm=64):
    """test-mode wrapper with the hash-RNG weights in all three networks (built and uploaded once per (preset, hm), shared by every serving test file);
    every fetch resets it: f32, unfrozen, eval mode, opt.hm_chunk = 256.  Returns (model, lift preset)."""
    from egotap_amd import models
    from egotap_amd.synthetic import synth_hm_state_dict
    key = ("serving", preset, hm)
    if key not in _cache:
        opt = make_opt(preset, hm)
        opt.model, opt.isTrain, opt.use_amp, opt.gpu_ids, opt.use_gt_heatmap = "egotap_autoencoder", False, False, [0], False
        m = models.create_model(opt)
        p = spec.lift_preset(preset, hm)
        J = p.n_joints_hm
        m.net_AutoEncoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
        m.net_HeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(J, "hm_pos.").items()})
        m.net_RotHeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(2 * J, "hm_rot.").items()})
        m.eval()
        _cache[key] = (m, p)
    m, p = _cache[key]
    m.set_precision("f32")
    m.unfreeze_weights()
    m.eval()
    m.opt.hm_chunk = 256
    return m, p


def timed_launches(m, fn):
    """(role, kernel, launches) of the timed launches `fn` makes on the serving handle of `m` (egotap_debug.h egotap_timing_*)"""
    import ctypes as C
    import json
    from egotap_amd import lib as L
    lib, h = L.load(), m._rgb["handle"].h
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        fn()
        torch.cuda.synchronize()
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        return [(d["role"], d["kernel"], d["launches"]) for d in json.loads(lib.egotap_timing_detail(h).decode())]
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
