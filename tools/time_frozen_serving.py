"""Times bf16 serving with and without frozen weights, device events after warm-up, all arms in ONE process:

    python tools/time_frozen_serving.py [--parent-lib PATH] [--reps 200] [--json OUT]

Arms, each driven through the C ABI by the same thin ctypes driver (so the host work per call is the same few lines for every arm):
  parent      a second library loaded from --parent-lib (a build of the parent commit: EGOTAP_LIB=... python -m egotap_amd.build there)
  not_frozen  this build, default behaviour
  frozen      this build after egotap_lift_freeze / egotap_hm_freeze
and the same three through a captured graph for the lifting head.  Lifting head: UnrealEgo, 64 x 64 heatmaps, B = 1, 8, 32;
estimators (position and limb net, resnet18, 256 x 256 RGB): B = 1, 8.  The arms are interleaved in rounds; per arm the median and the
10th / 90th percentile of the per-call times are printed.  The last block times the MODULE's predict_pose (host wall clock per call at
B = 1, frozen against not frozen): what the per-call staleness check of networks._FrozenWeights costs.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egotap_amd import lib as L  # noqa: E402
from egotap_amd import networks, spec  # noqa: E402
from egotap_amd.options import preset_defaults  # noqa: E402
from egotap_amd.synthetic import synth_hm_state_dict, synth_input, synth_state_dict  # noqa: E402

VP = C.c_void_p


def _open(path):
    """a library by path with the prototypes this tool needs (the parent build has no freeze entries: they are bound where present)"""
    lib = C.CDLL(path)
    for name, (res, args) in L._PROTOS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return lib


def _ok(lib, rc):
    if rc != 0:
        raise RuntimeError(lib.egotap_last_error().decode())


def _stream():
    return VP(torch.cuda.current_stream().cuda_stream)


class Raw:
    """one handle of `lib` bound to a module's parameter tensors, bf16 mode, scratch buffers of its own"""

    def __init__(self, lib, module, net_id):
        self.lib, self.net_id, self.keep = lib, net_id, []
        pr = module.preset
        blocks = (0, 0, 0, 0) if net_id == L.NET_LIFT else module.blocks
        cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), pr.n_joints_hm, int(pr.estimate_head), pr.hm_size, pr.hidden, pr.vit_dim, pr.vit_heads,
                             pr.vit_layers, pr.patch, pr.pu_hidden, (C.c_int32 * 4)(*blocks))
        self.h = VP()
        _ok(lib, lib.egotap_create(C.byref(cfg), C.byref(self.h)))
        sd = module.state_dict(keep_vars=True)
        for k, t in sd.items():
            _ok(lib, lib.egotap_bind_param(self.h, net_id, k.encode(), VP(t.data_ptr()), t.numel(), L.F32 if t.dtype == torch.float32 else L.I64))
        _ok(lib, lib.egotap_set_precision(self.h, L.PRECISIONS["bf16"]))
        self.module, self.arena = module, None

    def buf(self, n):
        t = torch.empty(int(n), dtype=torch.uint8, device="cuda")
        self.keep.append(t)
        return t

    def close(self):
        self.lib.egotap_destroy(self.h)


class RawLift(Raw):
    def __init__(self, lib, module, B):
        super().__init__(lib, module, L.NET_LIFT)
        pr = module.preset
        w = self.buf(2 * max(p.numel() for p in module.parameters() if p.dim() >= 2))
        _ok(lib, lib.egotap_set_weight_scratch(self.h, VP(w.data_ptr()), w.numel()))
        a = self.buf(2 * B * pr.seq * 4 * pr.vit_dim)
        _ok(lib, lib.egotap_set_act_scratch(self.h, VP(a.data_ptr()), a.numel()))
        need = C.c_size_t()
        _ok(lib, lib.egotap_lift_workspace_bytes(self.h, B, C.byref(need)))
        self.ws, self.B = self.buf(need.value), B
        self.x = torch.from_numpy(synth_input("hm_time", (1, pr.in_channels, pr.hm_size, pr.hm_size))).repeat(B, 1, 1, 1).contiguous().cuda()
        self.out = torch.empty((B, pr.out_joints, 3), device="cuda")

    def freeze(self):
        need = C.c_size_t()
        _ok(self.lib, self.lib.egotap_lift_frozen_bytes(self.h, C.byref(need)))
        self.arena = self.buf(need.value)
        _ok(self.lib, self.lib.egotap_lift_freeze(self.h, VP(self.arena.data_ptr()), need.value, _stream()))
        return need.value

    def __call__(self):
        _ok(self.lib, self.lib.egotap_lift_predict_pose(self.h, VP(self.x.data_ptr()), self.B, VP(self.out.data_ptr()), VP(self.ws.data_ptr()),
                                                        self.ws.numel(), _stream()))


class RawHm(Raw):
    def __init__(self, lib, module, B):
        super().__init__(lib, module, module._net)
        S = 4 * module.hm_size
        need = C.c_size_t()
        _ok(lib, lib.egotap_hm_workspace_bytes(self.h, B, C.byref(need)))
        self.ws, self.B = self.buf(need.value), B
        self.l = torch.from_numpy(synth_input("rgb_l_time", (1, 3, S, S), -2.0, 2.0)).repeat(B, 1, 1, 1).contiguous().cuda()
        self.r = torch.from_numpy(synth_input("rgb_r_time", (1, 3, S, S), -2.0, 2.0)).repeat(B, 1, 1, 1).contiguous().cuda()
        self.out = torch.empty((B, 2 * module.num_heatmap, module.hm_size, module.hm_size), device="cuda")

    def freeze(self):
        need = C.c_size_t()
        _ok(self.lib, self.lib.egotap_hm_frozen_bytes(self.h, self.net_id, self.B, C.byref(need)))
        self.arena = self.buf(need.value)
        _ok(self.lib, self.lib.egotap_hm_freeze(self.h, self.net_id, self.B, VP(self.arena.data_ptr()), need.value, _stream()))
        return need.value

    def __call__(self):
        hw = self.module.hm_size ** 2
        _ok(self.lib, self.lib.egotap_hm_forward(self.h, self.net_id, VP(self.l.data_ptr()), VP(self.r.data_ptr()), self.B, VP(self.out.data_ptr()),
                                                 self.out.shape[1] * hw, VP(self.ws.data_ptr()), self.ws.numel(), _stream()))


def graphed(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        fn()
    return g.replay


def measure(arms, reps, warmup=20, rounds=5):
    """arms: {name: callable}; interleaved rounds; returns {name: (median, p10, p90) in ms}"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    per = max(1, reps // rounds)
    for _ in range(rounds):
        for name, fn in arms.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            times[name] += [a.elapsed_time(b) for a, b in ev]
    out = {}
    for k, v in times.items():
        v = sorted(v)
        out[k] = (v[len(v) // 2], v[len(v) // 10], v[(9 * len(v)) // 10])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    new = L.load()
    new_raw = _open(L._build.LIB)
    parent = _open(a.parent_lib) if a.parent_lib else None
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": []}

    def show(what, B, r, extra=""):
        for k, (med, lo, hi) in r.items():
            print(f"{what:10s} B={B:<3d} {k:18s} median {med * 1e3:8.1f} us   p10 {lo * 1e3:8.1f}   p90 {hi * 1e3:8.1f} {extra}", flush=True)
            res["rows"].append(dict(what=what, B=B, arm=k, median_us=med * 1e3, p10_us=lo * 1e3, p90_us=hi * 1e3))

    pr = spec.lift_preset("UnrealEgo", 64)
    net = networks.EgoTAPAutoEncoder(preset_defaults("UnrealEgo", 64), input_channel_scale=2)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(pr)).items()})
    net = net.cuda().eval()
    for B in (1, 8, 32):
        hs = {"not_frozen": RawLift(new_raw, net, B), "frozen": RawLift(new_raw, net, B)}
        if parent is not None:
            hs = {"parent": RawLift(parent, net, B), **hs}
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        hs["frozen"]()
        hs["frozen"].freeze()                      # once untimed (first-launch costs), then timed
        torch.cuda.synchronize()
        t0.record()
        nbytes = hs["frozen"].freeze()
        t1.record()
        torch.cuda.synchronize()
        if B == 1:
            ms = t0.elapsed_time(t1)
            nw = sum(t.numel() for t in net._frozen_tensors())
            print(f"prep_weights_all_kernel: arena {nbytes / 1e6:.1f} MB, {ms * 1e3:.1f} us, {(6 * nw) / ms / 1e9:.2f} TB/s (fp32 read + bf16 written)", flush=True)
            res["freeze_us"], res["freeze_TBps"], res["arena_MB"] = ms * 1e3, 6 * nw / ms / 1e9, nbytes / 1e6
        outs = {}
        for k, h in hs.items():
            h()
            torch.cuda.synchronize()
            outs[k] = h.out.clone()
        assert all(torch.equal(v, outs["not_frozen"]) for v in outs.values()), "arms disagree"
        show("lift", B, measure(dict(hs), a.reps))
        show("lift+graph", B, measure({k: graphed(h) for k, h in hs.items()}, a.reps))
        for h in hs.values():
            h.close()
        del hs
        torch.cuda.empty_cache()

    for which, tag, nh in (("pos", "hm_pos.", 15), ("rot", "hm_rot.", 30)):
        opt = preset_defaults("UnrealEgo", 64)
        if which == "pos":
            opt.num_rot_heatmap = 0
        else:
            opt.num_heatmap = 0
        est = networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", 2)
        est.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(est.num_heatmap, tag).items()})
        est = est.cuda().eval()
        for B in (1, 8):
            hs = {"not_frozen": RawHm(new_raw, est, B), "frozen": RawHm(new_raw, est, B)}
            if parent is not None:
                hs = {"parent": RawHm(parent, est, B), **hs}
            hs["frozen"].freeze()
            outs = {}
            for k, h in hs.items():
                h()
                torch.cuda.synchronize()
                outs[k] = h.out.clone()
            assert all(torch.equal(v, outs["not_frozen"]) for v in outs.values()), "arms disagree"
            show("hm_" + which, B, measure(dict(hs), a.reps))
            for h in hs.values():
                h.close()
            del hs
            torch.cuda.empty_cache()

    # host cost of the module's per-call staleness check: wall clock per predict_pose call at B = 1, queue kept short
    net.set_precision("bf16")
    x = torch.from_numpy(synth_input("hm_time", (1, pr.in_channels, 64, 64))).cuda()
    host = {}
    for arm in ("not_frozen", "frozen", "not_frozen", "frozen"):
        net.freeze_weights() if arm == "frozen" else net.unfreeze_weights()
        for _ in range(20):
            net.predict_pose(x)
        torch.cuda.synchronize()
        n, t = 300, time.perf_counter()
        for _ in range(n):
            net.predict_pose(x)
        torch.cuda.synchronize()
        host.setdefault(arm, []).append((time.perf_counter() - t) / n * 1e6)
    tensors = net._frozen_tensors()
    t = time.perf_counter()
    for _ in range(2000):
        tuple((q.data_ptr(), q._version) for q in tensors)
    check_us = (time.perf_counter() - t) / 2000 * 1e6
    print(f"module predict_pose B=1 wall per call: not frozen {min(host['not_frozen']):.1f} us, frozen {min(host['frozen']):.1f} us; "
          f"the staleness tuple alone ({len(tensors)} tensors): {check_us:.1f} us", flush=True)
    res["module_wall_us"] = {k: min(v) for k, v in host.items()}
    res["staleness_check_us"] = check_us
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    _ = new


if __name__ == "__main__":
    main()
