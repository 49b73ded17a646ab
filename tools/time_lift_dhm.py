#!/usr/bin/env python3
"""Step time (train-mode forward + pose loss + backward) of the lifting head with and without the gradient w.r.t. its input heatmaps.

The two settings alternate within one process (hm.requires_grad on / off, one step each per round), so drift of the clock or of the
device affects both alike.  --repo runs the same measurement against another checkout (e.g. the parent commit, setting "off" only: it
has no heatmap gradient) so that builds can be alternated in one session.  Prints one JSON line per case.

usage: python tools/time_lift_dhm.py [--cases f32:256,bf16:1024] [--rounds 8] [--warmup 2] [--settings on,off] [--repo PATH]
"""
from __future__ import annotations

import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="f32:256,bf16:1024", help="precision:batch, comma separated (UnrealEgo, 64 x 64 heatmaps)")
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--settings", default="on,off")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    from egotap_amd import networks, spec
    from egotap_amd.options import preset_defaults
    from egotap_amd.synthetic import synth_state_dict
    from egotap_amd.training import PoseLossFn, release_scratch

    settings = args.settings.split(",")
    torch.cuda.set_device(0)
    for case in args.cases.split(","):
        mode, B = case.split(":")
        B = int(B)
        p = spec.lift_preset("UnrealEgo")
        net = networks.EgoTAPAutoEncoder(preset_defaults("UnrealEgo"), input_channel_scale=2)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
        net = net.cuda().train()
        net.set_precision(mode)
        g = torch.Generator(device="cuda").manual_seed(0)
        hm = torch.rand((B, p.in_channels, 64, 64), device="cuda", generator=g)
        gt = torch.rand((B, p.out_joints, 3), device="cuda", generator=g) * 2 - 1
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

        def step(on):
            x = hm.detach().requires_grad_(on)
            for q in net.parameters():
                q.grad = None
            ev[0].record()
            pose = net(x)[0]
            PoseLossFn.apply(net, pose, gt, 0.1, -0.01).sum().backward()
            ev[1].record()
            torch.cuda.synchronize()
            if on:
                res["dhm_returned"] = x.grad is not None
            return ev[0].elapsed_time(ev[1])

        res = {"repo": os.path.abspath(args.repo), "precision": mode, "B": B, "rounds": args.rounds}

        for _ in range(args.warmup):
            for s in settings:
                step(s == "on")
        ms = {s: [] for s in settings}
        for _ in range(args.rounds):
            for s in settings:
                ms[s].append(step(s == "on"))
        for s, v in ms.items():
            v = sorted(v)
            res[s] = {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1], "all_ms": [round(x, 3) for x in ms[s]]}
        if "on" in ms and "off" in ms:
            res["on_minus_off_ms"] = res["on"]["median_ms"] - res["off"]["median_ms"]
        print(json.dumps(res), flush=True)
        release_scratch(net)
        del net, hm, gt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
