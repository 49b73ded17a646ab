#!/usr/bin/env python3
"""Device time of the two heatmap estimators' fp32 eval forward at several heatmap sides, and its rate per FLOP relative to side 64.

usage: python tools/time_hm_sides.py [--sides 32 48 64 96] [--batch 64] [--iters 5]
Prints one line per (side, net) and a JSON summary.  FLOPs are counted from the layer shapes (2 x MACs of every convolution; the stem,
max-pool and upsamples included as convolutions only for the stem)."""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def hm_flops(hm, n_out, blocks=(2, 2, 2, 2)):
    """multiply-adds x 2 of one frame (two eyes) of HeatMap_UnrealEgo_Shared over a BasicBlock ResNet"""
    S0 = 4 * hm
    f = 2 * 64 * 3 * 49 * (S0 // 2) ** 2 * 2                   # stem, two eyes
    cin, side = 64, hm
    for i, c in enumerate((64, 128, 256, 512)):
        for b in range(blocks[i]):
            so = side // 2 if (b == 0 and i > 0) else side
            f += 2 * 2 * c * cin * 9 * so * so                    # conv1 (stride 2 in the first block of stages 2-4)
            if b == 0 and i > 0:
                f += 2 * 2 * c * cin * so * so                    # 1x1 downsample
            f += 2 * 2 * c * c * 9 * so * so                      # conv2
            cin, side = c, so
    s64, s32, s16, s8 = hm, hm // 2, hm // 4, hm // 8
    f += 2 * 1024 * 1024 * s8 * s8 + 2 * 516 * 512 * s16 * s16 + 2 * 1024 * 1540 * 9 * s16 * s16
    f += 2 * 256 * 256 * s32 * s32 + 2 * 512 * 1280 * 9 * s32 * s32
    f += 2 * 128 * 128 * s64 * s64 + 2 * 512 * 640 * 9 * s64 * s64 + 2 * n_out * 512 * s64 * s64
    return f


def kernel_detail(net, left, right):
    """per conv kernel of one forward: launches, event-bracketed ms, algorithmic FLOPs (egotap_debug.h egotap_timing_*)"""
    import ctypes as C
    from egotap_amd import lib as L
    lib, h = L.load(), net._ensure_handle()
    lib.egotap_timing_enable(h, 1)
    try:
        net(left, right)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        per = {}
        for d in json.loads(lib.egotap_timing_detail(h).decode()):
            k = per.setdefault(d["kernel"], {"launches": 0, "ms": 0.0, "gflop": 0.0})
            k["launches"] += d["launches"]
            k["ms"] += d["ms"]
            k["gflop"] += d["flops"] / 1e9
    finally:
        lib.egotap_timing_enable(h, 0)
    for k, v in sorted(per.items(), key=lambda kv: -kv[1]["ms"]):
        v["tflops"] = v["gflop"] / v["ms"] if v["ms"] > 0 else 0.0
        print(f"    {k:44s} {v['launches']:3d} x  {v['ms']:8.3f} ms  {v['gflop']:8.1f} GFLOP  {v['tflops']:6.1f} TFLOP/s", flush=True)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sides", type=int, nargs="+", default=[32, 48, 64, 96])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--detail", action="store_true", help="one more forward per net with the handle's GEMM timing hook: per-kernel ms / FLOPs")
    a = ap.parse_args()
    from gpu_util import hm_net
    from egotap_amd.synthetic import synth_input
    torch.cuda.set_device(0)
    out = {}
    for hm in a.sides:
        B = a.batch
        left = torch.from_numpy(synth_input(f"tL{hm}", (B, 3, 4 * hm, 4 * hm), -2.0, 2.0)).cuda()
        right = torch.from_numpy(synth_input(f"tR{hm}", (B, 3, 4 * hm, 4 * hm), -2.0, 2.0)).cuda()
        for which in ("pos", "rot"):
            net, _ = hm_net(which, hm=hm)
            net(left, right)                                        # warm-up (code objects, workspace)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                net(left, right)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            fl = hm_flops(hm, 2 * net.num_heatmap) * B
            out[f"{which}_{hm}"] = {"side": hm, "net": which, "B": B, "ms": ms, "gflop": fl / 1e9, "tflops": fl / ms / 1e9}
            print(f"hm {hm:4d} {which}: {ms:9.3f} ms  {fl / 1e9:9.1f} GFLOP  {fl / ms / 1e9:6.1f} TFLOP/s", flush=True)
            if a.detail:
                out[f"{which}_{hm}"]["kernels"] = kernel_detail(net, left, right)
            del net
            torch.cuda.empty_cache()
    for k, v in out.items():
        base = out.get(f"{v['net']}_64")
        if base:
            v["rate_vs_64"] = v["tflops"] / base["tflops"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
