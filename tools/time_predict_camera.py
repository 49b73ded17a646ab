"""Times "camera bytes in, pose out" with and without the byte entries, all arms in ONE process, alternating rounds:

    python tools/time_predict_camera.py [--batches 1,8,64,256] [--reps 20] [--rounds 3] [--json OUT]
    rocprofv3 --kernel-trace --stats -- python tools/time_predict_camera.py --once        # one call per arm: stem / converter durations

Both arms start from the same pinned host bytes uint8 [B, 256, 256, 3] x 2 and end with the pose on the device (wall clock around upload + call +
synchronize, median of --reps calls per round):
  A    what a caller does today on the device: upload the bytes, astype(float32) / 255, normalise in the reference's arithmetic (float64, .float()
       last: utils/util.py:188-197, :438), permute to CHW, contiguous(), predict_pose_from_rgb
  A32  the same with the normalisation in fp32 (what most callers would write; NOT the reference's bits -- timed for information only)
  B    upload the bytes, predict_pose_from_camera
A and B must give equal bits (asserted).  Configurations: bf16 frozen and fp32; graphed as well at B = 1 / 8."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egotap_amd import lib as L  # noqa: E402
from egotap_amd import models, spec  # noqa: E402
from egotap_amd.options import preset_defaults  # noqa: E402
from egotap_amd.synthetic import synth_hm_state_dict, synth_state_dict  # noqa: E402


def build_model():
    opt = preset_defaults("UnrealEgo", 64)
    opt.model, opt.isTrain, opt.use_amp, opt.gpu_ids, opt.use_gt_heatmap = "egotap_autoencoder", False, False, [0], False
    m = models.create_model(opt)
    p = spec.lift_preset("UnrealEgo", 64)
    J = p.n_joints_hm
    m.net_AutoEncoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
    m.net_HeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(J, "hm_pos.").items()})
    m.net_RotHeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(2 * J, "hm_rot.").items()})
    m.eval()
    return m


def host_frames(B, S0=256):
    g = torch.Generator().manual_seed(B)
    return [torch.randint(0, 256, (B, S0, S0, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(2)]


def arms(m, graphed):
    mean64 = torch.tensor(spec.RGB_MEAN, dtype=torch.float64, device="cuda").view(1, 1, 1, 3)
    std64 = torch.tensor(spec.RGB_STD, dtype=torch.float64, device="cuda").view(1, 1, 1, 3)
    mean32, std32 = mean64.float(), std64.float()
    d255 = torch.tensor(255.0, device="cuda")      # a TENSOR divisor: torch divides by a Python scalar as a multiplication by its reciprocal, which is not float32(v) / float32(255)

    def norm64(x8):
        return (((x8.float() / d255).double() - mean64) / std64).float().permute(0, 3, 1, 2).contiguous()

    def norm32(x8):
        return ((x8.float() / d255 - mean32) / std32).permute(0, 3, 1, 2).contiguous()

    def a(l, r):
        l8, r8 = l.cuda(non_blocking=True), r.cuda(non_blocking=True)
        return m.predict_pose_from_rgb(norm64(l8), norm64(r8), graphed=graphed)

    def a32(l, r):
        l8, r8 = l.cuda(non_blocking=True), r.cuda(non_blocking=True)
        return m.predict_pose_from_rgb(norm32(l8), norm32(r8), graphed=graphed)

    def b(l, r):
        return m.predict_pose_from_camera(l.cuda(non_blocking=True), r.cuda(non_blocking=True), graphed=graphed)
    return {"A": a, "A32": a32, "B": b}


def timed(fn, l, r, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(l, r)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def configure(m, mode, B):
    m.unfreeze_weights()
    m.set_precision("bf16" if mode == "bf16_frozen" else "f32")
    if mode == "bf16_frozen":
        m.freeze_weights(batch=min(B, int(getattr(m.opt, "hm_chunk", 256))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one call per arm and configuration at B = 64, and the converter alone at B = 256 (for a kernel trace)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    m = build_model()
    if args.once:
        l, r = host_frames(64)
        for mode in ("bf16_frozen", "f32"):
            configure(m, mode, 64)
            f = arms(m, False)
            for name in ("A", "B", "A", "B"):
                f[name](l, r)
            torch.cuda.synchronize()
        l8, r8 = (t.cuda() for t in host_frames(256))
        table = m.camera_table(l8.device)
        for _ in range(3):
            L.rgb_u8_to_f32(l8, r8, table)
        torch.cuda.synchronize()
        print("once: done")
        return
    rows = []
    for mode in ("bf16_frozen", "f32"):
        for B in [int(b) for b in args.batches.split(",")]:
            l, r = host_frames(B)
            for graphed in ((False, True) if B <= 8 else (False,)):
                configure(m, mode, B)
                f = arms(m, graphed)
                pa, pb = f["A"](l, r).clone(), f["B"](l, r).clone()
                p32 = f["A32"](l, r)
                torch.cuda.synchronize()
                assert torch.equal(pa, pb), (mode, B, graphed, float((pa - pb).abs().max()))
                d32 = float((p32 - pa).abs().max())
                for name in f:                                           # warm-up (graphs captured, workspaces grown)
                    timed(f[name], l, r, 3)
                per = {name: [] for name in f}
                for _ in range(args.rounds):
                    for name in f:                                       # alternating: A, A32, B, A, A32, B, ...
                        per[name].append(timed(f[name], l, r, args.reps))
                row = {"mode": mode, "batch": B, "graphed": graphed, "equal_bits_A_B": True, "max_abs_A32_minus_A": d32,
                       **{name: {"rounds_ms": [round(v, 4) for v in vs], "median_ms": round(statistics.median(vs), 4),
                                 "spread_ms": round(max(vs) - min(vs), 4)} for name, vs in per.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
                m._rgb["graphs"].clear()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
