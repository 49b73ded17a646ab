"""Times "sensor frames in, pose out" with and without the sensor entry, both arms in ONE process, alternating rounds:

    python tools/time_predict_sensor.py [--batches 1,8,64] [--sources 1024x1024,512x640] [--reps 20] [--rounds 3] [--json OUT] [--md OUT]
    rocprofv3 --kernel-trace --stats -- python tools/time_predict_sensor.py --once        # one call per arm: the resize kernel's duration

Both arms start from the same sensor frames uint8 [B, H, W, 3] x 2 ON THE DEVICE and end with the pose on the device (wall clock around call +
synchronize, median of --reps calls per round):
  A    what a caller does today: torch crop, flip of the right eye, permute to NCHW float, F.interpolate(bilinear, align_corners=False) to 4S,
       round to bytes, permute back to HWC, predict_pose_from_camera
  B    predict_pose_from_sensor(crop=..., mirror_right=True)
The two arms do not give equal bits (A rounds a float interpolation, B is the integer arithmetic of spec.resize_u8); the largest byte difference
between their resized frames is reported (at most 1 is expected from the bound 0.5 + 510 / 4096).  Configurations: bf16 frozen and fp32.

    python tools/time_predict_sensor.py --yuv [--batches 1,8,64,256] [--sources 1024x1024] [--reps 10] [--rounds 3] [--md OUT]

The same protocol from the camera's own buffer, tight NV12 frames uint8 [B, H * W * 3 / 2] x 2 on the device (report only, nothing is gated):
  A    colour conversion in torch on the device (planes unpacked, chroma replicated, float BT.601 limited-range matrix, round, clamp, to bytes), then
       predict_pose_from_sensor(crop=..., mirror_right=True) on the RGB frames
  B    predict_pose_from_sensor_yuv(layout, colour, crop=..., mirror_right=True)
The largest byte difference between A's RGB frames and spec.yuv_to_rgb_u8 is reported (at most 1 is expected: both are within 0.52 of the real value).

    python tools/time_predict_sensor.py --lens [--batches 1,8,64] [--sources 1024x1024] [--reps 10] [--rounds 3] [--md OUT]

The lens entry beside the sensor entry on the same RGB frames (report only, nothing is gated; the two arms compute different things):
  sensor   predict_pose_from_sensor(mirror_right=True): the full frame resized
  lens     predict_pose_from_lens through the maps of calibration 0 of tests/golden/ocam.npz seen by itself, 0.02 rad about the axis apart, the right
           eye mirrored
and, at B = 256, the two standalone kernels in each of their three fetches (egotap_rgb_u8_resize / egotap_yuv_u8_resize on tight NV12 and YUYV frames,
egotap_lens_remap on RGB8, NV12 and YUYV frames) timed with events, with the bytes per second each achieves counted the same way for all six: per
output pixel 3 bytes written and 12 source bytes for a pixel that has a source, plus the lens kernel's 8 map bytes.  EGOTAP_LIB=<another build's .so>
times that build with the same script (profiles/sensor_sources_summary.md: two builds alternating)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egotap_amd import lib as L  # noqa: E402
from egotap_amd import spec  # noqa: E402
from tools.time_predict_camera import build_model, configure  # noqa: E402


def sensor_frames(B, H, W):
    g = torch.Generator().manual_seed(B + H + W)
    return [torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]


def centre_crop(H, W):
    side = min(H, W)
    return ((W - side) // 2, (H - side) // 2, side, side)


def host_way(x8, rect, flip, S0):
    """arm A's resize: crop, flip, F.interpolate in fp32, round to bytes"""
    x0, y0, w, h = rect
    x = x8[:, y0:y0 + h, x0:x0 + w, :]
    if flip:
        x = x.flip(2)
    y = F.interpolate(x.permute(0, 3, 1, 2).float(), size=(S0, S0), mode="bilinear", align_corners=False)
    return y.round().clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def arms(m, rect, S0):
    def a(l8, r8):
        return m.predict_pose_from_camera(host_way(l8, rect, False, S0), host_way(r8, rect, True, S0))

    def b(l8, r8):
        return m.predict_pose_from_sensor(l8, r8, crop=rect, mirror_right=True)
    return {"A": a, "B": b}


def nv12_frames(B, H, W):
    g = torch.Generator().manual_seed(B + H + W + 12)
    return [torch.randint(0, 256, (B, H * W * 3 // 2), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]


def torch_nv12_to_rgb(f8, H, W, matrix, offset):
    """arm A's conversion of tight NV12 frames: unpack, replicate the chroma, float matrix, round, clamp, to bytes -> uint8 [B, H, W, 3]"""
    B = f8.shape[0]
    y = f8[:, :H * W].view(B, H, W)
    uv = f8[:, H * W:].view(B, H // 2, W // 2, 2).repeat_interleave(2, 1).repeat_interleave(2, 2)
    yuv = torch.cat([y.unsqueeze(-1), uv], dim=-1).float() - offset
    return (yuv @ matrix.t()).round_().clamp_(0, 255).to(torch.uint8)


def yuv_arms(m, layout, colour, rect):
    cy, rv, gu, gv, bu, y_off = colour.real_coefficients()
    matrix = torch.tensor([[cy, 0.0, rv], [cy, -gu, -gv], [cy, bu, 0.0]], dtype=torch.float32, device="cuda")
    offset = torch.tensor([float(y_off), 128.0, 128.0], dtype=torch.float32, device="cuda")

    def convert(f8):
        return torch_nv12_to_rgb(f8, layout.H, layout.W, matrix, offset)

    def a(l8, r8):
        return m.predict_pose_from_sensor(convert(l8), convert(r8), crop=rect, mirror_right=True)

    def b(l8, r8):
        return m.predict_pose_from_sensor_yuv(l8, r8, layout, colour, crop=rect, mirror_right=True)
    return {"A": a, "B": b}, convert


def yuv_rows(m, args):
    colour = spec.YuvColour("bt601", "limited")
    rows = []
    for mode in ("bf16_frozen", "f32"):
        for src in args.sources.split(","):
            H, W = (int(v) for v in src.split("x"))
            layout, rect = spec.YuvLayout.nv12(H, W), centre_crop(H, W)
            for B in [int(b) for b in args.batches.split(",")]:
                l8, r8 = nv12_frames(B, H, W)
                configure(m, mode, B)
                f, convert = yuv_arms(m, layout, colour, rect)
                dbyte = int((spec.yuv_to_rgb_u8(r8[:1], layout, colour).to(torch.int16) - convert(r8[:1]).to(torch.int16)).abs().max())
                pa, pb = f["A"](l8, r8).clone(), f["B"](l8, r8).clone()
                torch.cuda.synchronize()
                dpose = float((pa - pb).abs().max())
                for name in f:                                           # warm-up (workspaces grown)
                    timed(f[name], l8, r8, 3)
                per = {name: [] for name in f}
                for _ in range(args.rounds):
                    for name in f:                                       # alternating: A, B, A, B, ...
                        per[name].append(timed(f[name], l8, r8, args.reps))
                row = {"mode": mode, "source": f"nv12 {H}x{W}", "rect": list(rect), "batch": B, "max_byte_diff_A_B": dbyte, "max_abs_pose_A_minus_B": dpose,
                       **{name: {"rounds_ms": [round(v, 4) for v in vs], "median_ms": round(statistics.median(vs), 4),
                                 "spread_ms": round(max(vs) - min(vs), 4)} for name, vs in per.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def fixture_calibration(k=0):
    """calibration k of tests/golden/ocam.npz (tools/make_golden_ocam.py) as a spec.OcamModel"""
    import numpy as np
    g = dict(np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ocam.npz")))
    return spec.ocam_from_json({"name": str(g[f"c{k}_name"]), "polynomialC2W": g[f"c{k}_pol"].tolist(), "polynomialW2C": g[f"c{k}_invpol"].tolist(),
                                "image_center": g[f"c{k}_image_center"].tolist(), "affine": g[f"c{k}_affine"].tolist(), "size": g[f"c{k}_size"].tolist(),
                                "imageCircleRadius": float(g[f"c{k}_radius"])})


def lens_maps_for(m, H, W, S0):
    import math
    cam, a = fixture_calibration(0), 0.02
    R = [[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]]
    return m.lens_maps(spec.lens_map(cam, cam, S0, R, frame_size=(H, W)), spec.lens_map(cam, cam, S0, R, frame_size=(H, W), mirror=True))


def kernel_ms(fn, reps):
    """median of `reps` event-timed calls of a standalone operator"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def lens_rows(m, args, S0):
    rows = []
    for src in args.sources.split(","):
        H, W = (int(v) for v in src.split("x"))
        maps = lens_maps_for(m, H, W, S0)
        share = float(maps.left.valid.mean() + maps.right.valid.mean()) / 2
        for mode in ("bf16_frozen", "f32"):
            for B in [int(b) for b in args.batches.split(",")]:
                l8, r8 = sensor_frames(B, H, W)
                configure(m, mode, B)
                f = {"A": lambda l, r: m.predict_pose_from_sensor(l, r, mirror_right=True), "B": lambda l, r: m.predict_pose_from_lens(l, r, maps)}
                for name in f:                                           # warm-up (workspaces grown)
                    timed(f[name], l8, r8, 3)
                per = {name: [] for name in f}
                for _ in range(args.rounds):
                    for name in f:                                       # alternating: sensor, lens, sensor, lens, ...
                        per[name].append(timed(f[name], l8, r8, args.reps))
                row = {"mode": mode, "source": f"{H}x{W}", "batch": B, "max_byte_diff_A_B": "n/a", "valid_share": round(share, 4),
                       **{name: {"rounds_ms": [round(v, 4) for v in vs], "median_ms": round(statistics.median(vs), 4),
                                 "spread_ms": round(max(vs) - min(vs), 4)} for name, vs in per.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
        B = 256
        import ctypes as C
        lib, out_l, out_r = L.load(), torch.empty((B, S0, S0, 3), dtype=torch.uint8, device="cuda"), torch.empty((B, S0, S0, 3), dtype=torch.uint8, device="cuda")
        full, colour, outs = (C.c_int * 4)(0, 0, W, H), spec.YuvColour("bt601", "limited"), (L.ptr(out_l), L.ptr(out_r))
        for fmt, layout in (("rgb8", None), ("nv12", spec.YuvLayout.nv12(H, W)), ("yuyv", spec.YuvLayout.yuyv(H, W))):
            if layout is None:
                l8, r8 = sensor_frames(B, H, W)
                resize = lambda: L.check(lib.egotap_rgb_u8_resize(L.ptr(l8), L.ptr(r8), B, H, W, full, full, 0, 1, S0, *outs, L.stream()))
            else:
                g = torch.Generator().manual_seed(B + H + W + len(fmt))
                l8, r8 = (torch.randint(0, 256, (B, layout.frame_stride), generator=g, dtype=torch.uint8).cuda() for _ in range(2))
                ysrc = L.yuv_source(layout, colour)
                resize = lambda: L.check(lib.egotap_yuv_u8_resize(L.ptr(l8), L.ptr(r8), B, C.byref(ysrc), full, full, 0, 1, S0, *outs, L.stream()))
            desc = L.lens_source(maps, layout, colour if layout else None)
            remap = lambda: L.check(lib.egotap_lens_remap(L.ptr(l8), L.ptr(r8), B, C.byref(desc), S0, *outs, L.stream()))
            # (the same count for every fetch: 12 source bytes per pixel that has a source, whatever the format stores them in)
            for name, fn, per_pixel in ((("rgb" if layout is None else "yuv") + "_u8_resize " + fmt, resize, 15.0), ("lens_remap " + fmt, remap, 12.0 * share + 11.0)):
                for _ in range(3):
                    fn()
                ms = [kernel_ms(fn, args.reps) for _ in range(args.rounds)]
                nbytes = 2.0 * B * S0 * S0 * per_pixel
                print(json.dumps({"kernel": name, "source": f"{H}x{W}", "batch": B, "S0": S0, "rounds_ms": [round(v, 4) for v in ms],
                                  "median_ms": round(statistics.median(ms), 4), "counted_bytes": nbytes,
                                  "TB_per_s": round(nbytes / (statistics.median(ms) * 1e-3) / 1e12, 3)}), flush=True)
    return rows


def timed(fn, l, r, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(l, r)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--sources", default="1024x1024,512x640")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="one call per arm at B = 64 from 1024 x 1024, and the operator alone (for a kernel trace)")
    ap.add_argument("--yuv", action="store_true", help="the NV12 arms: torch conversion + predict_pose_from_sensor against predict_pose_from_sensor_yuv")
    ap.add_argument("--lens", action="store_true", help="report only: predict_pose_from_sensor beside predict_pose_from_lens, and the two standalone kernels at B = 256")
    ap.add_argument("--json", default=None)
    ap.add_argument("--md", default=None, help="write the table as markdown (profiles/predict_sensor_summary.md)")
    args = ap.parse_args()
    m = build_model()
    S0 = 4 * m.net_AutoEncoder.preset.hm_size
    if args.once:
        l8, r8 = sensor_frames(64, 1024, 1024)
        for mode in ("bf16_frozen", "f32"):
            configure(m, mode, 64)
            f = arms(m, centre_crop(1024, 1024), S0)
            for name in ("A", "B", "A", "B"):
                f[name](l8, r8)
            torch.cuda.synchronize()
        for _ in range(3):
            L.rgb_u8_resize(l8, r8, S0, mirror_right=True)
        torch.cuda.synchronize()
        print("once: done")
        return
    rows = yuv_rows(m, args) if args.yuv else lens_rows(m, args, S0) if args.lens else []
    heads = (("A: torch conversion + predict_pose_from_sensor", "B: predict_pose_from_sensor_yuv") if args.yuv else
             ("A: predict_pose_from_sensor", "B: predict_pose_from_lens") if args.lens else ("A: today's caller", "B: predict_pose_from_sensor"))
    for mode in () if args.yuv or args.lens else ("bf16_frozen", "f32"):
        for src in args.sources.split(","):
            H, W = (int(v) for v in src.split("x"))
            rect = centre_crop(H, W)
            for B in [int(b) for b in args.batches.split(",")]:
                l8, r8 = sensor_frames(B, H, W)
                configure(m, mode, B)
                f = arms(m, rect, S0)
                ours = spec.resize_u8(r8, rect, True, S0)
                dbyte = int((ours.to(torch.int16) - host_way(r8, rect, True, S0).to(torch.int16)).abs().max())
                pa, pb = f["A"](l8, r8).clone(), f["B"](l8, r8).clone()
                torch.cuda.synchronize()
                dpose = float((pa - pb).abs().max())
                for name in f:                                           # warm-up (workspaces grown)
                    timed(f[name], l8, r8, 3)
                per = {name: [] for name in f}
                for _ in range(args.rounds):
                    for name in f:                                       # alternating: A, B, A, B, ...
                        per[name].append(timed(f[name], l8, r8, args.reps))
                row = {"mode": mode, "source": f"{H}x{W}", "rect": list(rect), "batch": B, "max_byte_diff_A_B": dbyte, "max_abs_pose_A_minus_B": dpose,
                       **{name: {"rounds_ms": [round(v, 4) for v in vs], "median_ms": round(statistics.median(vs), 4),
                                 "spread_ms": round(max(vs) - min(vs), 4)} for name, vs in per.items()}}
                rows.append(row)
                print(json.dumps(row), flush=True)
    for path, text in ((args.json, json.dumps(rows, indent=1)),
                       (args.md, f"| mode | source | B | {heads[0]}, ms (spread) | {heads[1]}, ms (spread) | max byte diff |\n|---|---|---|---|---|---|\n" +
                        "".join(f"| {r['mode']} | {r['source']} | {r['batch']} | {r['A']['median_ms']} ({r['A']['spread_ms']}) | {r['B']['median_ms']} ({r['B']['spread_ms']}) | "
                                f"{r['max_byte_diff_A_B']} |\n" for r in rows))):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as fh:
                fh.write(text)


if __name__ == "__main__":
    main()
