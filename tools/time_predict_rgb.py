"""Times stereo RGB -> pose serving: the parent's route against egotap_predict_pose_rgb, device events after warm-up, all arms in
ONE process and interleaved:

    python tools/time_predict_rgb.py [--batches 1,8,64,256] [--settings bf16_frozen,f32] [--json OUT]
    python tools/time_predict_rgb.py --only handoff --batches 64       # one arm, a few calls: the run to put under a kernel trace
    python tools/time_predict_rgb.py --arms no_heatmaps,keypoints,heatmaps_argmax        # some arms only
    python tools/time_predict_rgb.py --kernel                          # heatmap_peaks_kernel and limb_decode_kernel alone: duration and bytes per second
                                                                       # 

Arms (UnrealEgo, 64 x 64 heatmaps, resnet18 estimators, opt.hm_chunk 256):
  parent      chunked forward_into x 2 + net_AutoEncoder.predict_pose: three module calls per batch, the only serving route before this entry
  heatmaps    predict_pose_from_rgb(return_heatmaps=True): one library call, fp32 heatmaps written for the caller
  no_heatmaps predict_pose_from_rgb(): in bf16 the hand-off (conv_heatmap writes the head's bf16 operand), in fp32 the heatmaps stay in the workspace
  graphed     predict_pose_from_rgb(graphed=True): the same pipeline replayed from a captured graph (includes the copy into its static inputs)
  keypoints   predict_pose_from_rgb(return_keypoints=True): the 2D joints and confidences from the same call
  limbs       predict_pose_from_rgb(return_limbs=True): the limb elevation angles and 2D segments from the same call
  triangulation  predict_pose_from_rgb(return_triangulation=True): the keypoints triangulated through a stereo rig, one more launch behind the call
  tracking    the triangulation arm followed by PoseTracker.update on its pose, joints3d and frame: the B frames as B consecutive steps of one stream, one
              more launch behind the triangulation's (report only)
  tracking_world  the same with a world PoseTracker and the rig's pose per frame (a head that turns and walks; every pose counts): the launch of
              egotap_pose_track_world in the place of egotap_pose_track's (report only)
  skeleton    the tracking arm followed by Skeleton.update on its placed and tracks (the first call's first frame taken as the rest pose): one more launch
              behind the tracker's, egotap_skeleton_fit (report only)
  skeleton_twist  the same with a twist table on the skeleton (the preset's pole rows, a hinge at right angles to every pole row's rest bone, the default
              thresholds): the launch of egotap_skeleton_fit_twist in the place of egotap_skeleton_fit's (report only)
  fusion      the tracking arm with StereoFusion.update between the serving call and the tracker (return_keypoints=True as well; sigma_prior 0.05, the other
              defaults): one more launch in front of the tracker's, egotap_stereo_fuse (report only)
  overlay     predict_pose_from_rgb(return_heatmaps=True, return_keypoints=True) followed by Overlay.draw of the heatmaps, the skeleton's bones and the
              keypoints onto two uint8 [B, 256, 256, 3] canvases (out of place, into preallocated outputs): two more launches behind the call, egotap_heat_u8
              and egotap_overlay_u8 (report only -- the heatmaps arm plus the keypoints launch is what it adds to)
  heatmaps_argmax  what a caller did for them before: return_heatmaps=True, then torch amax / argmax on the device over the 2J position channels
Settings: "bf16_frozen" (set_precision("bf16") + freeze_weights) and "f32".  Every arm is warmed up, then timed in three alternating rounds;
per arm the median over all calls and the lowest / highest of the three round medians (the run-to-run spread) are printed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from egotap_amd import models, spec  # noqa: E402
from egotap_amd.options import preset_defaults  # noqa: E402
from egotap_amd.synthetic import synth_hm_state_dict, synth_input, synth_state_dict  # noqa: E402

REPS = {1: 60, 8: 40, 64: 12, 256: 6}       # calls per arm and round


def build_model():
    opt = preset_defaults("UnrealEgo", 64)
    opt.model, opt.isTrain, opt.use_amp, opt.gpu_ids, opt.use_gt_heatmap, opt.hm_chunk = "egotap_autoencoder", False, False, [0], False, 256
    m = models.create_model(opt)
    p = spec.lift_preset("UnrealEgo", 64)
    m.net_AutoEncoder.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(spec.lift_state_spec(p)).items()})
    m.net_HeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(15, "hm_pos.").items()})
    m.net_RotHeatMap.load_state_dict({k: torch.from_numpy(v) for k, v in synth_hm_state_dict(30, "hm_rot.").items()})
    m.eval()
    # a rig for the triangulation arm: the launch's time depends on the polynomials' lengths, not on their values (a 5-coefficient pol as OCamCalib
    # exports it, 16 invpol coefficients)
    cam = spec.OcamModel(name="unreal_ego_pose", pol=(-330.0, 0.0, 1.1e-3, -4.0e-7, 1.2e-9), invpol=(480.0,) + (1.0,) * 15, xc=512.0, yc=512.0)
    m.set_stereo_rig(cam, cam, (0.12, 0.0, 0.0))
    return m, p


def frames(B):
    out = []
    for eye in "lr":
        x = torch.from_numpy(synth_input(f"rgb_{eye}_time", (min(B, 4), 3, 256, 256), -2.0, 2.0)).cuda()
        out.append(x[torch.arange(B, device="cuda") % x.shape[0]].contiguous())
    return out


def arms_for(m, p, left, right):
    B = left.shape[0]
    chunk = min(B, int(m.opt.hm_chunk))
    cat = torch.empty((B, p.in_channels, p.hm_size, p.hm_size), device="cuda")

    def parent():
        for net, c0 in ((m.net_HeatMap, 0), (m.net_RotHeatMap, 2 * p.n_joints_hm)):
            ws = m.net_HeatMap._workspace(chunk, left.device)
            for lo in range(0, B, chunk):
                net.forward_into(left[lo:lo + chunk], right[lo:lo + chunk], cat[lo:lo + chunk], c0, workspace=ws)
        return m.net_AutoEncoder.predict_pose(cat)

    def heatmaps_argmax():
        pose, hm = m.predict_pose_from_rgb(left, right, return_heatmaps=True)
        flat = hm[:, :2 * p.n_joints_hm].flatten(2)
        flat.amax(dim=2), flat.argmax(dim=2)
        return pose

    tracker = m.new_pose_tracker(streams=1)

    def tracking():
        pose, joints3d, frame = m.predict_pose_from_rgb(left, right, return_triangulation=True)
        tracker.update(pose, joints3d, frame, dt=1.0 / 30)
        return pose

    world_tracker = m.new_pose_tracker(streams=1, world=True)
    t = torch.arange(B, dtype=torch.float64) / 30
    half = 0.5 * torch.sin(2 * torch.pi * 0.5 * t)                     # a yaw of up to a radian at 0.5 Hz, as a quaternion about y
    quat = torch.stack([torch.cos(half), torch.zeros_like(t), torch.sin(half), torch.zeros_like(t)], dim=1)
    rig_pose = torch.from_numpy(spec.rig_pose(torch.stack([0.3 * t, 1.6 + 0.0 * t, 0.1 * t], dim=1).numpy(), quat=quat.numpy())).cuda()

    def tracking_world():
        pose, joints3d, frame = m.predict_pose_from_rgb(left, right, return_triangulation=True)
        world_tracker.update(pose, joints3d, frame, dt=1.0 / 30, rig_pose=rig_pose)
        return pose

    fuse_tracker, fusion = m.new_pose_tracker(streams=1), m.new_stereo_fusion(0.05)

    def fusion_arm():
        pose, keypoints, joints3d, frame = m.predict_pose_from_rgb(left, right, return_keypoints=True, return_triangulation=True)
        pose_fused, _, _ = fusion.update(pose, keypoints, frame)
        fuse_tracker.update(pose_fused, joints3d, frame, dt=1.0 / 30)
        return pose

    overlay = m.new_overlay()
    g = torch.Generator().manual_seed(30)
    canvases = [torch.randint(0, 256, (B, 4 * p.hm_size, 4 * p.hm_size, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]
    drawn = [torch.empty_like(c) for c in canvases]

    def overlay_arm():
        pose, hm, keypoints = m.predict_pose_from_rgb(left, right, return_heatmaps=True, return_keypoints=True)
        overlay.draw(canvases[0], canvases[1], keypoints=keypoints, heatmaps=hm, out=drawn)
        return pose

    skel_tracker, skeleton = m.new_pose_tracker(streams=1), m.new_skeleton(streams=1)

    def skeleton_arm():
        pose, joints3d, frame = m.predict_pose_from_rgb(left, right, return_triangulation=True)
        placed, tracks = skel_tracker.update(pose, joints3d, frame, dt=1.0 / 30)
        if skeleton.rig is None:
            skeleton.set_rest_pose(placed[0] - placed[0, :1])      # (synchronises once, outside the timed rounds: the warm-up makes this call)
        skeleton.update(placed, tracks)
        return pose

    twist_tracker, twisted = m.new_pose_tracker(streams=1), []

    def skeleton_twist_arm():
        import numpy as np
        pose, joints3d, frame = m.predict_pose_from_rgb(left, right, return_triangulation=True)
        placed, tracks = twist_tracker.update(pose, joints3d, frame, dt=1.0 / 30)
        if not twisted:                                            # (synchronises once, outside the timed rounds, as the skeleton arm does)
            rig = spec.skeleton_rig_from_pose("UnrealEgo", placed[0] - placed[0, :1])
            hinge = np.zeros((rig.P, 3))
            for j in spec.SKELETON_POLE["UnrealEgo"]:              # any axis at right angles to the rest bone: the launch's time does not depend on it
                hinge[j] = np.cross(rig.rest_dir[j], np.eye(3)[int(np.argmin(np.abs(rig.rest_dir[j])))])
            twisted.append(m.new_skeleton(rig, streams=1, twist=spec.skeleton_twist(rig, spec.SKELETON_POLE["UnrealEgo"], hinge)))
        twisted[0].update(placed, tracks)
        return pose

    return {"parent": parent,
            "keypoints": lambda: m.predict_pose_from_rgb(left, right, return_keypoints=True)[0],
            "limbs": lambda: m.predict_pose_from_rgb(left, right, return_limbs=True)[0],
            "triangulation": lambda: m.predict_pose_from_rgb(left, right, return_triangulation=True)[0],
            "tracking": tracking,
            "tracking_world": tracking_world,
            "fusion": fusion_arm,
            "overlay": overlay_arm,
            "skeleton": skeleton_arm,
            "skeleton_twist": skeleton_twist_arm,
            "heatmaps_argmax": heatmaps_argmax,
            "heatmaps": lambda: m.predict_pose_from_rgb(left, right, return_heatmaps=True)[0],
            "no_heatmaps": lambda: m.predict_pose_from_rgb(left, right),
            "graphed": lambda: m.predict_pose_from_rgb(left, right, graphed=True)}


def measure(arms, per, warmup=10, rounds=3):
    """interleaved rounds; {arm: (median ms over all calls, lowest round median, highest round median)}"""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    rmed = {k: [] for k in arms}
    every = {k: [] for k in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(per)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            t = sorted(a.elapsed_time(b) for a, b in ev)
            rmed[name].append(t[len(t) // 2])
            every[name] += t
    return {k: (sorted(v)[len(v) // 2], min(rmed[k]), max(rmed[k])) for k, v in every.items()}


def time_kernel(batches, J=15, S=64, C_all=90):
    """heatmap_peaks_kernel on its own, as the serving entries launch it (the 2J position maps of [B, 6J, S, S], two groups): launches back to back
    between two device events, over enough distinct tensors that no launch finds its maps in the 256 MiB Infinity Cache; beside it the LayerNorm
    kernel (the project's HBM yardstick) over as many bytes, timed the same way.  Bytes are the maps read (plus, for LayerNorm, the rows written).
    limb_decode_kernel the same way over the 4J limb maps of the same tensors (c0 = 2J, J limbs, two eyes), and beside it heatmap_peaks_kernel over those
    same 4J maps: the same bytes through both kernels."""
    from egotap_amd import lib as L
    aff = [(4.0, 0.0, 4.0, 0.0)] * 2
    rows = []
    for B in batches:
        for dtype in (torch.float32, torch.bfloat16):
            esz = 4 if dtype == torch.float32 else 2
            copies = max(2, -(-(600 << 20) // (B * C_all * S * S * esz)))
            hms = [torch.randn((B, C_all, S, S), device="cuda").to(dtype) for _ in range(min(copies, 64))]
            reps = max(len(hms), 200 // len(hms) * len(hms))
            for name, maps, fn in (("heatmap_peaks", 2 * J, lambda t: L.heatmap_peaks(t, 0, 2 * J, groups=2, affine=aff)),
                                   ("limb_decode", 4 * J, lambda t: L.limb_decode(t, 2 * J, J, eyes=2, affine=aff)),
                                   ("heatmap_peaks_limb_maps", 4 * J, lambda t: L.heatmap_peaks(t, 2 * J, 4 * J, groups=2, affine=aff))):
                for t in hms:
                    fn(t)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(reps):
                    fn(hms[i % len(hms)])
                b.record()
                torch.cuda.synchronize()
                us = a.elapsed_time(b) * 1e3 / reps
                nbytes = B * maps * S * S * esz
                rows.append(dict(kernel=name, B=B, dtype=str(dtype), us=us, bytes=nbytes, TBps=nbytes / us / 1e6, tensors=len(hms)))
                print(f"{name:23s} B={B:<4d} {str(dtype):15s} {us:9.2f} us per launch   {nbytes / 1e6:8.2f} MB read   {nbytes / us / 1e6:6.3f} TB/s", flush=True)
            del hms
        n_rows = B * 2 * J * S * S // 1024
        xs = [torch.randn((n_rows, 1024), device="cuda") for _ in range(max(2, min(64, -(-(600 << 20) // (n_rows * 4096)))))]
        g, be = torch.ones(1024, device="cuda"), torch.zeros(1024, device="cuda")
        reps = max(len(xs), 200 // len(xs) * len(xs))
        for x in xs:
            L.layernorm(x, g, be)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(reps):
            L.layernorm(xs[i % len(xs)], g, be)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / reps
        nbytes = 2 * n_rows * 4096
        rows.append(dict(kernel="layernorm_f32", B=B, us=us, bytes=nbytes, TBps=nbytes / us / 1e6, tensors=len(xs)))
        print(f"layernorm_f32 rows={n_rows:<7d} (the bytes of B={B})  {us:9.2f} us per launch (incl. its output allocation)   {nbytes / 1e6:8.2f} MB read + written   "
              f"{nbytes / us / 1e6:6.3f} TB/s", flush=True)
        del xs
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64,256")
    ap.add_argument("--settings", default="bf16_frozen,f32")
    ap.add_argument("--only", default=None, help="run this arm alone, --calls times, untimed (for a kernel trace)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--arms", default=None, help="comma-separated arms to time (default: all); parent is always run once, as the pose every arm must equal")
    ap.add_argument("--kernel", action="store_true", help="time heatmap_peaks_kernel and limb_decode_kernel alone (and the LayerNorm kernel over as many bytes), nothing else")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.kernel:
        res = {"device": torch.cuda.get_device_name(0), "kernel_rows": time_kernel([int(b) for b in a.batches.split(",")])}
        print(json.dumps(res))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)
        return
    m, p = build_model()
    res = {"device": torch.cuda.get_device_name(0), "rows": []}
    for setting in a.settings.split(","):
        for B in (int(b) for b in a.batches.split(",")):
            m.unfreeze_weights()
            m.set_precision("bf16" if setting == "bf16_frozen" else "f32")
            if setting == "bf16_frozen":
                skipped = m.freeze_weights(batch=min(B, int(m.opt.hm_chunk)))
                assert skipped == {}, skipped
            left, right = frames(B)
            arms = arms_for(m, p, left, right)
            ref = arms["parent"]().clone()
            if a.arms:
                arms = {k: arms[k] for k in a.arms.split(",")}
            for k, fn in arms.items():                       # every arm computes the parent's pose, bit for bit
                got = fn()
                torch.cuda.synchronize()
                assert torch.equal(got, ref), (setting, B, k)
            m.predict_pose_from_rgb(left, right)
            form = m.rgb_form()
            if a.only:
                for _ in range(a.calls):
                    arms[a.only]()
                torch.cuda.synchronize()
                print(f"{setting} B={B} arm {a.only}: {a.calls} calls done (no_heatmaps form: {form})", flush=True)
                continue
            r = measure(arms, REPS.get(B, 6))
            for k, (med, lo, hi) in r.items():
                note = f"({form})" if k in ("no_heatmaps", "graphed", "keypoints", "limbs", "triangulation", "tracking", "tracking_world", "fusion", "overlay", "skeleton", "skeleton_twist") else ""
                print(f"{setting:12s} B={B:<4d} {k:14s} median {med:9.3f} ms   round medians {lo:9.3f} .. {hi:9.3f} {note}", flush=True)
                res["rows"].append(dict(setting=setting, B=B, arm=k, median_ms=med, round_lo_ms=lo, round_hi_ms=hi, form=form))
            m._rgb["graphs"].clear()
            del arms, left, right
            torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
