"""A camera rig per stream on the device: egotap_stereo_triangulate_streams, egotap_stereo_fuse_streams (a table of S rigs in device memory, frame b
served by rig b % S), egotap_lens_remap_streams and the lens one-call entries with a map per stream, the model's set_stereo_rigs / update_stereo_rig.

The expected values are the single-rig entries on rows s, s + S, .. with rig (or map) s: both paths run the same device functions -- float64 without
contraction for the stereo operators, integers for the gather -- and where a value of the rig was loaded from does not enter the arithmetic, so the
gate is EQUAL IN BITS.  Against the float64 restatements (spec.stereo_triangulate_streams_ref, spec.stereo_fuse_streams_ref) the gates are the single-rig
tests' 2 fp32 ulp (test_gpu_stereo_triangulate.py, test_gpu_stereo_fuse.py: only divisions, square roots and atan may differ in the last float64
bit), through their own comparison functions; the gather equals spec.lens_remap_streams_u8 in every byte."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import ocam_inputs as I
import test_gpu_lens_remap as TLR
import test_gpu_stereo_fuse as TF
import test_gpu_stereo_triangulate as TT
import yuv_cases as Y_
from egotap_amd import lib as L
from egotap_amd import models
from egotap_amd import spec
from gpu_util import serving_model as _model, timed_launches as _launches

pytestmark = pytest.mark.gpu
THAT = np.array([0.25, -0.5, 0.75])
PRM = spec.FuseParams(sigma_prior=0.05)
# per stream: (cameras, a rotated R, the rig's size against tests/ocam_inputs.py's -- t = scale * I.T, the points scale with it and the pixels stay --,
# min_score).  Another pol / invpol (fisheye against pinhole), another t, a rotated R, another affine (the fisheye cases'), ue_flip on and off.
STREAMS = [("fisheye_ue", True, 1.0, 0.5), ("fisheye_cv", False, 1.5, 0.5), ("pinhole", False, 2.0, 0.25), ("pinhole", True, 1.0, 0.5), ("fisheye_ue", False, 0.75, 0.45)]


def _bits(got, want):
    TF._bits(got, want)


def _project(model, rot, X):
    """points in the left camera's frame (unit rig) -> the keypoints of both eyes as the case builders of tests/ocam_inputs.py make them"""
    Rm = I.SMALL_R if rot else np.eye(3)
    if model == "pinhole":
        return I.pinhole_pixels(X[0]), I.pinhole_pixels((X[1] - I.T) @ Rm)
    left, right = I.rig_models(model == "fisheye_ue")
    affine = np.array([[4.0, 3.0, 4.0, -2.0], [5.0, 0.0, 3.75, 1.5]])          # fisheye_case's
    out = []
    for e, p in enumerate((spec.ocam_world2cam_ref(X[0], left), spec.ocam_world2cam_ref((X[1] - I.T) @ Rm, right))):
        out.append(np.array([(p[0] - affine[e, 1]) / affine[e, 0], (p[1] - affine[e, 3]) / affine[e, 2]]))
    return out


@functools.lru_cache(maxsize=None)
def _stream_case(s, T, J, P):
    """stream s's rig and T frames of it: (spec.StereoRig, keypoints [T, 2, J, 4], pose [T, P, 3]); computed once, never written.  Joint 1 of frame 0
    is made a FALLBACK of the fusion: its two rays pass 2.7 gate-sigmas off the prior on opposite sides, so each eye alone passes the gate and the fit,
    which stays near the prior, is further than max_sigma ray-sigmas from both."""
    model, rot, scale, ms = STREAMS[s]
    R = I.SMALL_R if rot else None
    if model == "pinhole":
        kp64, X, _ = I.pinhole_case(T, J, seed=300 + 7 * s + J, R=R)
        left, right, affine = I.pinhole(), I.pinhole(), None
    else:
        kp64, affine, X, _ = I.fisheye_case(T, J, seed=400 + 7 * s + J, R=R, ue=model == "fisheye_ue")
        left, right = I.rig_models(model == "fisheye_ue")
        assert np.array_equal(affine, [[4.0, 3.0, 4.0, -2.0], [5.0, 0.0, 3.75, 1.5]])
    rng = np.random.default_rng(1000 + 10 * s + J)
    row0 = P - J
    noise = rng.normal(0, 0.03, X.shape)
    noise[0, 1] = 0.0
    pose = np.full((T, P, 3), 1e6, dtype=np.float32)
    pose[:, row0:] = (scale * (X + noise) - THAT).astype(np.float32)
    x = X[0, 1]
    sr = PRM.sigma_ray * scale * np.linalg.norm(x)
    d = 2.7 * np.sqrt(sr * sr + PRM.sigma_prior ** 2) / scale
    off = np.array([0.0, d, 0.0])
    pl, pr = _project(model, rot, (x + off, x - off))
    kp64[0, 0, 1, :2], kp64[0, 1, 1, :2] = pl, pr
    rig = spec.StereoRig(left, right, I.T * scale, R=R, affine=affine, min_score=ms)
    kp = np.ascontiguousarray(kp64.astype(np.float32))
    kp.setflags(write=False)
    pose.setflags(write=False)
    return rig, kp, pose


@functools.lru_cache(maxsize=None)
def _batch(S, T, J, P):
    """(rigs, keypoints [T * S, 2, J, 4], pose [T * S, P, 3]) time-major: frame b = t * S + s is frame t of stream s"""
    cases = [_stream_case(s, T, J, P) for s in range(S)]
    kp, pose = np.empty((T * S, 2, J, 4), dtype=np.float32), np.empty((T * S, P, 3), dtype=np.float32)
    for s, (_, k, p) in enumerate(cases):
        kp[s::S], pose[s::S] = k, p
    kp.setflags(write=False)
    pose.setflags(write=False)
    return [c[0] for c in cases], kp, pose


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _single(rig):
    return dict(left=rig.left, right=rig.right, t=rig.t, R=rig.R, affine=rig.affine, min_score=rig.min_score)


# ------------------------------------------------------------------------------------------------------------ 1. triangulate
def _triangulate_streams(table, S, dkp, dpose, P, row0):
    B, _, J, _ = dkp.shape
    _, out3, ok3 = TT._between_canaries(B * J * 8)
    _, outf, okf = TT._between_canaries(B * 8)
    L.check(L.load().egotap_stereo_triangulate_streams(L.ptr(dkp), B, J, L.ptr(table), S, L.ptr(dpose), P if dpose is not None else 0, row0, L.ptr(out3), L.ptr(outf),
                                                       L.stream()))
    torch.cuda.synchronize()
    assert ok3() and okf(), "a canary moved"
    return out3.view(B, J, 8), outf.view(B, 8)


@pytest.mark.parametrize("S,T", [(3, 3), (5, 1), (1, 9)], ids=["S3_T3", "S5_T1", "S1_T9"])
@pytest.mark.parametrize("J", [15, 17])
def test_triangulate_streams_equals_the_single_rig_entry_per_stream_in_bits(J, S, T):
    """B = 9 is no multiple of the four frames of a workgroup: the last workgroup is ragged and its waves still pick a row inside the table"""
    P = J + 1 if J == 15 else J
    row0 = P - J
    rigs, kp, pose = _batch(S, T, J, P)          # (S = 1: the single entry on the whole batch)
    table, host = L.stereo_rigs_table(rigs)
    assert table.dtype == torch.uint8 and table.numel() == S * 792 and table.data_ptr() % 8 == 0 and len(host) == S
    dkp, dpose = _dev(kp), _dev(pose)
    table0 = table.clone()
    for ps, dps in ((None, None), (pose, dpose)):
        got3, gotf = _triangulate_streams(table, S, dkp, dps, P, row0)
        for s, rig in enumerate(rigs):
            w3, wf = L.stereo_triangulate(dkp[s::S], pose=None if dps is None else dps[s::S], pose_row0=row0, **_single(rig))
            _bits(got3[s::S], w3)
            _bits(gotf[s::S], wf)
            assert bool((wf[:, 3] >= 4).all()), (s, wf[:, 3].tolist())          # every stream triangulates
        ref3, reff = spec.stereo_triangulate_streams_ref(kp, rigs, pose=ps, pose_row0=row0)
        TT._compare(got3, gotf, ref3, reff, f"S={S} T={T} J={J} pose={'no' if ps is None else 'yes'}")
        f3, ff = L.stereo_triangulate_streams(dkp, table, S, pose=dps, pose_row0=row0)          # the Python face: the same launch
        _bits(f3, got3)
        _bits(ff, gotf)
    if S > 1:           # the streams do differ: one rig for all frames gives other records
        o3, _ = L.stereo_triangulate(dkp, pose=dpose, pose_row0=row0, **_single(rigs[0]))
        assert not torch.equal(o3[1::S], got3[1::S])
    _bits(dkp, kp), _bits(dpose, pose)                  # the inputs and the table are read only
    assert torch.equal(table, table0)


# ------------------------------------------------------------------------------------------------------------ 2. fuse
def _fuse_streams(table, S, dkp, dpose, row0, dframe, inplace=False):
    B, _, J, _ = dkp.shape
    P = dpose.shape[1]
    fused, ok_f = TF._between_canaries(B * J * 8)
    stats, ok_s = TF._between_canaries(B * 8)
    pf, ok_p = TF._between_canaries(B * P * 3)
    if inplace:
        pf.copy_(dpose.reshape(-1))
    src = pf if inplace else dpose
    L.check(L.load().egotap_stereo_fuse_streams(L.ptr(dkp), B, J, L.ptr(table), S, L.ptr(src), P, row0, L.ptr(dframe), C.byref(L.fuse_params_struct(PRM)),
                                                L.ptr(fused), L.ptr(pf), L.ptr(stats), L.stream()))
    torch.cuda.synchronize()
    assert ok_f() and ok_p() and ok_s(), "a canary moved"
    return pf.view(B, P, 3), fused.view(B, J, 8), stats.view(B, 8)


@pytest.mark.parametrize("S,T", [(3, 3), (5, 1), (1, 9)], ids=["S3_T3", "S5_T1", "S1_T9"])
@pytest.mark.parametrize("J", [15, 17])
def test_fuse_streams_equals_the_single_rig_entry_per_stream_in_bits(J, S, T):
    P = J + 1 if J == 15 else J
    row0 = P - J
    rigs, kp, pose = _batch(S, T, J, P)
    B = kp.shape[0]
    frame = np.zeros((B, 8), dtype=np.float32)
    frame[:, :3], frame[:, 3] = THAT, 4 + np.arange(B)
    frame[:, 4:] = np.random.default_rng(J).normal(0, 1, (B, 4))          # the rest of the record is not read
    # on the host, before the launch: every stream has a kept fit of both eyes, a kept fit of one eye and a fallback
    ref = spec.stereo_fuse_streams_ref(kp, pose, frame, rigs, PRM, pose_row0=row0)
    mode = ref[1][..., 7].astype(int)
    for s in range(S):
        m = mode[s::S]
        kept = ((m & 6) != 0) & ((m & 128) == 0)
        assert (kept & ((m & 6) == 6)).any() and (kept & ((m & 6) != 6)).any() and ((m & 128) != 0).any(), (s, sorted(set(m.ravel().tolist())))
        assert mode[s, 1] & 128, (s, mode[s, 1])                          # the constructed joint is the fallback
    table, _ = L.stereo_rigs_table(rigs)
    dkp, dpose, dframe = _dev(kp), _dev(pose), _dev(frame)
    got = _fuse_streams(table, S, dkp, dpose, row0, dframe)
    for s, rig in enumerate(rigs):
        want = L.stereo_fuse(dkp[s::S], dpose[s::S], dframe[s::S], params=PRM, pose_row0=row0, **_single(rig))
        for a, b in zip(got, want):
            _bits(a[s::S], b)
    TF._compare(f"S={S} T={T} J={J}", got, ref, pose, row0)
    for a, b in zip(_fuse_streams(table, S, dkp, dpose, row0, dframe, inplace=True), got):          # pose_fused == pose gives the bits of out of place
        _bits(a, b)
    for a, b in zip(L.stereo_fuse_streams(dkp, dpose, dframe, table, S, PRM, pose_row0=row0), got):      # the Python face: the same launch
        _bits(a, b)
    _bits(dkp, kp), _bits(dpose, pose), _bits(dframe, frame)


# ------------------------------------------------------------------------------------------------------------ 3. lens remap
def _stream_maps(H, W, S0, S):
    """S pairs of maps from S different sensor models (the helper lenses of test_gpu_lens_remap.py): another focal length, another centre per stream; the
    left eye rotated, the right one mirrored"""
    model = TLR._helper(20.0, 31.25, 23.75, (48, 64))
    a = 0.4
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    pairs = []
    for s in range(S):
        f2 = 40.0 - 6.0 * s
        left = spec.lens_map(model, TLR._helper(f2, W - 1.5 - 0.5 * f2 - 2 * s, H - 1.25 - 0.5 * f2, (H, W)), S0, R=R)
        right = spec.lens_map(model, TLR._helper(f2 + 3.0, 0.45 * f2 + s, 0.55 * f2, (H, W)), S0, mirror=True)
        assert all(0.05 < m.valid.mean() < 0.95 for m in (left, right)), (s, left.valid.mean(), right.valid.mean())
        pairs.append((left, right))
    assert len({m.taps.tobytes() for pair in pairs for m in pair}) == 2 * S
    return pairs


def _remap_streams_between_canaries(l8, r8, B, maps, layout=None, colour=None):
    S0 = maps.S0
    n, pad, canary = B * S0 * S0 * 3, 1024, 0xA5
    flat = torch.full((2 * (n + pad) + pad,), canary, dtype=torch.uint8, device="cuda")
    out_l, out_r = flat[pad:pad + n], flat[2 * pad + n:2 * pad + 2 * n]
    L.check(L.load().egotap_lens_remap_streams(L.ptr(l8), L.ptr(r8), B, C.byref(L.lens_source(maps, layout, colour)), maps.S, S0, L.ptr(out_l), L.ptr(out_r),
                                               L.stream()))
    torch.cuda.synchronize()
    for lo, hi in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, flat.numel())):
        assert bool((flat[lo:hi] == canary).all()), (lo, hi)
    return out_l.view(B, S0, S0, 3), out_r.view(B, S0, S0, 3)


@pytest.mark.parametrize("fmt", ["rgb8", "nv12", "yuyv"])
def test_lens_remap_streams_equals_the_restatement_and_the_single_map_entry_per_stream(fmt):
    S, B, S0 = 3, 6, 8
    H, W = (37, 53) if fmt == "rgb8" else (38, 54)                    # the two YUV layouts need even sides
    pairs = _stream_maps(H, W, S0, S)
    fill = ((9, 200, 31), (255, 0, 128))
    maps = L.lens_maps(pairs, fill=fill)
    assert maps.S == S and tuple(maps.map_left.shape) == (S, S0 * S0, 2) and maps.map_left.data_ptr() % 16 == 0
    if fmt == "rgb8":
        layout = colour = None
        lh, rh = TLR._rgb(41, B, H, W), TLR._rgb(42, B, H, W)
        l8, r8 = TLR._odd(lh), TLR._odd(rh)
        rgb_l, rgb_r = lh, rh
    else:
        layout, colour = TLR._yuv_layout(fmt, H, W, 64 if fmt == "nv12" else 128), Y_.COLOURS[0]
        assert bool(Y_.padding_mask(layout).any())                       # a padded pitch
        lh, rh = Y_.frames(43, B, layout, TLR.POISON), Y_.frames(44, B, layout, TLR.POISON)
        l8, r8 = TLR._at_minimum_alignment(lh, layout), TLR._at_minimum_alignment(rh, layout)
        rgb_l, rgb_r = spec.yuv_to_rgb_u8(lh, layout, colour), spec.yuv_to_rgb_u8(rh, layout, colour)
    got = _remap_streams_between_canaries(l8, r8, B, maps, layout, colour)
    for e, (g, rgb) in enumerate(zip(got, (rgb_l, rgb_r))):
        want = spec.lens_remap_streams_u8(rgb, [pair[e] for pair in pairs], fill[e])
        assert torch.equal(g.cpu(), want), (fmt, e, int((g.cpu() != want).sum()))
    for s, pair in enumerate(pairs):                                     # rows s, s + S: the single-map entry with map s
        one = L.lens_maps(*pair, fill=fill)
        w_l, w_r = L.lens_remap(l8[s::S].contiguous(), r8[s::S].contiguous(), one, S0, layout, colour)
        assert torch.equal(got[0][s::S], w_l) and torch.equal(got[1][s::S], w_r), (fmt, s)
    assert not torch.equal(got[0][1::S], L.lens_remap(l8[1::S].contiguous(), r8[1::S].contiguous(), L.lens_maps(*pairs[0], fill=fill), S0, layout, colour)[0])
    for a, b in zip(L.lens_remap_streams(l8, r8, maps, S0, layout, colour), got):      # the Python face: the same launch
        assert torch.equal(a, b)
    # S = 1: the entry without _streams on the whole batch, in every byte
    one = L.lens_maps([pairs[1]], fill=fill)
    assert one.S == 1
    w = L.lens_remap(l8, r8, L.lens_maps(*pairs[1], fill=fill), S0, layout, colour)
    for a, b in zip(_remap_streams_between_canaries(l8, r8, B, one, layout, colour), w):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="lens_remap_streams gathers"):
        L.lens_remap(l8, r8, maps, S0, layout, colour)
    with pytest.raises(ValueError, match="multiple of the number of streams"):
        L.lens_remap_streams(l8[:4], r8[:4], maps, S0, layout, colour)


# ------------------------------------------------------------------------------------------------------------ 4. serving
HM = 32                                                               # the smallest side of test_gpu_lens_remap.py's one-call tests


def _serving_rigs():
    """two rigs of the model cameras: the UE pair rotated, and the same cameras half as far apart again"""
    left, right = I.rig_models(True)
    return [(left, right, I.T, I.SMALL_R), (left, right, I.T * 1.5, I.SMALL_R)]


def _clear(m, dev):
    m._rgb_state(dev).graphs.clear()
    m.__dict__.pop("_stereo_rigs", None)
    m.__dict__.pop("_stereo_rig", None)


def test_one_call_with_a_map_per_stream_in_pieces_that_start_on_an_odd_frame():
    """S = 2, B = 4, hm_chunk = 3: the second piece starts at frame 3, stream 1.  Every output equals, in bits, the camera entry on the frames
    lib.lens_remap_streams gathers, at the same B and chunk, followed by lib.stereo_triangulate_streams; graphed equals eager."""
    m, p = _model("UnrealEgo", HM)
    S, B, S0 = 2, 4, 4 * HM
    dev = torch.device("cuda", torch.cuda.current_device())
    cam, sensor = I.rig_models(True)
    pairs = []
    for Rl, Rr in ((I.SMALL_R, I.SMALL_R.T), (None, I.SMALL_R @ I.SMALL_R)):      # stream 1's headset is mounted at other angles
        left, right = (spec.lens_map(cam, sensor, S0, R, frame_size=(96, 80)) for R in (Rl, Rr))
        pairs.append(tuple(dataclasses.replace(x, model_size=(S0, S0)) for x in (left, right)))      # the camera entry's keypoint affine (test_gpu_lens_remap.py)
    assert len({x.taps.tobytes() for pair in pairs for x in pair}) == 4 and all(x.valid.mean() > 0.5 for pair in pairs for x in pair)
    maps = m.lens_maps(pairs, fill=((0, 0, 0), (90, 100, 110)))
    assert maps.S == S
    lh, rh = TLR._rgb(51, B, 96, 80), TLR._rgb(52, B, 96, 80)
    l8, r8 = lh.cuda(), rh.cuda()
    every = dict(return_heatmaps=True, return_keypoints=True, return_limbs=True)
    try:
        _clear(m, dev)
        m.opt.hm_chunk = 3
        cam_l, cam_r = L.lens_remap_streams(l8, r8, maps, S0)
        assert torch.equal(cam_l.cpu(), spec.lens_remap_streams_u8(lh, [pr[0] for pr in pairs], maps.fill[0]))
        want = TLR._clones(m.predict_pose_from_camera(cam_l, cam_r, **every))
        m.set_stereo_rigs(_serving_rigs(), min_score=0.0)
        rigs = [spec.StereoRig(l, r, t, R, spec.STEREO_IDENTITY_AFFINE, 0.0) for l, r, t, R in _serving_rigs()]      # the lens entries' keypoints are calibration pixels
        table, _ = L.stereo_rigs_table(rigs)
        w3, wf = L.stereo_triangulate_streams(want[2], table, S, pose=want[0], pose_row0=spec.stereo_pose_row0(p))
        for graphed in (False, True):
            got = m.predict_pose_from_lens(l8, r8, maps, graphed=graphed, return_triangulation=True, **every)
            torch.cuda.synchronize()
            assert len(got) == 6
            for name, a, b in zip(("pose", "heatmaps", "keypoints", "limbs", "joints3d", "frame"), got, want + (w3, wf)):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (graphed, name, float((a - b).abs().max()))
        assert all(bool((wf[s::S, 3] > 0).any()) for s in range(S)) and not torch.equal(w3[0::S], w3[1::S])          # both streams triangulate, each through its rig
        graphs = m._rgb_state(dev).graphs
        assert len(graphs) == 1 and sum("lens_streams" in k for k in graphs) == 1
        # the frames of stream 1 through stream 0's maps are other frames: the piece that starts on frame 3 did read map 1
        plain = m.lens_maps(*pairs[0], fill=maps.fill)
        assert not torch.equal(L.lens_remap(l8[3:], r8[3:], plain, S0)[0], cam_l[3:])
        launches = _launches(m, lambda: m.predict_pose_from_lens(l8, r8, maps, return_triangulation=True, **every))
        assert [x for x in launches if "lens" in x[0] or "resize" in x[0]] == [("lens_remap_streams", "lens_remap_streams_kernel", 2)], launches
        assert [x for x in launches if "stereo" in x[0]] == [("stereo_triangulate_streams", "stereo_triangulate_streams_kernel", 1)], launches
        with pytest.raises(ValueError, match="multiple of the maps' 2 streams"):
            m.predict_pose_from_lens(l8[:3], r8[:3], maps)
    finally:
        _clear(m, dev)


def test_update_stereo_rig_is_served_by_the_next_replay_without_a_new_graph():
    m, p = _model("UnrealEgo", HM)
    S, B, S0 = 2, 4, 4 * HM
    dev = torch.device("cuda", torch.cuda.current_device())
    row0 = spec.stereo_pose_row0(p)
    l8, r8 = TT._bytes8(61, (B, S0, S0, 3))
    try:
        _clear(m, dev)
        with pytest.raises(L.EgotapError, match="call set_stereo_rigs"):
            m.update_stereo_rig(0, *_serving_rigs()[0])
        m.set_stereo_rigs(_serving_rigs(), min_score=TT.MIN_SCORE)
        with pytest.raises(ValueError, match="multiple of the 2 streams"):
            m.predict_pose_from_camera(l8[:3], r8[:3], return_triangulation=True)
        flags = dict(return_keypoints=True, return_triangulation=True, graphed=True)
        pose, kp, j3, fr = TLR._clones(m.predict_pose_from_camera(l8, r8, **flags))
        graphs = m._rgb_state(dev).graphs
        assert len(graphs) == 1

        def single(rig, s):
            left, right, t, R = rig
            affine = (spec.stereo_pixel_affine(left, p.hm_size), spec.stereo_pixel_affine(right, p.hm_size))
            return L.stereo_triangulate(kp[s::S], left, right, t, R=R, affine=affine, min_score=TT.MIN_SCORE, pose=pose[s::S], pose_row0=row0)
        for s, rig in enumerate(_serving_rigs()):
            w3, wf = single(rig, s)
            _bits(j3[s::S], w3), _bits(fr[s::S], wf)
        left, right = I.rig_models(False)
        new = (left, right, I.T * 0.5, I.SMALL_R.T)                      # a headset recalibrated: other cameras, baseline and rotation
        m.update_stereo_rig(1, *new)
        pose2, kp2, j32, fr2 = m.predict_pose_from_camera(l8, r8, **flags)
        torch.cuda.synchronize()
        assert len(graphs) == 1                                          # replayed, not recaptured
        assert torch.equal(pose2, pose) and torch.equal(kp2, kp)
        w3, wf = single(new, 1)
        _bits(j32[1::S], w3), _bits(fr2[1::S], wf)
        assert not torch.equal(j32[1::S], j3[1::S])
        _bits(j32[0::S], j3[0::S]), _bits(fr2[0::S], fr[0::S])            # stream 0 keeps its bits
        e3, ef = m.predict_pose_from_camera(l8, r8, return_triangulation=True)[1:]      # eager reads the same table
        _bits(e3, j32), _bits(ef, fr2)
        with pytest.raises(L.EgotapError, match="rig 1: t must be finite"):
            m.update_stereo_rig(1, left, right, (0.0, float("nan"), 0.0))
        with pytest.raises(ValueError, match="stream 2 is not one of the 2"):
            m.update_stereo_rig(2, *new)
        # a fusion made from the rigs reads the same table: it serves the updated rig
        prm = spec.FuseParams(sigma_prior=0.5, max_sigma=float("inf"), min_joints=0)
        fusion = m.new_stereo_fusion(0.5, params=prm)
        assert isinstance(fusion, models.StreamStereoFusion) and fusion.streams == S
        got = fusion.update(pose2, kp2, fr2)
        for s, rig in enumerate((_serving_rigs()[0], new)):
            l_, r_, t_, R_ = rig
            affine = (spec.stereo_pixel_affine(l_, p.hm_size), spec.stereo_pixel_affine(r_, p.hm_size))
            want = L.stereo_fuse(kp2[s::S], pose2[s::S], fr2[s::S], l_, r_, t_, prm, R=R_, affine=affine, min_score=TT.MIN_SCORE, pose_row0=row0)
            for a, b in zip(got, want):
                _bits(a[s::S], b)
        # the later of the two calls wins
        m.set_stereo_rig(*_serving_rigs()[0][:3], R=I.SMALL_R, min_score=TT.MIN_SCORE)
        assert isinstance(m.new_stereo_fusion(0.5, params=prm), models.StereoFusion)
        one3, _ = m.predict_pose_from_camera(l8, r8, return_triangulation=True)[1:]
        _bits(one3[0::S], j32[0::S])
        assert not torch.equal(one3[1::S], j32[1::S])
    finally:
        _clear(m, dev)


# ------------------------------------------------------------------------------------------------------------ 5. the chain in front of the tracker
def test_triangulate_fuse_track_per_stream_equals_the_single_rig_chain():
    S, T, J, P = 2, 3, 15, 16
    row0 = P - J
    rigs, kp, pose = _batch(S, T, J, P)
    table, _ = L.stereo_rigs_table(rigs)
    dkp, dpose = _dev(kp), _dev(pose)
    tprm = spec.TrackParams(min_joints=1, max_hold=2)
    j3, fr = L.stereo_triangulate_streams(dkp, table, S, pose=dpose, pose_row0=row0)
    pf, fu, st = L.stereo_fuse_streams(dkp, dpose, fr, table, S, PRM, pose_row0=row0)
    placed, tracks = models.PoseTracker(P, J, streams=S, params=tprm).update(pf, j3, fr, dt=1.0 / 30)
    torch.cuda.synchronize()
    assert bool((st[:, 1] > 0).all()) and not torch.equal(pf, dpose)          # fits were kept in every frame
    for s, rig in enumerate(rigs):
        a = _single(rig)
        w3, wf = L.stereo_triangulate(dkp[s::S], pose=dpose[s::S], pose_row0=row0, **a)
        wpf, wfu, wst = L.stereo_fuse(dkp[s::S], dpose[s::S], wf, params=PRM, pose_row0=row0, **a)
        wplaced, wtracks = models.PoseTracker(P, J, streams=1, params=tprm).update(wpf, w3, wf, dt=1.0 / 30)
        torch.cuda.synchronize()
        for got, want in ((j3, w3), (fr, wf), (pf, wpf), (fu, wfu), (st, wst), (placed, wplaced), (tracks, wtracks)):
            _bits(got[s::S], want)
