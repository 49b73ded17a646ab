"""The bone twist on the device: egotap_skeleton_fit_twist (skeleton_fit.h, skeleton_fit_kernel<true>), lib.skeleton_fit_twist and a Skeleton with a
twist table.

The expected values are the float64 restatement spec.skeleton_fit_twist_ref on the inputs of tests/test_gpu_skeleton_fit.py (accepted, NaN, status-0,
outlier and zero-length samples from a state under way) with a twist table whose thresholds put the bends of those inputs below bend_lo, inside the ramp
and above bend_hi (tests/skeleton_twist_inputs.py; tests/test_skeleton_twist_cpu.py asserts that every branch is met and that no observed twist is near
the half turn).  Device and host run the same float64 operations in the same order, so the bounds are those of tests/test_gpu_skeleton_fit.py:
  * equal in bits: the flags (1 + 2 + 4), the all-zero records, the identity records and n;
  * rigid within 2 fp32 ulp of the frame's largest |coordinate|; quaternion components within 2 fp32 ulp of 1; lengths within 2 ulp of itself; the
    float64 state within 1e-13 max(1, |value|).
Measured on the MI355X: see MEASURED below."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ocam_inputs as OI
import pose_track_world_inputs as W
import skeleton_inputs as I
import skeleton_twist_inputs as TI
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model
from test_gpu_skeleton_fit import CANARY, _between_canaries, _bits, _compare, _dev
from test_skeleton_twist_cpu import half_turn_case

pytestmark = pytest.mark.gpu
# MEASURED (one run of this file on one MI355X): every output and every state value of all 24 cases below, and of the serving case behind both
# trackers, came out EQUAL IN BITS to the restatement (largest deviation / bound 0.0 for rigid, rotations, lengths and the state).
SHAPES = [(1, 1, "UnrealEgo"), (7, 1, "UnrealEgo"), (3, 6, "EgoCap"), (2, 4, "chain64"), (2, 4, "star64"), (1, 9, "UnrealEgo")]


@functools.lru_cache(maxsize=None)
def _expected(shape, fixed, with_tracks):
    """(rig, table, inputs, the restatement's records and state): computed once per case, shared, never written"""
    T, S, kind = shape
    r, tw, pts, trk, state0 = TI.case(kind, T, S, fixed, with_tracks)
    want = spec.skeleton_fit_twist_ref(pts, state0, r, tw, I.PARAMS, tracks=trk, streams=S)
    for a in (pts, trk, state0) + want:
        if a is not None:
            a.setflags(write=False)
    return r, tw, (pts, trk, state0), want


def _launch(r, tw, params, points, tracks, S, state_in, state_out, rigid, rotations, lengths, t0=0, n_t=None):
    """the raw entry on steps t0 .. t0 + n_t - 1 of the case's device inputs; tw None: egotap_skeleton_fit"""
    n_t = points.shape[0] // S if n_t is None else n_t
    lo, hi = t0 * S, (t0 + n_t) * S
    cut = lambda a: None if a is None else a[lo:hi]      # noqa: E731
    rig_c, prm_c = L.skeleton_rig_struct(r), L.skeleton_params_struct(params, track_rows=0 if tracks is None else tracks.shape[1])
    if tw is None:
        L.check(L.load().egotap_skeleton_fit(L.ptr(cut(points)), L.ptr(cut(tracks)), n_t, S, C.byref(rig_c), C.byref(prm_c), L.ptr(state_in), L.ptr(state_out),
                                             L.ptr(rigid), L.ptr(rotations), L.ptr(lengths), L.stream()))
    else:
        tw_c = L.skeleton_twist_struct(tw)
        L.check(L.load().egotap_skeleton_fit_twist(L.ptr(cut(points)), L.ptr(cut(tracks)), n_t, S, C.byref(rig_c), C.byref(tw_c), C.byref(prm_c), L.ptr(state_in),
                                                   L.ptr(state_out), L.ptr(rigid), L.ptr(rotations), L.ptr(lengths), L.stream()))


@pytest.mark.parametrize("with_tracks", [False, True], ids=["no_tracks", "tracks"])
@pytest.mark.parametrize("fixed", [False, True], ids=["calibrating", "fixed_length"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_S%d_%s" % s)
def test_skeleton_fit_twist_equals_the_float64_restatement(shape, fixed, with_tracks):
    T, S, kind = shape
    r, tw, (pts, trk, state0), want = _expected(shape, fixed, with_tracks)
    B, P = T * S, r.P
    points, tracks, state_in = _dev(pts), _dev(trk), _dev(state0)

    def run(table):
        rigid, ok_r = _between_canaries(B * P * 4)
        rotations, ok_q = _between_canaries(B * P * 8)
        lengths, ok_l = _between_canaries(B * P * 2)
        state_out, ok_s = _between_canaries(S * P * 2, dtype=torch.float64)
        _launch(r, table, I.PARAMS, points, tracks, S, state_in, None if fixed else state_out, rigid, rotations, lengths)
        torch.cuda.synchronize()
        assert ok_r() and ok_q() and ok_l() and ok_s(), tag
        if fixed:
            assert bool((state_out == CANARY).all())                  # no state is written
        else:
            _bits(state_in, state0)                                   # out of place: the state read is not written
        return rigid.view(B, P, 4), rotations.view(B, P, 8), lengths.view(B, P, 2), None if fixed else state_out.view(S, P, 2)
    tag = f"twist T={T} S={S} {kind} {'fixed_length' if fixed else 'calibrating'} tracks={'yes' if with_tracks else 'no'}"
    got = run(tw)
    _compare(tag, got, want, pts)
    flags = got[0][..., 3].cpu().numpy()
    assert (flags == 7).any() == (kind != "star64"), tag
    # the same inputs through egotap_skeleton_fit: positions, lengths and the state in bits; in the star, which can have no pole row, everything
    old = run(None)
    _bits(got[0][..., :3].contiguous(), old[0][..., :3].contiguous())
    _bits(got[2], old[2])
    if not fixed:
        _bits(got[3], old[3])
    _bits(torch.minimum(got[0][..., 3], torch.tensor(3.0, device="cuda")).contiguous(), old[0][..., 3].contiguous())
    if kind == "star64":
        _bits(got[0], old[0])
        _bits(got[1], old[1])
    # the Python face: the same launch, the state in place
    st = None if fixed else state_in.clone()
    r2, q2, l2 = L.skeleton_fit_twist(points, st, r, tw, params=I.PARAMS, tracks=tracks, streams=S)
    torch.cuda.synchronize()
    for a, b in zip((r2, q2, l2), got):
        _bits(a, b)
    if not fixed:
        _bits(st, got[3])


def test_the_half_turn_on_the_device_in_bits():
    r, tw, x, want = half_turn_case()
    points = _dev(x.astype(np.float32))
    state = torch.zeros(1, r.P, 2, dtype=torch.float64, device="cuda")
    prm = spec.SkeletonParams(min_samples=1)
    rigid, rot, _ = L.skeleton_fit_twist(points, state, r, tw, params=prm)
    torch.cuda.synchronize()
    assert rigid[0, :, 3].tolist() == [3, 3, 3, 3, 7, 3]
    _bits(rot[0, 4], np.array(want + want, dtype=np.float32))
    for a, b in zip((rigid, rot), spec.skeleton_fit_twist_ref(x, np.zeros((1, r.P, 2)), r, tw, prm)):
        _bits(a, b)


@pytest.mark.parametrize("with_tracks", [False, True], ids=["no_tracks", "tracks"])
def test_chunks_in_place_and_out_of_place_give_the_same_bits(with_tracks):
    T, S, kind = shape = (7, 1, "UnrealEgo")
    r, tw, (pts, trk, state0), _ = _expected(shape, False, with_tracks)
    B, P = T * S, r.P
    points, tracks = _dev(pts), _dev(trk)

    def run(parts, in_place):
        st = _dev(state0)
        rigid, rot, lens = torch.empty(B, P, 4, device="cuda"), torch.empty(B, P, 8, device="cuda"), torch.empty(B, P, 2, device="cuda")
        lo = 0
        for n_t in parts:
            nxt = st if in_place else torch.full_like(st, CANARY)
            _launch(r, tw, I.PARAMS, points, tracks, S, st, nxt, rigid[lo * S:], rot[lo * S:], lens[lo * S:], t0=lo, n_t=n_t)
            st, lo = nxt, lo + n_t
        torch.cuda.synchronize()
        return rigid, rot, lens, st
    whole = run([7], False)
    assert bool((whole[0][..., 3] == 7).any())
    for parts, in_place in (([3, 1, 3], False), ([3, 1, 3], True), ([7], True)):
        for a, b in zip(run(parts, in_place), whole):
            _bits(a, b)


def test_waves_past_the_last_stream_write_nothing():
    """S = 6 streams fill one workgroup and half of the second: the two waves past S store nothing (every array ends where stream 5's does)"""
    T, S, kind = shape = (3, 6, "EgoCap")
    r, tw, (pts, trk, state0), want = _expected(shape, False, True)
    P = r.P
    state, ok_s = _between_canaries(S * P * 2, dtype=torch.float64, pad=2 * P * 2)       # room for two more streams: none is written
    state.copy_(_dev(state0).view(-1))
    rigid, ok_r = _between_canaries(T * S * P * 4, pad=2 * P * 4)
    rot, ok_q = _between_canaries(T * S * P * 8, pad=2 * P * 8)
    lens, ok_l = _between_canaries(T * S * P * 2, pad=2 * P * 2)
    _launch(r, tw, I.PARAMS, _dev(pts), _dev(trk), S, state, state, rigid, rot, lens)
    torch.cuda.synchronize()
    assert ok_s() and ok_r() and ok_q() and ok_l()
    _bits(rigid.view(T * S, P, 4)[..., 3].contiguous(), want[0][..., 3].copy())
    _bits(state.view(S, P, 2)[..., 1].contiguous(), want[3][..., 1].copy())


# ------------------------------------------------------------------------------------------------------------ serving


def test_a_skeleton_with_a_twist_behind_the_serving_call_and_the_trackers():
    m, p = _model()
    left, right = OI.rig_models(True)
    m.set_stereo_rig(left, right, OI.T, R=OI.SMALL_R, min_score=-1e30)           # the synthetic estimators' peaks are no probabilities: every joint is "seen"
    dev = torch.device("cuda", torch.cuda.current_device())
    B, S0, P = 2, 4 * p.hm_size, p.out_joints
    g = torch.Generator().manual_seed(31)
    frames = [[torch.randint(0, 256, (B, S0, S0, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)] for _ in range(2)]
    tprm = spec.TrackParams(min_joints=1, max_hold=2)
    sprm = spec.SkeletonParams(window=3, min_samples=1)
    rigs = _dev(W.rigs(2 * B, 1, seed=5, bad=False))
    for world in (False, True):
        tracker = m.new_pose_tracker(streams=1, params=tprm, world=world)
        twisted = m.new_skeleton(streams=1, params=sprm)
        st_t, st_p = (torch.zeros(1, P, 2, dtype=torch.float64, device=dev) for _ in range(2))
        rig = tw = None
        for k, (l8, r8) in enumerate(frames):                         # two calls of T = 2 consecutive frames each
            pose, j3, fr = m.predict_pose_from_camera(l8, r8, return_triangulation=True)
            kw = dict(rig_pose=rigs[k * B:(k + 1) * B]) if world else {}
            res = tracker.update(pose, j3, fr, dt=1.0 / 30, **kw)
            placed, tracks = res[0], res[1]
            if rig is None:                                           # the first frame as the rest pose, the second as the bent frame
                rig = twisted.set_rest_pose(placed[0])
                plain = m.new_skeleton(rig=rig, streams=1, params=sprm)
                tw = twisted.set_hinges(placed[1], bend_lo=0.0, bend_hi=1e-3)
                assert twisted.twist is tw and plain.twist is None and tw.pole == spec.skeleton_twist(rig, spec.SKELETON_POLE["UnrealEgo"], tw.hinge).pole
            got, old = twisted.update(placed, tracks), plain.update(placed, tracks)
            want = L.skeleton_fit_twist(placed, st_t, rig, tw, params=sprm, tracks=tracks, streams=1)
            want_old = L.skeleton_fit(placed, st_p, rig, params=sprm, tracks=tracks, streams=1)
            torch.cuda.synchronize()
            for a, b in zip(got + old, want + want_old):
                _bits(a, b)
            _bits(twisted.state, st_t)
            _bits(plain.state, st_p)
            _bits(twisted.state, plain.state)                         # the calibration does not depend on the twist
            assert (got[0][:, :, 3] >= 3).all() and (got[0][:, list(spec.SKELETON_POLE["UnrealEgo"]), 3] == 7).all() and (old[0][:, :, 3] == 3).all()
            if k == 0:                                                # against the restatement, from the tensors the tracker returned
                ref = spec.skeleton_fit_twist_ref(placed.cpu().numpy(), np.zeros((1, P, 2)), rig, tw, sprm, tracks=tracks.cpu().numpy())
                _compare(f"serving twist world={world}", got + (twisted.state.clone(),), ref, placed.cpu().numpy())
                # frame 1 is the frame the hinges were taken from: its twist is the identity, so it equals the untwisted fit to the bounds' width
                assert (got[1][1] - old[1][1]).abs().max() <= 4 * np.spacing(np.float32(1.0))
    # the timing hook records the launch under its own name
    h = m._rgb_state(dev).handle.h
    lib = L.load()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        twisted.update(placed, tracks)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 1 and '"role": "skeleton_fit_twist"' in detail, detail
