"""The temporal filter on the device: egotap_pose_track (pose_track.h), lib.pose_track and the model's PoseTracker.

The expected values are the float64 restatement spec.pose_track_ref on inputs with accepted, rejected, NaN, gated and expiring tracks mixed in, from a
state that is already under way (tests/pose_track_inputs.py).  Device and host run the same float64 operations in the same order; only the divisions
and the square root may differ in the last float64 bit, which the one rounding to fp32 can turn into one fp32 ulp:
  * equal in bits: status, the all-zero records, the state's age and live, and gap_t (every step time here is a power of two);
  * x^ and placed within 2 fp32 ulp of the largest |x^| component of the track over the call (for placed: of the pose track, the root track and the
    placed row itself -- the sum is rounded at its own size); cutoff within 2 ulp of itself; v^ within 2 fp32 ulp of the track's largest |v^| component
    plus 1e-12 max|m| / dt for the cancellation in m - m_prev; the float64 state within 1e-13 max(1, |value|).
Measured on the MI355X: every output and every state value of every case below came out EQUAL IN BITS (largest deviation / bound 0.0), so the gates
above have their whole width to spare.
The serving test's expected value is lib.pose_track on the same tensors: the same kernel on the same inputs, hence equal bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ocam_inputs as OI
import pose_track_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
CANARY = -12345.0
DT = I.DT
NK = spec.POSE_TRACK_STATE
DTS = np.array([DT, 2 * DT, DT, 0.0, DT, np.nan, DT / 2], dtype=np.float32)       # two steps without a usable time among them
SHAPES = [(1, 1, 16, 15), (7, 1, 16, 15), (3, 5, 17, 0), (2, 4, 64, 64), (1, 9, 16, 15)]


def _bits(got, want):
    got, want = (np.ascontiguousarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t) for t in (got, want))
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    view = np.int64 if got.dtype == np.float64 else np.int32
    assert np.array_equal(got.view(view), want.view(view)), np.argwhere(got.view(view) != want.view(view))[:8]


def _between_canaries(n, dtype=torch.float32, pad=64):
    """(the view an operator writes, a check that nothing around it moved)"""
    flat = torch.full((n + 2 * pad,), CANARY, device="cuda", dtype=dtype)

    def untouched():
        return bool((flat[:pad] == CANARY).all()) and bool((flat[pad + n:] == CANARY).all())
    return flat[pad:pad + n], untouched


@functools.lru_cache(maxsize=None)
def _expected(shape, clock, with_frame):
    """(inputs, the restatement's records and state): computed once per case, shared, never written"""
    T, S, P, J = shape
    pose, frame, j3, state0 = I.case(T, S, P, J)
    if not with_frame:
        frame = None
    want = spec.pose_track_ref(pose, state0, DT if clock == "dt" else DTS[:T], I.PARAMS, frame=frame, joints3d=j3, streams=S)
    for a in (pose, frame, j3, state0) + want:
        if a is not None:
            a.setflags(write=False)
    return (pose, frame, j3, state0), want


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _launch(inputs, shape, clock, state_in, state_out, tracks, placed, t0=0, n_t=None):
    """the raw entry on steps t0 .. t0 + n_t - 1 of the case's device inputs"""
    T, S, P, J = shape
    pose, frame, j3, dts = inputs
    n_t = T if n_t is None else n_t
    lo, hi = t0 * S, (t0 + n_t) * S
    cut = lambda a: None if a is None else a[lo:hi]      # noqa: E731
    prm = L.track_params_struct(I.PARAMS)
    L.check(L.load().egotap_pose_track(L.ptr(cut(pose)), L.ptr(cut(frame)), L.ptr(cut(j3)), n_t, S, P, J, L.ptr(dts[t0:t0 + n_t]) if clock == "dts" else None,
                                       C.c_double(DT if clock == "dt" else 0.0), C.byref(prm), L.ptr(state_in), L.ptr(state_out), L.ptr(tracks), L.ptr(placed),
                                       L.stream()))


def _compare(tag, got, want, inputs, S, dt_min):
    gt, gp, gs = (t.detach().cpu().numpy() for t in got)
    wt, wp, ws = want
    B, K, _ = wt.shape
    T, P = B // S, wp.shape[1]
    assert np.isfinite(gt).all() and np.isfinite(gp).all() and np.isfinite(gs).all(), tag
    _bits(gt[..., 7], wt[..., 7])
    zero = wt[..., 7] == 0
    _bits(gt[zero], wt[zero])                                         # the all-zero records, in bits
    _bits(gp[zero[:, :P]], wp[zero[:, :P]])
    _bits(gs[..., 9:12], ws[..., 9:12])                               # gap_t (sums of powers of two), age, live
    g4, w4 = gt.reshape(T, S, K, 8).astype(np.float64), wt.reshape(T, S, K, 8).astype(np.float64)
    ulp2 = lambda top: 2.0 * np.spacing(top.astype(np.float32)).astype(np.float64)      # noqa: E731
    top_x, top_v = np.abs(w4[..., 0:3]).max(axis=(0, 3)), np.abs(w4[..., 3:6]).max(axis=(0, 3))
    m_max = max(float(np.abs(a[np.isfinite(a)]).max()) for a in inputs[:3] if a is not None)
    bx, bv = ulp2(top_x), ulp2(top_v) + 1e-12 * m_max / dt_min
    dx, dv = np.abs(g4[..., 0:3] - w4[..., 0:3]).max(axis=(0, 3)), np.abs(g4[..., 3:6] - w4[..., 3:6]).max(axis=(0, 3))
    dc, bc = np.abs(g4[..., 6] - w4[..., 6]), ulp2(np.abs(w4[..., 6]))
    gp4, wp4 = gp.reshape(T, S, P, 3).astype(np.float64), wp.reshape(T, S, P, 3).astype(np.float64)
    bp = ulp2(np.maximum(np.maximum(top_x[:, :P], top_x[:, P:P + 1]), np.abs(wp4).max(axis=(0, 3))))
    dp = np.abs(gp4 - wp4).max(axis=(0, 3))
    ds, bs = np.abs(gs - ws), 1e-13 * np.maximum(1.0, np.abs(ws))
    print(tag, "largest deviation / bound: x^", (dx / bx).max(), "v^", (dv / bv).max(), "cutoff", (dc / bc).max(), "placed", (dp / bp).max(), "state", (ds / bs).max(),
          "| records that differ in any bit:", int((gt.view(np.int32) != wt.view(np.int32)).any(axis=-1).sum()), "of", B * K,
          " state values:", int((gs.view(np.int64) != ws.view(np.int64)).sum()))
    assert (dx <= bx).all(), (tag, "x^", (dx / bx).max())
    assert (dv <= bv).all(), (tag, "v^", (dv / bv).max())
    assert (dc <= bc).all(), (tag, "cutoff", (dc / bc).max())
    assert (dp <= bp).all(), (tag, "placed", (dp / bp).max())
    assert (ds <= bs).all(), (tag, "state", (ds / bs).max())


@pytest.mark.parametrize("with_frame", [True, False], ids=["frame", "no_frame"])
@pytest.mark.parametrize("clock", ["dt", "dts"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_S%d_P%d_J%d" % s)
def test_pose_track_equals_the_float64_restatement(shape, clock, with_frame):
    T, S, P, J = shape
    B, K = T * S, P + 1 + J
    (pose, frame, j3, state0), want = _expected(shape, clock, with_frame)
    inputs = (_dev(pose), _dev(frame), _dev(j3), _dev(DTS[:T]))
    state_in = _dev(state0)
    tracks, ok_t = _between_canaries(B * K * 8)
    placed, ok_p = _between_canaries(B * P * 3)
    state_out, ok_s = _between_canaries(S * K * NK, dtype=torch.float64)
    _launch(inputs, shape, clock, state_in, state_out, tracks, placed)
    torch.cuda.synchronize()
    tag = f"T={T} S={S} P={P} J={J} {clock} frame={'yes' if with_frame else 'no'}"
    assert ok_t() and ok_p() and ok_s(), tag
    _bits(state_in, state0)                                           # out of place: the state read is not written
    got = (tracks.view(B, K, 8), placed.view(B, P, 3), state_out.view(S, K, NK))
    dt_min = DT if clock == "dt" else float(np.nanmin(np.where(DTS[:T] > 0, DTS[:T], np.nan)))
    _compare(tag, got, want, (pose, frame, j3), S, dt_min)
    assert with_frame or (want[0][:, P, 7] != 1).all()                  # no frame record: the root is held or forgotten, never updated
    # the Python face: the same launch, the state in place
    st = state_in.clone()
    t2, p2 = L.pose_track(inputs[0], st, dt=DT if clock == "dt" else None, dts=inputs[3] if clock == "dts" else None, params=I.PARAMS, frame=inputs[1],
                          joints3d=inputs[2], streams=S)
    torch.cuda.synchronize()
    _bits(t2, got[0])
    _bits(p2, got[1])
    _bits(st, got[2])


@pytest.mark.parametrize("clock", ["dt", "dts"])
def test_chunks_in_place_and_repeats_give_the_same_bits(clock):
    shape = T, S, P, J = (7, 1, 16, 15)
    B, K = T * S, P + 1 + J
    (pose, frame, j3, state0), _ = _expected(shape, clock, True)
    inputs = (_dev(pose), _dev(frame), _dev(j3), _dev(DTS[:T]))

    def run(parts, in_place, start):
        st = _dev(start)
        tracks, placed = torch.empty(B, K, 8, device="cuda"), torch.empty(B, P, 3, device="cuda")
        lo = 0
        for n_t in parts:
            nxt = st if in_place else torch.full_like(st, CANARY)
            _launch(inputs, shape, clock, st, nxt, tracks[lo * S:], placed[lo * S:], t0=lo, n_t=n_t)
            st, lo = nxt, lo + n_t
        torch.cuda.synchronize()
        return tracks, placed, st
    for start in (state0, np.zeros_like(state0)):
        whole = run([7], False, start)
        for parts, in_place in (([3, 1, 3], False), ([3, 1, 3], True), ([7], True), ([7], False), ([1] * 7, True)):
            again = run(parts, in_place, start)
            for a, b in zip(again, whole):
                _bits(a, b)


def test_ragged_last_workgroup_leaves_the_other_streams_alone():
    """S = 5 streams fill one workgroup and a quarter of the second: the three waves past S store nothing (the state array ends where stream 4's does)"""
    shape = T, S, P, J = (3, 5, 17, 0)
    (pose, frame, j3, state0), want = _expected(shape, "dt", True)
    assert j3 is None
    inputs = (_dev(pose), _dev(frame), None, None)
    state, ok_s = _between_canaries(S * (P + 1) * NK, dtype=torch.float64, pad=3 * (P + 1) * NK)       # room for three more streams: none is written
    state.copy_(_dev(state0).view(-1))
    tracks, ok_t = _between_canaries(T * S * (P + 1) * 8, pad=3 * (P + 1) * 8)
    placed, ok_p = _between_canaries(T * S * P * 3, pad=3 * P * 3)
    _launch(inputs, shape, "dt", state, state, tracks, placed)
    torch.cuda.synchronize()
    assert ok_s() and ok_t() and ok_p()
    _bits(state.view(S, P + 1, NK), want[2])


# ------------------------------------------------------------------------------------------------------------ serving


def test_tracker_behind_the_serving_call():
    m, p = _model()
    left, right = OI.rig_models(True)
    m.set_stereo_rig(left, right, OI.T, R=OI.SMALL_R, min_score=-1e30)           # the synthetic estimators' peaks are no probabilities: every joint is "seen"
    dev = torch.device("cuda", torch.cuda.current_device())
    B, S0, P, J = 2, 4 * p.hm_size, p.out_joints, p.n_joints_hm
    g = torch.Generator().manual_seed(31)
    frames = [[torch.randint(0, 256, (B, S0, S0, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(2)] for _ in range(2)]
    before = [tuple(t.clone() for t in m.predict_pose_from_camera(l8, r8, return_triangulation=True)) for l8, r8 in frames]
    ws_bytes = m._rgb_state(dev).ws.numel()
    n_graphs = len(m._rgb_state(dev).graphs)
    prm = spec.TrackParams(min_joints=1, max_hold=2)
    tracker = m.new_pose_tracker(streams=1, params=prm)
    assert tuple(tracker.state.shape) == (1, P + 1 + J, NK) and tracker.state.dtype == torch.float64 and not tracker.state.any()
    state = torch.zeros_like(tracker.state)
    outs = []
    for k, (l8, r8) in enumerate(frames):                             # two calls of T = 2 consecutive frames each
        pose, j3, fr = m.predict_pose_from_camera(l8, r8, return_triangulation=True)
        placed, tracks = tracker.update(pose, j3, fr, dt=1.0 / 30)
        want_t, want_p = L.pose_track(pose, state, dt=1.0 / 30, params=prm, frame=fr, joints3d=j3, streams=1)
        torch.cuda.synchronize()
        assert tuple(placed.shape) == (B, P, 3) and tuple(tracks.shape) == (B, P + 1 + J, 8)
        _bits(tracks, want_t)
        _bits(placed, want_p)
        _bits(tracker.state, state)
        for a, b in zip((pose, j3, fr), before[k]):                   # the serving call's own outputs: the tracker changes nothing
            assert torch.equal(a, b), k
        outs.append((placed.clone(), tracks.clone()))
        assert (tracks[:, :P, 7] == 1).all() and bool((fr[:, 3] >= 1).all()) == bool((tracks[:, P, 7] == 1).all())
    assert m._rgb_state(dev).ws.numel() == ws_bytes and len(m._rgb_state(dev).graphs) == n_graphs
    assert not torch.equal(outs[1][0], outs[0][0])
    # and against the restatement, from the tensors the serving call returned
    pose, j3, fr = before[0]
    wt, wp, _ = spec.pose_track_ref(pose.cpu().numpy(), np.zeros((1, P + 1 + J, NK)), 1.0 / 30, prm, frame=fr.cpu().numpy(), joints3d=j3.cpu().numpy())
    _compare("serving", (outs[0][1], outs[0][0], torch.zeros(1, P + 1 + J, NK, dtype=torch.float64)), (wt, wp, np.zeros((1, P + 1 + J, NK))),
             tuple(t.cpu().numpy() for t in before[0]), 1, 1.0 / 30)
    # reset: the next frame is a first frame again; a held frame (no joints, no root seen) keeps the last estimate
    tracker.reset()
    assert not tracker.state.any()
    placed, tracks = tracker.update(*before[0], dt=1.0 / 30)
    _bits(placed, outs[0][0])
    _bits(tracks, outs[0][1])
    held_p, held_t = tracker.update(torch.full_like(before[1][0], float("nan")), dt=1.0 / 30)
    torch.cuda.synchronize()
    live = tracks[1, :, 7] != 0
    assert (held_t[0, live, 7] == 2).all() and (held_t[0, ~live, 7] == 0).all()
    _bits(held_t[0, live, 0:6], tracks[1, live, 0:6])
    _bits(held_p[0], placed[1])
    tracker.reset(streams=[0])
    assert not tracker.state.any()
    with pytest.raises(ValueError, match="streams are"):
        tracker.reset(streams=[1])
    # the timing hook records the launch
    h = m._rgb_state(dev).handle.h
    lib = L.load()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        tracker.update(*before[0], dt=1.0 / 30)
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 1 and '"role": "pose_track"' in detail, detail
