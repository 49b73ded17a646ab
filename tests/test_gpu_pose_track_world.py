"""The temporal filter in a world frame on the device: egotap_pose_track_world (pose_track.h), lib.pose_track_world and the model's world PoseTracker.

The expected values are the float64 restatement spec.pose_track_world_ref on the inputs of tests/pose_track_world_inputs.py: accepted, unseen, NaN,
inf, gated and expiring samples under rig poses that count and rig poses that do not (a NaN, an inf, a matrix that is no rotation, a reflection), from
a world-frame state that is already under way.  Device and host run the same float64 operations in the same order; the rig transform adds products
and sums only, so as in tests/test_gpu_pose_track.py only the divisions and the square root may differ in the last float64 bit.  The gates are those
of that file, restated:
  * equal in bits: status, the all-zero records, the state's age and live, and gap_t (every step time here is a power of two);
  * x^, placed_world and placed_cam within 2 fp32 ulp of the largest magnitude of the row over the call (for the placed outputs: of the pose track, the
    root track and the placed row itself), placed_cam with 1e-12 max|t| more for the cancellation in p - t; cutoff within 2 ulp of itself; v^ within
    2 fp32 ulp of the track's largest |v^| component plus 1e-12 max|m_w| / dt; the float64 state within 1e-13 max(1, |value|).
Measured on the MI355X: every output and every state value of every case below came out EQUAL IN BITS (largest deviation / bound 0.0), as in the
camera frame, so the gates above have their whole width to spare.
The serving test's expected value is lib.pose_track_world on the same tensors: the same kernel on the same inputs, hence equal bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ocam_inputs as OI
import pose_track_world_inputs as W
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model

pytestmark = pytest.mark.gpu
CANARY = -12345.0
DT = W.DT
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
    pose, frame, j3, rig, state0 = W.case(T, S, P, J)
    if not with_frame:
        frame = None
    want = spec.pose_track_world_ref(pose, state0, rig, DT if clock == "dt" else DTS[:T], W.PARAMS, frame=frame, joints3d=j3, streams=S, ortho_tol=W.ORTHO_TOL)
    for a in (pose, frame, j3, rig, state0) + want:
        if a is not None:
            a.setflags(write=False)
    return (pose, frame, j3, rig, state0), want


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _launch(inputs, shape, clock, state_in, state_out, tracks, placed_world, placed_cam, t0=0, n_t=None):
    """the raw entry on steps t0 .. t0 + n_t - 1 of the case's device inputs"""
    T, S, P, J = shape
    pose, frame, j3, rig, dts = inputs
    n_t = T if n_t is None else n_t
    lo, hi = t0 * S, (t0 + n_t) * S
    cut = lambda a: None if a is None else a[lo:hi]      # noqa: E731
    prm = L.track_params_struct(W.PARAMS)
    L.check(L.load().egotap_pose_track_world(L.ptr(cut(pose)), L.ptr(cut(frame)), L.ptr(cut(j3)), L.ptr(cut(rig)), n_t, S, P, J,
                                             L.ptr(dts[t0:t0 + n_t]) if clock == "dts" else None, C.c_double(DT if clock == "dt" else 0.0), C.byref(prm),
                                             C.c_double(W.ORTHO_TOL), L.ptr(state_in), L.ptr(state_out), L.ptr(tracks), L.ptr(placed_world), L.ptr(placed_cam),
                                             L.stream()))


def _compare(tag, got, want, m_max, t_max, S, dt_min):
    """``m_max``: the largest finite world measurement, ``t_max``: the largest finite rig translation"""
    gt, gw, gc, gs = (t.detach().cpu().numpy() for t in got)
    wt, ww, wc, ws = want
    B, K, _ = wt.shape
    T, P = B // S, ww.shape[1]
    assert all(np.isfinite(a).all() for a in (gt, gw, gc, gs)), tag
    _bits(gt[..., 7], wt[..., 7])
    zero = wt[..., 7] == 0
    _bits(gt[zero], wt[zero])                                         # the all-zero records, in bits
    _bits(gw[zero[:, :P]], ww[zero[:, :P]])
    cam_zero = (wc == 0).all(axis=-1)                                 # those, and every row of a frame whose rig pose is not seen
    _bits(gc[cam_zero], wc[cam_zero])
    _bits(gs[..., 9:12], ws[..., 9:12])                               # gap_t (sums of powers of two), age, live
    g4, w4 = gt.reshape(T, S, K, 8).astype(np.float64), wt.reshape(T, S, K, 8).astype(np.float64)
    ulp2 = lambda top: 2.0 * np.spacing(top.astype(np.float32)).astype(np.float64)      # noqa: E731
    top_x, top_v = np.abs(w4[..., 0:3]).max(axis=(0, 3)), np.abs(w4[..., 3:6]).max(axis=(0, 3))
    bx, bv = ulp2(top_x), ulp2(top_v) + 1e-12 * m_max / dt_min
    dx, dv = np.abs(g4[..., 0:3] - w4[..., 0:3]).max(axis=(0, 3)), np.abs(g4[..., 3:6] - w4[..., 3:6]).max(axis=(0, 3))
    dc, bc = np.abs(g4[..., 6] - w4[..., 6]), ulp2(np.abs(w4[..., 6]))
    row = lambda a: a.reshape(T, S, P, 3).astype(np.float64)      # noqa: E731
    top_p = np.maximum(top_x[:, :P], top_x[:, P:P + 1])
    bw = ulp2(np.maximum(top_p, np.abs(row(ww)).max(axis=(0, 3))))
    bcam = ulp2(np.maximum(np.maximum(top_p, np.abs(row(ww)).max(axis=(0, 3))), np.abs(row(wc)).max(axis=(0, 3)))) + 1e-12 * t_max
    dw, dcam = np.abs(row(gw) - row(ww)).max(axis=(0, 3)), np.abs(row(gc) - row(wc)).max(axis=(0, 3))
    ds, bs = np.abs(gs - ws), 1e-13 * np.maximum(1.0, np.abs(ws))
    print(tag, "largest deviation / bound: x^", (dx / bx).max(), "v^", (dv / bv).max(), "cutoff", (dc / bc).max(), "placed_world", (dw / bw).max(), "placed_cam",
          (dcam / bcam).max(), "state", (ds / bs).max(), "| records that differ in any bit:", int((gt.view(np.int32) != wt.view(np.int32)).any(axis=-1).sum()), "of",
          B * K, " placed rows:", int((gw.view(np.int32) != ww.view(np.int32)).any(axis=-1).sum()), "+",
          int((gc.view(np.int32) != wc.view(np.int32)).any(axis=-1).sum()), "of", B * P, " state values:", int((gs.view(np.int64) != ws.view(np.int64)).sum()))
    assert (dx <= bx).all(), (tag, "x^", (dx / bx).max())
    assert (dv <= bv).all(), (tag, "v^", (dv / bv).max())
    assert (dc <= bc).all(), (tag, "cutoff", (dc / bc).max())
    assert (dw <= bw).all(), (tag, "placed_world", (dw / bw).max())
    assert (dcam <= bcam).all(), (tag, "placed_cam", (dcam / bcam).max())
    assert (ds <= bs).all(), (tag, "state", (ds / bs).max())


def _maxima(pose, frame, j3, rig):
    """(the largest |m_w| component among the finite measurements of the frames whose rig pose counts, the largest |t| among those rig poses)"""
    g = rig.reshape(-1, 3, 4)
    R, t = g[:, :, :3], g[:, :, 3]
    with np.errstate(all="ignore"):
        seen = np.isfinite(g).all(axis=(1, 2)) & (np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max(axis=(1, 2)) <= W.ORTHO_TOL)
        seen &= np.linalg.det(np.where(np.isfinite(R), R, 0.0)) > 0
    assert seen.any()
    m_max = 0.0
    for a, point in ((pose, False), (None if frame is None else frame[:, None, 0:3], True), (None if j3 is None else j3[..., 0:3], True)):
        if a is not None:
            with np.errstate(all="ignore"):
                w = np.einsum("bij,bkj->bki", R, a.astype(np.float64)) + (t[:, None] if point else 0.0)
            w = w[seen]
            m_max = max(m_max, float(np.abs(w[np.isfinite(w)]).max()))
    return m_max, float(np.abs(t[seen]).max())


@pytest.mark.parametrize("with_frame", [True, False], ids=["frame", "no_frame"])
@pytest.mark.parametrize("clock", ["dt", "dts"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_S%d_P%d_J%d" % s)
def test_pose_track_world_equals_the_float64_restatement(shape, clock, with_frame):
    T, S, P, J = shape
    B, K = T * S, P + 1 + J
    (pose, frame, j3, rig, state0), want = _expected(shape, clock, with_frame)
    inputs = (_dev(pose), _dev(frame), _dev(j3), _dev(rig), _dev(DTS[:T]))
    state_in = _dev(state0)
    tracks, ok_t = _between_canaries(B * K * 8)
    placed_world, ok_w = _between_canaries(B * P * 3)
    placed_cam, ok_c = _between_canaries(B * P * 3)
    state_out, ok_s = _between_canaries(S * K * NK, dtype=torch.float64)
    _launch(inputs, shape, clock, state_in, state_out, tracks, placed_world, placed_cam)
    torch.cuda.synchronize()
    tag = f"T={T} S={S} P={P} J={J} {clock} frame={'yes' if with_frame else 'no'}"
    assert ok_t() and ok_w() and ok_c() and ok_s(), tag
    _bits(state_in, state0)                                           # out of place: the state read is not written
    got = (tracks.view(B, K, 8), placed_world.view(B, P, 3), placed_cam.view(B, P, 3), state_out.view(S, K, NK))
    dt_min = DT if clock == "dt" else float(np.nanmin(np.where(DTS[:T] > 0, DTS[:T], np.nan)))
    _compare(tag, got, want, *_maxima(pose, frame, j3, rig), S, dt_min)
    assert with_frame or (want[0][:, P, 7] != 1).all()                  # no frame record: the root is held or forgotten, never updated
    # the Python face: the same launch, the state in place
    st = state_in.clone()
    t2, w2, c2 = L.pose_track_world(inputs[0], st, inputs[3], dt=DT if clock == "dt" else None, dts=inputs[4] if clock == "dts" else None, params=W.PARAMS,
                                    frame=inputs[1], joints3d=inputs[2], streams=S, ortho_tol=W.ORTHO_TOL)
    torch.cuda.synchronize()
    _bits(t2, got[0])
    _bits(w2, got[1])
    _bits(c2, got[2])
    _bits(st, got[3])


@pytest.mark.parametrize("clock", ["dt", "dts"])
def test_chunks_in_place_and_repeats_give_the_same_bits(clock):
    shape = T, S, P, J = (7, 1, 16, 15)
    B, K = T * S, P + 1 + J
    (pose, frame, j3, rig, state0), _ = _expected(shape, clock, True)
    inputs = (_dev(pose), _dev(frame), _dev(j3), _dev(rig), _dev(DTS[:T]))

    def run(parts, in_place, start):
        st = _dev(start)
        tracks, pw, pc = torch.empty(B, K, 8, device="cuda"), torch.empty(B, P, 3, device="cuda"), torch.empty(B, P, 3, device="cuda")
        lo = 0
        for n_t in parts:
            nxt = st if in_place else torch.full_like(st, CANARY)
            _launch(inputs, shape, clock, st, nxt, tracks[lo * S:], pw[lo * S:], pc[lo * S:], t0=lo, n_t=n_t)
            st, lo = nxt, lo + n_t
        torch.cuda.synchronize()
        return tracks, pw, pc, st
    for start in (state0, np.zeros_like(state0)):
        whole = run([7], False, start)
        for parts, in_place in (([3, 1, 3], False), ([3, 1, 3], True), ([7], True), ([1] * 7, True)):
            again = run(parts, in_place, start)
            for a, b in zip(again, whole):
                _bits(a, b)


def test_ragged_last_workgroup_leaves_the_other_streams_alone():
    """S = 5 streams fill one workgroup and a quarter of the second: the three waves past S store nothing (the state array ends where stream 4's does)"""
    shape = T, S, P, J = (3, 5, 17, 0)
    (pose, frame, j3, rig, state0), want = _expected(shape, "dt", True)
    assert j3 is None
    inputs = (_dev(pose), _dev(frame), None, _dev(rig), None)
    state, ok_s = _between_canaries(S * (P + 1) * NK, dtype=torch.float64, pad=3 * (P + 1) * NK)       # room for three more streams: none is written
    state.copy_(_dev(state0).view(-1))
    tracks, ok_t = _between_canaries(T * S * (P + 1) * 8, pad=3 * (P + 1) * 8)
    pw, ok_w = _between_canaries(T * S * P * 3, pad=3 * P * 3)
    pc, ok_c = _between_canaries(T * S * P * 3, pad=3 * P * 3)
    _launch(inputs, shape, "dt", state, state, tracks, pw, pc)
    torch.cuda.synchronize()
    assert ok_s() and ok_t() and ok_w() and ok_c()
    _bits(state.view(S, P + 1, NK), want[3])


def test_identity_rig_pose_equals_the_camera_frame_entry():
    """in value: an identity transform turns a negative zero into a positive one (-0 + 0 = +0)"""
    shape = T, S, P, J = (7, 1, 16, 15)
    pose, frame, j3, state0 = W.I.case(T, S, P, J)                    # (a camera-frame state: under the identity the two frames are one)
    pose, frame, j3 = _dev(pose), _dev(frame), _dev(j3)
    rig = _dev(np.tile(W.IDENTITY, (T * S, 1)))
    st_c, st_w = _dev(state0), _dev(state0)
    tracks, placed = L.pose_track(pose, st_c, dt=DT, params=W.PARAMS, frame=frame, joints3d=j3, streams=S)
    t2, pw, pc = L.pose_track_world(pose, st_w, rig, dt=DT, params=W.PARAMS, frame=frame, joints3d=j3, streams=S, ortho_tol=0.0)
    torch.cuda.synchronize()
    assert (tracks[..., 7] == 1).any() and (tracks[..., 7] == 2).any()
    for a, b in ((t2, tracks), (pw, placed), (pc, placed), (st_w, st_c)):
        assert torch.equal(a, b)                                      # (-0 == +0)


# ------------------------------------------------------------------------------------------------------------ serving


def test_world_tracker_behind_the_serving_call():
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
    tracker = m.new_pose_tracker(streams=1, params=prm, world=True)
    assert tracker.world and tuple(tracker.state.shape) == (1, P + 1 + J, NK) and tracker.state.dtype == torch.float64 and not tracker.state.any()
    state = torch.zeros_like(tracker.state)
    rigs = _dev(W.rigs(2 * B, 1, seed=5, bad=False))                  # the headset's pose of the four consecutive frames
    outs = []
    for k, (l8, r8) in enumerate(frames):                             # two calls of T = 2 consecutive frames each
        pose, j3, fr = m.predict_pose_from_camera(l8, r8, return_triangulation=True)
        rig = rigs[k * B:(k + 1) * B]
        placed_world, tracks, placed_cam = tracker.update(pose, j3, fr, dt=1.0 / 30, rig_pose=rig)
        want_t, want_w, want_c = L.pose_track_world(pose, state, rig, dt=1.0 / 30, params=prm, frame=fr, joints3d=j3, streams=1)
        torch.cuda.synchronize()
        assert tuple(placed_world.shape) == tuple(placed_cam.shape) == (B, P, 3) and tuple(tracks.shape) == (B, P + 1 + J, 8)
        _bits(tracks, want_t)
        _bits(placed_world, want_w)
        _bits(placed_cam, want_c)
        _bits(tracker.state, state)
        for a, b in zip((pose, j3, fr), before[k]):                   # the serving call's own outputs: the tracker changes nothing
            assert torch.equal(a, b), k
        outs.append((placed_world.clone(), tracks.clone(), placed_cam.clone()))
        assert (tracks[:, :P, 7] == 1).all() and bool((fr[:, 3] >= 1).all()) == bool((tracks[:, P, 7] == 1).all())
    assert m._rgb_state(dev).ws.numel() == ws_bytes and len(m._rgb_state(dev).graphs) == n_graphs
    # and against the restatement, from the tensors the serving call returned
    pose, j3, fr = (t.cpu().numpy() for t in before[0])
    rig0 = rigs[:B].cpu().numpy()
    want = spec.pose_track_world_ref(pose, np.zeros((1, P + 1 + J, NK)), rig0, 1.0 / 30, prm, frame=fr, joints3d=j3)
    z = torch.zeros(1, P + 1 + J, NK, dtype=torch.float64)
    _compare("serving", (outs[0][1], outs[0][0], outs[0][2], z), want[:3] + (z.numpy(),), *_maxima(pose, fr, j3, rig0), 1, 1.0 / 30)
    # a frame without a usable rig pose holds every track and draws nothing
    bad = rigs[:B].clone()
    bad[:, 3] = float("nan")
    held_w, held_t, held_c = tracker.update(*before[0], dt=1.0 / 30, rig_pose=bad)
    torch.cuda.synchronize()
    assert (held_t[:, :P, 7] == 2).all() and not held_c.any()
    _bits(held_w[0], outs[1][0][1])
    with pytest.raises(ValueError, match="needs rig_pose"):
        tracker.update(*before[0], dt=1.0 / 30)
    with pytest.raises(ValueError, match="rig_pose goes with a world tracker"):
        m.new_pose_tracker().update(*before[0], dt=1.0 / 30, rig_pose=rigs[:B])
    # the timing hook records the launch
    h = m._rgb_state(dev).handle.h
    lib = L.load()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        tracker.update(*before[0], dt=1.0 / 30, rig_pose=rigs[:B])
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 1 and '"role": "pose_track_world"' in detail, detail
