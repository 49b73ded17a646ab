"""The skeleton fit on the device: egotap_skeleton_fit (skeleton_fit.h), lib.skeleton_fit and the model's Skeleton.

The expected values are the float64 restatement spec.skeleton_fit_ref on inputs with accepted, NaN, status-0, outlier and zero-length samples mixed in,
from a state that is already under way (tests/skeleton_inputs.py; no ok rotation there is near the antiparallel branch, v . u > -0.99, which
tests/test_skeleton_fit_cpu.py asserts).  Device and host run the same float64 operations in the same order; only sqrt and the divisions may differ in
the last float64 bit, which the one rounding to fp32 can turn into one fp32 ulp:
  * equal in bits: the flags, the all-zero records, the identity records and n;
  * rigid within 2 fp32 ulp of the frame's largest |coordinate|; quaternion components within 2 fp32 ulp of 1; lengths within 2 ulp of itself; the
    float64 state within 1e-13 max(1, |value|).
Measured on the MI355X: see MEASURED below.
The serving test's expected value is lib.skeleton_fit on the same tensors: the same kernel on the same inputs, hence equal bits."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ocam_inputs as OI
import pose_track_world_inputs as W
import skeleton_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from gpu_util import serving_model as _model
from test_skeleton_fit_cpu import antiparallel_case

pytestmark = pytest.mark.gpu
# MEASURED (one run of this file on one MI355X): every output and every state value of every case below came out EQUAL IN BITS to the restatement
# (largest deviation / bound 0.0 for rigid, rotations, lengths and the state), so the gates above have their whole width to spare.
CANARY = -12345.0
FIXED_SCALE = 1.3
SHAPES = [(1, 1, "UnrealEgo"), (7, 1, "UnrealEgo"), (3, 5, "EgoCap"), (2, 4, "chain64"), (2, 4, "star64"), (1, 9, "UnrealEgo")]


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
def _expected(shape, fixed, with_tracks, mirror):
    """(rig, inputs, the restatement's records and state): computed once per case, shared, never written"""
    T, S, kind = shape
    r, pts, trk, state0 = I.case(kind, T, S, mirror, with_tracks)
    if fixed:
        r, state0 = I.rig(kind, mirror=mirror, fixed_scale=FIXED_SCALE), None
    want = spec.skeleton_fit_ref(pts, state0, r, I.PARAMS, tracks=trk, streams=S)
    for a in (pts, trk, state0) + want:
        if a is not None:
            a.setflags(write=False)
    return r, (pts, trk, state0), want


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _launch(r, params, points, tracks, S, state_in, state_out, rigid, rotations, lengths, t0=0, n_t=None):
    """the raw entry on steps t0 .. t0 + n_t - 1 of the case's device inputs"""
    n_t = points.shape[0] // S if n_t is None else n_t
    lo, hi = t0 * S, (t0 + n_t) * S
    cut = lambda a: None if a is None else a[lo:hi]      # noqa: E731
    rig_c, prm_c = L.skeleton_rig_struct(r), L.skeleton_params_struct(params, track_rows=0 if tracks is None else tracks.shape[1])
    L.check(L.load().egotap_skeleton_fit(L.ptr(cut(points)), L.ptr(cut(tracks)), n_t, S, C.byref(rig_c), C.byref(prm_c), L.ptr(state_in), L.ptr(state_out),
                                         L.ptr(rigid), L.ptr(rotations), L.ptr(lengths), L.stream()))


def _compare(tag, got, want, points):
    g_rigid, g_rot, g_len = (t.detach().cpu().numpy() for t in got[:3])
    w_rigid, w_rot, w_len, w_state = want
    assert np.isfinite(g_rigid).all() and np.isfinite(g_rot).all() and np.isfinite(g_len).all(), tag
    _bits(g_rigid[..., 3], w_rigid[..., 3])                          # the flags
    no_pos, no_rot = (w_rigid[..., 3] % 2) == 0, w_rigid[..., 3] < 2
    _bits(g_rigid[no_pos], w_rigid[no_pos])                           # the all-zero records
    _bits(g_rot[no_rot], w_rot[no_rot])                               # the identity records
    assert (w_rigid[no_pos][:, :3] == 0).all() and (w_rot[no_rot] == np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32)).all()
    _bits(g_len[..., 1], w_len[..., 1])                               # n
    ulp2 = lambda top: 2.0 * np.spacing(np.asarray(top, dtype=np.float32)).astype(np.float64)      # noqa: E731
    fin = np.where(np.isfinite(points), np.abs(points), 0.0).astype(np.float64)
    top = np.maximum(fin.max(axis=(1, 2)), np.abs(w_rigid[..., :3]).max(axis=(1, 2)))[:, None, None]      # the frame's largest |coordinate|
    d_rigid, b_rigid = np.abs(g_rigid[..., :3].astype(np.float64) - w_rigid[..., :3]), ulp2(top)
    d_rot, b_rot = np.abs(g_rot.astype(np.float64) - w_rot), ulp2(1.0)
    d_len, b_len = np.abs(g_len[..., 0].astype(np.float64) - w_len[..., 0]), ulp2(np.abs(w_len[..., 0]))
    ratios = [(d_rigid / b_rigid).max(), (d_rot / b_rot).max(), (d_len / np.maximum(b_len, 1e-300)).max()]
    differ = int((g_rigid.view(np.int32) != w_rigid.view(np.int32)).sum() + (g_rot.view(np.int32) != w_rot.view(np.int32)).sum()
                 + (g_len.view(np.int32) != w_len.view(np.int32)).sum())
    if w_state is not None:
        g_state = got[3].detach().cpu().numpy()
        assert np.isfinite(g_state).all(), tag
        _bits(g_state[..., 1], w_state[..., 1])
        d_st, b_st = np.abs(g_state - w_state), 1e-13 * np.maximum(1.0, np.abs(w_state))
        ratios.append((d_st / b_st).max())
        differ += int((g_state.view(np.int64) != w_state.view(np.int64)).sum())
    print(tag, "largest deviation / bound: rigid", ratios[0], "rotations", ratios[1], "lengths", ratios[2], "state", ratios[3] if w_state is not None else "-",
          "| values that differ in any bit:", differ)
    assert (d_rigid <= b_rigid).all(), (tag, "rigid", ratios[0])
    assert (d_rot <= b_rot).all(), (tag, "rotations", ratios[1])
    assert (d_len <= b_len).all(), (tag, "lengths", ratios[2])
    assert w_state is None or (d_st <= b_st).all(), (tag, "state", ratios[3])


@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
@pytest.mark.parametrize("with_tracks", [False, True], ids=["no_tracks", "tracks"])
@pytest.mark.parametrize("fixed", [False, True], ids=["calibrating", "fixed_length"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_S%d_%s" % s)
def test_skeleton_fit_equals_the_float64_restatement(shape, fixed, with_tracks, mirror):
    T, S, kind = shape
    r, (pts, trk, state0), want = _expected(shape, fixed, with_tracks, mirror)
    B, P = T * S, r.P
    points, tracks, state_in = _dev(pts), _dev(trk), _dev(state0)
    rigid, ok_r = _between_canaries(B * P * 4)
    rotations, ok_q = _between_canaries(B * P * 8)
    lengths, ok_l = _between_canaries(B * P * 2)
    state_out, ok_s = _between_canaries(S * P * 2, dtype=torch.float64)
    _launch(r, I.PARAMS, points, tracks, S, state_in, None if fixed else state_out, rigid, rotations, lengths)
    torch.cuda.synchronize()
    tag = f"T={T} S={S} {kind} {'fixed_length' if fixed else 'calibrating'} tracks={'yes' if with_tracks else 'no'} mirror={'yes' if mirror else 'no'}"
    assert ok_r() and ok_q() and ok_l() and ok_s(), tag
    if fixed:
        assert bool((state_out == CANARY).all())                      # no state is written
    else:
        _bits(state_in, state0)                                       # out of place: the state read is not written
    got = (rigid.view(B, P, 4), rotations.view(B, P, 8), lengths.view(B, P, 2), None if fixed else state_out.view(S, P, 2))
    _compare(tag, got, want, pts)
    # the Python face: the same launch, the state in place
    st = None if fixed else state_in.clone()
    r2, q2, l2 = L.skeleton_fit(points, st, r, params=I.PARAMS, tracks=tracks, streams=S)
    torch.cuda.synchronize()
    for a, b in zip((r2, q2, l2), got):
        _bits(a, b)
    if not fixed:
        _bits(st, got[3])


def test_the_antiparallel_case_on_the_device_in_bits():
    r, x, want = antiparallel_case()
    points = _dev(x.astype(np.float32))
    state = torch.zeros(1, r.P, 2, dtype=torch.float64, device="cuda")
    rigid, rot, _ = L.skeleton_fit(points, state, r, params=spec.SkeletonParams(min_samples=1))
    torch.cuda.synchronize()
    assert (rigid[0, :, 3] == 3).all()
    _bits(rot[0, 0], np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float32))
    _bits(rot[0, 4], np.array(want + want, dtype=np.float32))
    _bits(rigid[0, 4, :3], np.array([-2, 0, 0], dtype=np.float32))
    for a, b in zip((rigid, rot), spec.skeleton_fit_ref(x, np.zeros((1, r.P, 2)), r, spec.SkeletonParams(min_samples=1))):
        _bits(a, b)


@pytest.mark.parametrize("with_tracks", [False, True], ids=["no_tracks", "tracks"])
def test_chunks_in_place_and_repeats_give_the_same_bits(with_tracks):
    T, S, kind = shape = (7, 1, "UnrealEgo")
    r, (pts, trk, state0), _ = _expected(shape, False, with_tracks, True)
    B, P = T * S, r.P
    points, tracks = _dev(pts), _dev(trk)

    def run(parts, in_place, start):
        st = _dev(start)
        rigid, rot, lens = torch.empty(B, P, 4, device="cuda"), torch.empty(B, P, 8, device="cuda"), torch.empty(B, P, 2, device="cuda")
        lo = 0
        for n_t in parts:
            nxt = st if in_place else torch.full_like(st, CANARY)
            _launch(r, I.PARAMS, points, tracks, S, st, nxt, rigid[lo * S:], rot[lo * S:], lens[lo * S:], t0=lo, n_t=n_t)
            st, lo = nxt, lo + n_t
        torch.cuda.synchronize()
        return rigid, rot, lens, st
    for start in (state0, np.zeros_like(state0)):
        whole = run([7], False, start)
        for parts, in_place in (([3, 1, 3], False), ([3, 1, 3], True), ([7], True), ([7], False), ([1] * 7, True)):
            again = run(parts, in_place, start)
            for a, b in zip(again, whole):
                _bits(a, b)


def test_ragged_last_workgroup_leaves_the_other_streams_alone():
    """S = 5 streams fill one workgroup and a quarter of the second: the three waves past S store nothing (every array ends where stream 4's does)"""
    T, S, kind = shape = (3, 5, "EgoCap")
    r, (pts, trk, state0), want = _expected(shape, False, True, False)
    P = r.P
    state, ok_s = _between_canaries(S * P * 2, dtype=torch.float64, pad=3 * P * 2)       # room for three more streams: none is written
    state.copy_(_dev(state0).view(-1))
    rigid, ok_r = _between_canaries(T * S * P * 4, pad=3 * P * 4)
    rot, ok_q = _between_canaries(T * S * P * 8, pad=3 * P * 8)
    lens, ok_l = _between_canaries(T * S * P * 2, pad=3 * P * 2 + 2)           # (+ 2 floats: the view stays 16-byte aligned)
    _launch(r, I.PARAMS, _dev(pts), _dev(trk), S, state, state, rigid, rot, lens)
    torch.cuda.synchronize()
    assert ok_s() and ok_r() and ok_q() and ok_l()
    _bits(state.view(S, P, 2)[..., 1], want[3][..., 1])
    assert np.abs(state.view(S, P, 2).cpu().numpy() - want[3]).max() <= 1e-13


# ------------------------------------------------------------------------------------------------------------ serving


def test_skeleton_behind_the_serving_call_and_the_trackers():
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
    tprm = spec.TrackParams(min_joints=1, max_hold=2)
    sprm = spec.SkeletonParams(window=3, min_samples=1)
    rigs = _dev(W.rigs(2 * B, 1, seed=5, bad=False))                  # the headset's pose of the four consecutive frames
    for world in (False, True):
        tracker, shadow = (m.new_pose_tracker(streams=1, params=tprm, world=world) for _ in range(2))
        skeleton = m.new_skeleton(streams=1, params=sprm)
        with pytest.raises(ValueError, match="no rig: the project ships no avatar"):
            skeleton.update(before[0][0])
        rig = skeleton.set_rest_pose(before[0][0][0])                  # the first frame's pose rows as the rest pose
        assert rig.P == P and tuple(skeleton.state.shape) == (1, P, 2) and skeleton.state.dtype == torch.float64 and not skeleton.state.any()
        state = torch.zeros_like(skeleton.state)
        outs = []
        for k, (l8, r8) in enumerate(frames):                         # two calls of T = 2 consecutive frames each
            pose, j3, fr = m.predict_pose_from_camera(l8, r8, return_triangulation=True)
            kw = dict(rig_pose=rigs[k * B:(k + 1) * B]) if world else {}
            res, want_res = tracker.update(pose, j3, fr, dt=1.0 / 30, **kw), shadow.update(pose, j3, fr, dt=1.0 / 30, **kw)
            placed, tracks = res[0], res[1]
            got = skeleton.update(placed, tracks)
            want = L.skeleton_fit(placed, state, rig, params=sprm, tracks=tracks, streams=1)
            torch.cuda.synchronize()
            assert tuple(got[0].shape) == (B, P, 4) and tuple(got[1].shape) == (B, P, 8) and tuple(got[2].shape) == (B, P, 2)
            for a, b in zip(got, want):
                _bits(a, b)
            _bits(skeleton.state, state)
            for a, b in zip((pose, j3, fr), before[k]):               # the serving call's own outputs: the skeleton changes nothing
                assert torch.equal(a, b), k
            for a, b in zip(res, want_res):                           # nor the tracker's
                _bits(a, b)
            _bits(tracker.state, shadow.state)
            outs.append(tuple(t.clone() for t in got))
            assert (got[0][:, :, 3] == 3).all()
            for t in range(B):                                        # n counts the frames so far, up to the window
                assert (got[2][t, 1:, 1] == min(B * k + t + 1, sprm.window)).all(), (k, t)
        assert m._rgb_state(dev).ws.numel() == ws_bytes and len(m._rgb_state(dev).graphs) == n_graphs
        # against the restatement, from the tensors the tracker returned
        tracker.reset()
        kw = dict(rig_pose=rigs[:B]) if world else {}
        res = tracker.update(*before[0], dt=1.0 / 30, **kw)
        want = spec.skeleton_fit_ref(res[0].cpu().numpy(), np.zeros((1, P, 2)), rig, sprm, tracks=res[1].cpu().numpy())
        _compare(f"serving world={world}", outs[0] + (torch.from_numpy(want[3]),), want, res[0].cpu().numpy())
        # reset: the next frame is a first frame again; frozen: the state stays and is used
        skeleton.reset()
        assert not skeleton.state.any()
        again = skeleton.update(res[0], res[1])
        for a, b in zip(again, outs[0]):
            _bits(a, b)
        kept = skeleton.state.clone()
        skeleton.freeze()
        frozen = skeleton.update(res[0], res[1])
        torch.cuda.synchronize()
        _bits(skeleton.state, kept)
        _bits(frozen[2][:, :, 1], again[2][1:, :, 1].expand(B, P).contiguous())
        skeleton.freeze(False)
        skeleton.reset(streams=[0])
        assert not skeleton.state.any()
        with pytest.raises(ValueError, match="streams are"):
            skeleton.reset(streams=[1])
    # the timing hook records the launch
    h = m._rgb_state(dev).handle.h
    lib = L.load()
    L.check(lib.egotap_timing_enable(h, 1))
    try:
        skeleton.update(res[0], res[1])
        n, ms, fl = C.c_int(), C.c_double(), C.c_double()
        L.check(lib.egotap_timing_read(h, C.byref(n), C.byref(ms), C.byref(fl)))
        detail = lib.egotap_timing_detail(h).decode()
    finally:
        L.check(lib.egotap_timing_enable(h, 0))
    assert n.value == 1 and '"role": "skeleton_fit"' in detail, detail
