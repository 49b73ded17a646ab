"""CPU-side checks of the temporal filter (egotap.h: egotap_pose_track): the float64 restatement spec.pose_track_ref pinned by closed forms that do
not depend on it -- a constant, a step, a ramp with and without the speed term, dropped frames against a longer dt, the hold / expiry sequence, the
root's gates, bad step times, chunking and stream permutation -- and the ABI's exports and refusals (fake pointers: nothing is launched)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import pose_track_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec

DT = 1.0 / 64
NK = spec.POSE_TRACK_STATE


def _alpha(fc, te):
    r = 2.0 * math.pi * fc * te
    return r / (r + 1.0)


def _run(m, params, dt=DT, state=None, **kw):
    """one pose track per column of m [T, P, 3] on one stream, float64 records"""
    m = np.asarray(m, dtype=np.float64)
    if state is None:
        state = np.zeros((1, m.shape[1] + 1, NK))
    return spec.pose_track_ref(m, state, dt, params, dtype="float64", **kw)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a.view(np.int64 if a.dtype == np.float64 else np.int32), b.view(np.int64 if a.dtype == np.float64 else np.int32))


# ------------------------------------------------------------------------------------------------ closed forms
def test_constant_input_comes_back_in_bits():
    x0 = np.array([0.3, -1.7, 2.0 / 3.0])
    tracks, placed, state = _run(np.tile(x0, (50, 1, 1)), spec.TrackParams())
    _bits(tracks[:, 0, 0:3], np.tile(x0, (50, 1)))
    assert (tracks[:, 0, 3:6] == 0).all() and (tracks[:, 0, 6] == 1.0).all() and (tracks[:, 0, 7] == 1).all()
    _bits(placed[:, 0], np.tile(x0, (50, 1)))                         # no frame: no root, the pose row alone
    assert (tracks[:, 1] == 0).all() and (state[0, 1] == 0).all()
    _bits(state[0, 0], np.concatenate([x0, np.zeros(3), x0, [0.0, 0.0, 1.0]]))


def test_step_response_is_the_exponential():
    x0, x1 = np.array([0.5, -2.0, 10.0]), np.array([1.5, 3.0, -7.0])
    n = 400
    m = np.concatenate([x0[None], np.tile(x1, (n, 1))])[:, None]
    tracks, _, _ = _run(m, spec.TrackParams.uniform(beta=0.0))
    a = _alpha(1.0, DT)
    want = x1 - (1.0 - a) ** np.arange(n + 1)[:, None] * (x1 - x0)
    err = np.abs(tracks[:, 0, 0:3] - want).max()
    print("step: max |x^ - closed form| =", err, "relative", err / np.abs(x1).max())
    assert err <= 1e-12 * np.abs(x1).max()
    assert (tracks[:, 0, 6] == 1.0).all()                             # beta = 0: the cutoff never moves


SLOPE = np.array([20.0, -25.0, 0.4])


def _ramp(beta, n=600):
    t = np.arange(n) * DT
    m = (np.array([1.0, 2.0, -3.0]) + SLOPE * t[:, None])[:, None]
    tracks, _, _ = _run(m, spec.TrackParams.uniform(beta=beta))
    return m[:, 0], tracks[:, 0]


def test_ramp_lag_and_velocity():
    m, rec = _ramp(0.0)
    a = _alpha(1.0, DT)
    lag = rec[500:, 0:3] - m[500:]
    print("ramp: max |lag - closed form| =", np.abs(lag - (-SLOPE * DT * (1.0 - a) / a)).max(), " max |v^ - s| =", np.abs(rec[500:, 3:6] - SLOPE).max())
    assert np.abs(lag - (-SLOPE * DT * (1.0 - a) / a)).max() <= 1e-9
    assert np.abs(rec[500:, 3:6] - SLOPE).max() <= 1e-9


def test_ramp_with_the_speed_term_opens_the_cutoff_and_shortens_the_lag():
    m, rec0 = _ramp(0.0)
    _, rec = _ramp(0.05)
    speed = float(np.sqrt((SLOPE * SLOPE).sum()))
    print("ramp, beta = 0.05: cutoff", rec[-1, 6], "against", 1.0 + 0.05 * speed, " lag", np.linalg.norm(rec[-1, 0:3] - m[-1]), "against",
          np.linalg.norm(rec0[-1, 0:3] - m[-1]))
    assert np.abs(rec[500:, 6] - (1.0 + 0.05 * speed)).max() <= 1e-9
    assert (np.linalg.norm(rec[500:, 0:3] - m[500:], axis=-1) < np.linalg.norm(rec0[500:, 0:3] - m[500:], axis=-1)).all()
    a = _alpha(1.0 + 0.05 * speed, DT)                                # and the lag is the closed form at the opened cutoff
    assert np.abs(rec[500:, 0:3] - m[500:] + SLOPE * DT * (1.0 - a) / a).max() <= 1e-9


def test_dropped_frames_equal_a_longer_dt_in_bits():
    rng = np.random.default_rng(3)
    m = rng.normal(0, 1, (20, 2, 3))
    prm = spec.TrackParams()
    holes = m.copy()
    holes[7, :, 0] = np.nan                                           # a pose row is rejected by being not finite
    holes[8, :, 2] = np.inf
    full = _run(holes, prm, dt=np.full(20, DT))
    assert (full[0][[7, 8], :2, 7] == 2).all() and (np.delete(full[0][:, :2, 7], [7, 8], axis=0) == 1).all()
    dts = np.full(18, DT)
    dts[7] = 3.0 / 64
    short = _run(np.delete(m, [7, 8], axis=0), prm, dt=dts)
    _bits(np.delete(full[0], [7, 8], axis=0), short[0])
    _bits(np.delete(full[1], [7, 8], axis=0), short[1])
    _bits(full[2], short[2])
    # held records repeat the last estimate with cutoff 0
    _bits(full[0][7, :, 0:6], full[0][6, :, 0:6])
    assert (full[0][[7, 8], :2, 6] == 0).all()


def test_hold_and_expiry_sequence():
    accept = np.array([0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1], dtype=bool)
    want = [0, 1, 1, 2, 2, 2, 1, 2, 2, 2, 0, 1, 1]
    T = len(accept)
    rng = np.random.default_rng(4)
    m = rng.normal(0, 1, (T, 3))
    pose = np.where(accept[:, None], m, np.nan)[:, None]              # the pose track: rejected = not finite
    frame = np.zeros((T, 8))
    frame[:, 0:3], frame[:, 3] = m + 1.0, np.where(accept, 5.0, 0.0)    # the root: rejected = too few joints
    frame[4, 0:3] = np.nan                                            # (a NaN inside a hold, here and in the joint)
    j3 = np.zeros((T, 1, 8))
    j3[:, 0, 0:3], j3[:, 0, 7] = m - 1.0, accept                      # the joint: rejected = not valid
    j3[8, 0, 0:3] = np.nan
    prm = spec.TrackParams(max_hold=3)
    tracks, placed, state = spec.pose_track_ref(pose, np.zeros((1, 3, NK)), DT, prm, frame=frame, joints3d=j3, dtype="float64")
    for k in range(3):
        assert tracks[:, k, 7].tolist() == want, (k, tracks[:, k, 7])
    assert np.isfinite(tracks).all() and np.isfinite(placed).all() and np.isfinite(state).all()
    assert (tracks[[0, 10]] == 0).all() and (placed[[0, 10]] == 0).all()
    for k, meas in enumerate((m, m + 1.0, m - 1.0)):                  # re-initialised: the measurement itself, at rest, at min_cutoff
        _bits(tracks[11, k, 0:3], meas[11])
        assert (tracks[11, k, 3:6] == 0).all() and tracks[11, k, 6] == 1.0
    # the state between: after step 10 the track is "never seen" again
    s10 = spec.pose_track_ref(pose[:11], np.zeros((1, 3, NK)), DT, prm, frame=frame[:11], joints3d=j3[:11], dtype="float64")[2]
    assert (s10 == 0).all()
    s9 = spec.pose_track_ref(pose[:10], np.zeros((1, 3, NK)), DT, prm, frame=frame[:10], joints3d=j3[:10], dtype="float64")[2]
    assert (s9[0, :, 10] == 3).all() and (s9[0, :, 11] == 1).all() and (s9[0, :, 9] == 3 * DT).all()
    # max_hold = 0: nothing is held
    t0 = spec.pose_track_ref(pose, np.zeros((1, 3, NK)), DT, spec.TrackParams(max_hold=0), frame=frame, joints3d=j3)[0]
    assert t0[:, 0, 7].tolist() == [0, 1, 1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 1]


def test_root_gates_and_placed():
    rng = np.random.default_rng(5)
    T, P = 4, 3
    pose = rng.normal(0, 1, (T, P, 3)).astype(np.float32)
    good = np.zeros((T, 8))
    good[:, 0:3], good[:, 3], good[:, 4], good[:, 6] = rng.normal(0, 1, (T, 3)), 3.0, 2.0 ** -5, 2.0 ** -6
    good = good.astype(np.float32)
    prm = spec.TrackParams(max_disagree=2.0 ** -5, max_gap=2.0 ** -6, min_joints=3)
    z = np.zeros((1, P + 1, NK))
    assert (spec.pose_track_ref(pose, z, DT, prm, frame=good)[0][:, P, 7] == 1).all()       # the thresholds themselves pass
    for col, val in ((3, 2.0), (1, np.nan), (0, np.inf), (4, np.nextafter(np.float32(2.0 ** -5), np.float32(1))), (6, np.nextafter(np.float32(2.0 ** -6), np.float32(1))), (4, np.nan), (6, np.nan), (3, np.nan)):
        bad = good.copy()
        bad[2, col] = val
        st = spec.pose_track_ref(pose, z, DT, prm, frame=bad)[0][:, P, 7]
        assert st.tolist() == [1, 1, 2, 1], (col, val, st)
    off = spec.TrackParams()                                           # +inf: the two rms gates are off, a NaN still fails
    wild = good.copy()
    wild[:, 4], wild[:, 6] = 1e30, np.inf
    assert (spec.pose_track_ref(pose, z, DT, off, frame=wild)[0][:, P, 7] == 1).all()
    # placed: the pose row alone without a root, pose + root in one rounding with it
    t64, p64, _ = spec.pose_track_ref(pose, z, DT, prm, dtype="float64")
    assert (t64[:, P] == 0).all()
    _bits(p64, t64[:, :P, 0:3])
    bad = good.copy()
    bad[0, 3] = 0.0                                                    # the first frame has no root yet
    t64, p64, _ = spec.pose_track_ref(pose, z, DT, prm, frame=bad, dtype="float64")
    t32, p32, _ = spec.pose_track_ref(pose, z, DT, prm, frame=bad)
    assert t64[:, P, 7].tolist() == [0, 1, 1, 1]
    _bits(p64[0], t64[0, :P, 0:3])
    _bits(p64[1:], t64[1:, :P, 0:3] + t64[1:, P:P + 1, 0:3])
    assert p32.dtype == np.float32 and t32.dtype == np.float32
    _bits(p32, p64.astype(np.float32))
    _bits(t32, t64.astype(np.float32))
    nanrow = pose.copy()
    nanrow[:, 1, 1] = np.nan                                           # a pose row that was never seen: zeros, whatever the root does
    assert (spec.pose_track_ref(nanrow, z, DT, prm, frame=good)[1][:, 1] == 0).all()


@pytest.mark.parametrize("bad", [0.0, -DT, np.nan, np.inf, -np.inf])
def test_a_bad_step_time_holds_and_adds_nothing(bad):
    rng = np.random.default_rng(6)
    m = rng.normal(0, 1, (4, 1, 3))
    prm = spec.TrackParams()
    tracks, _, state = _run(m[:2], prm, dt=np.array([DT, bad]))
    assert tracks[:, 0, 7].tolist() == [1, 2]
    _bits(tracks[1, 0, 0:6], tracks[0, 0, 0:6])
    assert state[0, 0, 9] == 0.0 and state[0, 0, 10] == 1.0 and state[0, 0, 11] == 1.0 and np.isfinite(state).all()
    _bits(state[0, 0, 6:9], m[0, 0])                                  # the sample of the held step was not read
    # the whole run equals the one with that step's frame missing and no time added
    a = _run(m, prm, dt=np.array([DT, bad, DT, DT]))
    b = _run(np.delete(m, 1, axis=0), prm, dt=np.array([DT, DT, DT]))
    _bits(np.delete(a[0], 1, axis=0), b[0])
    assert a[2][0, 0, 10] == 0.0
    _bits(a[2], b[2])
    # a first sample needs no dt
    assert _run(m[:1], prm, dt=np.array([bad]))[0][0, 0, 7] == 1
    with pytest.raises(ValueError, match="finite and > 0"):
        _run(m, prm, dt=bad)


def _compositions(n):
    for cuts in itertools.product((0, 1), repeat=n - 1):
        parts, run = [], 1
        for c in cuts:
            if c:
                parts.append(run)
                run = 1
            else:
                run += 1
        yield parts + [run]


def test_any_chunking_gives_the_bits_of_one_call():
    T, S, P, J = 7, 2, 5, 4
    pose, frame, j3, state0 = I.case(T, S, P, J, seed=8)
    dts = np.array([DT, 2 * DT, DT, 0.0, DT, DT / 2, DT], dtype=np.float32)
    whole = spec.pose_track_ref(pose, state0, dts, I.PARAMS, frame=frame, joints3d=j3, streams=S)
    assert set(whole[0][..., 7].ravel()) == {0.0, 1.0, 2.0}
    n = 0
    for parts in _compositions(T):
        st, lo, tr, pl = state0, 0, [], []
        for n_t in parts:
            sl = slice(lo * S, (lo + n_t) * S)
            t, p, st = spec.pose_track_ref(pose[sl], st, dts[lo:lo + n_t], I.PARAMS, frame=frame[sl], joints3d=j3[sl], streams=S)
            tr.append(t)
            pl.append(p)
            lo += n_t
        _bits(np.concatenate(tr), whole[0])
        _bits(np.concatenate(pl), whole[1])
        _bits(st, whole[2])
        n += 1
    assert n == 64


def test_permuting_the_streams_permutes_the_outputs():
    T, S, P, J = 5, 4, 6, 3
    pose, frame, j3, state0 = I.case(T, S, P, J, seed=9)
    perm = np.array([2, 0, 3, 1])

    def by_stream(a):
        return a.reshape((T, S) + a.shape[1:])[:, perm].reshape(a.shape)
    a = spec.pose_track_ref(pose, state0, DT, I.PARAMS, frame=frame, joints3d=j3, streams=S)
    b = spec.pose_track_ref(by_stream(pose), state0[perm], DT, I.PARAMS, frame=by_stream(frame), joints3d=by_stream(j3), streams=S)
    _bits(by_stream(a[0]), b[0])
    _bits(by_stream(a[1]), b[1])
    _bits(a[2][perm], b[2])
    assert not np.array_equal(a[0], b[0])


def test_the_shared_case_meets_every_branch():
    """the inputs the device tests use: from a state under way, every status follows every status somewhere, and every kind of reject occurs"""
    pose, frame, j3, state0 = I.case(7, 5, 17, 15, seed=1)
    assert (state0[..., 11] == 1).any() and (state0[..., 11] == 0).any() and (state0[..., 10] > 0).any() and (state0[..., 9] > 0).any()
    tracks = spec.pose_track_ref(pose, state0, DT, I.PARAMS, frame=frame, joints3d=j3, streams=5)[0].reshape(7, 5, 33, 8)
    seen = {(int(a), int(b)) for a, b in zip(tracks[:-1, ..., 7].ravel(), tracks[1:, ..., 7].ravel())}
    assert seen == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 1), (2, 2), (2, 0)}, seen       # (1 -> 0 needs max_hold = 0)
    assert np.isnan(pose).any() and np.isinf(pose).any() and np.isnan(frame).any() and np.isnan(j3).any() and (j3[..., 7] == 0).any()
    assert (j3[..., 3] > I.PARAMS.max_joint_gap).any() and (frame[:, 4] > I.PARAMS.max_disagree).any() and (frame[:, 6] > I.PARAMS.max_gap).any()


def test_params_and_restatement_refuse_by_name():
    for kw, word in ((dict(pose=(0.0, 0.0, 1.0)), "min_cutoff"), (dict(root=(1.0, -1.0, 1.0)), "beta"), (dict(joints=(1.0, 0.0, np.inf)), "d_cutoff"),
                     (dict(pose=(1.0, 0.0)), "3|got 2"), (dict(max_disagree=-1.0), "max_disagree"), (dict(max_gap=np.nan), "max_gap"),
                     (dict(max_joint_gap=-0.1), "max_joint_gap"), (dict(min_joints=-1), "min_joints"), (dict(max_hold=-1), "max_hold")):
        with pytest.raises(ValueError, match=word):
            spec.TrackParams(**kw)
    d = spec.TrackParams()
    assert d.pose == d.root == d.joints == (1.0, 0.007, 1.0) and d.max_disagree == d.max_gap == d.max_joint_gap == math.inf
    assert d.min_joints == 3 and d.max_hold == 8 and spec.POSE_TRACK_STATE == 12
    z = np.zeros((1, 3, NK))
    with pytest.raises(ValueError, match="pose is"):
        spec.pose_track_ref(np.zeros((3, 2, 3)), z, DT, streams=2)
    with pytest.raises(ValueError, match="state is"):
        spec.pose_track_ref(np.zeros((3, 2, 3)), np.zeros((1, 2, NK)), DT)
    with pytest.raises(ValueError, match="frame is"):
        spec.pose_track_ref(np.zeros((3, 2, 3)), z, DT, frame=np.zeros((2, 8)))
    with pytest.raises(ValueError, match="joints3d is"):
        spec.pose_track_ref(np.zeros((3, 2, 3)), z, DT, joints3d=np.zeros((3, 1, 4)))
    with pytest.raises(ValueError, match="dts holds"):
        spec.pose_track_ref(np.zeros((3, 2, 3)), z, np.full(2, DT))


# ------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entry_is_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    assert "egotap_pose_track" in L.exported_symbols() and hasattr(lib, "egotap_pose_track") and "int egotap_pose_track(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert C.sizeof(L.EgotapTrackParams) == 12 * 8 + 2 * 4
    o = L.track_params_struct(I.PARAMS)
    assert (o.pose_min_cutoff, o.pose_beta, o.pose_d_cutoff) == I.PARAMS.pose and (o.root_min_cutoff, o.root_beta, o.root_d_cutoff) == I.PARAMS.root
    assert (o.joints_min_cutoff, o.joints_beta, o.joints_d_cutoff) == I.PARAMS.joints and o.max_joint_gap == 0.03 and o.min_joints == 3 and o.max_hold == 2
    assert L.track_params_struct().max_gap == math.inf


def test_pose_track_refuses_by_name_before_any_launch():
    lib = L.load()
    V = C.c_void_p
    T, S, P, J = 3, 2, 16, 15
    B, K = T * S, P + 1 + J
    pose, frame, j3, dts, sin, sout, tracks, placed = (0x100000 * (k + 1) for k in range(8))
    nbytes = dict(pose=B * P * 12, frame=B * 32, j3=B * J * 32, dts=T * 4, sin=S * K * 96, sout=S * K * 96, tracks=B * K * 32, placed=B * P * 12)
    ok = dict(pose=V(pose), frame=V(frame), j3=V(j3), T=T, S=S, P=P, J=J, dts=V(dts), dt=0.0, prm=L.track_params_struct(), sin=V(sin), sout=V(sout),
              tracks=V(tracks), placed=V(placed))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_pose_track(a["pose"], a["frame"], a["j3"], a["T"], a["S"], a["P"], a["J"], a["dts"], a["dt"],
                                   C.byref(a["prm"]) if a["prm"] is not None else None, a["sin"], a["sout"], a["tracks"], a["placed"], None)
        return rc, lib.egotap_last_error().decode()

    def prm(**kw):
        o = L.track_params_struct()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    nan, inf = float("nan"), float("inf")
    cases = [(dict(pose=None), "null"), (dict(sin=None), "null"), (dict(sout=None), "null"), (dict(tracks=None), "null"), (dict(placed=None), "null"),
             (dict(prm=None), "params"),
             (dict(pose=V(pose + 2)), "pose"), (dict(frame=V(frame + 1)), "frame"), (dict(j3=V(j3 + 2)), "joints3d"), (dict(dts=V(dts + 3)), "dts"),
             (dict(placed=V(placed + 2)), "placed"), (dict(tracks=V(tracks + 8)), "tracks must be 16-byte"), (dict(tracks=V(tracks + 4)), "tracks must be 16-byte"),
             (dict(sin=V(sin + 4)), "state_in"), (dict(sout=V(sout + 4)), "state_out"),
             (dict(T=0), "T, S and P"), (dict(S=0), "T, S and P"), (dict(P=0), "T, S and P"), (dict(T=-1), "T, S and P"), (dict(P=65), "at most 64 pose rows"),
             (dict(J=-1), "J must be"), (dict(J=65), "J must be"), (dict(j3=None), "joints3d"), (dict(J=0), "joints3d"),
             (dict(dts=None, dt=0.0), "dt must be"), (dict(dts=None, dt=-1.0), "dt must be"), (dict(dts=None, dt=nan), "dt must be"), (dict(dts=None, dt=inf), "dt must be")]
    for c in spec.TRACK_CLASSES:
        cases += [(dict(prm=prm(**{f"{c}_min_cutoff": v})), f"{c}_min_cutoff") for v in (0.0, -1.0, nan, inf)]
        cases += [(dict(prm=prm(**{f"{c}_d_cutoff": v})), f"{c}_d_cutoff") for v in (0.0, nan, inf)]
        cases += [(dict(prm=prm(**{f"{c}_beta": v})), f"{c}_beta") for v in (-0.1, nan, inf)]
    for g in ("max_disagree", "max_gap", "max_joint_gap"):
        cases += [(dict(prm=prm(**{g: v})), g) for v in (nan, -1.0, -inf)]
    cases += [(dict(prm=prm(min_joints=-1)), "min_joints"), (dict(prm=prm(max_hold=-1)), "max_hold")]
    # an output on an input, or on another output: first byte, last byte
    for out in ("sout", "tracks", "placed"):
        name = {"sout": "state_out", "tracks": "tracks", "placed": "placed"}[out]
        for inp in ("pose", "frame", "j3", "dts", "sin"):
            if (out, inp) == ("sout", "sin"):
                continue
            cases += [({out: V(ok[inp].value)}, f"{name} overlaps"), ({out: V(ok[inp].value + (nbytes[inp] - 1) // 16 * 16)}, f"{name} overlaps"),
                      ({inp: V(ok[out].value + (nbytes[out] - 1) // 16 * 16)}, f"{name} overlaps")]
    cases += [(dict(tracks=V(sout + 96)), "state_out overlaps tracks"), (dict(placed=V(sout)), "state_out overlaps placed"),
              (dict(placed=V(tracks + nbytes["tracks"] - 16)), "tracks overlaps placed"),
              (dict(sout=V(sin + 96)), "state_out overlaps state_in"), (dict(sout=V(sin - 8)), "state_out overlaps state_in")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_pose_track:") and word in msg, (kw, rc, msg)
    # +inf gates, the gate 0, beta 0, max_hold 0, dts given with any dt: not refused for those (the first refusal is a later one, made on purpose)
    fine = prm(max_disagree=inf, max_gap=0.0, max_joint_gap=inf, pose_beta=0.0, max_hold=0, min_joints=0)
    rc, msg = call(prm=fine, dt=nan, tracks=V(tracks + 8))
    assert rc == 1 and "tracks must be 16-byte" in msg


def test_python_face_checks_its_arguments_without_a_gpu():
    import torch
    P, J = 16, 15
    pose, state = torch.zeros(4, P, 3), torch.zeros(2, P + 1 + J, 12, dtype=torch.float64)
    j3, frame = torch.zeros(4, J, 8), torch.zeros(4, 8)
    with pytest.raises(ValueError, match="pose is a tensor"):
        L.pose_track(torch.zeros(4, P, 2), state, dt=0.1, streams=2)
    with pytest.raises(ValueError, match="pose is a tensor"):
        L.pose_track(torch.zeros(5, P, 3), state, dt=0.1, streams=2)
    with pytest.raises(ValueError, match="64 pose rows"):
        L.pose_track(torch.zeros(4, 65, 3), state, dt=0.1, streams=2)
    with pytest.raises(ValueError, match="joints3d is a tensor"):
        L.pose_track(pose, state, dt=0.1, joints3d=torch.zeros(4, J, 4), streams=2)
    with pytest.raises(ValueError, match="joints3d is a tensor"):
        L.pose_track(pose, state, dt=0.1, joints3d=torch.zeros(2, J, 8), streams=2)
    with pytest.raises(ValueError, match="frame is a tensor"):
        L.pose_track(pose, state, dt=0.1, joints3d=j3, frame=torch.zeros(4, 4), streams=2)
    with pytest.raises(ValueError, match="state is a contiguous float64"):
        L.pose_track(pose, state.float(), dt=0.1, joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="state is a contiguous float64"):
        L.pose_track(pose, state, dt=0.1, streams=2)                   # no joints: K = P + 1
    with pytest.raises(ValueError, match="exactly one of dt"):
        L.pose_track(pose, state, joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="exactly one of dt"):
        L.pose_track(pose, state, dt=0.1, dts=torch.zeros(2), joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="dts is a float32 tensor"):
        L.pose_track(pose, state, dts=torch.zeros(3), joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="dts is a float32 tensor"):
        L.pose_track(pose, state, dts=torch.zeros(2, dtype=torch.float64), joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="dt must be finite"):
        L.pose_track(pose, state, dt=0.0, joints3d=j3, streams=2)
    with pytest.raises(ValueError, match="min_cutoff"):
        L.pose_track(pose, state, dt=0.1, joints3d=j3, streams=2, params=spec.TrackParams(pose=(-1.0, 0.0, 1.0)))
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.pose_track(pose, state, dt=0.1, joints3d=j3, frame=frame, streams=2)
    from egotap_amd import models
    tr = models.PoseTracker(P, J, streams=2)
    with pytest.raises(ValueError, match="pose is a tensor"):
        tr.update(torch.zeros(4, P + 1, 3), dt=0.1)
    with pytest.raises(ValueError, match="joints3d is a tensor"):
        tr.update(pose, joints3d=torch.zeros(4, J + 1, 8), dt=0.1)
    with pytest.raises(L.EgotapError, match="GPU only"):
        tr.update(pose, j3, frame, dt=0.1)
    with pytest.raises(ValueError, match="streams"):
        models.PoseTracker(P, J, streams=0)
    tr.reset()                                                         # before the first update: nothing to forget
