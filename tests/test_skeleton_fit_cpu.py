"""The float64 restatement of the skeleton fit (spec.skeleton_fit_ref) against closed forms that do not depend on it -- forward kinematics, recovery of a
generated articulation, the length recurrence, missing data, the antiparallel branch, chunking and stream permutation -- and the ABI's export and refusals
(fake pointers: nothing is launched).  Each tolerance is an upper bound from float64 rounding; the value seen on this code stands beside it."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import skeleton_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec

IDENT = (1.0, 0.0, 0.0, 0.0)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    view = np.int64 if a.dtype == np.float64 else np.int32
    assert np.array_equal(a.view(view), b.view(view)), np.argwhere(a.view(view) != b.view(view))[:8]


def _run(points, rig, params=None, state=None, streams=1, **kw):
    st = np.zeros((streams, rig.P, 2)) if state is None and rig.fixed_length is None else state
    return spec.skeleton_fit_ref(points, st, rig, params, streams=streams, dtype="float64", **kw)


def _sign_ok(q):
    w, x, y, z = q
    return w > 0 or (w == 0 and (x > 0 or (x == 0 and (y > 0 or (y == 0 and z > 0)))))


# ------------------------------------------------------------------------------------------------ forward kinematics
@pytest.mark.parametrize("kind", ["UnrealEgo", "EgoCap"])
def test_the_outputs_alone_rebuild_the_skeleton(kind):
    """root position + local quaternions chained from the root + rest_dir + lengths give rigid to 1e-12 max|coordinate| (seen: 2e-15 relative);
    rotate(Q_j, rest_dir_j) == u_j to 1e-12 (seen: 4e-16); every quaternion has norm 1 to 1e-12 (seen: 4e-16) and obeys the sign rule"""
    r = I.rig(kind, mirror=True)
    x = I.articulated(r, 6, 11, max_angle=3.0, jitter=0.05)[0]
    rigid, rot, lens, _ = _run(x, r)
    assert (rigid[..., 3] == 3).all()
    worst = [0.0, 0.0, 0.0]
    for t in range(6):
        Q, pos = [None] * r.P, np.zeros((r.P, 3))
        for j, p in enumerate(r.parents):
            if p < 0:
                Q[j], pos[j] = tuple(rot[t, j, 4:]), rigid[t, j, :3]
            else:
                Q[j] = spec.quat_mul(Q[p], tuple(rot[t, j, 4:]))
                d = np.array(spec.quat_rotate(Q[j], tuple(r.rest_dir[j])))
                pos[j] = pos[p] + lens[t, j, 0] * d
                u = (x[t, j] - x[t, p]) / np.linalg.norm(x[t, j] - x[t, p])
                worst[1] = max(worst[1], np.abs(np.array(spec.quat_rotate(tuple(rot[t, j, :4]), tuple(r.rest_dir[j]))) - u).max())
        worst[0] = max(worst[0], np.abs(pos - rigid[t, :, :3]).max() / np.abs(rigid[t, :, :3]).max())
        q = rot[t].reshape(-1, 4)
        worst[2] = max(worst[2], np.abs(np.sqrt((q * q).sum(axis=1)) - 1).max())
        assert all(_sign_ok(v) for v in q)
    print(kind, "rebuild / max|coordinate|", worst[0], "rotate(Q, rest) - u", worst[1], "norm - 1", worst[2])
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-12


# ------------------------------------------------------------------------------------------------ recovery
@pytest.mark.parametrize("kind", I.KINDS)
def test_a_generated_articulation_comes_back(kind):
    """rest pose, scaled bones, a root rotation W and shortest-arc swings below 170 degrees on every bone but those leading to a, b, c: Q_root = W and
    local = the swing to 1e-12 (seen: 4e-14, the 64-row chain), the identity on the unarticulated bones, rigid = the input (1e-12 max|coordinate|;
    seen 2e-15) and lengths = the scaled lengths to 1e-13 relative (seen: 2e-15)"""
    r = I.rig(kind)
    n = 4
    x, Ws, locs, lens = I.articulated(r, n, 5, max_angle=math.radians(169.0), rigid_frame=True)
    rigid, rot, got_len, _ = _run(x, r)
    assert (rigid[..., 3] == 3).all()
    keep = I.leads_to_frame(r)
    roots = [j for j, p in enumerate(r.parents) if p < 0]
    worst_q = worst_l = 0.0
    for t in range(n):
        for j in range(r.P):
            want = Ws[t] if j in roots else locs[t][j]
            worst_q = max(worst_q, np.abs(np.array(want) - rot[t, j, 4:]).max())
            if j in keep:
                assert np.abs(rot[t, j, 4:] - np.array(IDENT)).max() <= 1e-12
        worst_q = max(worst_q, np.abs(np.array(Ws[t]) - rot[t, roots[0], :4]).max())
        bone = np.array(r.parents) >= 0
        worst_l = max(worst_l, (np.abs(got_len[t, bone, 0] - lens[t, bone]) / lens[t, bone]).max())
    print(kind, "quaternion", worst_q, "length rel", worst_l, "rigid", np.abs(rigid[..., :3] - x).max() / np.abs(x).max())
    assert worst_q <= 1e-12 and worst_l <= 1e-13
    assert np.abs(rigid[..., :3] - x).max() <= 1e-12 * np.abs(x).max()


# ------------------------------------------------------------------------------------------------ calibration
def _one_bone(lengths, direction=(0.6, 0.0, 0.8)):
    """a star rig and one pose per entry of ``lengths`` [n, P]: row j sits lengths[., j] from the root along its rest direction"""
    r = I.rig("star64")
    n = len(lengths)
    x = np.zeros((n, r.P, 3))
    for j in range(1, r.P):
        x[:, j] = np.asarray(lengths)[:, j, None] * r.rest_dir[j]
    return r, x


def test_constant_lengths_come_back_in_bits_from_the_first_frame():
    r = I.rig("UnrealEgo")
    x1 = I.articulated(r, 1, 3)[0]
    x = np.repeat(x1, 5, axis=0)
    _, _, lens, st = _run(x, r, spec.SkeletonParams(window=3, min_samples=0 + 1))
    for t in range(1, 5):
        _bits(lens[t, :, 0], lens[0, :, 0])
    ell = np.array([math.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])) for d in (x1[0] - x1[0][list(max(p, 0) for p in r.parents)])])
    _bits(st[0, 1:, 0], ell[1:])
    assert (st[0, 1:, 1] == 3).all() and (st[0, 0] == 0).all()


def test_jittered_lengths_are_the_mean_then_the_exponential_average():
    """n <= window: the arithmetic mean to 1e-13 relative (seen: 4e-16); past the window L_k = L_(k-1) + (l_k - L_(k-1)) / window, computed here"""
    rng = np.random.default_rng(2)
    window, n = 6, 15
    base = rng.uniform(0.2, 0.6, 64)
    seq = base[None] * (1.0 + 0.05 * rng.normal(size=(n, 64)))
    r, x = _one_bone(seq)
    prm = spec.SkeletonParams(window=window, min_samples=2)
    st = np.zeros((1, 64, 2))
    ells = np.zeros((n, 64))
    worst = 0.0
    for k in range(n):
        d = x[k] - x[k, 0]
        ells[k] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        _, _, lens, st = _run(x[k:k + 1], r, prm, state=st)
        if k < window:
            mean = ells[:k + 1, 1:].mean(axis=0)
            worst = max(worst, (np.abs(st[0, 1:, 0] - mean) / mean).max())
            assert (st[0, 1:, 1] == k + 1).all()
        else:
            want = want + (ells[k, 1:] - want) / window
            _bits(st[0, 1:, 0], want)
            assert (st[0, 1:, 1] == window).all()
        if k == window - 1:
            want = st[0, 1:, 0].copy()
        _bits(lens[0, 1:, 0], st[0, 1:, 0])
    print("mean rel", worst)
    assert worst <= 1e-13


def test_outliers_freeze_and_mirror():
    seq = np.full((6, 64), 0.5)
    seq[2, 5] = 0.9                         # before min_samples: averaged in
    seq[4, 5] = 0.9                         # after: beyond max_dev 0.5 of ~0.63, rejected
    seq[:, 6] = 0.25
    r, x = _one_bone(seq)
    prm = spec.SkeletonParams(window=100, min_samples=3, max_dev=0.3)
    outs = [_run(x[:k], r, prm) for k in range(1, 7)]
    s3, s4, s5, s6 = (o[3] for o in outs[2:])
    assert s3[0, 5, 1] == 3 and abs(s3[0, 5, 0] - (0.5 + 0.5 + 0.9) / 3) < 1e-15
    assert s4[0, 5, 1] == 4
    _bits(s5[0, 5], s4[0, 5])               # the outlier leaves the state in bits ...
    assert s5[0, 7, 1] == 5 and s6[0, 5, 1] == 5
    o5 = outs[4]
    assert o5[0][4, 5, 3] == 3 and abs(o5[2][4, 5, 0] - s4[0, 5, 0]) == 0      # ... and the step still uses the length
    want = s4[0, 5, 0] * np.asarray(r.rest_dir[5])
    assert np.abs(o5[0][4, 5, :3] - want).max() <= 1e-15
    # freeze: the state stays in bits, the outputs go on using it
    frozen = spec.SkeletonParams(window=100, min_samples=3, max_dev=0.3, freeze=True)
    rg, _, ln, st = _run(x[4:], r, frozen, state=s4)
    _bits(st, s4)
    _bits(ln[:, :, 0], np.broadcast_to(s4[0, :, 0], (2, 64)).copy())
    assert (rg[..., 3] == 3).all()
    # mirror: both sides get equal bits, the mean of the two
    parents, frame_rows, mir = I.tree("star64")
    rm = spec.skeleton_rig(parents, r.rest_pos, frame_rows, mirror=mir)
    _, _, ln, st = _run(x[:2], rm, prm)
    assert mir[6] == 7 and abs(st[0, 6, 0] - 0.25) < 1e-15 and abs(st[0, 7, 0] - 0.5) < 1e-15
    _bits(ln[:, 6], ln[:, 7])
    assert ln[1, 6, 0] == 0.5 * (st[0, 6, 0] + st[0, 7, 0]) and ln[1, 5, 0] == st[0, 5, 0]


def test_fixed_length_scales_the_skeleton_and_keeps_the_rotations():
    """rigid_j - rigid_root is k times the k = 1 value to 1e-12 relative (seen: 3e-16), rotations equal in bits, no state"""
    x = I.articulated(I.rig("UnrealEgo"), 3, 9, jitter=0.1)[0]
    r1, r3 = I.rig("UnrealEgo", fixed_scale=1.0), I.rig("UnrealEgo", fixed_scale=2.5)
    a, b = _run(x, r1), _run(x, r3)
    assert a[3] is None and b[3] is None
    _bits(a[1], b[1])
    da, db = a[0][:, :, :3] - a[0][:, :1, :3], b[0][:, :, :3] - b[0][:, :1, :3]
    rel = np.abs(db - 2.5 * da).max() / np.abs(db).max()
    print("fixed_length scale rel", rel)
    assert rel <= 1e-12
    _bits(b[2][:, 1:, 0], np.broadcast_to(2.5 * r1.rest_len[1:], (3, 15)).copy())
    assert (b[2][..., 1] == 0).all() and (b[0][..., 3] == 3).all()
    state = np.full((1, 16, 2), 7.0)
    assert spec.skeleton_fit_ref(x, state, r3, dtype="float64")[3] is None and (state == 7.0).all()


# ------------------------------------------------------------------------------------------------ missing data
def test_a_missing_row_zeroes_its_subtree_and_nothing_else():
    r = I.rig("UnrealEgo")
    x = I.articulated(r, 2, 4)[0]
    prm = spec.SkeletonParams(min_samples=1)
    st0 = _run(x[:1], r, prm)[3]
    base = _run(x[1:], r, prm, state=st0)
    K = r.P + 2
    tracks = np.ones((1, K, 8))
    for j in (4, 9):                                                    # lowerarm_l: hand_l below it; thigh_r: calf_r, foot_r, ball_r
        gone = I.subtree(r, j)
        bad = x[1:].copy()
        bad[0, j, 1] = np.nan
        trk = tracks.copy()
        trk[0, j, 7] = 0.0
        for got in (_run(bad, r, prm, state=st0), _run(x[1:], r, prm, state=st0, tracks=trk)):
            for k in range(r.P):
                if k in gone:
                    _bits(got[0][0, k], np.zeros(4))
                    _bits(got[1][0, k], np.array(IDENT + IDENT))
                else:
                    _bits(got[0][0, k], base[0][0, k])
                    _bits(got[1][0, k], base[1][0, k])
            others = [k for k in range(r.P) if k not in gone]
            ends = [k for k in range(r.P) if k == j or r.parents[k] == j]      # the bones with the missing row at one end: no sample, their state stays
            _bits(got[3][0, ends], st0[0, ends])
            rest = [k for k in range(r.P) if k not in ends]             # (a bone further down still has both ends: it is sampled, and not placed)
            _bits(got[3][0, rest], base[3][0, rest])
            _bits(got[2][0, others], base[2][0, others])
    held = tracks.copy()
    held[0, :, 7] = 2.0                                                 # a held track counts as seen
    for a, b in zip(_run(x[1:], r, prm, state=st0, tracks=held), base):
        _bits(a, b)


def test_a_missing_or_collinear_triangle_turns_every_rotation_off():
    parents = (-1, 0, 0, 0, 0)
    rest = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, -1)]
    r = spec.skeleton_rig(parents, rest, (1, 2, 3))
    x = np.array(rest, dtype=np.float64)[None]
    rigid, rot, _, _ = _run(x, r, spec.SkeletonParams(min_samples=1))
    assert (rigid[0, :, 3] == 3).all()
    _bits(rot[0], np.tile(np.array(IDENT + IDENT), (5, 1)))          # the rest pose itself: every rotation the identity, in bits
    for row in (1, 2, 3):
        bad = x.copy()
        bad[0, row, 0] = np.inf
        rigid, rot, _, _ = _run(bad, r, spec.SkeletonParams(min_samples=1))
        assert list(rigid[0, :, 3]) == [1.0 if k != row else 0.0 for k in range(5)]
        _bits(rot[0], np.tile(np.array(IDENT + IDENT), (5, 1)))
    flat = x.copy()
    flat[0, 1] = (0.5, 0.0, 0.0)                                      # a on the line through b and c
    rigid, rot, _, _ = _run(flat, r, spec.SkeletonParams(min_samples=1))
    assert (rigid[0, :, 3] == 1).all()
    _bits(rigid[0, :, :3], flat[0])
    same = x.copy()
    same[0, 3] = same[0, 2]                                             # b == c: the first norm is zero
    assert (_run(same, r, spec.SkeletonParams(min_samples=1))[0][0, :, 3] == 1).all()
    # a child on its parent: an invalid sample -- no position, no rotation, no update
    on = x.copy()
    on[0, 4] = on[0, 0]
    rigid, _, lens, st = _run(on, r, spec.SkeletonParams(min_samples=1))
    assert list(rigid[0, :, 3]) == [3, 3, 3, 3, 0] and (st[0, 4] == 0).all() and (lens[0, 4] == 0).all()


# ------------------------------------------------------------------------------------------------ the antiparallel branch
def antiparallel_case():
    """an axis-aligned rig whose rest pose is its own frame (Q_root = identity in bits) and a pose with row 4 exactly opposite its rest direction
    (1, 0, 0): k = 1 (the lowest index of the smallest |v_k|), axis = (1, 0, 0) x (0, 1, 0) = (0, 0, 1), a half turn about z"""
    parents = (-1, 0, 0, 0, 0)
    rest = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (2, 0, 0)]
    r = spec.skeleton_rig(parents, rest, (1, 2, 3))
    x = np.array(rest, dtype=np.float64)[None]
    x[0, 4] = (-2.0, 0.0, 0.0)
    return r, x, (0.0, 0.0, 0.0, 1.0)


def test_the_antiparallel_branch_in_bits():
    r, x, want = antiparallel_case()
    rigid, rot, _, _ = _run(x, r, spec.SkeletonParams(min_samples=1))
    assert (rigid[0, :, 3] == 3).all()
    _bits(rot[0, 0], np.array(IDENT + IDENT))
    _bits(rot[0, 4], np.array(want + want))
    assert spec.quat_rotate(want, (1.0, 0.0, 0.0)) == (-1.0, 0.0, 0.0)
    _bits(rigid[0, 4, :3], np.array([-2.0, 0.0, 0.0]))
    # just above the threshold: the regular branch (w > 0), and the quaternion still maps v to u
    th = 2e-6
    x[0, 4] = (-2.0 * math.cos(th), 2.0 * math.sin(th), 0.0)
    c = -math.cos(th)
    assert spec.SKELETON_ANTIPARALLEL < c < -1 + 1e-11
    q = _run(x, r, spec.SkeletonParams(min_samples=1))[1][0, 4, :4]
    assert q[0] > 0 and abs(q[0] - math.sin(th / 2)) < 1e-10
    assert np.abs(np.array(spec.quat_rotate(tuple(q), (1.0, 0.0, 0.0))) - x[0, 4] / 2.0).max() < 1e-9
    for v in ((0.0, 0.0, 1.0), (0.0, -1.0, 0.0), (0.6, 0.0, -0.8)):    # the other axes' ties and a general direction
        s = spec.quat_shortest_arc(v, tuple(-a for a in v))
        assert s[0] == 0.0 and np.abs(np.array(spec.quat_rotate(s, v)) + np.array(v)).max() <= 1e-15


# ------------------------------------------------------------------------------------------------ structure
def _compositions(n):
    for k in range(n):
        for cuts in itertools.combinations(range(1, n), k):
            edges = (0,) + cuts + (n,)
            yield [b - a for a, b in zip(edges, edges[1:])]


def test_any_chunking_gives_the_bits_of_one_call():
    T, S = 7, 2
    r, pts, trk, st0 = I.case("UnrealEgo", T, S, mirror=True, with_tracks=True)
    whole = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S)
    keep = st0.copy()
    for parts in _compositions(T):
        st, lo, outs = st0, 0, []
        for n in parts:
            o = spec.skeleton_fit_ref(pts[lo * S:(lo + n) * S], st, r, I.PARAMS, tracks=trk[lo * S:(lo + n) * S], streams=S)
            outs.append(o[:3])
            st, lo = o[3], lo + n
        for k in range(3):
            _bits(np.concatenate([o[k] for o in outs]), whole[k])
        _bits(st, whole[3])
    _bits(st0, keep)                                                    # the state given is not written
    assert not np.array_equal(whole[3], st0)


def test_permuting_the_streams_permutes_the_outputs():
    T, S = 3, 5
    r, pts, trk, st0 = I.case("EgoCap", T, S, with_tracks=True)
    perm = np.array([3, 0, 4, 1, 2])
    a = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S)
    sh = lambda v: v.reshape(T, S, *v.shape[1:])[:, perm].reshape(v.shape)      # noqa: E731
    b = spec.skeleton_fit_ref(sh(pts), st0[perm], r, I.PARAMS, tracks=sh(trk), streams=S)
    for k in range(3):
        _bits(b[k], sh(a[k]))
    _bits(b[3], a[3][perm])


def test_the_shared_case_meets_every_branch():
    """what the device test relies on: in the mixed case every kind of sample occurs and no ok rotation is near the antiparallel branch
    (local w = cos(angle / 2) > 0.0708 is v . u > -0.99)"""
    for kind, T, S in (("UnrealEgo", 7, 1), ("EgoCap", 3, 5), ("chain64", 2, 4), ("star64", 2, 4), ("UnrealEgo", 1, 9)):
        for mirror, with_tracks in itertools.product((False, True), repeat=2):
            r, pts, trk, st0 = I.case(kind, T, S, mirror, with_tracks)
            rigid, rot, lens, st = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S, dtype="float64")
            ok = rigid[..., 3] >= 2
            bone = np.array(r.parents) >= 0
            assert rot[ok & bone[None], 4].min() > 0.0708, kind
            if kind == "star64" or (kind, T) == ("UnrealEgo", 1):
                continue
            flags = set(rigid[..., 3].ravel())
            assert {0.0, 3.0} <= flags, (kind, flags)
            assert not np.isfinite(pts).all() and (st0[:, bone, 1] >= 1).all()
            assert (st[:, bone, 1] < st0[:, bone, 1] + T).any()         # some valid sample was rejected or missing


def test_rig_params_and_restatement_refuse_by_name():
    par, rest = (-1, 0, 0, 0, 1), [(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 2, 0)]
    ok = spec.skeleton_rig(par, rest, (1, 2, 3), mirror=(-1, -1, 3, 2, -1), fixed_length=[0, 1, 1, 1, 2])
    assert ok.depth == (0, 1, 1, 1, 2) and ok.fixed_length[0] == 0
    for kw, word in ((dict(parents=(-1, 0, 3, 0, 1)), "earlier row"), (dict(parents=(-1, 0, 0, 0, 5)), "earlier row"), (dict(parents=(-1, 0, 0, -2, 1)), "earlier row"),
                     (dict(parents=()), "1 .. 64 rows"), (dict(parents=(-1,) + (0,) * 64), "1 .. 64 rows"),
                     (dict(frame_rows=(1, 2, 5)), "three distinct rows"), (dict(frame_rows=(1, 2, 2)), "three distinct rows"), (dict(frame_rows=(1, 2)), "three distinct"),
                     (dict(rest_pos=rest[:4]), "rest_pos is"), (dict(rest_pos=[(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0)]), "rest bone of row 4"),
                     (dict(rest_pos=[(0, 0, 0), (0, 1, 0), (1, 0, 0), (math.nan, 0, 0), (0, 2, 0)]), "finite"),
                     (dict(rest_pos=[(0, 0, 0), (0.5, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 2, 0)]), "degenerate"),
                     (dict(mirror=(-1, -1, 3, -1, -1)), "involution"), (dict(mirror=(-1, -1, 7, 2, -1)), "involution"), (dict(mirror=(-1, -1, 3)), "one row per row"),
                     (dict(fixed_length=[0, 1, 0, 1, 2]), "fixed_length[2]"), (dict(fixed_length=[0, 1, math.inf, 1, 2]), "fixed_length[2]"),
                     (dict(fixed_length=[0, 1, 1]), "one length per row")):
        args = dict(dict(parents=par, rest_pos=rest, frame_rows=(1, 2, 3)), **kw)
        with pytest.raises(ValueError, match="skeleton_rig: .*" + word.replace("[", r"\[").replace("]", r"\]")):
            spec.skeleton_rig(**args)
    with pytest.raises(ValueError, match="no root row"):
        spec.skeleton_rig((0, 0), [(0, 0, 0), (1, 0, 0)], (0, 1, 1))
    with pytest.raises(ValueError, match="pairs a root row"):
        spec.skeleton_rig((-1, -1, 0, 0, 0), rest, (2, 3, 4), mirror=(1, 0, -1, -1, -1))
    for kw, word in ((dict(window=0), "window"), (dict(min_samples=-1), "min_samples"), (dict(max_dev=-0.1), "max_dev"), (dict(max_dev=math.nan), "max_dev")):
        with pytest.raises(ValueError, match="SkeletonParams: " + word):
            spec.SkeletonParams(**kw)
    assert spec.SkeletonParams() == spec.SkeletonParams(120, 10, math.inf, False)
    with pytest.raises(ValueError, match="joint_preset"):
        spec.skeleton_parents("Human36M")
    assert spec.skeleton_parents("UnrealEgo") == (-1, 0, 1, 1, 2, 3, 4, 5, 2, 3, 8, 9, 10, 11, 12, 13)
    assert spec.skeleton_parents("EgoCap") == (-1, 0, 1, 2, 3, 0, 5, 6, 7, 1, 9, 10, 11, 5, 13, 14, 15)
    for preset in ("UnrealEgo", "EgoCap"):
        m = spec.SKELETON_MIRROR[preset]
        assert all(v == -1 or m[v] == j for j, v in enumerate(m))
        rg = spec.skeleton_rig_from_pose(preset, I.rest_pose(preset) + 3.0)
        assert rg.mirror == m and rg.frame_rows == spec.SKELETON_FRAME_ROWS[preset] and np.abs(rg.rest_pos - I.rest_pose(preset)).max() < 1e-15
    with pytest.raises(ValueError, match="one frame"):
        spec.skeleton_rig_from_pose("UnrealEgo", np.zeros((17, 3)))
    r = I.rig("UnrealEgo")
    x = np.zeros((4, 16, 3))
    for args, kw, word in (((x[:, :15], np.zeros((1, 16, 2)), r), {}, "points is"), ((x[:3], np.zeros((2, 16, 2)), r), dict(streams=2), "points is"),
                           ((x, np.zeros((2, 16, 3)), r), dict(streams=2), "state is"), ((x, None, r), {}, "state is"),
                           ((x, np.zeros((1, 16, 2)), r), dict(tracks=np.zeros((4, 15, 8))), "tracks is"), ((x, np.zeros((1, 16, 2)), "rig"), {}, "rig is")):
        with pytest.raises(ValueError, match="skeleton_fit_ref: " + word):
            spec.skeleton_fit_ref(*args, **kw)


# ------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entry_is_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    assert "egotap_skeleton_fit" in L.exported_symbols() and hasattr(lib, "egotap_skeleton_fit") and "int egotap_skeleton_fit(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert C.sizeof(L.EgotapSkeletonRig) == 2584 < 4096 and C.sizeof(L.EgotapSkeletonParams) == 24
    assert "2584 bytes" in text and "TWIST" in text
    r = I.rig("EgoCap", mirror=True, fixed_scale=2.0)
    o = L.skeleton_rig_struct(r)
    assert (o.P, o.has_mirror, o.has_fixed_length, tuple(o.frame_rows)) == (17, 1, 1, (0, 9, 13))
    assert tuple(o.parent[:17]) == r.parents and tuple(o.mirror[:17]) == r.mirror and o.fixed_length[5] == 2.0 * r.rest_len[5]
    assert tuple(o.rest_pos[16]) == tuple(r.rest_pos[16])
    p = L.skeleton_params_struct(I.PARAMS, track_rows=20)
    assert (p.window, p.min_samples, p.max_dev, p.freeze, p.track_rows) == (8, 3, 0.5, 0, 20) and L.skeleton_params_struct().max_dev == math.inf


def test_skeleton_fit_refuses_by_name_before_any_launch():
    lib = L.load()
    V = C.c_void_p
    T, S, P = 3, 2, 16
    B, K = T * S, P + 3
    points, tracks, sin, sout, rigid, rot, lens = (0x100000 * (k + 1) for k in range(7))
    nbytes = dict(points=B * P * 12, tracks=B * K * 32, sin=S * P * 16, sout=S * P * 16, rigid=B * P * 16, rot=B * P * 32, lens=B * P * 8)
    rig0 = I.rig("UnrealEgo", mirror=True)
    ok = dict(points=V(points), tracks=V(tracks), T=T, S=S, rig=L.skeleton_rig_struct(rig0), prm=L.skeleton_params_struct(track_rows=K), sin=V(sin), sout=V(sout),
              rigid=V(rigid), rot=V(rot), lens=V(lens))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_skeleton_fit(a["points"], a["tracks"], a["T"], a["S"], C.byref(a["rig"]) if a["rig"] is not None else None,
                                     C.byref(a["prm"]) if a["prm"] is not None else None, a["sin"], a["sout"], a["rigid"], a["rot"], a["lens"], None)
        return rc, lib.egotap_last_error().decode()

    def rig(fixed=False, **kw):
        o = L.skeleton_rig_struct(I.rig("UnrealEgo", mirror=True, fixed_scale=1.0 if fixed else None))
        for k, v in kw.items():
            if isinstance(v, dict):
                for i, x in v.items():
                    if isinstance(x, tuple):
                        getattr(o, k)[i][:] = x
                    else:
                        getattr(o, k)[i] = x
            else:
                setattr(o, k, v)
        return o

    def prm(**kw):
        o = L.skeleton_params_struct(track_rows=K)
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    nan, inf = float("nan"), float("inf")
    cases = [(dict(points=None), "null"), (dict(rig=None), "null"), (dict(prm=None), "null"), (dict(rigid=None), "null"), (dict(rot=None), "null"),
             (dict(lens=None), "null"), (dict(sin=None), "state_in and state_out are required"), (dict(sout=None), "state_in and state_out are required"),
             (dict(points=V(points + 2)), "points and tracks must be 4-byte"), (dict(tracks=V(tracks + 1)), "points and tracks must be 4-byte"),
             (dict(rigid=V(rigid + 8)), "16-byte"), (dict(rot=V(rot + 4)), "16-byte"), (dict(lens=V(lens + 8)), "16-byte"),
             (dict(sin=V(sin + 4)), "8-byte"), (dict(sout=V(sout + 4)), "8-byte"),
             (dict(T=0), "T, S and P"), (dict(S=0), "T, S and P"), (dict(T=-1), "T, S and P"), (dict(rig=rig(P=0)), "T, S and P"), (dict(rig=rig(P=65)), "at most 64 rows"),
             (dict(rig=rig(parent={3: 3})), "parent[3] = 3"), (dict(rig=rig(parent={3: 7})), "parent[3] = 7"), (dict(rig=rig(parent={3: -2})), "parent[3] = -2"),
             (dict(rig=rig(parent={0: 0})), "no root row"), (dict(rig=rig(parent={0: 0, 1: -1})), "parent[0] = 0"),
             (dict(rig=rig(frame_rows={2: 16})), "frame_rows"), (dict(rig=rig(frame_rows={2: -1})), "frame_rows"), (dict(rig=rig(frame_rows={2: 2})), "frame_rows"),
             (dict(rig=rig(rest_pos={5: (nan, 0.0, 0.0)})), "rest_pos[5][0]"), (dict(rig=rig(rest_pos={5: tuple(rig0.rest_pos[3])})), "rest bone of row 5"),
             (dict(rig=rig(rest_pos={1: tuple(0.5 * (rig0.rest_pos[2] + rig0.rest_pos[3]))})), "degenerate"),
             (dict(rig=rig(mirror={4: 6})), "mirror[4] = 6 is not an involution"), (dict(rig=rig(mirror={4: 16})), "involution"), (dict(rig=rig(mirror={4: -2})), "involution"),
             (dict(rig=rig(mirror={0: 1, 1: 0})), "pairs a root row"),
             (dict(rig=rig(fixed=True, fixed_length={3: 0.0})), "fixed_length[3]"), (dict(rig=rig(fixed=True, fixed_length={3: inf})), "fixed_length[3]"),
             (dict(rig=rig(fixed=True, fixed_length={3: nan})), "fixed_length[3]"), (dict(rig=rig(fixed=True, fixed_length={3: -1.0})), "fixed_length[3]"),
             (dict(prm=prm(window=0)), "window"), (dict(prm=prm(min_samples=-1)), "min_samples"), (dict(prm=prm(max_dev=nan)), "max_dev"),
             (dict(prm=prm(max_dev=-0.5)), "max_dev"), (dict(prm=prm(track_rows=P - 1)), "track_rows")]
    no_root = rig()
    no_root.P = 1
    no_root.parent[0] = 0
    cases.append((dict(rig=no_root), "no root row"))
    # an output on an input, or on another output: first byte, last byte
    names = dict(sout="state_out", rigid="rigid", rot="rotations", lens="lengths")
    for out in names:
        for inp in ("points", "tracks", "sin"):
            if (out, inp) == ("sout", "sin"):
                continue
            cases += [({out: V(ok[inp].value)}, f"{names[out]} overlaps"), ({out: V(ok[inp].value + (nbytes[inp] - 1) // 16 * 16)}, f"{names[out]} overlaps"),
                      ({inp: V(ok[out].value + (nbytes[out] - 1) // 16 * 16)}, f"{names[out]} overlaps")]
    cases += [(dict(rigid=V(sout + 16)), "state_out overlaps rigid"), (dict(rot=V(rigid + nbytes["rigid"] - 16)), "rigid overlaps rotations"),
              (dict(lens=V(rot)), "rotations overlaps lengths"), (dict(sout=V(sin + 16)), "state_out overlaps state_in"),
              (dict(sout=V(sin - 8)), "state_out overlaps state_in")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_skeleton_fit:") and word in msg, (kw, rc, msg)
    # what is NOT refused (the first refusal is a later one, made on purpose): NULL states and tracks with fixed_length, track_rows 0, window 1,
    # min_samples 0, max_dev +inf and 0, a mirror of -1 everywhere, state_out == state_in
    fine = prm(window=1, min_samples=0, max_dev=inf, track_rows=0)
    for kw in (dict(rig=rig(fixed=True), sin=None, sout=None, tracks=None), dict(rig=rig(has_mirror=0)), dict(sout=V(sin)), dict(prm=prm(max_dev=0.0))):
        rc, msg = call(**dict(dict(prm=fine), **kw, lens=V(lens + 8)))
        assert rc == 1 and "16-byte" in msg, (kw, msg)


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch

    from egotap_amd import models
    r = I.rig("UnrealEgo")
    pts, state = torch.zeros(4, 16, 3), torch.zeros(2, 16, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="rig is a spec.SkeletonRig"):
        L.skeleton_fit(pts, state, "rig", streams=2)
    with pytest.raises(ValueError, match="params is a spec.SkeletonParams"):
        L.skeleton_fit(pts, state, r, params=spec.TrackParams(), streams=2)
    with pytest.raises(ValueError, match="points is a tensor"):
        L.skeleton_fit(torch.zeros(4, 16, 2), state, r, streams=2)
    with pytest.raises(ValueError, match="points is a tensor"):
        L.skeleton_fit(torch.zeros(5, 16, 3), state, r, streams=2)
    with pytest.raises(ValueError, match="the rig has P = 16 rows, points has 17"):
        L.skeleton_fit(torch.zeros(4, 17, 3), state, r, streams=2)
    with pytest.raises(ValueError, match="points is a contiguous float32"):
        L.skeleton_fit(pts.double(), state, r, streams=2)
    with pytest.raises(ValueError, match="points is a contiguous float32"):
        L.skeleton_fit(torch.zeros(4, 3, 16).transpose(1, 2), state, r, streams=2)
    with pytest.raises(ValueError, match="tracks is a tensor"):
        L.skeleton_fit(pts, state, r, tracks=torch.zeros(4, 15, 8), streams=2)
    with pytest.raises(ValueError, match="tracks is a contiguous float32"):
        L.skeleton_fit(pts, state, r, tracks=torch.zeros(4, 32, 16)[:, :, :8], streams=2)
    with pytest.raises(ValueError, match="state is a contiguous float64"):
        L.skeleton_fit(pts, state.float(), r, streams=2)
    with pytest.raises(ValueError, match="state is a contiguous float64"):
        L.skeleton_fit(pts, state, r, streams=1)
    with pytest.raises(ValueError, match="reads and writes no state"):
        L.skeleton_fit(pts, state, I.rig("UnrealEgo", fixed_scale=1.0), streams=2)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.skeleton_fit(pts, state, r, streams=2)
    sk = models.Skeleton(16, joint_preset="UnrealEgo", streams=2)
    with pytest.raises(ValueError, match="no rig: the project ships no avatar"):
        sk.update(pts)
    with pytest.raises(ValueError, match="the rig has P = 17 rows"):
        models.Skeleton(16, rig=I.rig("EgoCap"))
    with pytest.raises(ValueError, match="streams must be at least 1"):
        models.Skeleton(16, streams=0)
    with pytest.raises(ValueError, match="one frame"):
        sk.set_rest_pose(torch.zeros(2, 16, 3))
    assert sk.set_rest_pose(torch.from_numpy(I.rest_pose("UnrealEgo"))).mirror == spec.SKELETON_MIRROR["UnrealEgo"]
    with pytest.raises(L.EgotapError, match="GPU only"):
        sk.update(pts)
    sk.freeze()
    assert sk.params.freeze and sk._structs[1].freeze == 1
    sk.freeze(False)
    assert not sk.params.freeze and sk._structs[1].freeze == 0
    sk.reset()                                                          # no state yet: nothing to forget
