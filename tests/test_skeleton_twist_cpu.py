"""The float64 restatement of the bone twist (spec.skeleton_fit_twist_ref, spec.skeleton_twist, spec.skeleton_hinges_from_pose) against closed forms
that do not depend on it -- equality with spec.skeleton_fit_ref where no twist can be observed, a generated articulation with known rolls, a pure
flexion of an elbow, the two thresholds, continuity over the ramp, the half turn, missing data, chunking, the calibration's round trip -- and the ABI's
export and refusals (fake pointers: nothing is launched).  Each tolerance is an upper bound from float64 rounding or is derived where it stands; the
value seen on this code stands beside it."""
import ctypes as C
import math

import numpy as np
import pytest

import skeleton_inputs as I
import skeleton_twist_inputs as TI
from egotap_amd import lib as L
from egotap_amd import spec
from test_skeleton_fit_cpu import _bits, _compositions, _sign_ok

IDENT = (1.0, 0.0, 0.0, 0.0)
PRM1 = spec.SkeletonParams(min_samples=1)


def _plain(points, rig, params=None, state=None, streams=1, **kw):
    st = np.zeros((streams, rig.P, 2)) if state is None and rig.fixed_length is None else state
    return spec.skeleton_fit_ref(points, st, rig, params, streams=streams, dtype="float64", **kw)


def _twisted(points, rig, tw, params=None, state=None, streams=1, **kw):
    st = np.zeros((streams, rig.P, 2)) if state is None and rig.fixed_length is None else state
    return spec.skeleton_fit_twist_ref(points, st, rig, tw, params, streams=streams, dtype="float64", **kw)


def _qdist(a, b):
    """the distance of two unit quaternions as rotations: q and -q are the same rotation"""
    a, b = np.asarray(a), np.asarray(b)
    return min(np.abs(a - b).max(), np.abs(a + b).max())


# ------------------------------------------------------------------------------------------------ where nothing can be observed
@pytest.mark.parametrize("kind", ["UnrealEgo", "chain64"])
def test_without_pole_rows_or_below_bend_lo_it_is_skeleton_fit_in_bits(kind):
    T, S = 3, 2
    r, pts, trk, st0 = I.case(kind, T, S, mirror=True, with_tracks=True)
    want = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S)
    none = spec.skeleton_twist(r, {})
    assert none.pole == (-1,) * r.P and not none.g.any()
    top = np.nanmax(TI.bends(r, TI.pole_rows(kind), pts))
    assert top < 1.0 - 1e-9                                             # every bend of the data lies below this bend_lo
    high = TI.table(kind, r, bend_lo=1.0 - 1e-9, bend_hi=1.0)
    for tw in (none, high):
        got = spec.skeleton_fit_twist_ref(pts, st0, r, tw, I.PARAMS, tracks=trk, streams=S)
        for a, b in zip(got, want):
            _bits(a, b)
        assert set(got[0][..., 3].ravel()) <= {0.0, 1.0, 2.0, 3.0}      # (2, a rotation without a position, is skeleton_fit's own: a root row not seen)
        # where skeleton_fit gives no 2 (every root row seen, every length there): the flags stay in {0, 1, 3}
        x = I.articulated(r, 3, 6)[0]
        x[1, r.P - 1, 0] = np.nan                                       # a leaf is missing in one frame,
        x[2, list(r.frame_rows)[0]] = np.inf                            # a frame row in another: positions without rotations
        rigid = _twisted(x, r, tw, PRM1)[0]
        assert set(rigid[..., 3].ravel()) == {0.0, 1.0, 3.0}
        _bits(rigid, _plain(x, r, PRM1)[0])
    # the star has no row that could have a pole: a root row has no bone, a leaf no child
    star = I.rig("star64")
    for j, c in ((0, 1), (1, 2)):
        with pytest.raises(ValueError, match="skeleton_twist: pole"):
            spec.skeleton_twist(star, {j: c}, np.ones((64, 3)))


@pytest.mark.parametrize("kind", ["UnrealEgo", "EgoCap", "chain64"])
def test_positions_lengths_and_state_do_not_depend_on_the_twist(kind):
    T, S = 3, 2
    r, pts, trk, st0 = I.case(kind, T, S, mirror=True, with_tracks=True)
    tw = TI.table(kind, r)
    want = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S)
    got = spec.skeleton_fit_twist_ref(pts, st0, r, tw, I.PARAMS, tracks=trk, streams=S)
    _bits(got[0][..., :3], want[0][..., :3])
    _bits(got[2], want[2])
    _bits(got[3], want[3])
    flags = got[0][..., 3]
    assert set(flags.ravel()) <= {0.0, 1.0, 2.0, 3.0, 6.0, 7.0} and (flags == 7).any()
    _bits(np.minimum(flags, 3.0), want[0][..., 3])                     # the twist adds 4 and nothing else
    assert not np.array_equal(got[1], want[1])
    poled = np.array([c >= 0 for c in tw.pole])
    assert not (flags[:, ~poled] == 7).any()


@pytest.mark.parametrize("kind", ["UnrealEgo", "EgoCap", "chain64"])
def test_every_rotation_is_a_unit_quaternion_that_takes_the_rest_bone_to_the_bone(kind):
    """rotate(Q_j, rest_dir_j) = u_j to 1e-12 on every ok row, twisted or below a twisted row (seen: 5e-15; the chain 1.4e-14); norms to 1e-12 (4e-16)"""
    r = I.rig(kind)
    tw = TI.table(kind, r, bend_lo=spec.SKELETON_BEND_LO, bend_hi=spec.SKELETON_BEND_HI)
    x = I.articulated(r, 5, 21, max_angle=2.5)[0]
    rigid, rot, _, _ = _twisted(x, r, tw)
    assert (rigid[..., 3] >= 3).all() and (rigid[..., 3] == 7).any()
    worst = [0.0, 0.0]
    for t in range(5):
        for j, p in enumerate(r.parents):
            if p >= 0:
                u = (x[t, j] - x[t, p]) / np.linalg.norm(x[t, j] - x[t, p])
                worst[0] = max(worst[0], np.abs(np.array(spec.quat_rotate(tuple(rot[t, j, :4]), tuple(r.rest_dir[j]))) - u).max())
                # local is the parent's rotation undone
                back = spec.quat_mul(tuple(rot[t, p, :4]), tuple(rot[t, j, 4:]))
                assert _qdist(back, rot[t, j, :4]) <= 1e-12
        q = rot[t].reshape(-1, 4)
        worst[1] = max(worst[1], np.abs(np.sqrt((q * q).sum(axis=1)) - 1).max())
        assert all(_sign_ok(v) for v in q)
    print(kind, "rotate(Q, rest) - u", worst[0], "norm - 1", worst[1])
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


# ------------------------------------------------------------------------------------------------ recovery
@pytest.mark.parametrize("kind", ["UnrealEgo", "EgoCap", "chain64"])
def test_a_generated_articulation_with_rolls_comes_back(kind):
    """A rest pose bent by 40 degrees at every pole joint (its own hinges), a root rotation W, a swing AND a roll on every pole row that is no pole
    child, a flexion about the parent's hinge on every pole child (the bend stays past bend_hi), swings elsewhere.  Every pole row is observed, with
    rotate(Q_j, g_j) . n_j >= 1 - 1e-12 (seen: 1 - 7e-16), and -- the closed form -- the GLOBAL rotation of every row equals the generated one, roll
    included, to 1e-12 as rotations (seen: 6e-16; 2e-15 down the 64-row chain).  Without the twist step the same data misses the rolls (by 0.9)."""
    r, pole = TI.bent_rig(kind)
    tw = spec.skeleton_twist(r, pole)                                  # the hinges from the rest pose itself
    n = 4
    x, Qs = TI.rolled_articulation(r, pole, tw, n, 17)
    assert np.nanmin(TI.bends(r, pole, x)[:, list(pole)]) >= spec.SKELETON_BEND_HI
    rigid, rot, _, _ = _twisted(x, r, tw)
    plain = _plain(x, r)[1]
    worst_n, worst_q, miss = 1.0, 0.0, 0.0
    for t in range(n):
        for j, p in enumerate(r.parents):
            assert rigid[t, j, 3] == (7 if j in pole else 3), (t, j)
            worst_q = max(worst_q, _qdist(Qs[t][j], rot[t, j, :4]))
            miss = max(miss, _qdist(Qs[t][j], plain[t, j, :4]))
            if j in pole:
                c = pole[j]
                uj, uc = (x[t, j] - x[t, p]) / np.linalg.norm(x[t, j] - x[t, p]), (x[t, c] - x[t, j]) / np.linalg.norm(x[t, c] - x[t, j])
                nrm = np.cross(uj, uc) / np.linalg.norm(np.cross(uj, uc))
                worst_n = min(worst_n, float(np.dot(spec.quat_rotate(tuple(rot[t, j, :4]), tuple(tw.g[j])), nrm)))
    print(kind, "1 - rotate(Q, g) . n", 1.0 - worst_n, "global quaternion", worst_q, "without the twist", miss)
    assert worst_n >= 1.0 - 1e-12 and worst_q <= 1e-12
    assert kind == "chain64" or miss > 0.1                              # (the chain has no rolled row: all its pole rows are pole children)


def test_a_pure_flexion_of_the_elbow_is_a_rotation_about_its_hinge():
    """The arm of skeleton_twist_inputs: the body turned by W, the upper arm swung and ROLLED about its own axis, then the elbow flexed by theta about
    its hinge g = +z and nothing else.  The forearm's local quaternion is (cos theta/2, sin theta/2 g) to 1e-12 (seen: 6e-16) -- the hinge in the rest
    pose's coordinates, which is what a joint limit or a retargeting step reads.  egotap_skeleton_fit on the same data misses it by the roll: the upper
    arm follows its parent there and the forearm's swing absorbs the difference (seen: 0.15 in a component at the least)."""
    r = TI.arm_rig()
    tw = spec.skeleton_twist(r, TI.ARM_POLE)
    assert np.abs(tw.g[4] - np.array(TI.ARM_HINGE)).max() <= 1e-15
    rng = np.random.default_rng(5)
    upper = spec.quat_mul(I.swing(rng, r.rest_dir[4], 1.2), TI.axis_angle(r.rest_dir[4], 0.9))
    W = I.random_rotation(rng)
    worst, miss = 0.0, 1.0
    for theta in (-0.2, 0.0, 0.3, 0.8, 1.3):                            # the bend is 40 degrees + theta: 28.5 .. 114.5 degrees, past sin 25 degrees
        x, Q = TI.arm_pose(r, upper, theta, W)
        want = TI.axis_angle(TI.ARM_HINGE, theta)
        rigid, rot, _, _ = _twisted(x[None], r, tw)
        assert rigid[0, 4, 3] == 7 and (rigid[0, [5, 6], 3] == 3).all()
        worst = max(worst, np.abs(rot[0, 5, 4:] - np.array(spec.quat_sign(want))).max(), _qdist(rot[0, 4, :4], Q[4]), np.abs(rot[0, 6, 4:] - IDENT).max())
        miss = min(miss, np.abs(_plain(x[None], r)[1][0, 5, 4:] - np.array(spec.quat_sign(want))).max())
    print("flexion: local - (cos, sin g)", worst, "| without the twist step", miss)
    assert worst <= 1e-12
    assert miss > 0.1


# ------------------------------------------------------------------------------------------------ the thresholds
def _arm_sigma(r, x):
    """sigma of the elbow as the restatement takes it, from float64 positions"""
    u = []
    for j in (4, 5):
        d = tuple(float(x[j, i]) - float(x[r.parents[j], i]) for i in range(3))
        n = spec._sk_norm3(d)
        u.append((d[0] / n, d[1] / n, d[2] / n))
    return spec._sk_norm3(spec._sk_cross(u[0], u[1]))


def test_at_bend_lo_nothing_is_observed_and_at_bend_hi_everything():
    r = TI.arm_rig()
    upper = spec.quat_mul(I.swing(np.random.default_rng(8), r.rest_dir[4], 1.0), TI.axis_angle(r.rest_dir[4], -0.7))
    x, Q = TI.arm_pose(r, upper, 0.1)
    sigma = _arm_sigma(r, x)
    assert 0.7 < sigma < 0.8
    plain = _plain(x[None], r)
    hinge = np.zeros((7, 3))
    hinge[4] = TI.ARM_HINGE

    def run(lo, hi):
        return _twisted(x[None], r, spec.skeleton_twist(r, TI.ARM_POLE, hinge, bend_lo=lo, bend_hi=hi))
    at_lo = run(sigma, 0.9)                                             # sigma > bend_lo is false: not observed, skeleton_fit's bits
    assert at_lo[0][0, 4, 3] == 3
    for a, b in zip(at_lo, plain):
        _bits(a, b)
    above = run(math.nextafter(sigma, 0.0), 0.9)                        # one ulp further: observed, with a weight of about 1e-31
    assert above[0][0, 4, 3] == 7 and _qdist(above[1][0, 4, :4], plain[1][0, 4, :4]) <= 1e-15
    at_hi, past = run(0.1, sigma), run(0.1, 0.5 * sigma)                # sigma >= bend_hi: w = 1 exactly, the bits of any lower bend_hi
    assert at_hi[0][0, 4, 3] == 7
    for a, b in zip(at_hi, past):
        _bits(a, b)
    assert _qdist(at_hi[1][0, 4, :4], Q[4]) <= 1e-12                     # ... and the whole roll is taken
    below = run(0.1, math.nextafter(sigma, 1.0))                        # one ulp short of bend_hi: w = 1 - 3e-32 rounds to ... at most an ulp off
    assert _qdist(below[1][0, 4, :4], Q[4]) <= 1e-12
    half = run(2.0 * sigma - 0.9, 0.9)                                  # the middle of the ramp: w = 1/2, b bisects h' and n
    assert 0.0 < 2.0 * sigma - 0.9
    norm = lambda a, b: min(np.linalg.norm(np.asarray(a) - b), np.linalg.norm(np.asarray(a) + b))      # noqa: E731
    d_full, d_half = norm(Q[4], half[1][0, 4, :4]), norm(plain[1][0, 4, :4], half[1][0, 4, :4])
    assert abs(d_full - d_half) <= 1e-9 and d_full > 0.05, (d_full, d_half)      # (w = 1/2 to a few ulp: 2 sigma - 0.9 is rounded)


def test_the_rotation_is_continuous_over_the_ramp():
    """The elbow of the arm flexes so that the sine of its bend runs from bend_lo to bend_hi in 200 equal steps; body and upper arm stand still, and
    the table's hinge stands alpha = 1 rad off the bend normal.  h' and n do not move then, only w does, and Q_4 = tw (x) Q_s with Q_s fixed, so
    |dQ_4| = |d tw| (multiplying by a unit quaternion keeps distances).  tw turns h' by the angle beta of b = normalize((1 - w) h' + w n):
    d beta / d w = sin(alpha) / |(1 - w) h' + w n|^2 <= sin(alpha) / cos^2(alpha / 2) = 2 tan(alpha / 2), the norm being smallest at w = 1/2;
    a quaternion of angle beta moves by at most |d beta| / 2 (it holds the half angle, and a chord is shorter than its arc); the smoothstep's
    slope is at most 1.5 / (bend_hi - bend_lo) per unit sine, and a step is (bend_hi - bend_lo) / 200 of sine.  Together
        |Q_4(i + 1) - Q_4(i)| <= (1 / 2) 2 tan(alpha / 2) 1.5 / 200 = 0.0075 tan(alpha / 2) = 4.0973e-3 for alpha = 1,
    plus 1e-12 for rounding and for the sines of the steps, which the positions (built with sin and cos) meet to 1e-14 only.  Seen: 4.0970e-3, at
    the middle of the ramp, where both slopes are at their largest: the bound is the supremum.  The whole sweep moves Q_4 by 2 sin(alpha / 4) =
    0.495, so the largest step cannot be below 1/200 of that: the bound is within a factor 1.7 of the least any rule could reach."""
    r = TI.arm_rig()
    alpha, steps = 1.0, 200
    lo, hi = spec.SKELETON_BEND_LO, spec.SKELETON_BEND_HI
    # the upper arm is swung and not rolled, so Q_s is its true rotation and n = rotate(Q_s, +z); the table's hinge is +z rolled by -alpha about the
    # rest bone, so h' stands alpha off n
    upper = I.swing(np.random.default_rng(2), r.rest_dir[4], 0.8)
    rolled = spec.quat_rotate(TI.axis_angle(r.rest_dir[4], -alpha), TI.ARM_HINGE)
    hinge = np.zeros((7, 3))
    hinge[4] = rolled
    tw = spec.skeleton_twist(r, TI.ARM_POLE, hinge, bend_lo=lo, bend_hi=hi)
    poses = []
    for i in range(steps + 1):
        sine = lo + (hi - lo) * i / steps
        poses.append(TI.arm_pose(r, upper, math.asin(sine) - TI.REST_BEND)[0])
    x = np.array(poses)
    sig = np.array([_arm_sigma(r, p) for p in x])
    assert np.abs(sig - (lo + (hi - lo) * np.arange(steps + 1) / steps)).max() <= 1e-14
    rigid, rot, _, _ = _twisted(x, r, tw)
    plain = _plain(x, r)[1]
    q = rot[:, 4, :4]
    assert (rigid[1:, 4, 3] == 7).all() and rigid[0, 4, 3] in (3, 7)
    jumps = np.array([min(np.linalg.norm(q[i] - q[i + 1]), np.linalg.norm(q[i] + q[i + 1])) for i in range(steps)])      # (as rotations: q = -q)
    bound = 0.5 * 2.0 * math.tan(alpha / 2.0) * 1.5 / steps + 1e-12
    print("largest step", jumps.max(), "at", int(jumps.argmax()), "bound", bound, "whole sweep", np.linalg.norm(q[0] - q[-1]), "=", 2 * math.sin(alpha / 4))
    assert jumps.max() <= bound
    assert _qdist(q[0], plain[0, 4, :4]) <= 1e-12                         # it starts at the untwisted rotation ...
    assert abs(np.linalg.norm(q[0] - q[-1]) - 2.0 * math.sin(alpha / 4.0)) <= 1e-9      # ... and ends a roll of alpha away
    assert np.abs(plain[:, 4, :4] - plain[0, 4, :4]).max() <= 1e-12       # Q_s stood still


# ------------------------------------------------------------------------------------------------ edge cases
def half_turn_case():
    """an axis-aligned arm whose rest pose is its own frame (Q_root = identity in bits): upper arm row 4 along +x, forearm row 5 along +y, hinge +z.
    The pose keeps the upper arm and bends the forearm to -y: Q_s is the identity, h' = +z, n = x x (-y) = -z, w = 1, b = n = -h', k = -1: the half turn
    about the bone, tw = (0, 1, 0, 0) = Q_4; it takes the forearm's rest direction +y to -y, so the forearm's swing is the identity"""
    parents = (-1, 0, 0, 0, 0, 4)
    rest = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (2, 0, 0), (2, 1, 0)]
    r = spec.skeleton_rig(parents, rest, (1, 2, 3))
    x = np.array(rest, dtype=np.float64)[None]
    x[0, 5] = (2.0, -1.0, 0.0)
    return r, spec.skeleton_twist(r, {4: 5}), x, (0.0, 1.0, 0.0, 0.0)


def test_the_half_turn_is_about_the_bone_in_bits():
    r, tw, x, want = half_turn_case()
    assert tuple(tw.g[4]) == (0.0, 0.0, 1.0)
    rigid, rot, _, _ = _twisted(x, r, tw, PRM1)
    assert list(rigid[0, :, 3]) == [3, 3, 3, 3, 7, 3]
    _bits(rot[0, 4], np.array(want + want))                             # global and, the parent being the identity, local
    assert np.array_equal(rot[0, 5, :4], np.array(want)) and np.array_equal(rot[0, 5, 4:], np.array(IDENT))
    assert spec.quat_rotate(want, (1.0, 0.0, 0.0)) == (1.0, 0.0, 0.0)   # the bone stays, the hinge turns over
    assert spec.quat_rotate(want, (0.0, 0.0, 1.0)) == (0.0, 0.0, -1.0)
    # without the step the upper arm does not move and the forearm takes the half turn about an axis of its own choosing
    plain = _plain(x, r, PRM1)[1]
    _bits(plain[0, 4], np.array(IDENT + IDENT))
    assert plain[0, 5, 0] == 0.0


def test_a_missing_pole_child_leaves_the_row_as_skeleton_fit_has_it():
    r = I.rig("UnrealEgo")
    tw = TI.table("UnrealEgo", r, bend_lo=0.01, bend_hi=0.02)
    x = I.articulated(r, 2, 4, max_angle=1.2)[0]
    st0 = _plain(x[:1], r, PRM1)[3]
    base, plain = _twisted(x[1:], r, tw, PRM1, state=st0), _plain(x[1:], r, PRM1, state=st0)
    assert (base[0][0, list(TI.pole_rows("UnrealEgo")), 3] == 7).all()
    tracks = np.ones((1, r.P + 2, 8))
    for j, c in ((4, 6), (10, 12)):                                     # the left elbow; the left knee, whose child is a pole row itself
        nan, on, off = x[1:].copy(), x[1:].copy(), tracks.copy()
        nan[0, c, 2] = np.nan
        on[0, I.subtree(r, c)] += x[1, j] - x[1, c]                     # the child on its parent: a zero-length bone, its subtree moved along
        off[0, c, 7] = 0.0
        for got, ref in ((_twisted(nan, r, tw, PRM1, state=st0), _plain(nan, r, PRM1, state=st0)),
                         (_twisted(on, r, tw, PRM1, state=st0), _plain(on, r, PRM1, state=st0)),
                         (_twisted(x[1:], r, tw, PRM1, state=st0, tracks=off), _plain(x[1:], r, PRM1, state=st0, tracks=off))):
            assert got[0][0, j, 3] == 3 and got[0][0, c, 3] in (0, 1)
            _bits(got[1][0, j], ref[1][0, j])                           # row j: the untwisted rotation, in bits
            gone = I.subtree(r, c)
            _bits(got[1][0, gone], np.tile(np.array(IDENT + IDENT), (len(gone), 1)))
            others = [k for k in range(r.P) if k not in I.subtree(r, j)]
            _bits(got[0][0, others], base[0][0, others])                # the other limbs keep their twist
            _bits(got[1][0, others], base[1][0, others])
    # a NaN on the pole row itself, or on its parent: no sample, no rotation, as before
    bad = x[1:].copy()
    bad[0, 4, 0] = np.inf
    got = _twisted(bad, r, tw, PRM1, state=st0)
    assert (got[0][0, I.subtree(r, 4), 3] == 0).all() and np.isfinite(got[1]).all()
    held = tracks.copy()
    held[0, :, 7] = 2.0                                                 # a held track counts as seen
    for a, b in zip(_twisted(x[1:], r, tw, PRM1, state=st0, tracks=held), base):
        _bits(a, b)


def test_any_split_of_five_steps_gives_the_bits_of_one_call():
    T, S = 5, 2
    r, pts, trk, st0 = I.case("UnrealEgo", T, S, mirror=True, with_tracks=True)
    tw = TI.table("UnrealEgo", r)
    whole = spec.skeleton_fit_twist_ref(pts, st0, r, tw, I.PARAMS, tracks=trk, streams=S)
    assert (whole[0][..., 3] == 7).any()
    for parts in _compositions(T):
        st, lo, outs = st0, 0, []
        for n in parts:
            o = spec.skeleton_fit_twist_ref(pts[lo * S:(lo + n) * S], st, r, tw, I.PARAMS, tracks=trk[lo * S:(lo + n) * S], streams=S)
            outs.append(o[:3])
            st, lo = o[3], lo + n
        for k in range(3):
            _bits(np.concatenate([o[k] for o in outs]), whole[k])
        _bits(st, whole[3])


def test_the_shared_case_meets_every_branch():
    """what the device test relies on: in its inputs bends lie below bend_lo, inside the ramp and above bend_hi, pole children are missing, and no
    observed twist is near the half turn, where a last-bit difference could pick the other branch (a twist quaternion with w > 1e-3 is
    k = h' . b > -1 + 2e-6, against the branch at -1 + 1e-12)"""
    for kind, T, S in (("UnrealEgo", 7, 1), ("EgoCap", 3, 6), ("chain64", 2, 4)):
        for fixed in (False, True):
            r, tw, pts, trk, st0 = TI.case(kind, T, S, fixed, True)
            pole = TI.pole_rows(kind)
            rigid, rot, _, _ = spec.skeleton_fit_twist_ref(pts, st0, r, tw, I.PARAMS, tracks=trk, streams=S, dtype="float64")
            plain = spec.skeleton_fit_ref(pts, st0, r, I.PARAMS, tracks=trk, streams=S, dtype="float64")[1]
            sig = TI.bends(r, pole, pts, trk)[:, list(pole)]
            assert (sig < TI.BEND_LO).any() and ((sig > TI.BEND_LO) & (sig < TI.BEND_HI)).any() and (sig > TI.BEND_HI).any() and np.isnan(sig).any(), kind
            flags = rigid[..., 3]
            assert {0.0, 3.0, 7.0} <= set(flags.ravel()), (kind, set(flags.ravel()))
            first = [j for j in pole if r.parents[j] not in pole]       # there the twist is Q_j (x) conj(Q_s) with Q_s skeleton_fit's rotation
            for b, j in zip(*np.nonzero(flags[:, first] == 7)):
                j = first[j]
                t = spec.quat_mul(tuple(rot[b, j, :4]), spec.quat_conj(tuple(plain[b, j, :4])))
                assert abs(t[0]) > 1e-3, (kind, b, j, t)


def _straighten(r, frame, j, c):
    """the frame with row c's bone laid along row j's (its subtree moved along): no bend at j"""
    out = np.array(frame, dtype=np.float64)
    along = (out[j] - out[r.parents[j]]) / np.linalg.norm(out[j] - out[r.parents[j]])
    out[I.subtree(r, c)] += (out[j] + np.linalg.norm(out[c] - out[j]) * along) - out[c]
    return out


def test_hinges_from_a_bent_frame_make_that_frame_twist_free():
    """skeleton_hinges_from_pose, then a fit of the same frame: the observed twist Q_j (x) conj(Q_s) is the identity to 1e-12 on every pole row
    (seen: 3e-16), so the twisted fit equals skeleton_fit's there; on another frame it does not.  A straight frame is refused by name."""
    for kind in ("UnrealEgo", "EgoCap"):
        r = I.rig(kind, mirror=True)                                    # a random rest pose, T-pose or not: the hinges come from the bent frame
        pole = spec.SKELETON_POLE[kind]
        frames = I.articulated(r, 40, 23, max_angle=1.5)[0]
        sig = TI.bends(r, pole, frames)[:, list(pole)]
        bent = int(np.argmax(sig.min(axis=1)))
        assert sig[bent].min() >= spec.SKELETON_BEND_HI, sig[bent]
        hinge = spec.skeleton_hinges_from_pose(r, pole, frames[bent])
        assert hinge.shape == (r.P, 3) and not hinge[[j for j in range(r.P) if j not in pole]].any()
        for j in pole:                                                  # a unit vector at right angles to the rest bone
            assert abs(np.linalg.norm(hinge[j]) - 1.0) <= 1e-12 and abs(np.dot(hinge[j], r.rest_dir[j])) <= 1e-12
        tw = spec.skeleton_twist(r, pole, hinge)
        got, plain = _twisted(frames[bent][None], r, tw), _plain(frames[bent][None], r)
        assert (got[0][0, list(pole), 3] == 7).all()
        worst = max(_qdist(got[1][0, j, :4], plain[1][0, j, :4]) for j in range(r.P))
        print(kind, "round trip", worst)
        assert worst <= 1e-12
        other = (bent + 1) % 40
        assert max(_qdist(a, b) for a, b in zip(_twisted(frames[other][None], r, tw)[1][0, :, :4], _plain(frames[other][None], r)[1][0, :, :4])) > 1e-3
        j, c = next(iter(pole.items()))
        straight = _straighten(r, frames[bent], j, c)
        with pytest.raises(ValueError, match=f"skeleton_hinges_from_pose: the frame is straight at row {j}"):
            spec.skeleton_hinges_from_pose(r, pole, straight)
        gone = frames[bent].copy()
        gone[c, 0] = np.nan
        with pytest.raises(ValueError, match="skeleton_hinges_from_pose: row .* has no rotation"):
            spec.skeleton_hinges_from_pose(r, pole, gone)
        with pytest.raises(ValueError, match="skeleton_hinges_from_pose: pose_rows is one frame"):
            spec.skeleton_hinges_from_pose(r, pole, frames[:2])


# ------------------------------------------------------------------------------------------------ refusals
def test_the_table_and_the_restatement_refuse_by_name():
    r = I.rig("UnrealEgo")
    pole = spec.SKELETON_POLE["UnrealEgo"]
    hinge = TI.table("UnrealEgo", r).hinge
    ok = spec.skeleton_twist(r, pole, hinge)
    assert (ok.bend_lo, ok.bend_hi) == (spec.SKELETON_BEND_LO, spec.SKELETON_BEND_HI) == (0.17364817766693033, 0.42261826174069944)
    assert abs(ok.bend_lo - math.sin(math.radians(10))) < 1e-16 and abs(ok.bend_hi - math.sin(math.radians(25))) < 1e-16
    assert ok.pole == (-1, -1, -1, -1, 6, 7, -1, -1, -1, -1, 12, 13, 14, 15, -1, -1) and spec.skeleton_twist(r, ok.pole, hinge).pole == ok.pole
    for j in pole:
        assert abs(np.dot(ok.g[j], r.rest_dir[j])) <= 1e-15 and abs(np.linalg.norm(ok.g[j]) - 1) <= 1e-15
    with pytest.raises(Exception):
        ok.bend_lo = 0.5                                                # frozen
    for preset in ("UnrealEgo", "EgoCap"):                              # the presets name children, on no root row, and leave the EgoCap wrists out
        par = spec.skeleton_parents(preset)
        assert all(par[c] == j and par[j] >= 0 for j, c in spec.SKELETON_POLE[preset].items())
    assert 3 not in spec.SKELETON_POLE["EgoCap"] and 7 not in spec.SKELETON_POLE["EgoCap"]
    bad = hinge.copy()
    bad[4] = (np.nan, 0, 0)
    par_hinge = hinge.copy()
    par_hinge[5] = 3.0 * r.rest_dir[5] + 1e-7 * ok.g[5]
    for kw, word in ((dict(pole={4: 16}), r"pole\[4\] = 16 is -1 or a row"), (dict(pole={4: -2}), r"pole\[4\] = -2"), (dict(pole={4: 7}), r"pole\[4\] = 7: the pole of a row is one of its children"),
                     (dict(pole={0: 1}), r"pole\[0\] = 1 is set on a root row"), (dict(pole={16: 1}), "pole names row 16"), (dict(pole=[-1] * 15), "pole holds one row per row"),
                     (dict(hinge=hinge[:15]), r"hinge is \[P, 3\]"), (dict(hinge=bad), r"hinge\[4\] is not finite"), (dict(hinge=par_hinge), r"hinge\[5\] is \(nearly\) parallel"),
                     (dict(bend_lo=-0.1), "0 <= bend_lo < bend_hi <= 1"), (dict(bend_lo=0.5, bend_hi=0.5), "0 <= bend_lo"), (dict(bend_hi=1.5), "0 <= bend_lo"),
                     (dict(bend_lo=math.nan), "0 <= bend_lo"), (dict(bend_hi=math.nan), "0 <= bend_lo"), (dict(rig="rig"), "rig is a spec.SkeletonRig")):
        args = dict(dict(rig=r, pole=pole, hinge=hinge), **kw)
        with pytest.raises(ValueError, match="skeleton_twist: " + word):
            spec.skeleton_twist(**args)
    # a hinge on a row without a pole is not read; bend_lo = 0 and bend_hi = 1 are allowed
    free = hinge.copy()
    free[0] = np.nan
    assert spec.skeleton_twist(r, pole, free, bend_lo=0.0, bend_hi=1.0).hinge[0].tolist() == [0, 0, 0]
    # hinge=None on a straight rest pose: a T-pose has no hinge of its own
    tpose = r.rest_pos.copy()
    tpose[I.subtree(r, 6)] += (tpose[4] + 0.3 * r.rest_dir[4]) - tpose[6]
    with pytest.raises(ValueError, match=r"skeleton_twist: the rest pose is straight at row 4.*T-pose has straight arms.*skeleton_hinges_from_pose.*explicit axis"):
        spec.skeleton_twist(spec.skeleton_rig(r.parents, tpose, r.frame_rows), pole)
    x, st = np.zeros((4, 16, 3)), np.zeros((1, 16, 2))
    with pytest.raises(ValueError, match="skeleton_fit_twist_ref: twist is a spec.SkeletonTwist"):
        spec.skeleton_fit_twist_ref(x, st, r, None)
    with pytest.raises(ValueError, match="skeleton_fit_twist_ref: the twist table has P = 17 rows, the rig 16"):
        spec.skeleton_fit_twist_ref(x, st, r, spec.skeleton_twist(I.rig("EgoCap"), {}))
    with pytest.raises(ValueError, match="skeleton_fit_twist_ref: pole"):      # a table made for another tree of the same size
        spec.skeleton_fit_twist_ref(x, st, spec.skeleton_rig((-1,) + (0,) * 15, r.rest_pos, (1, 2, 3)), ok)
    for args, kw, word in (((x[:, :15], st, r, ok), {}, "points is"), ((x, None, r, ok), {}, "state is"), ((x, st, "rig", ok), {}, "rig is"),
                           ((x, st, r, ok), dict(tracks=np.zeros((4, 15, 8))), "tracks is")):
        with pytest.raises(ValueError, match="skeleton_fit_twist_ref: " + word):
            spec.skeleton_fit_twist_ref(*args, **kw)


# ------------------------------------------------------------------------------------------------ the ABI
def test_the_twist_entry_is_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    assert "egotap_skeleton_fit_twist" in L.exported_symbols() and hasattr(lib, "egotap_skeleton_fit_twist") and "int egotap_skeleton_fit_twist(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    assert C.sizeof(L.EgotapSkeletonTwist) == 1808 and "a HOST struct of 1808 bytes" in text and "1616 bytes" in text
    assert C.sizeof(L.EgotapSkeletonRig) == 2584 and C.sizeof(L.EgotapSkeletonParams) == 24      # the old entry's structs are as they were
    assert "TWIST about a bone cannot be observed from positions: it follows the parent." in text
    r = I.rig("EgoCap")
    tw = TI.table("EgoCap", r, bend_lo=0.25, bend_hi=0.5)
    o = L.skeleton_twist_struct(tw)
    assert tuple(o.pole[:17]) == tw.pole and set(o.pole[17:]) == {-1} and (o.bend_lo, o.bend_hi) == (0.25, 0.5)
    assert tuple(o.hinge[11]) == tuple(tw.hinge[11]) and tuple(o.hinge[0]) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="twist is a spec.SkeletonTwist"):
        L.skeleton_twist_struct(r)


def test_skeleton_fit_twist_refuses_by_name_before_any_launch():
    lib = L.load()
    V = C.c_void_p
    T, S, P = 3, 2, 16
    B, K = T * S, P + 3
    points, tracks, sin, sout, rigid, rot, lens = (0x100000 * (k + 1) for k in range(7))
    nbytes = dict(points=B * P * 12, tracks=B * K * 32, sin=S * P * 16, sout=S * P * 16, rigid=B * P * 16, rot=B * P * 32, lens=B * P * 8)
    rig0 = I.rig("UnrealEgo", mirror=True)
    tw0 = TI.table("UnrealEgo", rig0)
    ok = dict(points=V(points), tracks=V(tracks), T=T, S=S, rig=L.skeleton_rig_struct(rig0), tw=L.skeleton_twist_struct(tw0), prm=L.skeleton_params_struct(track_rows=K),
              sin=V(sin), sout=V(sout), rigid=V(rigid), rot=V(rot), lens=V(lens))

    def call(**kw):
        a = dict(ok, **kw)
        ref = lambda s: C.byref(s) if s is not None else None      # noqa: E731
        rc = lib.egotap_skeleton_fit_twist(a["points"], a["tracks"], a["T"], a["S"], ref(a["rig"]), ref(a["tw"]), ref(a["prm"]), a["sin"], a["sout"], a["rigid"],
                                           a["rot"], a["lens"], None)
        return rc, lib.egotap_last_error().decode()

    def edit(o, **kw):
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

    def rig(fixed=False, **kw):
        return edit(L.skeleton_rig_struct(I.rig("UnrealEgo", mirror=True, fixed_scale=1.0 if fixed else None)), **kw)

    def twist(**kw):
        return edit(L.skeleton_twist_struct(tw0), **kw)

    def prm(**kw):
        return edit(L.skeleton_params_struct(track_rows=K), **kw)
    nan, inf = float("nan"), float("inf")
    along = tuple(2.0 * rig0.rest_dir[5] + 1e-7 * tw0.g[5])
    # what the twist adds
    cases = [(dict(tw=None), "null argument (twist is required"),
             (dict(tw=twist(pole={4: 16})), "pole[4] = 16 is -1 or a row"), (dict(tw=twist(pole={4: -2})), "pole[4] = -2"), (dict(tw=twist(pole={4: 64})), "pole[4] = 64"),
             (dict(tw=twist(pole={4: 7})), "pole[4] = 7: the pole of a row is one of its children"), (dict(tw=twist(pole={4: 2})), "pole[4] = 2: the pole"),
             (dict(tw=twist(pole={4: 4})), "pole[4] = 4: the pole"), (dict(tw=twist(pole={0: 1})), "pole[0] = 1 is set on a root row"),
             (dict(tw=twist(hinge={4: (nan, 0.0, 0.0)})), "hinge[4] is not finite"), (dict(tw=twist(hinge={5: (0.0, inf, 0.0)})), "hinge[5] is not finite"),
             (dict(tw=twist(hinge={5: along})), "hinge[5] is (nearly) parallel"), (dict(tw=twist(hinge={5: (0.0, 0.0, 0.0)})), "hinge[5] is (nearly) parallel"),
             (dict(tw=twist(bend_lo=-0.1)), "bend_lo"), (dict(tw=twist(bend_lo=0.8, bend_hi=0.8)), "bend_lo"), (dict(tw=twist(bend_hi=1.5)), "bend_lo"),
             (dict(tw=twist(bend_lo=nan)), "bend_lo"), (dict(tw=twist(bend_hi=nan)), "bend_lo")]
    # everything egotap_skeleton_fit refuses
    cases += [(dict(points=None), "null"), (dict(rig=None), "null"), (dict(prm=None), "null"), (dict(rigid=None), "null"), (dict(rot=None), "null"),
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
    # a rig whose tree no longer matches the table: row 6 moved under row 2
    cases.append((dict(rig=rig(parent={6: 2})), "pole[4] = 6: the pole of a row is one of its children (parent[6] = 2)"))
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
        assert rc == 1 and msg.startswith("egotap_skeleton_fit_twist:") and word in msg, (kw, rc, msg)
    # what is NOT refused (the first refusal is a later one, made on purpose): no pole row at all, a bad hinge on a row without a pole, bend_lo = 0 and
    # bend_hi = 1, a hinge barely off the bone (1e-5), NULL states and tracks with fixed_length, state_out == state_in
    barely = tuple(2.0 * rig0.rest_dir[5] + 1e-5 * tw0.g[5])
    for kw in (dict(tw=twist(pole={j: -1 for j in range(16)})), dict(tw=twist(hinge={0: (nan, nan, nan), 6: (0.0, 0.0, 0.0)})), dict(tw=twist(bend_lo=0.0, bend_hi=1.0)),
               dict(tw=twist(hinge={5: barely})), dict(rig=rig(fixed=True), sin=None, sout=None, tracks=None), dict(sout=V(sin))):
        rc, msg = call(**dict(kw, lens=V(lens + 8)))
        assert rc == 1 and msg.startswith("egotap_skeleton_fit_twist:") and "16-byte" in msg, (kw, msg)
    # the old entry still names itself
    rc = lib.egotap_skeleton_fit(None, None, T, S, None, None, None, None, None, None, None, None)
    assert rc == 1 and lib.egotap_last_error().decode().startswith("egotap_skeleton_fit: null argument")


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch

    from egotap_amd import models
    r = I.rig("UnrealEgo")
    tw = TI.table("UnrealEgo", r)
    pts, state = torch.zeros(4, 16, 3), torch.zeros(2, 16, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="twist is a spec.SkeletonTwist"):
        L.skeleton_fit_twist(pts, state, r, "twist", streams=2)
    with pytest.raises(ValueError, match="rig is a spec.SkeletonRig"):
        L.skeleton_fit_twist(pts, state, "rig", tw, streams=2)
    with pytest.raises(ValueError, match="the twist table has P = 16 rows, the rig 17"):
        L.skeleton_fit_twist(torch.zeros(4, 17, 3), state, I.rig("EgoCap"), tw, streams=2)
    with pytest.raises(ValueError, match="skeleton_fit_twist: points is a tensor"):
        L.skeleton_fit_twist(torch.zeros(5, 16, 3), state, r, tw, streams=2)
    with pytest.raises(ValueError, match="skeleton_fit_twist: state is a contiguous float64"):
        L.skeleton_fit_twist(pts, state.float(), r, tw, streams=2)
    with pytest.raises(L.EgotapError, match="skeleton_fit_twist runs on the GPU only"):
        L.skeleton_fit_twist(pts, state, r, tw, streams=2)
    with pytest.raises(ValueError, match="a twist table belongs to a rig"):
        models.Skeleton(16, joint_preset="UnrealEgo", twist=tw)
    with pytest.raises(ValueError, match="the twist table has P = 17 rows, the rig 16"):
        models.Skeleton(16, rig=r, twist=spec.skeleton_twist(I.rig("EgoCap"), {}))
    with pytest.raises(ValueError, match="twist is a spec.SkeletonTwist"):
        models.Skeleton(16, rig=r, twist="twist")
    sk = models.Skeleton(16, joint_preset="UnrealEgo", streams=2)
    with pytest.raises(ValueError, match="Skeleton.set_hinges: no rig"):
        sk.set_hinges(pts[0])
    frames = I.articulated(r, 40, 23, max_angle=1.5)[0]
    sig = TI.bends(r, spec.SKELETON_POLE["UnrealEgo"], frames)[:, list(spec.SKELETON_POLE["UnrealEgo"])]
    bent = frames[int(np.argmax(sig.min(axis=1)))]
    sk.set_rest_pose(torch.from_numpy(np.array(r.rest_pos)))
    assert sk.twist is None and len(sk._structs) == 2
    with pytest.raises(ValueError, match="the frame is straight at row 4"):
        sk.set_hinges(torch.from_numpy(_straighten(r, bent, 4, 6)))
    got = sk.set_hinges(torch.from_numpy(bent))
    want = spec.skeleton_twist(sk.rig, spec.SKELETON_POLE["UnrealEgo"], spec.skeleton_hinges_from_pose(sk.rig, spec.SKELETON_POLE["UnrealEgo"], bent))
    assert got is sk.twist and got.pole == want.pole and np.array_equal(got.g, want.g) and len(sk._structs) == 3 and tuple(sk._structs[2].pole[:16]) == want.pole
    with pytest.raises(L.EgotapError, match="GPU only"):
        sk.update(pts)
    sk.freeze()
    assert sk._structs[1].freeze == 1 and len(sk._structs) == 3
    sk.set_rest_pose(torch.from_numpy(np.array(r.rest_pos)))            # a new rest pose: the old hinges go
    assert sk.twist is None and len(sk._structs) == 2
    nameless = models.Skeleton(16, rig=r)
    with pytest.raises(ValueError, match="made without a joint preset; name the pole rows"):
        nameless.set_hinges(bent)
    assert nameless.set_hinges(bent, pole={4: 6}).pole[4] == 6
    assert models.Skeleton(16, rig=r, twist=tw).twist is tw
