"""Inputs shared by tests/test_skeleton_twist_cpu.py and tests/test_gpu_skeleton_twist.py: the pole rows of every kind of rig of
tests/skeleton_inputs.py, seeded twist tables, rest poses that are bent at every pole joint, articulations with a known swing AND roll, a three-bone
arm whose elbow flexes about a known hinge, and the mixed case of the device test (skeleton_inputs.case with a twist table whose thresholds put its
bends below bend_lo, inside the ramp and above bend_hi)."""
import math

import numpy as np

import skeleton_inputs as I
from egotap_amd import spec

BEND_LO, BEND_HI = 0.35, 0.8            # the device case's thresholds: random swings of up to 1.6 rad put bends on both sides and in between
REST_BEND = math.radians(40.0)          # the bend of every pole joint in bent_rig's rest pose


def pole_rows(kind):
    """{row: pole child}: the presets' own; every inner row of the 64-row chain; none in the star (no row there has a bone AND a child)"""
    if kind in spec.SKELETON_POLE:
        return dict(spec.SKELETON_POLE[kind])
    return {j: j + 1 for j in range(1, 63)} if kind == "chain64" else {}


def _perp(rng, d):
    """a seeded unit vector at right angles to the unit vector d"""
    while True:
        a = rng.normal(size=3)
        a -= np.dot(a, d) * np.asarray(d)
        if np.linalg.norm(a) > 0.3:
            return a / np.linalg.norm(a)


def table(kind, r, bend_lo=BEND_LO, bend_hi=BEND_HI, seed=3):
    """a twist table for the rig r of `kind` with seeded hinges: at right angles to the rest bone plus a part along it, which the table takes out"""
    rng = np.random.default_rng(seed)
    hinge = np.zeros((r.P, 3))
    for j in pole_rows(kind):
        hinge[j] = rng.uniform(0.5, 2.0) * _perp(rng, r.rest_dir[j]) + rng.uniform(-0.7, 0.7) * r.rest_dir[j]
    return spec.skeleton_twist(r, pole_rows(kind), hinge, bend_lo=bend_lo, bend_hi=bend_hi)


def bends(r, pole, points, tracks=None):
    """the sine of the bend at every pole row of every frame, NaN where either sample is missing: float64 [B, P]"""
    pts = np.asarray(points, dtype=np.float64)
    out = np.full(pts.shape[:2], np.nan)
    with np.errstate(all="ignore"):
        for j, c in pole.items():
            p = r.parents[j]
            a, b = pts[:, j] - pts[:, p], pts[:, c] - pts[:, j]
            a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
            out[:, j] = np.linalg.norm(np.cross(a, b), axis=1)
            if tracks is not None:
                out[(tracks[:, [p, j, c], 7] == 0).any(axis=1), j] = np.nan
    return out


# ------------------------------------------------------------------------------------------------ a rest pose with hinges of its own
def bent_rig(kind, seed=7):
    """the rig of `kind` with a rest pose in which every pole child stands REST_BEND off its parent's bone: skeleton_twist(r, pole) then finds the
    hinges in the rest pose itself -> (rig, pole)"""
    parents, frame_rows, _ = I.tree(kind)
    pole = pole_rows(kind)
    child_of = {c: j for j, c in pole.items()}
    rng = np.random.default_rng(seed)
    pos, dirs = np.zeros((len(parents), 3)), {}
    for j, p in enumerate(parents):
        if p < 0:
            continue
        if j in child_of:
            d = dirs[p]
            dirs[j] = math.cos(REST_BEND) * d + math.sin(REST_BEND) * np.cross(_perp(rng, d), d)
        else:
            dirs[j] = I._unit(rng)
        pos[j] = pos[p] + rng.uniform(0.1, 0.5) * dirs[j]
    return spec.skeleton_rig(parents, pos, frame_rows), pole


def axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    s = math.sin(angle / 2.0)
    return (math.cos(angle / 2.0), float(s * a[0]), float(s * a[1]), float(s * a[2]))


def rolled_articulation(r, pole, tw, n, seed, flex=(-0.15, 1.3)):
    """n poses of a body whose every roll is observable: a random root rotation W; a pole child's local rotation is a FLEXION about its parent's rest
    hinge g by an angle in `flex` (the bend stays between 31 and 115 degrees: past sin 25 deg); a pole row that is no pole child gets a random swing
    times a random ROLL about its own rest direction; every other bone a random swing, the identity on the bones that lead to the frame rows.
    -> (poses [n, P, 3], the true global rotation of every row [n][P])"""
    rng = np.random.default_rng(seed)
    keep = I.leads_to_frame(r)
    child_of = {c: j for j, c in pole.items()}
    ident = (1.0, 0.0, 0.0, 0.0)
    poses, Qs = [], []
    for _ in range(n):
        local = []
        for j, p in enumerate(r.parents):
            if p < 0 or j in keep:
                local.append(ident)
            elif j in child_of:
                local.append(axis_angle(tw.g[child_of[j]], rng.uniform(*flex)))
            else:
                q = I.swing(rng, r.rest_dir[j], 2.0)
                if j in pole:
                    q = spec.quat_mul(q, axis_angle(r.rest_dir[j], rng.uniform(-2.5, 2.5)))
                local.append(q)
        scale = rng.uniform(0.7, 1.4, r.P)
        scale[list(keep)] = 1.15                                        # the frame's triangle keeps its shape
        x, Q = I.forward(r, rng.normal(0, 0.5, 3), I.random_rotation(rng), local, r.rest_len * scale)
        poses.append(x), Qs.append(Q)
    return np.array(poses), Qs


# ------------------------------------------------------------------------------------------------ one arm
ARM_PARENTS = (-1, 0, 0, 0, 1, 4, 5)        # a root, the three frame rows, then shoulder row 1 -> upper arm 4 -> forearm 5 -> hand 6
ARM_POLE = {4: 5}
ARM_HINGE = (0.0, 0.0, 1.0)


def arm_rig():
    """axis-aligned: the rest pose is its own frame (Q_root = identity in bits); the upper arm along x, the forearm REST_BEND off it in the xy plane,
    so the elbow's rest hinge rest_dir_4 x rest_dir_5 is +z"""
    c, s = math.cos(REST_BEND), math.sin(REST_BEND)
    rest = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (1.5, 1, 0), (1.5 + 0.8 * c, 1 + 0.8 * s, 0), (1.5 + 1.1 * c, 1 + 1.1 * s, 0)]
    return spec.skeleton_rig(ARM_PARENTS, rest, (1, 2, 3))


def arm_pose(r, upper, flexion, W=(1.0, 0.0, 0.0, 0.0)):
    """the arm with the body rotated by W, the upper arm's local rotation `upper` (any rotation: swing and roll) and the elbow flexed by `flexion`
    about its rest hinge; the hand stays straight on the forearm -> (pose [P, 3], the true global rotations)"""
    ident = (1.0, 0.0, 0.0, 0.0)
    local = [ident, ident, ident, ident, upper, axis_angle(ARM_HINGE, flexion), ident]
    return I.forward(r, (0.2, -0.1, 0.7), W, local, r.rest_len)


# ------------------------------------------------------------------------------------------------ the device test's case
def case(kind, T, S, fixed, with_tracks):
    """(rig, twist table, points, tracks, state0) of skeleton_inputs.case with the table of `table`; `fixed`: the rig with fixed lengths, no state"""
    r, pts, trk, state0 = I.case(kind, T, S, False, with_tracks)
    if fixed:
        r, state0 = I.rig(kind, fixed_scale=1.3), None
    return r, table(kind, r), pts, trk, state0
