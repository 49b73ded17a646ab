"""Inputs shared by tests/test_skeleton_fit_cpu.py and tests/test_gpu_skeleton_fit.py: seeded rigs (the two presets, a 64-row chain and a 64-row star),
articulated poses made by forward kinematics from a rig's rest pose, and the mixed case of the device test -- accepted samples, NaN rows, rows whose
track status is 0, outliers beyond max_dev, zero-length bones -- from a state that is already under way."""
import math

import numpy as np

from egotap_amd import spec

PARAMS = spec.SkeletonParams(window=8, min_samples=3, max_dev=0.5)      # a short window: a 7-step call crosses it
WARMUP = 5                                                          # steps behind the state a case starts from
EXTRA_TRACKS = 3                                                    # tracks rows past P (a tracker's root and joints): K = P + 3
KINDS = ("UnrealEgo", "EgoCap", "chain64", "star64")


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def tree(kind):
    """(parents, frame_rows, mirror) of a kind of rig"""
    if kind in ("UnrealEgo", "EgoCap"):
        return spec.skeleton_parents(kind), spec.SKELETON_FRAME_ROWS[kind], spec.SKELETON_MIRROR[kind]
    P = 64
    parents = (-1,) + (tuple(range(P - 1)) if kind == "chain64" else (0,) * (P - 1))
    return parents, (1, 2, 3), (-1, -1) + tuple(j ^ 1 for j in range(2, P))


def rest_pose(kind, seed=7):
    """a seeded rest pose [P, 3], root at the origin: bones 0.1 .. 0.5 long in random directions (no avatar's: the project ships none)"""
    parents = tree(kind)[0]
    rng = np.random.default_rng(seed)
    pos = np.zeros((len(parents), 3))
    for j, p in enumerate(parents):
        if p >= 0:
            pos[j] = pos[p] + rng.uniform(0.1, 0.5) * _unit(rng)
    return pos


def rig(kind, mirror=False, fixed_scale=None, seed=7):
    parents, frame_rows, mir = tree(kind)
    r = spec.skeleton_rig(parents, rest_pose(kind, seed), frame_rows, mirror=mir if mirror else None)
    if fixed_scale is None:
        return r
    return spec.skeleton_rig(parents, r.rest_pos, frame_rows, mirror=mir if mirror else None, fixed_length=fixed_scale * r.rest_len + (np.array(parents) < 0))


def leads_to_frame(r):
    """the rows whose bones lead from a root row to one of the frame rows: they stay unarticulated where the root's rotation is to be recovered"""
    rows = set()
    for j in r.frame_rows:
        while r.parents[j] >= 0:
            rows.add(j)
            j = r.parents[j]
    return rows


def swing(rng, rest_dir, max_angle):
    """a shortest-arc local rotation of the unit vector rest_dir by a random angle below max_angle"""
    a = _unit(rng)
    axis = np.cross(rest_dir, a)
    axis /= np.linalg.norm(axis)
    th = rng.uniform(0.05, max_angle)
    to = math.cos(th) * np.asarray(rest_dir) + math.sin(th) * np.cross(axis, rest_dir)
    return spec.quat_shortest_arc(tuple(float(v) for v in rest_dir), tuple(float(v) for v in to / np.linalg.norm(to)))


def random_rotation(rng):
    q = rng.normal(size=4)
    return spec.quat_sign(spec.quat_normalize(tuple(float(v) for v in q)))


def forward(r, root_pos, W, local, length):
    """forward kinematics in float64: the root rows at root_pos with rotation W, Q_j = Q_p (x) local_j, x_j = x_p + length_j rotate(Q_j, rest_dir_j)"""
    P = r.P
    x, Q = np.zeros((P, 3)), [None] * P
    for j, p in enumerate(r.parents):
        if p < 0:
            x[j], Q[j] = np.asarray(root_pos) + r.rest_pos[j], W        # (several root rows keep their rest offsets, unrotated: the tests use one)
        else:
            Q[j] = spec.quat_mul(Q[p], local[j])
            x[j] = x[p] + length[j] * np.array(spec.quat_rotate(Q[j], tuple(float(v) for v in r.rest_dir[j])))
    return x, Q


def articulated(r, n, seed, max_angle=2.0, jitter=0.0, rigid_frame=False):
    """n float64 poses [n, P, 3] of one body: bone lengths = rest lengths x a per-bone scale (one scale for the bones that lead to the frame rows),
    times 1 + jitter N(0, 1) per frame; a random root position and rotation W per frame; every bone a random shortest-arc swing below max_angle,
    but the identity on the bones that lead to the frame rows when ``rigid_frame``.  -> (poses, W [n], local [n][P], lengths [n, P])"""
    rng = np.random.default_rng(seed)
    keep = leads_to_frame(r)
    scale = rng.uniform(0.7, 1.4, r.P)
    scale[list(keep)] = 1.15
    poses, Ws, locs, lens = [], [], [], []
    ident = (1.0, 0.0, 0.0, 0.0)
    for _ in range(n):
        length = r.rest_len * scale * (1.0 + jitter * rng.normal(size=r.P))
        if jitter:
            length[list(keep)] = r.rest_len[list(keep)] * 1.15 * (1.0 + jitter * rng.normal())      # the triangle keeps its shape
        W = random_rotation(rng)
        local = [ident if (p < 0 or (rigid_frame and j in keep)) else swing(rng, r.rest_dir[j], max_angle) for j, p in enumerate(r.parents)]
        x, _ = forward(r, rng.normal(0, 0.5, 3) + np.array([0.1, -0.3, 1.2]), W, local, length)
        poses.append(x), Ws.append(W), locs.append(local), lens.append(length)
    return np.array(poses), Ws, locs, np.array(lens)


def subtree(r, j):
    rows = [j]
    for k in range(j + 1, r.P):
        if r.parents[k] in rows:
            rows.append(k)
    return rows


def frames(r, T, S, seed, with_tracks):
    """float32 (points [T * S, P, 3], tracks [T * S, K, 8] or None) of T steps of S bodies, time-major, with per step and stream: a NaN or inf row now
    and then, an outlier (one bone three times as long, its subtree moved along) and a zero-length bone (a child on its parent, its subtree moved
    along), every bone but those that lead to the frame rows swung by up to 1.6 rad; tracks with statuses 0, 1 and 2 on the pose rows and anything on the rows past P"""
    rng = np.random.default_rng(seed * 7919 + 13)
    P = r.P
    pts = np.zeros((T, S, P, 3))
    for s in range(S):
        pts[:, s] = articulated(r, T, seed * 100 + s, max_angle=1.6, jitter=0.02, rigid_frame=True)[0]
    bones = [j for j, p in enumerate(r.parents) if p >= 0]
    for t in range(T):
        for s in range(S):
            for k, factor in ((rng.choice(bones), 3.0), (rng.choice(bones), 0.0)):
                if rng.random() < 0.6:
                    move = (factor - 1.0) * (pts[t, s, k] - pts[t, s, r.parents[k]])
                    pts[t, s, subtree(r, k)] += move
                    if factor == 0.0:
                        pts[t, s, k] = pts[t, s, r.parents[k]]
            for _ in range(max(1, P // 12)):
                if rng.random() < 0.5:
                    pts[t, s, rng.integers(0, P), rng.integers(0, 3)] = rng.choice([np.nan, np.inf, -np.inf])
    points = np.ascontiguousarray(pts.reshape(T * S, P, 3).astype(np.float32))
    for t in range(T):                                              # the zero-length bones survive the rounding: the child takes its parent's float32 bits
        for s in range(S):
            for j in bones:
                if np.array_equal(pts[t, s, j], pts[t, s, r.parents[j]]):
                    points[t * S + s, j] = points[t * S + s, r.parents[j]]
    tracks = None
    if with_tracks:
        K = P + EXTRA_TRACKS
        tracks = rng.normal(size=(T * S, K, 8)).astype(np.float32)
        tracks[..., 7] = rng.choice([0.0, 1.0, 2.0], (T * S, K), p=[0.08, 0.72, 0.2])
    return points, tracks


_cache = {}


def case(kind, T, S, mirror=False, with_tracks=False, seed=1):
    """(rig, points, tracks, state0): the inputs of a calibrating call of T steps and the float64 state it starts from, WARMUP steps into the same bodies"""
    key = (kind, T, S, mirror, with_tracks, seed)
    if key not in _cache:
        r = rig(kind, mirror=mirror)
        pts, trk = frames(r, WARMUP + T, S, seed, with_tracks)
        cut = WARMUP * S
        state0 = spec.skeleton_fit_ref(pts[:cut], np.zeros((S, r.P, 2)), r, PARAMS, tracks=None if trk is None else trk[:cut], streams=S)[3]
        _cache[key] = (r, pts[cut:].copy(), None if trk is None else trk[cut:].copy(), state0)
    r, pts, trk, st = _cache[key]
    return r, pts.copy(), None if trk is None else trk.copy(), st.copy()
