"""Inputs shared by tests/test_pose_track_world_cpu.py and tests/test_gpu_pose_track_world.py: the seeded serving outputs of tests/pose_track_inputs.py
seen from a rig that moves, with rig poses that do not count mixed in (a NaN, a matrix that is no rotation, a reflection), a world-frame state that
is already under way, and the scenario the world-frame entry exists for: a motionless skeleton under a turning head."""
import numpy as np

import pose_track_inputs as I
from egotap_amd import spec

DT = I.DT
PARAMS = I.PARAMS
WARMUP = I.WARMUP
ORTHO_TOL = 1e-6
IDENTITY = np.array(spec.RIG_IDENTITY)


def rot(axis, angle):
    """the rotation about a coordinate axis (0, 1, 2) by ``angle`` radians, [..., 3, 3]"""
    angle = np.asarray(angle, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.zeros(angle.shape + (3, 3))
    R[..., axis, axis] = 1.0
    R[..., i, i], R[..., i, j], R[..., j, i], R[..., j, j] = c, -s, s, c
    return R


def rigs(T, S, seed, t0=0, bad=True):
    """float64 [T * S, 12], time-major, for steps t0 .. t0 + T - 1: per stream a head that turns about all three axes and walks, at a few pose units from
    the origin.  ``bad``: about a quarter of the poses do not count -- a NaN entry, an inf translation, a scaled matrix, a reflection"""
    rng = np.random.default_rng(7000 + seed)
    rate, phase = rng.uniform(0.5, 3.0, (1, S, 3)), rng.uniform(0, 6.28, (1, S, 3))
    base, vel = rng.normal(0, 2.0, (1, S, 3)), rng.normal(0, 0.5, (1, S, 3))
    t = (np.arange(t0, t0 + T) * DT)[:, None, None]
    ang = phase + rate * t
    R = rot(2, ang[..., 0]) @ rot(1, 0.6 * np.sin(ang[..., 1])) @ rot(0, 0.3 * np.sin(ang[..., 2]))
    g = spec.rig_pose(base + vel * t, R=R)                              # [T, S, 12]
    if bad:
        rng = np.random.default_rng(seed * 1000 + t0 + 77)
        kind = rng.integers(0, 16, (T, S))
        g[kind == 0, rng.integers(0, 12)] = np.nan
        g[kind == 1, 7] = np.inf                                      # t_y
        g[kind == 2, 0:3] *= 1.0 + 1e-4                               # row 0 too long for ORTHO_TOL
        g[kind == 3, 4:7] *= -1.0                                     # a reflection: orthonormal, det = -1
    return np.ascontiguousarray(g.reshape(T * S, 12))


_cache = {}


def case(T, S, P, J, seed=1):
    """(pose, frame, joints3d, rig_pose, state0): the inputs of a call of T steps and the float64 WORLD state it starts from, WARMUP steps into the same
    streams under the same moving rigs"""
    key = (T, S, P, J, seed)
    if key not in _cache:
        wp, wf, wj = I.frames(WARMUP, S, P, J, seed)
        state0 = spec.pose_track_world_ref(wp, np.zeros((S, P + 1 + J, spec.POSE_TRACK_STATE)), rigs(WARMUP, S, seed), DT, PARAMS, frame=wf, joints3d=wj,
                                           streams=S, ortho_tol=ORTHO_TOL)[3]
        pose, frame, j3 = I.frames(T, S, P, J, seed, t0=WARMUP)
        _cache[key] = (pose, frame, j3, rigs(T, S, seed, t0=WARMUP), state0)
    return tuple(None if a is None else a.copy() for a in _cache[key])


def clean_case(T, S, P, J, seed):
    """float64 (pose, frame, joints3d, rig_pose) in which every sample and every rig pose is accepted and no value is a negative zero"""
    rng = np.random.default_rng(seed)
    pose = rng.normal(0, 1.0, (T * S, P, 3)) + 0.0
    frame = np.zeros((T * S, 8))
    frame[:, 0:3], frame[:, 3] = rng.normal(0, 1.0, (T * S, 3)) + np.array([0.1, -0.3, 1.2]), 9.0
    j3 = np.zeros((T * S, J, 8))
    j3[..., 0:3], j3[..., 7] = rng.normal(0, 1.0, (T * S, J, 3)), 1.0
    return pose, frame, j3, rigs(T, S, seed, bad=False)


# ---- a motionless world under a moving rig: 60 Hz, 240 frames, one stream, 16 pose rows, the root, 15 joints; the rig yaws +-60 degrees at 0.5 Hz and
# pitches +-20 degrees at 0.3 Hz about a head that sways a little; no noise, float64 measurements
STILL_HZ, STILL_T, STILL_P, STILL_J = 60.0, 240, 16, 15


def still_world():
    """dict: the world truth (pose_w [P, 3] offsets, root_w [3], joints_w [J, 3]), rig [T, 12], the camera-frame measurements (pose, frame, joints3d,
    float64) that a perfect estimator would return, placed_w [P, 3] and placed_c [T, P, 3] (the truth of the two placed outputs), top = max |coordinate|"""
    rng = np.random.default_rng(2024)
    root_w = np.array([90.0, -40.0, 200.0])                            # with offsets of up to 82: coordinates of up to 282 pose units
    pose_w = rng.uniform(-82.0, 82.0, (STILL_P, 3))
    pose_w[0] = [82.0, -82.0, 82.0]
    joints_w = root_w + rng.uniform(-82.0, 82.0, (STILL_J, 3))
    t = np.arange(STILL_T) / STILL_HZ
    yaw = np.radians(60.0) * np.sin(2 * np.pi * 0.5 * t)
    pitch = np.radians(20.0) * np.sin(2 * np.pi * 0.3 * t)
    R = rot(1, yaw) @ rot(0, pitch)                                   # [T, 3, 3], camera in the world
    tr = np.array([5.0, 160.0, -3.0]) + np.stack([4.0 * np.sin(2 * np.pi * 0.5 * t), 1.5 * np.sin(2 * np.pi * 0.6 * t), 3.0 * np.cos(2 * np.pi * 0.5 * t)], axis=-1)
    Rt = np.swapaxes(R, -1, -2)
    to_cam = lambda x, point: np.einsum("tij,tkj->tki", Rt, (x[None] - tr[:, None]) if point else np.broadcast_to(x[None], (STILL_T,) + x.shape))      # noqa: E731
    pose = to_cam(pose_w, False)
    frame = np.zeros((STILL_T, 8))
    frame[:, 0:3], frame[:, 3] = to_cam(root_w[None], True)[:, 0], float(STILL_J)
    j3 = np.zeros((STILL_T, STILL_J, 8))
    j3[..., 0:3], j3[..., 7] = to_cam(joints_w, True), 1.0
    placed_w = pose_w + root_w
    top = max(np.abs(a).max() for a in (pose_w, root_w, joints_w, placed_w))
    return dict(pose_w=pose_w, root_w=root_w, joints_w=joints_w, rig=spec.rig_pose(tr, R=R), pose=pose, frame=frame, joints3d=j3, placed_w=placed_w,
                placed_c=to_cam(placed_w, True), top=float(top), dt=1.0 / STILL_HZ)
