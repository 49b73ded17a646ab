"""Inputs shared by tests/test_ocam_cpu.py and tests/test_gpu_stereo_triangulate.py: the two synthetic calibrations of tests/golden/ocam.npz
(tools/make_golden_ocam.py), pinhole models whose rays are exact, and stereo keypoint sets with a known mix of valid and invalid joints."""
import os

import numpy as np

from egotap_amd import spec

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ocam.npz")
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(GOLDEN))
    return _cache["g"]


def calibration_json(k):
    """calibration k of the fixture in the layout of the reference's fisheye.calibration_{side}.json"""
    g = golden()
    return {"name": str(g[f"c{k}_name"]), "polynomialC2W": g[f"c{k}_pol"].tolist(), "polynomialW2C": g[f"c{k}_invpol"].tolist(),
            "image_center": g[f"c{k}_image_center"].tolist(), "affine": g[f"c{k}_affine"].tolist(), "size": g[f"c{k}_size"].tolist(),
            "imageCircleRadius": float(g[f"c{k}_radius"])}


def calibration(k):
    if ("m", k) not in _cache:
        _cache[("m", k)] = spec.ocam_from_json(calibration_json(k))
    return _cache[("m", k)]


def rig_models(ue=True):
    """the fixture's two calibrations as ONE rig: both cameras in the same convention (a rig's points live in one frame) -- both with the UE flip, or
    both without; the calibration values are untouched, only the name that switches the flip changes"""
    import dataclasses
    name = "unreal_ego_pose" if ue else "synthetic_rig"
    return tuple(dataclasses.replace(calibration(k), name=name + ("" if ue else "_" + "lr"[k])) for k in (0, 1))


def pinhole(f=300.0, name="pinhole"):
    """pol = [f]: cam2world((u, v)) = (u, v, f) / |(u, v, f)| -- the ray through (X, Y, Z), Z > 0, is hit by the pixel f (X / Z, Y / Z) to rounding.
    (1 / f) * f == 1 exactly for f = 300: the centre pixel's ray is (0, 0, 1) in bits, so two centre pixels are exactly parallel)"""
    assert (1.0 / f) * f == 1.0
    return spec.OcamModel(name=name, pol=[f], invpol=[0.0, f], xc=0.0, yc=0.0)


def pinhole_pixels(X, f=300.0):
    return f * X[..., :2] / X[..., 2:3]


SMALL_R = np.array([[0.9998000066665778, -0.019998666693333084, 0.0], [0.019998666693333084, 0.9998000066665778, 0.0], [0.0, 0.0, 1.0]])      # 0.02 rad about z
T = np.array([0.12, -0.01, 0.02])           # the right camera's origin in the left frame: a 12 cm baseline, in metres
KINDS = ("valid", "low_left", "low_right", "nan_score", "nan_x", "inf_y", "parallel", "behind")


def joints_in_view(B, J, seed):
    """[B, J, 3] points 0.4 .. 1.5 in front of both pinhole cameras (z > 0), spread sideways: the two rays of every point meet at 0.05 rad and more"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.4, 0.4, (B, J)), rng.uniform(-0.4, 0.4, (B, J)), rng.uniform(0.4, 1.5, (B, J))], axis=-1)


def pinhole_case(B, J, seed, R=None, f=300.0):
    """(keypoints float64 [B, 2, J, 4], X [B, J, 3], kind [B, J]) for two pinhole cameras T (and R) apart: joint j of frame b is of kind
    KINDS[(b + j) % len(KINDS)] for j >= 4 and "valid" below, so every frame keeps valid joints"""
    X = joints_in_view(B, J, seed)
    Rm = np.eye(3) if R is None else np.asarray(R)
    Xr = (X - T) @ Rm                                             # R^T (X - t): the point in the right camera's own axes
    kp = np.zeros((B, 2, J, 4))
    kp[:, 0, :, :2], kp[:, 1, :, :2] = pinhole_pixels(X, f), pinhole_pixels(Xr, f)
    kp[..., 2] = 0.9
    kind = np.empty((B, J), dtype=object)
    for b in range(B):
        for j in range(J):
            k = kind[b, j] = "valid" if j < 4 else KINDS[(b + j) % len(KINDS)]
            if k == "low_left":
                kp[b, 0, j, 2] = 0.49
            elif k == "low_right":
                kp[b, 1, j, 2] = 0.1
            elif k == "nan_score":
                kp[b, 0, j, 2] = np.nan
            elif k == "nan_x":
                kp[b, 1, j, 0] = np.nan
            elif k == "inf_y":
                kp[b, 0, j, 1] = np.inf
            elif k == "parallel":
                kp[b, :, j, :2] = 0.0                             # both centre pixels: both rays are the optical axis (identity R)
            elif k == "behind":
                kp[b, 0, j, :2], kp[b, 1, j, :2] = kp[b, 1, j, :2].copy(), kp[b, 0, j, :2].copy()      # swapped eyes: the rays meet behind the cameras
    return kp, X, kind


def fisheye_case(B, J, seed, R=None, units=4.0, ue=True):
    """(keypoints float64 [B, 2, J, 4], affine [2, 4], X, kind) through the fixture's two fisheye calibrations as ``rig_models(ue)``: points
    along rays of left-eye pixels inside the image circle, 0.4 .. 1.5 away, projected with each camera's world2cam; keypoints in units of
    calibration pixels / `units` with an offset, undone by the affine.  The score and coordinate kinds of pinhole_case."""
    left, right = rig_models(ue)
    rng = np.random.default_rng(seed)
    rad = float(golden()["c0_radius"])
    ang, rr = rng.uniform(0, 2 * np.pi, (B, J)), rng.uniform(0.05, 0.55, (B, J)) * rad
    pix = np.stack([left.xc + rr * np.cos(ang), left.yc + rr * np.sin(ang)], axis=-1)
    X = spec.ocam_cam2world_ref(pix, left) * rng.uniform(0.4, 1.5, (B, J, 1))
    Rm = np.eye(3) if R is None else np.asarray(R)
    pl, pr = spec.ocam_world2cam_ref(X, left), spec.ocam_world2cam_ref((X - T) @ Rm, right)
    affine = np.array([[units, 3.0, units, -2.0], [units * 1.25, 0.0, units * 0.9375, 1.5]])
    kp = np.zeros((B, 2, J, 4))
    for e, p in enumerate((pl, pr)):
        kp[:, e, :, 0] = (p[..., 0] - affine[e, 1]) / affine[e, 0]
        kp[:, e, :, 1] = (p[..., 1] - affine[e, 3]) / affine[e, 2]
    kp[..., 2] = 0.8
    kind = np.empty((B, J), dtype=object)
    for b in range(B):                                            # (no "parallel" / "behind" here: through fitted polynomials neither is exact)
        for j in range(J):
            k = kind[b, j] = "valid" if j < 4 else KINDS[(b + j) % 6]
            if k == "low_left":
                kp[b, 0, j, 2] = 0.49
            elif k == "low_right":
                kp[b, 1, j, 2] = 0.1
            elif k == "nan_score":
                kp[b, 0, j, 2] = np.nan
            elif k == "nan_x":
                kp[b, 1, j, 0] = np.nan
            elif k == "inf_y":
                kp[b, 0, j, 1] = np.inf
    return kp, affine, X, kind
