"""Writes tests/golden/ocam.npz: two SYNTHETIC OCamCalib calibrations pushed through the reference's own numpy float64 world2cam and cam2world
(utils/projection.py:55-144).  Run where the reference checkout is (never on the GPU machine); the file holds numbers only -- calibration values,
inputs, outputs -- and is what tests/test_ocam_cpu.py pins spec.ocam_world2cam_ref / ocam_cam2world_ref against.

The reference's module imports packages that need not be installed (skimage, cv2, PIL, matplotlib ...): every one that fails to import is replaced by
an empty stub, the way tools/make_golden.py does; none of them is touched by the two functions used here.

Per calibration k = 0 (named "unreal_ego_pose": the UE flip is on) and k = 1 (another name: no flip), keys c{k}_*:
  name, pol (polynomialC2W), invpol (polynomialW2C), image_center ([yc, xc] as the JSON has it), affine ([c, d, e]), size, radius
  w2c_in [n, 3] -> w2c_out [n, 2]     world2cam(w2c_in, o); row 0 is exactly on the axis, row 1 inside isclose's 1e-8, row 2 just outside it, the last
                                      rows lie behind the image plane (an elevation beyond the fitted range)
  c2w_in [n, 2] -> c2w_out [n, 3]     cam2world as the inverse CONVENTION of world2cam: with the flip, v <- 2 yc - v before and (rx, -ry, -rz) after (the
                                      two wrapper steps are this tool's; everything between is the reference's function); row 0 is the centre pixel
pol is chosen; invpol is least-squares fitted here to r = invpol(arctan(pol(r) / r)) over [0, radius].

usage: python tools/make_golden_ocam.py [reference checkout, default /root/reference]"""
import importlib
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "ocam.npz")


def import_reference_projection(ref):
    sys.path.insert(0, ref)
    for name in ("skimage", "skimage.draw", "scipy.ndimage.filters", "PIL", "PIL.Image", "mpl_toolkits", "mpl_toolkits.mplot3d", "matplotlib",
                 "matplotlib.pyplot", "cv2"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
    for mod, attr in (("skimage.draw", "line_aa"), ("scipy.ndimage.filters", "gaussian_filter"), ("PIL", "Image"), ("mpl_toolkits.mplot3d", "Axes3D"),
                      ("matplotlib", "pyplot")):
        if not hasattr(sys.modules[mod], attr):
            setattr(sys.modules[mod], attr, None)
    return importlib.import_module("utils.projection")


def fit_invpol(pol, radius, n_coef):
    r = np.linspace(0.0, radius, 4001)[1:]
    z = sum(c * r ** k for k, c in enumerate(pol))
    theta = np.arctan(z / r)
    V = np.stack([theta ** k for k in range(n_coef)], axis=1)
    coef, *_ = np.linalg.lstsq(V, r, rcond=None)
    return coef


CALIBRATIONS = [
    dict(name="unreal_ego_pose", pol=[-330.0, 0.0, 1.1e-3, -4.0e-7, 1.2e-9], image_center=[515.8, 510.3], affine=[1.0007, 0.0004, -0.0003], size=[1024, 1024],
         radius=500.0, n_invpol=16),
    dict(name="synthetic_rig_right", pol=[-420.0, 0.0, 9.0e-4, 2.0e-7], image_center=[470.2, 640.7], affine=[0.9991, -0.0006, 0.0008], size=[960, 1280],
         radius=600.0, n_invpol=24),
]


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    P = import_reference_projection(ref)
    out = {}
    for k, cal in enumerate(CALIBRATIONS):
        rng = np.random.default_rng(100 + k)
        invpol = fit_invpol(cal["pol"], cal["radius"], cal["n_invpol"])
        o = dict(name=cal["name"], pol=list(cal["pol"]), length_pol=len(cal["pol"]), invpol=[float(v) for v in invpol], length_invpol=len(invpol),
                 xc=cal["image_center"][1], yc=cal["image_center"][0], c=cal["affine"][0], d=cal["affine"][1], e=cal["affine"][2])
        sign = -1.0 if cal["name"] == "unreal_ego_pose" else 1.0          # the points' own frame: world2cam negates y and z of UnrealEgo points itself
        n = 300
        rays_r = rng.uniform(5.0, cal["radius"], n)
        phi = rng.uniform(0.0, 2 * np.pi, n)
        zr = sum(c * rays_r ** i for i, c in enumerate(cal["pol"]))
        depth = rng.uniform(0.2, 3.0, n)
        pts = np.stack([rays_r * np.cos(phi), sign * rays_r * np.sin(phi), sign * zr], axis=1) / np.sqrt(rays_r ** 2 + zr ** 2)[:, None] * depth[:, None]
        pts[0] = [0.0, 0.0, sign * -1.5]                                  # exactly on the axis
        pts[1] = [3.0e-9, -4.0e-9, sign * -0.7]                           # norm 5e-9: inside isclose(norm, 0)
        pts[2] = [1.2e-8, 1.6e-8, sign * -0.7]                            # norm 2e-8: just outside it
        pts[-8:, 2] = sign * np.abs(pts[-8:, 2]) * 3.0                    # behind the image plane: elevations beyond the fitted range
        w2c = P.world2cam(pts.copy(), o)
        pix = np.stack([o["xc"] + rng.uniform(-1, 1, n) * cal["radius"] * 0.7, o["yc"] + rng.uniform(-1, 1, n) * cal["radius"] * 0.7], axis=1)
        pix[0] = [o["xc"], o["yc"]]
        pix[-4:] += cal["radius"]                                         # outside the image circle
        q = pix.copy()
        if sign < 0:
            q[:, 1] = o["yc"] * 2 - q[:, 1]
        rays = P.cam2world(q, o)
        if sign < 0:
            rays[:, 1:] *= -1.0
        # reported only: how well the fitted invpol inverts pol (a property of the fit, not of the code)
        inside = np.linalg.norm(pix - [o["xc"], o["yc"]], axis=1) <= cal["radius"]
        back = P.world2cam(rays.copy(), o)
        print(f"calibration {k} ({cal['name']}): {len(invpol)} fitted invpol coefficients; project(unproject(p)) - p inside the image circle: max "
              f"{np.abs(back - pix)[inside].max():.3e} px")
        for key in ("name", "pol", "image_center", "affine", "size", "radius"):
            out[f"c{k}_{key}"] = np.array(cal[key])
        out[f"c{k}_invpol"] = np.asarray(invpol, dtype=np.float64)
        out[f"c{k}_w2c_in"], out[f"c{k}_w2c_out"] = pts, w2c
        out[f"c{k}_c2w_in"], out[f"c{k}_c2w_out"] = pix, rays
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
