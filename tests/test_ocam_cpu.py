"""CPU-side checks of the fisheye camera model and the stereo triangulation (egotap.h: egotap_ocam_project / egotap_ocam_unproject /
egotap_stereo_triangulate): the float64 restatements in spec.py against the reference's own functions (tests/golden/ocam.npz, written by
tools/make_golden_ocam.py), the triangulation record on exact rays and on every kind of invalid joint, the presets and affines, the JSON
loader, and the ABI's exports and refusals (fake pointers: nothing is launched)."""
import ctypes as C
import json

import numpy as np
import pytest

import ocam_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec

NEW = ("egotap_ocam_project", "egotap_ocam_unproject", "egotap_stereo_triangulate")


# ------------------------------------------------------------------------------------------------ the restatements against the reference
def _close(got, ref):
    """both sides are float64 in the same operation order: a few roundings of a degree <= 24 polynomial apart; the gate is about 100 x that"""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print("max relative deviation", np.nanmax(err))
    assert np.nanmax(err) <= 1e-12, np.nanmax(err)


@pytest.mark.parametrize("k", [0, 1])
def test_world2cam_restatement_matches_the_reference(k):
    g, m = I.golden(), I.calibration(k)
    assert m.ue_flip == (k == 0)
    got = spec.ocam_world2cam_ref(g[f"c{k}_w2c_in"], m)
    _close(got, g[f"c{k}_w2c_out"])
    # the on-axis point and the one inside isclose's 1e-8 give the centre exactly; the one just outside does not take that branch
    assert got[0].tolist() == [m.xc, m.yc] and got[1].tolist() == [m.xc, m.yc]
    assert g[f"c{k}_w2c_out"][0].tolist() == [m.xc, m.yc]
    assert np.hypot(*g[f"c{k}_w2c_in"][2, :2]) > 1e-8


@pytest.mark.parametrize("k", [0, 1])
def test_cam2world_restatement_matches_the_reference(k):
    g, m = I.golden(), I.calibration(k)
    got = spec.ocam_cam2world_ref(g[f"c{k}_c2w_in"], m)
    _close(got, g[f"c{k}_c2w_out"])
    assert np.abs(np.linalg.norm(got, axis=-1) - 1.0).max() <= 1e-15 * 4


@pytest.mark.parametrize("k", [0, 1])
def test_round_trip_is_reported_not_asserted(k):
    """project(unproject(p)) - p is a property of the fitted invpol of the synthetic calibration, not of this code: printed (DESIGN 3.22 quotes it)"""
    g, m = I.golden(), I.calibration(k)
    pix = g[f"c{k}_c2w_in"]
    inside = np.hypot(pix[:, 0] - m.xc, pix[:, 1] - m.yc) <= float(g[f"c{k}_radius"])
    back = spec.ocam_world2cam_ref(spec.ocam_cam2world_ref(pix, m), m)
    print(f"calibration {k}: max |project(unproject(p)) - p| inside the image circle = {np.abs(back - pix)[inside].max():.3e} px")


# ------------------------------------------------------------------------------------------------ the triangulation record
def _all_valid(B, J, seed, R):
    kp, X, _ = I.pinhole_case(B, J, seed=seed, R=R)
    kp[:, 0, :, :2] = I.pinhole_pixels(X)
    kp[:, 1, :, :2] = I.pinhole_pixels((X - I.T) @ (np.eye(3) if R is None else R))
    kp[..., 2] = 1.0
    return kp, X


@pytest.mark.parametrize("R", [None, I.SMALL_R], ids=["parallel_axes", "rotated"])
def test_triangulation_recovers_points_from_exact_rays(R):
    """pinhole models (pol = [f]) turn the pixels f X / Z into the rays X / |X| and (X - t) / |X - t| to float64 rounding"""
    cam = I.pinhole()
    kp, X = _all_valid(3, 17, 5, R)
    rec, frame = spec.stereo_triangulate_ref(kp, cam, cam, I.T, R=R, dtype="float64")
    assert (rec[..., 7] == 1).all() and (frame[:, 3] == 17).all()
    assert (rec[..., 4] >= 1e-4).all(), rec[..., 4].min()                      # den: no joint is excused
    norm = np.linalg.norm(X, axis=-1)
    print("max |X - truth| / |X|", (np.linalg.norm(rec[..., :3] - X, axis=-1) / norm).max(), "max gap / |X|", (rec[..., 3] / norm).max(), "min den", rec[..., 4].min())
    assert (np.linalg.norm(rec[..., :3] - X, axis=-1) <= 1e-9 * norm).all()
    assert (rec[..., 3] <= 1e-9 * norm).all()
    assert np.allclose(rec[..., 5], norm, rtol=1e-9)                           # s is the distance along the left ray
    assert (frame[:, :3] == 0).all() and (frame[:, 4:6] == 0).all()            # no pose: no translation, no disagreement
    assert (frame[:, 7] <= 1e-9 * norm.max()).all() and (frame[:, 6] <= frame[:, 7]).all()
    # the float32 record is the float64 one rounded once
    rec32, frame32 = spec.stereo_triangulate_ref(kp, cam, cam, I.T, R=R)
    assert rec32.dtype == np.float32 and np.array_equal(rec32, rec.astype(np.float32)) and np.array_equal(frame32, frame.astype(np.float32))


def test_translation_and_disagreement():
    cam = I.pinhole()
    kp, X = _all_valid(2, 15, 6, None)
    t0 = np.array([0.03, -0.21, 0.35])
    pose = np.zeros((2, 16, 3))
    pose[:, 1:] = X - t0                                                       # the pelvis-relative pose in rows 1 .. 15 (the head at row 0)
    pose[:, 0] = 7.0
    rec, frame = spec.stereo_triangulate_ref(kp, cam, cam, I.T, pose=pose, pose_row0=1, dtype="float64")
    assert np.abs(frame[:, :3] - t0).max() <= 1e-9 and np.abs(rec[..., 6]).max() <= 1e-9 and (frame[:, 3] == 15).all()
    assert np.abs(frame[:, 4:6]).max() <= 1e-9
    # one joint of the pose moved by 0.05: its disagreement is 0.05 less the share the mean takes (14 / 15 of it), the others' 0.05 / 15
    pose[0, 1 + 4, 0] += 0.05
    rec, frame = spec.stereo_triangulate_ref(kp, cam, cam, I.T, pose=pose, pose_row0=1, dtype="float64")
    assert abs(rec[0, 4, 6] - 0.05 * 14 / 15) <= 1e-9 and np.abs(np.delete(rec[0, :, 6], 4) - 0.05 / 15).max() <= 1e-9
    assert abs(frame[0, 5] - 0.05 * 14 / 15) <= 1e-9 and abs(frame[0, 0] - (t0[0] - 0.05 / 15)) <= 1e-9
    with pytest.raises(ValueError, match="pose_row0"):
        spec.stereo_triangulate_ref(kp, cam, cam, I.T, pose=pose, pose_row0=2)


def test_validity_and_frame_statistics():
    cam = I.pinhole()
    B, J = 5, 17
    kp, X, kind = I.pinhole_case(B, J, seed=7)
    assert set(kind.ravel()) == set(I.KINDS)
    rec, frame = spec.stereo_triangulate_ref(kp, cam, cam, I.T, dtype="float64")
    ok = kind == "valid"
    assert np.array_equal(rec[..., 7] == 1, ok), (kind[(rec[..., 7] == 1) != ok])
    assert (rec[~ok] == 0).all() and not np.signbit(rec[~ok]).any()            # an invalid joint is all (positive) zeros
    assert np.array_equal(frame[:, 3], ok.sum(axis=1)) and (ok.sum(axis=1) < J).all()
    assert (rec[ok][:, 4] >= 1e-4).all()
    gap = np.where(ok, rec[..., 3], 0.0)
    assert np.allclose(frame[:, 6], np.sqrt((gap ** 2).sum(axis=1) / ok.sum(axis=1)), rtol=1e-12, atol=0) and np.array_equal(frame[:, 7], gap.max(axis=1))
    # each kind on its own lowers n by one
    full, _ = _all_valid(1, J, 8, None)
    n0 = spec.stereo_triangulate_ref(full, cam, cam, I.T)[1][0, 3]
    assert n0 == J
    for what in I.KINDS[1:]:
        one = full.copy()
        if what == "low_left":
            one[0, 0, 9, 2] = np.nextafter(0.5, 0)
        elif what == "low_right":
            one[0, 1, 9, 2] = -1.0
        elif what == "nan_score":
            one[0, 1, 9, 2] = np.nan
        elif what == "nan_x":
            one[0, 0, 9, 0] = np.nan
        elif what == "inf_y":
            one[0, 1, 9, 1] = -np.inf
        elif what == "parallel":
            one[0, :, 9, :2] = 0.0
        elif what == "behind":
            one[0, 0, 9, :2], one[0, 1, 9, :2] = full[0, 1, 9, :2], full[0, 0, 9, :2]
        r, f = spec.stereo_triangulate_ref(one, cam, cam, I.T)
        assert f[0, 3] == J - 1 and (r[0, 9] == 0).all() and (np.delete(r[0, :, 7], 9) == 1).all(), what
    one = full.copy()
    one[0, 0, 9, 2] = 0.5                                                      # the threshold itself is seen
    assert spec.stereo_triangulate_ref(one, cam, cam, I.T)[1][0, 3] == J
    # a pose row that is not finite takes its joint out; nothing valid at all: a zero frame
    pose = np.zeros((1, J, 3))
    pose[0, 3, 1] = np.nan
    r, f = spec.stereo_triangulate_ref(full, cam, cam, I.T, pose=pose)
    assert f[0, 3] == J - 1 and (r[0, 3] == 0).all() and np.isfinite(f).all()
    none = full.copy()
    none[..., 2] = 0.0
    r, f = spec.stereo_triangulate_ref(none, cam, cam, I.T, pose=np.ones((1, J, 3)))
    assert (r == 0).all() and (f == 0).all()
    with pytest.raises(ValueError, match="joints"):
        spec.stereo_triangulate_ref(np.zeros((1, 2, 65, 4)), cam, cam, I.T)


# ------------------------------------------------------------------------------------------------ presets and affines
def test_pose_row0_and_default_affines():
    ue, ec = spec.lift_preset("UnrealEgo"), spec.lift_preset("EgoCap")
    # UnrealEgo estimates the head: the pose has J + 1 rows, the head at row 0, heatmap joint j (gt_camera_2d[1:]) pairs with row 1 + j
    assert ue.estimate_head and ue.out_joints == ue.n_joints_hm + 1 == 16 and spec.stereo_pose_row0(ue) == 1
    assert not ec.estimate_head and ec.out_joints == ec.n_joints_hm == 17 and spec.stereo_pose_row0(ec) == 0
    assert spec.STEREO_MIN_SCORE == 0.5 and spec.STEREO_MAX_JOINTS == 64
    # RGB / byte entries: keypoints are pixels of the 4S x 4S frame; the calibration's image is size = (height, width)
    assert spec.stereo_pixel_affine(I.calibration(0), 64) == (4.0, 0.0, 4.0, 0.0)
    assert spec.stereo_pixel_affine(I.calibration(1), 64) == (5.0, 0.0, 3.75, 0.0)
    assert spec.stereo_pixel_affine(I.calibration(0), 128) == (2.0, 0.0, 2.0, 0.0)
    assert spec.STEREO_IDENTITY_AFFINE == ((1.0, 0.0, 1.0, 0.0), (1.0, 0.0, 1.0, 0.0))


def test_sensor_keypoints_need_the_identity_affine():
    """The sensor entry's keypoints are sensor pixels already (spec.sensor_keypoint_affine, a mirrored right eye included): a hot pixel rendered where a
    sensor pixel lands after crop, mirror and resize reads out within half a heatmap pixel of it, so the calibration's pixels ARE the keypoints."""
    S, rect = 64, (70, 30, 300, 200)
    x0, y0, w, h = rect
    truth = np.array([[100.3, 60.9], [333.0, 201.5], [215.2, 131.1]])
    for mirror in (False, True):
        u = (truth[:, 0] - x0) / w * S
        v = (truth[:, 1] - y0) / h * S
        if mirror:
            u = S - u
        hm = np.zeros((1, len(truth), S, S), dtype=np.float32)
        hm[0, np.arange(len(truth)), v.astype(int), u.astype(int)] = 1.0
        rec = spec.heatmap_peaks_ref(hm, groups=1, affine=[spec.sensor_keypoint_affine(rect, mirror, S)])[0]
        assert (np.abs(rec[:, 0] - truth[:, 0]) <= 0.5 * w / S + 1e-3).all() and (np.abs(rec[:, 1] - truth[:, 1]) <= 0.5 * h / S + 1e-3).all(), (mirror, rec)
    cam = I.pinhole()
    kp, _ = _all_valid(1, 15, 9, None)
    a, b = spec.stereo_triangulate_ref(kp, cam, cam, I.T), spec.stereo_triangulate_ref(kp, cam, cam, I.T, affine=spec.STEREO_IDENTITY_AFFINE)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # and an affine is applied before the camera model: keypoints in quarter units with the x4 affine give the same pixels, hence the same bits
    q = kp.copy()
    q[..., :2] /= 4.0
    c = spec.stereo_triangulate_ref(q, cam, cam, I.T, affine=[(4.0, 0.0, 4.0, 0.0)] * 2)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])


# ------------------------------------------------------------------------------------------------ the JSON loader
def test_json_loader_mapping_and_refusals(tmp_path):
    d = I.calibration_json(1)
    path = tmp_path / "fisheye.calibration_right.json"
    path.write_text(json.dumps(d))
    for m in (spec.ocam_from_json(str(path)), spec.ocam_from_json(d)):
        assert m.name == d["name"] and not m.ue_flip
        assert m.xc == d["image_center"][1] and m.yc == d["image_center"][0] and m.xc != m.yc          # the swapped centre
        assert (m.c, m.d, m.e) == tuple(d["affine"])
        assert m.pol == tuple(d["polynomialC2W"]) and m.invpol == tuple(d["polynomialW2C"]) and len(m.invpol) == 24
        assert m.size == tuple(d["size"]) and m.radius == d["imageCircleRadius"]
    assert spec.ocam_from_json(dict(d, name="unreal_ego_pose")).ue_flip
    assert not spec.ocam_from_json(dict(d, name="Unreal_ego_pose")).ue_flip
    for bad, word in ((dict(polynomialC2W=[1.0] * 9), "polynomialC2W"), (dict(polynomialC2W=[]), "polynomialC2W"), (dict(polynomialW2C=[1.0] * 25), "polynomialW2C"),
                      (dict(polynomialW2C=[]), "polynomialW2C"), (dict(affine=[0.5, 0.5, 1.0]), "c - d \\* e"), (dict(affine=[1.0, 0.0]), "affine"),
                      (dict(affine=[1.0, float("nan"), 0.0]), "not finite"), (dict(image_center=[float("inf"), 3.0]), "not finite")):
        with pytest.raises(ValueError, match=word):
            spec.ocam_from_json(dict(d, **bad))


# ------------------------------------------------------------------------------------------------ the ABI
def test_the_new_entries_are_declared_bound_and_exported():
    lib = L.load()
    text = open(L._build.REPO + "/include/egotap.h").read()
    for name in NEW:
        assert name in L.exported_symbols() and hasattr(lib, name) and f"int {name}(" in text
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2
    o = L.ocam_struct(I.calibration(0))
    assert C.sizeof(L.EgotapOcam) == 8 * (8 + 24 + 6) + 8 and o.n_pol == 5 and o.n_invpol == 16 and o.ue_flip == 1.0 and o.xc == I.calibration(0).xc
    assert L.ocam_struct(I.calibration(1)).ue_flip == 0.0


def _cam(**kw):
    o = L.ocam_struct(I.calibration(1))
    for k, v in kw.items():
        if k in ("pol", "invpol"):
            getattr(o, k)[v[0]] = v[1]
        else:
            setattr(o, k, v)
    return o


BAD_CAMERAS = [(dict(n_pol=0), "n_pol"), (dict(n_pol=9), "n_pol"), (dict(n_invpol=0), "n_invpol"), (dict(n_invpol=25), "n_invpol"),
               (dict(c=0.5, d=0.5, e=1.0), "c - d * e == 0"), (dict(xc=float("nan")), "not finite"), (dict(e=float("inf")), "not finite"),
               (dict(pol=(2, float("nan"))), "not finite"), (dict(invpol=(23, float("-inf"))), "not finite"), (dict(ue_flip=0.5), "ue_flip")]


@pytest.mark.parametrize("name", NEW[:2])
def test_project_and_unproject_refuse_by_name_before_any_launch(name):
    lib = L.load()
    fn = getattr(lib, name)
    P = C.c_void_p
    n_in, n_out = (3, 2) if name == "egotap_ocam_project" else (2, 3)
    ok = dict(src=P(0x100000), N=100, cam=_cam(), dst=P(0x200000))

    def call(**kw):
        a = dict(ok, **kw)
        rc = fn(a["src"], a["N"], C.byref(a["cam"]) if a["cam"] is not None else None, a["dst"], None)
        return rc, lib.egotap_last_error().decode()
    cases = [(dict(src=None), "null"), (dict(dst=None), "null"), (dict(cam=None), "null camera model"), (dict(N=0), "must be positive"), (dict(N=-3), "must be positive"),
             (dict(dst=P(0x200002)), "4-byte aligned"), (dict(src=P(0x100001)), "4-byte aligned"),
             (dict(dst=P(0x100000)), "overlaps"), (dict(dst=P(0x100000 + 100 * n_in * 4 - 4)), "overlaps"), (dict(dst=P(0x100000 - 100 * n_out * 4 + 4)), "overlaps")]
    cases += [(dict(cam=_cam(**kw)), word) for kw, word in BAD_CAMERAS]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith(name + ":") and word in msg, (kw, rc, msg)


def test_stereo_triangulate_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    B, J, Pn = 3, 15, 16
    kp, pose, j3, fr = 0x100000, 0x200000, 0x300000, 0x400000
    D3, D9, D8 = C.c_double * 3, C.c_double * 9, C.c_double * 8
    ok = dict(kp=P(kp), B=B, J=J, left=_cam(), right=_cam(), R=None, t=D3(0.1, 0.0, 0.0), aff=None, ms=0.5, pose=P(pose), P=Pn, row0=1, j3=P(j3), fr=P(fr))

    def call(**kw):
        a = dict(ok, **kw)
        by = lambda m: C.byref(m) if m is not None else None      # noqa: E731
        rc = lib.egotap_stereo_triangulate(a["kp"], a["B"], a["J"], by(a["left"]), by(a["right"]), a["R"], a["t"], a["aff"], a["ms"], a["pose"], a["P"], a["row0"],
                                           a["j3"], a["fr"], None)
        return rc, lib.egotap_last_error().decode()
    nan, inf = float("nan"), float("inf")
    kp_bytes, pose_bytes, j3_bytes = B * 2 * J * 16, B * Pn * 12, B * J * 32
    cases = [(dict(kp=None), "null"), (dict(j3=None), "null"), (dict(fr=None), "null"), (dict(t=None), "null"),
             (dict(left=None), "left: null camera model"), (dict(right=None), "right: null camera model"),
             (dict(B=0), "must be positive"), (dict(J=0), "must be positive"), (dict(B=-1), "must be positive"), (dict(J=65), "at most 64 joints"),
             (dict(j3=P(j3 + 8)), "16-byte aligned"), (dict(fr=P(fr + 4)), "16-byte aligned"), (dict(kp=P(kp + 8)), "16-byte aligned"), (dict(pose=P(pose + 2)), "aligned"),
             (dict(row0=2), "pose rows"), (dict(row0=-1), "pose rows"), (dict(P=14, row0=0), "pose rows"),
             (dict(ms=nan), "must be finite"), (dict(ms=inf), "must be finite"), (dict(t=D3(0.1, nan, 0.0)), "must be finite"),
             (dict(R=D9(1, 0, 0, 0, 1, 0, 0, inf, 1)), "must be finite"), (dict(aff=D8(4, 0, 4, 0, 4, nan, 4, 0)), "must be finite"),
             (dict(j3=P(kp)), "overlap"), (dict(j3=P(kp + kp_bytes - 16)), "overlap"), (dict(fr=P(kp + 32)), "overlap"), (dict(j3=P(pose + pose_bytes - 16)), "overlap"),
             (dict(fr=P(pose)), "overlap"), (dict(fr=P(j3 + j3_bytes - 32)), "overlap"), (dict(j3=P(fr - j3_bytes + 16)), "overlap")]
    for side in ("left", "right"):
        cases += [({side: _cam(**kw)}, f"{side}: ") for kw, _ in BAD_CAMERAS]
        cases += [({side: _cam(**kw)}, word) for kw, word in BAD_CAMERAS]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("egotap_stereo_triangulate:") and word in msg, (kw, rc, msg)


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch
    cam = I.calibration(0)
    with pytest.raises(ValueError, match=r"\[\.\.\., 3\]"):
        L.ocam_project(torch.zeros(4, 2), cam)
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        L.ocam_unproject(torch.zeros(4, 3), cam)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.ocam_project(torch.zeros(4, 3), cam)
    kp = torch.zeros(2, 2, 15, 4)
    with pytest.raises(ValueError, match="3 values"):
        L.stereo_triangulate(kp, cam, cam, (0.1, 0.0))
    with pytest.raises(ValueError, match="3 x 3"):
        L.stereo_triangulate(kp, cam, cam, (0.1, 0.0, 0.0), R=[[1.0, 0.0], [0.0, 1.0]])
    with pytest.raises(ValueError, match=r"\[2, 4\]"):
        L.stereo_triangulate(kp, cam, cam, (0.1, 0.0, 0.0), affine=[(4.0, 0.0, 4.0, 0.0)])
    with pytest.raises(ValueError, match="keypoints"):
        L.stereo_triangulate(kp[:, :1], cam, cam, (0.1, 0.0, 0.0))
    with pytest.raises(ValueError, match="pose_row0"):
        L.stereo_triangulate(kp, cam, cam, (0.1, 0.0, 0.0), pose=torch.zeros(2, 15, 3), pose_row0=1)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.stereo_triangulate(kp, cam, cam, (0.1, 0.0, 0.0))
