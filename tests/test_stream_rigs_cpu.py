"""Host side of a camera rig per stream: the rig table (egotap_stereo_rig, egotap_stereo_rigs_check), the per-stream entries' refusals (fake pointers:
nothing is launched) and the restatements, which apply the single-rig ones to rows s, s + S, .. and add no arithmetic.  Needs no GPU."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import ocam_inputs as I
from egotap_amd import lib as L
from egotap_amd import spec
from test_lens_map_cpu import BAD_DESCS, _desc
from test_sensor_resize_cpu import _handle, _refused

REPO = L._build.REPO
INVALID = 1
NEW = ("egotap_stereo_rigs_check", "egotap_stereo_triangulate_streams", "egotap_stereo_fuse_streams", "egotap_lens_remap_streams",
       "egotap_predict_pose_lens_streams", "egotap_predict_pose_lens_streams_kp", "egotap_predict_pose_lens_streams_kpl")


def _rigs():
    """three rigs that really differ: the UE pair rotated, the plain pair with another baseline and an affine, two pinholes"""
    ue, cv = I.rig_models(True), I.rig_models(False)
    return [spec.StereoRig(ue[0], ue[1], I.T, R=I.SMALL_R), spec.StereoRig(cv[0], cv[1], I.T * 1.5, affine=((4.0, 3.0, 4.0, -2.0), (5.0, 0.0, 3.75, 1.5))),
            spec.StereoRig(I.pinhole(), I.pinhole(), (0.1, 0.0, 0.0), min_score=0.25)]


def _table(rigs):
    return (L.EgotapStereoRig * len(rigs))(*[L.stereo_rig_struct(r) for r in rigs])


# ------------------------------------------------------------------------------------------------------------ symbols and layout
def test_new_symbols_are_declared_and_exported():
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egotap.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", L._build.LIB], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(egotap_[a-z0-9_]+)$", out, flags=re.M))
    for name in NEW:
        assert hasattr(lib, name) and name in L.exported_symbols() and name in exported, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert lib.egotap_abi_version() == 2 and L.ABI_VERSION == 2 and re.search(r"#define\s+EGOTAP_ABI_VERSION\s+2\b", header)      # additive: the version stays
    assert re.search(r"}\s*egotap_stereo_rig\s*;", header) and re.search(r"#define\s+EGOTAP_MAX_STREAM_RIGS\s+4096\b", header)
    assert spec.STEREO_MAX_STREAMS == 4096


def test_the_rig_struct_is_the_header_s():
    """sizeof(egotap_stereo_rig), as a C compiler lays the header's struct out, is the ctypes struct's: 792 bytes, doubles at 8-byte offsets"""
    R = L.EgotapStereoRig
    assert C.sizeof(L.EgotapOcam) == 312 and C.sizeof(R) == 792 == L.STEREO_RIG_BYTES and C.alignment(R) == 8
    assert (R.left.offset, R.right.offset, R.R.offset, R.t.offset, R.affine.offset, R.min_score.offset) == (0, 312, 624, 696, 720, 784)
    try:
        hipcc = L._build._hipcc()
    except RuntimeError:
        return
    probe = '#include "egotap.h"\n#include <stddef.h>\nstatic_assert(sizeof(egotap_stereo_rig) == 792 && offsetof(egotap_stereo_rig, right) == 312 && ' \
            'offsetof(egotap_stereo_rig, R) == 624 && offsetof(egotap_stereo_rig, t) == 696 && offsetof(egotap_stereo_rig, affine) == 720 && ' \
            'offsetof(egotap_stereo_rig, min_score) == 784, "layout");\n'
    res = subprocess.run([hipcc, "-x", "c++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(REPO, "include"), "-"], input=probe, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]


def test_a_rig_row_spells_out_the_identities():
    o = L.stereo_rig_struct(spec.StereoRig(I.pinhole(), I.calibration(0), (1.0, 2.0, 3.0)))
    assert list(o.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(o.t) == [1, 2, 3] and [list(r) for r in o.affine] == [[1, 0, 1, 0]] * 2 and o.min_score == 0.5
    assert o.left.n_pol == 1 and o.right.n_pol == len(I.calibration(0).pol) and o.right.ue_flip == 1.0
    with pytest.raises(ValueError, match="spec.StereoRig"):
        L.stereo_rig_struct((I.pinhole(), I.pinhole(), (0, 0, 0)))
    for bad, word in ((dict(t=(1.0, 2.0)), "3 values"), (dict(R=((1, 0), (0, 1))), "3 x 3"), (dict(affine=((1, 0, 1, 0),)), r"\[2, 4\]"), (dict(left=None), "OcamModel")):
        with pytest.raises(ValueError, match=word):
            spec.StereoRig(**dict(dict(left=I.pinhole(), right=I.pinhole(), t=(0.1, 0, 0)), **bad))


# ------------------------------------------------------------------------------------------------------------ the check
def test_rigs_check_accepts_three_valid_rigs_and_names_field_and_stream():
    lib = L.load()
    f, who = lib.egotap_stereo_rigs_check, b"egotap_stereo_rigs_check"
    rigs = _rigs()
    assert f(_table(rigs), 3) == 0 and f(_table(rigs[:1]), 1) == 0
    assert len(L.stereo_rigs_host(rigs)) == 3
    _refused(lib, f, who, None, 3, word=b"null rig table")
    _refused(lib, f, who, _table(rigs), 0, word=b"between 1 and 4096")
    _refused(lib, f, who, _table(rigs), -2, word=b"between 1 and 4096")
    _refused(lib, f, who, _table(rigs), 4097, word=b"between 1 and 4096")
    nan, inf = float("nan"), float("inf")

    def cam(side, **kw):
        def edit(row):
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(getattr(row, side), v[0])[v[1]] = v[2]
                else:
                    setattr(getattr(row, side), k, v)
        return edit

    def arr(name, k, v):
        def edit(row):
            a = getattr(row, name)
            if name == "affine":
                a[k // 4][k % 4] = v
            else:
                a[k] = v
        return edit

    def score(v):
        return lambda row: setattr(row, "min_score", v)
    bad = [(cam("left", n_pol=0), b"left: polynomialC2W (n_pol)"), (cam("left", n_pol=9), b"left: polynomialC2W (n_pol)"),
           (cam("right", n_invpol=0), b"right: polynomialW2C (n_invpol)"), (cam("right", n_invpol=25), b"right: polynomialW2C (n_invpol)"),
           (cam("left", c=0.0, d=0.0), b"left: the affine is singular (c - d * e == 0)"), (cam("right", c=2.0, d=4.0, e=0.5), b"right: the affine is singular"),
           (cam("left", xc=nan), b"left: a calibration value is not finite"), (cam("right", e=inf), b"right: a calibration value is not finite"),
           (cam("right", p=("pol", 0, nan)), b"right: a calibration value is not finite"), (cam("left", p=("invpol", 0, -inf)), b"left: a calibration value is not finite"),
           (cam("left", ue_flip=0.5), b"left: ue_flip must be 0 or 1"), (cam("right", ue_flip=nan), b"right: ue_flip must be 0 or 1"),
           (arr("R", 7, nan), b"R must be finite"), (arr("R", 0, inf), b"R must be finite"), (arr("t", 2, nan), b"t must be finite"),
           (arr("affine", 5, inf), b"affine must be finite"), (arr("affine", 0, nan), b"affine must be finite"),
           (score(nan), b"min_score must be finite"), (score(-inf), b"min_score must be finite")]
    for s in range(3):
        for edit, word in bad:
            t = _table(rigs)
            edit(t[s])
            _refused(lib, f, who, t, 3, word=b"rig %d: " % s + word)
            if s:
                assert f(t, s) == 0          # the rows in front of the bad one pass
    # a coefficient behind the length is not read: a NaN there is no refusal
    t = _table(rigs)
    t[2].left.pol[7] = nan
    assert f(t, 3) == 0
    # the Python faces: the same refusals, the stream's index kept
    with pytest.raises(L.EgotapError, match="rig 1: t must be finite"):
        L.stereo_rigs_host([rigs[0], dataclasses.replace(rigs[1], t=(0.0, nan, 0.0)), rigs[2]])
    with pytest.raises(L.EgotapError, match="rig 4: min_score must be finite"):
        L.stereo_rig_check(dataclasses.replace(rigs[0], min_score=inf), 4)
    with pytest.raises(L.EgotapError, match="between 1 and 4096"):
        L.stereo_rigs_host([])


# ------------------------------------------------------------------------------------------------------------ the launching entries
RIGS_DEV = 0x700000


def test_triangulate_streams_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    B, J, Pn, S = 6, 15, 16, 3
    kp, pose, j3, fr = 0x100000, 0x200000, 0x300000, 0x400000
    ok = dict(kp=P(kp), B=B, J=J, rigs=P(RIGS_DEV), S=S, pose=P(pose), P=Pn, row0=1, j3=P(j3), fr=P(fr))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_stereo_triangulate_streams(a["kp"], a["B"], a["J"], a["rigs"], a["S"], a["pose"], a["P"], a["row0"], a["j3"], a["fr"], None)
        return rc, lib.egotap_last_error().decode()
    kp_b, pose_b = B * 2 * J * 16, B * Pn * 12
    cases = [(dict(S=0), "between 1 and 4096"), (dict(S=-1), "between 1 and 4096"), (dict(S=4097, B=4097), "between 1 and 4096"),
             (dict(S=4), "multiple of the number of streams"), (dict(B=7), "multiple of the number of streams"), (dict(B=2), "multiple of the number of streams"),
             (dict(rigs=None), "null rig table"), (dict(rigs=P(RIGS_DEV + 4)), "8-byte aligned"), (dict(rigs=P(RIGS_DEV + 1)), "8-byte aligned"),
             # everything the twin refuses of the arguments the two share
             (dict(kp=None), "null"), (dict(j3=None), "null"), (dict(fr=None), "null"),
             (dict(B=0), "must be positive"), (dict(J=0), "must be positive"), (dict(B=-3), "must be positive"), (dict(J=65), "at most 64 joints"),
             (dict(kp=P(kp + 8)), "16-byte aligned"), (dict(j3=P(j3 + 4)), "16-byte aligned"), (dict(fr=P(fr + 8)), "16-byte aligned"), (dict(pose=P(pose + 2)), "4-byte aligned"),
             (dict(row0=2), "pose rows"), (dict(row0=-1), "pose rows"), (dict(P=14, row0=0), "pose rows"),
             (dict(j3=P(kp)), "must not overlap"), (dict(j3=P(kp + kp_b - 16)), "must not overlap"), (dict(fr=P(pose + pose_b - 16)), "must not overlap"),
             (dict(fr=P(j3 + 32)), "must not overlap")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == INVALID and msg.startswith("egotap_stereo_triangulate_streams:") and word in msg, (kw, rc, msg)
    rc, msg = call(pose=None, P=0, row0=99, B=0)          # without a pose its rows are not looked at; the batch is
    assert rc == INVALID and "must be positive" in msg


def test_fuse_streams_refuses_by_name_before_any_launch():
    lib = L.load()
    P = C.c_void_p
    B, J, Pn, S = 6, 15, 16, 3
    kp, pose, fr, fu, pf, st = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000

    def prm(**kw):
        o = L.fuse_params_struct(spec.FuseParams(sigma_prior=0.05))
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    ok = dict(kp=P(kp), B=B, J=J, rigs=P(RIGS_DEV), S=S, pose=P(pose), P=Pn, row0=1, fr=P(fr), prm=prm(), fu=P(fu), pf=P(pf), st=P(st))

    def call(**kw):
        a = dict(ok, **kw)
        rc = lib.egotap_stereo_fuse_streams(a["kp"], a["B"], a["J"], a["rigs"], a["S"], a["pose"], a["P"], a["row0"], a["fr"],
                                            C.byref(a["prm"]) if a["prm"] is not None else None, a["fu"], a["pf"], a["st"], None)
        return rc, lib.egotap_last_error().decode()
    nan, inf = float("nan"), float("inf")
    kp_b, pose_b, fr_b, fu_b = B * 2 * J * 16, B * Pn * 12, B * 32, B * J * 32
    cases = [(dict(S=0), "between 1 and 4096"), (dict(S=-7), "between 1 and 4096"), (dict(S=4097, B=4097), "between 1 and 4096"),
             (dict(S=4), "multiple of the number of streams"), (dict(B=5), "multiple of the number of streams"),
             (dict(rigs=None), "null rig table"), (dict(rigs=P(RIGS_DEV + 4)), "8-byte aligned"),
             (dict(kp=None), "null"), (dict(pose=None), "null"), (dict(fr=None), "null"), (dict(prm=None), "null"), (dict(fu=None), "null"), (dict(pf=None), "null"),
             (dict(st=None), "null"), (dict(B=0), "must be positive"), (dict(J=0), "must be positive"), (dict(J=65), "at most 64 joints"),
             (dict(kp=P(kp + 8)), "16-byte aligned"), (dict(fr=P(fr + 4)), "16-byte aligned"), (dict(fu=P(fu + 8)), "16-byte aligned"), (dict(st=P(st + 4)), "16-byte aligned"),
             (dict(pose=P(pose + 2)), "4-byte aligned"), (dict(pf=P(pf + 1)), "4-byte aligned"),
             (dict(row0=2), "pose rows"), (dict(row0=-1), "pose rows"), (dict(P=14, row0=0), "pose rows"),
             (dict(prm=prm(sigma_ray=0.0)), "sigma_ray"), (dict(prm=prm(sigma_ray=nan)), "sigma_ray"), (dict(prm=prm(sigma_prior=-0.05)), "sigma_prior"),
             (dict(prm=prm(sigma_prior=inf)), "sigma_prior"), (dict(prm=prm(max_sigma=nan)), "max_sigma"), (dict(prm=prm(max_sigma=-1.0)), "max_sigma"),
             (dict(prm=prm(min_joints=-1)), "min_joints"),
             (dict(fu=P(kp)), "fused overlaps keypoints"), (dict(fu=P(pose + pose_b - 16)), "fused overlaps pose"), (dict(fu=P(fr)), "fused overlaps frame"),
             (dict(st=P(fr + fr_b - 32)), "stats overlaps frame"), (dict(pf=P(kp)), "pose_fused overlaps keypoints"), (dict(pf=P(pose + 12)), "pose_fused overlaps pose"),
             (dict(pf=P(fu + fu_b - 4)), "fused overlaps pose_fused"), (dict(st=P(fu)), "fused overlaps stats")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == INVALID and msg.startswith("egotap_stereo_fuse_streams:") and word in msg, (kw, rc, msg)


def test_lens_remap_streams_refusals():
    lib = L.load()
    f, who = lib.egotap_lens_remap_streams, b"egotap_lens_remap_streams"
    l8, r8, ol, orr = (C.c_void_p(a) for a in (0x200001, 0x300003, 0x500000, 0x600000))
    d = C.byref(_desc())
    for S in (0, -1, 4097):
        _refused(lib, f, who, l8, r8, 6, d, S, 64, ol, orr, None, word=b"between 1 and 4096")
    _refused(lib, f, who, l8, r8, 6, d, 4, 64, ol, orr, None, word=b"multiple of the number of streams")
    _refused(lib, f, who, l8, r8, 2, d, 3, 64, ol, orr, None, word=b"multiple of the number of streams")
    # what the entry without _streams refuses
    _refused(lib, f, who, l8, r8, 0, d, 3, 64, ol, orr, None, word=b"batch must be positive")
    _refused(lib, f, who, None, r8, 6, d, 3, 64, ol, orr, None, word=b"null frames")
    _refused(lib, f, who, l8, r8, 6, None, 3, 64, ol, orr, None, word=b"null source descriptor")
    _refused(lib, f, who, l8, r8, 6, d, 3, 64, None, orr, None, word=b"null output")
    _refused(lib, f, who, l8, r8, 6, d, 3, 64, ol, C.c_void_p(0x600001), None, word=b"4-byte aligned")
    for S0 in (0, 62, 4100):
        _refused(lib, f, who, l8, r8, 6, d, 3, S0, ol, orr, None, word=b"multiple of 4")
    even, quad = (C.c_void_p(0x200002), C.c_void_p(0x300006)), (C.c_void_p(0x200004), C.c_void_p(0x300008))
    for kw, word in BAD_DESCS:
        a, b = quad if kw.get("fmt") == "yuyv" else even
        _refused(lib, f, who, a, b, 6, C.byref(_desc(**kw)), 3, 64, ol, orr, None, word=word)


@pytest.mark.parametrize("suffix", ["", "_kp", "_kpl"])
def test_one_call_streams_refusals(suffix):
    lib, h = _handle(hm=32)
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_lens_workspace_bytes(h, 4, 3, C.byref(need)) == 0          # the workspace is the entry's without _streams
        name = "egotap_predict_pose_lens_streams" + suffix
        fn, who = getattr(lib, name), name.encode()
        extra = {"": (), "_kp": (C.c_void_p(0x4000000),), "_kpl": (C.c_void_p(0x4000000), C.c_void_p(0x5000000))}[suffix]

        def f(*a):
            return fn(*a, *extra)
        l8, r8, tab, pose, hmp, ws = (C.c_void_p(a) for a in (0x200002, 0x300002, 0x400000, 0x500000, 0x600000, 0x700000))
        d = C.byref(_desc())
        for S in (0, -1, 4097):
            _refused(lib, f, who, h, l8, r8, 4, d, S, tab, pose, hmp, 3, ws, need.value, None, word=b"between 1 and 4096")
        _refused(lib, f, who, h, l8, r8, 4, d, 3, tab, pose, hmp, 3, ws, need.value, None, word=b"multiple of the number of streams")
        _refused(lib, f, who, None, l8, r8, 4, d, 2, tab, pose, hmp, 3, ws, need.value, None, word=b"null handle")
        _refused(lib, f, who, h, None, r8, 4, d, 2, tab, pose, hmp, 3, ws, need.value, None, word=b"null frames")
        _refused(lib, f, who, h, l8, r8, 4, None, 2, tab, pose, hmp, 3, ws, need.value, None, word=b"null source descriptor")
        _refused(lib, f, who, h, l8, r8, 4, d, 2, None, pose, hmp, 3, ws, need.value, None, word=b"null table")
        _refused(lib, f, who, h, l8, r8, 0, d, 2, tab, pose, hmp, 3, ws, need.value, None, word=b"batch must be positive")
        _refused(lib, f, who, h, l8, r8, 4, d, 2, tab, pose, hmp, -1, ws, need.value, None, word=b"chunk")
        _refused(lib, f, who, h, l8, r8, 4, d, 2, tab, pose, hmp, 3, ws, need.value - 1, None, word=b"workspace too small")
        quad = (C.c_void_p(0x200004), C.c_void_p(0x300008))
        for kw, word in BAD_DESCS:
            a, b = quad if kw.get("fmt") == "yuyv" else (l8, r8)
            _refused(lib, f, who, h, a, b, 4, C.byref(_desc(**kw)), 2, tab, pose, hmp, 3, ws, need.value, None, word=word)
        _refused(lib, f, who, h, l8, r8, 4, C.byref(_desc(model_h=0)), 2, tab, pose, hmp, 3, ws, need.value, None, word=b"model camera's calibration image")
        form = C.c_int(-1)
        assert lib.egotap_debug_predict_pose_rgb_form(h, C.byref(form)) == 0 and form.value == 0          # nothing ran
    finally:
        lib.egotap_destroy(h)


# ------------------------------------------------------------------------------------------------------------ the restatements
def test_lens_remap_streams_u8_with_one_stream_is_lens_remap_u8():
    H, W, S0 = 37, 53, 8
    model = dataclasses.replace(I.pinhole(20.0, "helper"), xc=31.25, yc=23.75, size=(48, 64))
    lenses = [spec.lens_map(model, dataclasses.replace(I.pinhole(f, "helper"), xc=xc, yc=yc, size=(H, W)), S0, mirror=bool(k & 1))
              for k, (f, xc, yc) in enumerate(((40.0, 30.0, 16.0), (30.0, 20.0, 20.0), (50.0, 26.0, 18.0)))]
    assert len({m.taps.tobytes() for m in lenses}) == 3 and all(0.05 < m.valid.mean() for m in lenses)
    frames = np.random.default_rng(5).integers(0, 256, (6, H, W, 3), dtype=np.uint8)
    one = spec.lens_remap_streams_u8(frames, lenses[:1], (9, 8, 7))
    assert one.dtype == np.uint8 and np.array_equal(one, spec.lens_remap_u8(frames, lenses[0], (9, 8, 7)))
    three = spec.lens_remap_streams_u8(frames, lenses, (9, 8, 7))
    for s, m in enumerate(lenses):
        assert np.array_equal(three[s::3], spec.lens_remap_u8(frames[s::3], m, (9, 8, 7)))
    assert not np.array_equal(three, spec.lens_remap_u8(frames, lenses[0], (9, 8, 7)))          # the streams do differ
    import torch
    assert torch.equal(spec.lens_remap_streams_u8(torch.from_numpy(frames), lenses, (9, 8, 7)), torch.from_numpy(three))
    with pytest.raises(ValueError, match="multiple of the number of streams"):
        spec.lens_remap_streams_u8(frames[:5], lenses)
    with pytest.raises(ValueError, match="one S0"):
        spec.lens_remap_streams_u8(frames, [lenses[0], spec.lens_map(model, model, 4)])
    with pytest.raises(ValueError, match="list of spec.LensMap"):
        spec.lens_remap_streams_u8(frames, [])


def test_stereo_streams_restatements_are_the_single_rig_ones_on_strided_rows():
    rigs = _rigs()
    S, T, J, P = 3, 2, 15, 16
    kp, _, _ = I.pinhole_case(S * T, J, seed=3)
    kp = kp.astype(np.float32)
    pose = np.random.default_rng(1).normal(0, 0.3, (S * T, P, 3)).astype(np.float32)
    j3, fr = spec.stereo_triangulate_streams_ref(kp, rigs, pose=pose, pose_row0=1)
    prm = spec.FuseParams(sigma_prior=0.05)
    fused = spec.stereo_fuse_streams_ref(kp, pose, fr, rigs, prm, pose_row0=1)
    for s, g in enumerate(rigs):
        w3, wf = spec.stereo_triangulate_ref(kp[s::S], g.left, g.right, g.t, R=g.R, affine=g.affine, min_score=g.min_score, pose=pose[s::S], pose_row0=1)
        assert np.array_equal(j3[s::S].view(np.int32), w3.view(np.int32)) and np.array_equal(fr[s::S].view(np.int32), wf.view(np.int32))
        want = spec.stereo_fuse_ref(kp[s::S], pose[s::S], fr[s::S], g.left, g.right, g.t, prm, R=g.R, affine=g.affine, min_score=g.min_score, pose_row0=1)
        for a, b in zip(fused, want):
            assert a.dtype == b.dtype and np.array_equal(a[s::S].view(np.int32), b.view(np.int32))
    w3, wf = spec.stereo_triangulate_streams_ref(kp, rigs[:1])
    r3, rf = spec.stereo_triangulate_ref(kp, rigs[0].left, rigs[0].right, rigs[0].t, R=rigs[0].R)
    assert np.array_equal(w3.view(np.int32), r3.view(np.int32)) and np.array_equal(wf.view(np.int32), rf.view(np.int32))
    with pytest.raises(ValueError, match="multiple of the number of streams"):
        spec.stereo_triangulate_streams_ref(kp[:4], rigs)
    with pytest.raises(ValueError, match="list of 1 .. 4096 spec.StereoRig"):
        spec.stereo_fuse_streams_ref(kp, pose, fr, [], prm)


def test_python_faces_check_their_arguments_without_a_gpu():
    import torch
    kp, pose, fr = torch.zeros(6, 2, 15, 4), torch.zeros(6, 16, 3), torch.zeros(6, 8)
    table = torch.zeros(3 * 792, dtype=torch.uint8)
    prm = spec.FuseParams(sigma_prior=0.05)
    with pytest.raises(ValueError, match="keypoints are a tensor"):
        L.stereo_triangulate_streams(kp[:, :1], table, 3)
    with pytest.raises(ValueError, match="pose_row0"):
        L.stereo_triangulate_streams(kp, table, 3, pose=pose, pose_row0=2)
    with pytest.raises(ValueError, match="what stereo_rigs_table returns"):
        L.stereo_triangulate_streams(kp, table[:-1], 3)
    with pytest.raises(ValueError, match="what stereo_rigs_table returns"):
        L.stereo_triangulate_streams(kp, table, 0)
    with pytest.raises(ValueError, match="multiple of the number of streams"):
        L.stereo_triangulate_streams(kp[:5], table, 3)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.stereo_triangulate_streams(kp, table, 3)
    with pytest.raises(ValueError, match="FuseParams"):
        L.stereo_fuse_streams(kp, pose, fr, table, 3, None)
    with pytest.raises(ValueError, match="frame is a tensor"):
        L.stereo_fuse_streams(kp, pose, fr[:, :7], table, 3, prm)
    with pytest.raises(ValueError, match="multiple of the number of streams"):
        L.stereo_fuse_streams(kp[:4], pose[:4], fr[:4], table, 3, prm)
    with pytest.raises(L.EgotapError, match="GPU only"):
        L.stereo_fuse_streams(kp, pose, fr, table, 3, prm)
    with pytest.raises(L.EgotapError, match="lives on the GPU"):
        L.stereo_rigs_table(_rigs(), device="cpu")
    a = spec.LensMap(np.full((4, 4, 2), -1, dtype=np.int32), 4, 5, 7, (8, 8))
    b = spec.LensMap(np.full((4, 4, 2), -1, dtype=np.int32), 4, 5, 7, (8, 8), mirror=True)
    with pytest.raises(ValueError, match="list of 1 .. 4096"):
        L.lens_maps([])
    with pytest.raises(ValueError, match="list of 1 .. 4096"):
        L.lens_maps([(a, a, a)])
    with pytest.raises(ValueError, match="stream 1's maps differ"):
        L.lens_maps([(a, a), (a, b)])
    with pytest.raises(ValueError, match="are spec.LensMap"):
        L.lens_maps([(a, None)])
