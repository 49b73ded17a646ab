"""Inputs and comparison rules shared by tests/test_limb_decode_cpu.py and tests/test_gpu_limb_decode.py (not a test module).

One host tensor per (preset, side, storage): [3, 6J + 2, S, S] float32 (bf16-representable when asked); the operator reads the slice
[:, 1:1 + 6J] with c0 = 2J, so the image stride exceeds the slice.  Frame 0 holds the oracle's target maps of seeded joints, frame 1 the targets of
other joints plus uniform noise of amplitude 0.05 on every limb channel, frame 2 one special pair per (eye, limb): KINDS in turn."""
import functools

import numpy as np

from egotap_amd import spec
from oracle import heatmap_synth_ref as R

PRESETS = {15: "UnrealEgo", 17: "EgoCap"}
B = 3
NOISE = 0.05
JOINT_SEED = 0
KINDS = ["first", "last", "wave0", "wave1", "wave2", "wave3", "zero", "nan", "inf", "run_h", "run_v", "run_d", "single"]
SINGLE = ("first", "last", "wave0", "wave1", "wave2", "wave3", "single")
RUNS = ("run_h", "run_v", "run_d")
EMPTY = ("zero", "nan", "inf")
RUN_K = 7
MIRROR = [(4.0, 0.0, 4.0, 0.0), (-4.0, 256.0, 4.0, 0.0)]          # the right eye mirrored (|ax| = |ay|: length stays exact)


def bf16_round(a):
    """float32 -> the nearest bf16 (ties to even), as float32; NaN and inf pass"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return np.where(np.isfinite(a), r.view(np.float32), a).astype(np.float32)


@functools.lru_cache(maxsize=None)
def targets(J, S):
    """the oracle's maps of two seeded frames: [2, 6J, S, S] float32 (computed once per shape; treat as read-only)"""
    rng = np.random.default_rng(JOINT_SEED + J)
    p2l, p2r = (rng.uniform(-60.0, 1080.0, (2, J + 1, 2)) for _ in range(2))
    p3 = rng.uniform(-40.0, 40.0, (2, J + 1, 3))
    out = np.stack([R.process_frame(p2l[b], p2r[b], p3[b], PRESETS[J], S)[0] for b in range(2)])
    out.setflags(write=False)
    return out


def wave_positions(S, bf16):
    """an element in each wave's share: maps of 4096 elements and more are read by four waves, 64 consecutive 16-byte vectors of every 256 each (the
    second pass where the map has one); smaller maps by one wave: an element in each quarter"""
    HW, span = S * S, 256 * (8 if bf16 else 4)
    return [(span if HW >= 2 * span else 0) + (span // 4) * w + 37 if HW >= 4096 else (HW // 4) * w + 37 for w in range(4)]


def kind_of(J, eye, limb):
    return KINDS[(eye * J + limb) % len(KINDS)]


@functools.lru_cache(maxsize=None)
def tensor(J, S, bf16):
    """[3, 6J + 2, S, S] float32 on the host, read-only"""
    rng = np.random.default_rng(100 * J + S)
    h = rng.standard_normal((B, 6 * J + 2, S, S)).astype(np.float32)              # filler around and in front of the limb channels
    t = targets(J, S)
    lo = 1 + 2 * J                                                                  # first limb channel of the big tensor
    h[0, 1:1 + 6 * J] = t[0]
    h[1, lo:lo + 4 * J] = t[1, 2 * J:] + rng.uniform(-NOISE, NOISE, (4 * J, S, S)).astype(np.float32)
    HW, waves = S * S, wave_positions(S, bf16)
    for eye in range(2):
        for limb in range(J):
            c, s = (h[2, lo + eye * 2 * J + k * J + limb].reshape(HW) for k in range(2))
            c[:] = 0
            s[:] = 0
            kind = kind_of(J, eye, limb)
            if kind in SINGLE:
                at = {"first": 0, "last": HW - 1, "single": 5 * S + 9}.get(kind)
                at = waves[int(kind[4])] if at is None else at
                c[at], s[at] = 3.0, 4.0
            elif kind in RUNS:
                for i in range(RUN_K):
                    at = {"run_h": 6 * S + 3 + i, "run_v": (3 + i) * S + 6, "run_d": (3 + i) * S + 4 + i}[kind]
                    c[at], s[at] = 0.5, -1.0
            elif kind in ("nan", "inf"):
                c[2 * S + 3], s[2 * S + 3] = 1.0, 2.0
                c[2 * S + 4] = np.nan if kind == "nan" else np.inf
    if bf16:
        h = bf16_round(h)
    h.setflags(write=False)
    return h


def reference(J, S, bf16, affine):
    return spec.limb_decode_ref(tensor(J, S, bf16)[:, 1:1 + 6 * J], 2 * J, J, 2, affine=affine)


def category(J):
    """[3, 2, J] of str: 'target', 'noisy' or the special kind of each record"""
    cat = np.empty((B, 2, J), dtype=object)
    cat[0], cat[1] = "target", "noisy"
    for eye in range(2):
        for limb in range(J):
            cat[2, eye, limb] = kind_of(J, eye, limb)
    return cat


def ulps(got, want):
    """distance in float32 steps (finite values of one sign, or equal zeros)"""
    g, w = (np.ascontiguousarray(t, dtype=np.float32).view(np.int32).astype(np.int64) for t in (got, want))
    g, w = (np.where(t < 0, -(t & 0x7FFFFFFF), t) for t in (g, w))
    return np.abs(g - w)


def compare(got, want, J, affine, out=print):
    """The issue's tolerances, derived there: both sides sum in float64, so each output is one float32 rounding of nearly the same float64 value.
    coherence, x, y, peak, mass: 2 ulp; theta: 2^-22 pi where coherence >= 1e-3; phi: 2^-22 pi modulo pi where length >= 1 heatmap pixel;
    length^2 / 12: 1e-4 max(ax^2, ay^2) absolute plus 2^-21 relative; empty records bit-equal (NaN mass = NaN mass).  Returns the share of records each
    gate excluded per category.  Prints every figure before asserting."""
    got, want = (np.ascontiguousarray(t, dtype=np.float32) for t in (got, want))
    assert got.shape == want.shape == (B, 2, J, 8), (got.shape, want.shape)
    a = np.array([(1.0, 0.0, 1.0, 0.0)] * 2 if affine is None else affine, dtype=np.float64)
    scale2 = np.maximum(a[:, 0] ** 2, a[:, 2] ** 2).reshape(1, 2, 1)
    px = np.sqrt(scale2)                                                           # output units per heatmap pixel
    empty = ~((want[..., 7] > 0) & np.isfinite(want[..., 7]))
    # empty records: equal bits, a NaN mass equal to a NaN mass
    ge, we = got[empty], want[empty]
    nan = np.isnan(we)
    assert np.array_equal(np.isnan(ge), nan) and np.array_equal(ge.view(np.int32)[~nan], we.view(np.int32)[~nan]), (ge, we)
    full = ~empty
    assert np.isfinite(got[full]).all()
    u = ulps(got[full][:, [1, 2, 3, 6, 7]], want[full][:, [1, 2, 3, 6, 7]])
    theta_ok = full & (want[..., 1] >= 1e-3)
    phi_ok = full & (want[..., 5] >= px)
    tol = 2.0 ** -22 * np.pi
    dth = np.abs(got[..., 0].astype(np.float64) - want[..., 0])
    dphi = np.abs(got[..., 4].astype(np.float64) - want[..., 4])
    dphi = np.minimum(dphi, np.pi - dphi)
    l2g, l2w = got[..., 5].astype(np.float64) ** 2 / 12, want[..., 5].astype(np.float64) ** 2 / 12
    dl = np.abs(l2g - l2w) - (1e-4 * scale2 + 2.0 ** -21 * l2w)
    out(f"limb_decode compare: {int(full.sum())} full, {int(empty.sum())} empty; max ulp (coherence, x, y, peak, mass) {u.max(axis=0).tolist() if u.size else []}; "
        f"max |dtheta| {dth[theta_ok].max() if theta_ok.any() else 0:.3e}, max |dphi| {dphi[phi_ok].max() if phi_ok.any() else 0:.3e} (tol {tol:.3e}); "
        f"max length^2/12 excess {dl[full].max() if full.any() else 0:.3e}")
    assert (u <= 2).all(), u.max(axis=0)
    assert (dth[theta_ok] <= tol).all() and (dphi[phi_ok] <= tol).all()
    assert (dl[full] <= 0).all()
    return excluded(want, J, affine)


def excluded(want, J, affine):
    """per category: (records that are not empty, of those excluded by the theta gate, by the phi gate)"""
    a = np.array([(1.0, 0.0, 1.0, 0.0)] * 2 if affine is None else affine, dtype=np.float64)
    px = np.sqrt(np.maximum(a[:, 0] ** 2, a[:, 2] ** 2)).reshape(1, 2, 1)
    full = (want[..., 7] > 0) & np.isfinite(want[..., 7])
    cat = category(J)
    res = {}
    for name in ["target", "noisy"] + KINDS:
        sel = full & (cat == name)
        res[name] = (int(sel.sum()), int((sel & ~(want[..., 1] >= 1e-3)).sum()), int((sel & ~(want[..., 5] >= px)).sum()))
    return res


def check_gates(ex):
    """the gates exclude nothing on targets and runs, the theta gate nothing on a single mass (a point has no orientation: its length is 0 and phi is
    not defined), and on the noisy frame the two gates together at most 5 % of the records"""
    for name, (n, no_theta, no_phi) in ex.items():
        if name in EMPTY:
            assert n == 0, (name, n)
        elif name == "noisy":
            assert n > 0 and no_theta + no_phi <= 0.05 * n, (name, n, no_theta, no_phi)
        elif name in SINGLE:
            assert no_theta == 0, (name, n, no_theta)
        else:
            assert no_theta == 0 and no_phi == 0, (name, n, no_theta, no_phi)
    assert ex["target"][0] > 0 and all(ex[k][0] > 0 for k in RUNS + SINGLE)
