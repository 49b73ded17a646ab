"""The modes of attention_f32_kernel (csrc/attention_f32.h) that only whole-head tests used to reach, one operator call each against float64:
a ragged sequence (N % 32 != 0: the last key tile and query block start at N - 32, the re-covered keys are masked), the key split with its
merge kernel, the live-query launch of the pose-only forward and the log-sum-exp output of the training forward.

Every output buffer (ctx, lse, split scratch) is filled with a NaN bit pattern and carries a tail behind what the call may write -- 32 rows, or 4096
floats -- that must keep those bits; a row the kernel should have written and did not stays NaN and fails its comparison.  All inputs lie in
bounds.  Failure messages name the mode, N, the overlap of the ragged tile, the split count and the (b, h, query row) of the worst element."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DH = 128
TAIL_ROWS, TAIL_FLOATS = 32, 4096
SENT_BITS = 0x7FC5A5A5                 # a quiet NaN with a payload no kernel produces
RAGGED = [36, 40, 44, 48, 52, 56, 60, 76, 100, 132, 144]      # overlaps 28 .. 4 in two tiles; a middle tile; two query groups; an idle second wave; side 32
SHAPES = [(1, 1), (2, 2)]


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


def _tiles(N):
    return (N + 31) // 32


def _overlap(N):
    return _tiles(N) * 32 - N


def _per_split(B, N, heads):
    return B * N * heads * DH + B * heads * N


def _sentinel(*shape):
    return torch.full(shape, SENT_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _tail_intact(buf, used, what, label):
    tail = buf.view(-1)[used:].view(torch.int32)
    bad = (tail != SENT_BITS).nonzero()
    assert bad.numel() == 0, f"{label}: {what} written {bad.numel()} floats past its end, first at +{int(bad[0])} of a {tail.numel()}-float tail"


def _ref(B, q, k, v):
    """THE reference: float64 softmax(q k^T / sqrt(128)) v and logsumexp on the CPU.  q [B*Nq, D], k / v [B*N, D] (heads side by side) ->
    ctx [B*Nq, D], lse [B, heads, Nq]"""
    heads = k.shape[1] // DH
    q, k, v = [t.double().reshape(B, -1, heads, DH).transpose(1, 2) for t in (q, k, v)]
    s = q @ k.transpose(-1, -2) / math.sqrt(float(DH))
    ctx = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(-1, heads * DH)
    return ctx, torch.logsumexp(s, -1)


@functools.lru_cache(maxsize=None)
def _case(B, N, heads, seed=41, lo=-2.0, hi=2.0):
    """random qkv [B*N, 3D] (CPU, never modified) with its float64 ctx and lse: computed once, shared by the tests"""
    D = heads * DH
    qkv = _rand((B * N, 3 * D), seed, lo, hi)
    ctx, lse = _ref(B, *qkv.split(D, dim=1))
    return qkv, ctx, lse


def _check(got, ref, tol, rows_per_image, heads, label):
    """max |got - ref| <= tol over the first ref.shape[0] rows of got; the message names the worst (b, h, query row)"""
    err = (got[:ref.shape[0]].cpu().double() - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    i = int(err.argmax())
    row, col = divmod(i, ref.shape[1])
    worst = float(err.view(-1)[i])
    print(f"[attention_f32 modes] {label}: max|err| = {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol, (f"{label}: max|err| = {worst:.3e} > {tol:.3e} at (b, h, query row) = ({row // rows_per_image}, {col // DH}, {row % rows_per_image}), "
                          f"channel {col % DH}: got {float(got[row, col])}, float64 {float(ref[row, col])}")
    return worst


def _label(mode, B, N, heads, k=1, extra=""):
    return f"mode={mode} N={N} overlap={_overlap(N)} k={k} B={B} heads={heads}{extra}"


def _split_plan(B, N, heads, k, via):
    """(scratch_floats, num_cu) under which the planner must pick k: 'scratch' = room for exactly k partial sets on a whole chip, 'cu' = room
    for 8 sets but only as many compute units as k ranges of workgroups fill"""
    per = _per_split(B, N, heads)
    if via == "scratch":
        return k * per, 256
    wgs = B * heads * ((_tiles(N) + 1) // 2)
    return 8 * per, -(-2 * wgs * k // 9)


def _run_split(qkv, B, N, heads, k, via, label):
    """the forward's launch through the split hook, k asserted first (a condition: no case runs unsplit), sentinels behind ctx and the scratch"""
    from egotap_amd import lib
    scratch_floats, cu = _split_plan(B, N, heads, k, via)
    picked = lib.attention_f32_ksplit(B, N, heads, scratch_floats, cu)
    assert picked == k and k > 1, f"{label}: the planner picked k = {picked} for scratch_floats = {scratch_floats}, num_cu = {cu}; this case needs k = {k}"
    dev = qkv.cuda()
    outs = []
    for _ in range(2):
        ctx = _sentinel(B * N + TAIL_ROWS, heads * DH)
        scratch = _sentinel(scratch_floats + TAIL_FLOATS)
        lib.attention_f32_split(dev, B, N, heads, scratch, scratch_floats, cu, out=ctx)
        _tail_intact(ctx, B * N * heads * DH, "ctx", label)
        _tail_intact(scratch, scratch_floats, "the split scratch", label)
        if via == "scratch":      # the partials end exactly at scratch_floats: each of them was written
            unwritten = int((scratch[:scratch_floats].view(torch.int32) == SENT_BITS).sum())
            assert unwritten == 0, f"{label}: {unwritten} floats of the {k} partial sets were never written"
        outs.append(ctx)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{label}: two calls differ in bits"
    return outs[0]


# ------------------------------------------------------------------------------------------------ a. ragged forward
@pytest.mark.parametrize("B,heads", SHAPES)
@pytest.mark.parametrize("N", RAGGED, ids=[f"N{n}-ov{_overlap(n)}" for n in RAGGED])
def test_ragged_forward(N, B, heads):
    from egotap_amd import lib
    qkv, ref, _ = _case(B, N, heads)
    label = _label("ragged", B, N, heads)
    dev = qkv.cuda()
    ctx = _sentinel(B * N + TAIL_ROWS, heads * DH)
    lib.attention(dev, B, N, heads, out=ctx)
    _tail_intact(ctx, B * N * heads * DH, "ctx", label)
    _check(ctx, ref, 3e-6, N, heads, label)
    again = lib.attention(dev, B, N, heads)
    assert torch.equal(again, ctx[:B * N]), f"{label}: two calls differ in bits"
    for mode in ("bf16x3", "bf16"):       # the documented fallback by name: a ragged sequence runs the exact-fp32 kernel in every precision
        assert torch.equal(lib.attention(dev, B, N, heads, precision=mode), ctx[:B * N]), f"{label}: precision={mode} differs in bits from f32"


# ------------------------------------------------------------------------------------------------ b. key accounting
def _key_home(N, key):
    t = min(key // 32, _tiles(N) - 1)
    if key >= (_tiles(N) - 1) * 32:
        return f"key {key}: tile {t} (the ragged tile, rows from {N - 32}), register row {key - (N - 32)} of it"
    note = f", re-covered and masked in the ragged tile {_tiles(N) - 1}" if key >= N - 32 and _overlap(N) else ""
    return f"key {key}: tile {t}{note}"


@pytest.mark.parametrize("path", ["attention", "split", "live"])
@pytest.mark.parametrize("N", [n for n in RAGGED if n <= 100], ids=[f"N{n}-ov{_overlap(n)}" for n in RAGGED if n <= 100])
def test_every_key_counted_once(N, path):
    """q = k = 0: a uniform softmax over V[j, d] = (d == j), so ctx is 1 / N in the columns of the N keys and 0 elsewhere -- a key counted twice
    or dropped is one wrong column"""
    from egotap_amd import lib
    B, heads = 2, 2
    D = heads * DH
    qkv = torch.zeros(B * N, 3 * D)
    v = torch.zeros(N, DH)
    v[torch.arange(N), torch.arange(N) % DH] = 1.0
    qkv[:, 2 * D:] = v.repeat(B, heads)
    dev = qkv.cuda()
    k = _tiles(N) if path == "split" else 1
    label = _label("keys/" + path, B, N, heads, k)
    Nq = N
    if path == "attention":
        ctx = _sentinel(B * N + TAIL_ROWS, D)
        lib.attention(dev, B, N, heads, out=ctx)
    elif path == "split":
        ctx = _run_split(qkv, B, N, heads, k, "scratch", label)       # one key tile per range
    else:
        Nq = 32
        ctx = _sentinel(B * Nq + TAIL_ROWS, D)
        lib.attention_f32_live(torch.zeros(B * Nq, D, device="cuda"), D, Nq, dev, B, N, heads, out=ctx)
    _tail_intact(ctx, B * Nq * D, "ctx", label)
    want = torch.zeros(DH, dtype=torch.float64)
    want[:N] = 1.0 / N
    got = ctx[:B * Nq].cpu().double().reshape(B * Nq, heads, DH)
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    worst = float(err.max())
    print(f"[attention_f32 modes] {label}: max|err| = {worst:.3e} (tolerance 3.000e-06)")
    if worst > 3e-6:
        row, h, d = [int(i) for i in (err == err.max()).nonzero()[0]]
        where = _key_home(N, d) if d < N else f"column {d}: no key's column"
        raise AssertionError(f"{label}: column {d} of (b, h, query row) = ({row // Nq}, {h}, {row % Nq}) is {float(got[row, h, d])!r}, expected "
                             f"{float(want[d])!r} (a weight of {float(got[row, h, d]) * N:.3f} instead of {1 if d < N else 0}) -- {where}")


# ------------------------------------------------------------------------------------------------ c. log-sum-exp at a ragged N
@pytest.mark.parametrize("N", [36, 52, 100, 144], ids=[f"N{n}-ov{_overlap(n)}" for n in (36, 52, 100, 144)])
def test_ragged_lse(N):
    from egotap_amd import train_ops as T
    B, heads = 2, 2
    D = heads * DH
    qkv, ref, lse_ref = _case(B, N, heads, 31, -1.5, 1.5)
    label = _label("lse", B, N, heads)
    ctx, lse = _sentinel(B * N + TAIL_ROWS, D), _sentinel(B * heads * N + TAIL_FLOATS)
    T.attention_fwd(qkv.cuda(), B, N, heads, out=(ctx, lse))
    _tail_intact(ctx, B * N * D, "ctx", label)
    _tail_intact(lse, B * heads * N, "lse", label)
    _check(ctx, ref, 5e-6, N, heads, label + " ctx")
    err = (lse[:B * heads * N].cpu().double().reshape(B, heads, N) - lse_ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    b, h, n = [int(i) for i in (err == err.max()).nonzero()[0]]
    print(f"[attention_f32 modes] {label} lse: max|err| = {float(err.max()):.3e} (tolerance 1.000e-05)")
    assert float(err.max()) <= 1e-5, (f"{label}: lse max|err| = {float(err.max()):.3e} > 1e-5 at (b, h, query row) = ({b}, {h}, {n}): got "
                                      f"{float(lse[(b * heads + h) * N + n])}, float64 {float(lse_ref[b, h, n])}")


# ------------------------------------------------------------------------------------------------ d. key split + merge
def _split_tol(lse_ref, v):
    """3e-6, the project's bound for one normalised partial (a convex combination of partials cannot exceed it), plus four fp32 roundings of a
    stored log-sum-exp -- 2^-24 |lse| each, doubled -- carried into the merge weights, times the largest value they weigh.  Derived, not measured."""
    return 3e-6 + 8 * 2.0 ** -24 * float(lse_ref.abs().max()) * float(v.abs().max())


SPLITS = [(64, 2, "cu"), (36, 2, "cu"), (144, 5, "cu"), (192, 3, "cu"), (192, 6, "cu"), (224, 7, "cu"), (256, 8, "cu"), (256, 4, "cu"), (192, 3, "scratch")]


@pytest.mark.parametrize("B,heads", SHAPES)
@pytest.mark.parametrize("N,k,via", SPLITS, ids=[f"N{n}-ov{_overlap(n)}-k{k}-{via}" for n, k, via in SPLITS])
def test_key_split(N, k, via, B, heads):
    qkv, ref, lse_ref = _case(B, N, heads)
    label = _label("split", B, N, heads, k, f" via={via}")
    ctx = _run_split(qkv, B, N, heads, k, via, label)
    _check(ctx, ref, _split_tol(lse_ref, qkv[:, 2 * heads * DH:]), N, heads, label)


@pytest.mark.parametrize("B,heads", SHAPES)
@pytest.mark.parametrize("shape", ["one-key-of-the-last-range-40-above", "first-range-40-below"])
def test_key_split_k6_ranges_far_apart(shape, B, heads):
    """N = 192, k = 6 (one key tile per range) with ranges whose log-sum-exps lie ~40 natural units apart: the merge's exp(lse_s - max) underflows
    towards 0 for the light ranges and the result must still be finite and the float64 one"""
    N, k, D = 192, 6, heads * DH
    qkv = _rand((B * N, 3 * D), 47, -0.5, 0.5).reshape(B, N, 3, heads, DH)
    big = 40.0 * math.sqrt(float(DH)) / 8.0
    qkv[:, :, 0, :, 0] = 8.0                     # every query: 8 in channel 0 ...
    qkv[:, :, 1, :, 0] = 0.0                     # ... which no key answers, except
    if shape.startswith("one-key"):
        qkv[:, 170, 1, :, 0] = big               # key 170 (range 5): score 40 above the rest
    else:
        qkv[:, :32, 1, :, 0] = -big              # the keys of range 0: 40 below the rest
    qkv = qkv.reshape(B * N, 3 * D)
    ref, lse_ref = _ref(B, *qkv.split(D, dim=1))
    label = _label("split", B, N, heads, k, f" {shape}")
    ctx = _run_split(qkv, B, N, heads, k, "cu", label)
    assert torch.isfinite(ctx[:B * N]).all(), f"{label}: non-finite ctx"
    _check(ctx, ref, _split_tol(lse_ref, qkv[:, 2 * D:]), N, heads, label)


# ------------------------------------------------------------------------------------------------ e. live queries
LIVE = [(64, 32), (64, 36), (64, 64), (100, 32), (100, 36), (100, 68), (100, 100)]


@pytest.mark.parametrize("layout", ["compact", "inplace"])
@pytest.mark.parametrize("N,Nq", LIVE, ids=[f"N{n}-ov{_overlap(n)}-Nq{q}" for n, q in LIVE])
def test_live_queries(N, Nq, layout):
    """compact: Q in a buffer of its own (ldq = D), the Q columns of qkv all NaN; inplace, the product's layout: query (b, i) in the Q columns of row
    b * Nq + i of qkv (ldq = 3 D), the Q columns of the rows behind them NaN.  Neither NaN may be read."""
    from egotap_amd import lib
    B, heads = 2, 2
    D = heads * DH
    base, _, _ = _case(B, N, heads)
    q = _rand((B * Nq, D), 43, -2, 2)
    qkv = base.clone()
    qkv[:, :D] = float("nan")
    if layout == "inplace":
        qkv[:B * Nq, :D] = q
    ref, _ = _ref(B, q, qkv[:, D:2 * D], qkv[:, 2 * D:])
    label = _label("live/" + layout, B, N, heads, extra=f" Nq={Nq}")
    dev = qkv.cuda()
    ctx = _sentinel(B * Nq + TAIL_ROWS, D)
    if layout == "compact":
        lib.attention_f32_live(q.cuda(), D, Nq, dev, B, N, heads, out=ctx)
    else:
        lib.attention_f32_live(dev, 3 * D, Nq, dev, B, N, heads, out=ctx)
    _tail_intact(ctx, B * Nq * D, "ctx", label)
    _check(ctx, ref, 3e-6, Nq, heads, label)
    if layout == "inplace" and Nq == N:
        assert torch.equal(ctx[:B * N], lib.attention(dev, B, N, heads)), f"{label}: differs in bits from the full launch on the same buffer"
