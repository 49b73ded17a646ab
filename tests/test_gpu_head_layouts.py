"""The lifting head's gather and scatter kernels, operator by operator and element by element, against tests/head_layout_cases.py (the
oracle's view / permute statements; scatters by autograd): the loaders ALoadPatch / ALoadTokens / ALoadRot of the fp32 GEMMs, the scattering
epilogues of both GEMM families (EpiScatterPatch / EpiScatterRot, SEpiScatterTokens / SEpiScatterPatch / SEpiScatterRot),
tokens_scatter_kernel and patch_split_kernel.  Whole training steps reach them too, but behind gates that a misplaced heatmap cell passes.

Placement tests are exact: one-hot rows against coded integer weights (head_layout_cases.coded) give a product that is known without
multiplying and is the same in fp32, bf16x3 and bf16, so every output element is compared with ==, the elements an operator must not write
keep a NaN pattern, and a guard region behind the output keeps its sentinel.  Numeric tests use random operands against float64 on the same
operands with the tolerances of the plain-operand tests of the same kernels (test_gpu_ops.py::test_linear_bias,
test_gpu_train_ops.py::test_gemm_tn, test_gpu_bf16s.py::test_fc1_weight_gradients_on_gathered_rows).

Shapes: UnrealEgo 64^2 at B = 1, 3, 5 -- B T = 30, 90, 150 rows (less than a tile, a ragged tile, past a 128-row boundary), B seq = 576, 1728,
2880; EgoCap 64^2 at B = 4 -- T = 34 of 36 cells, so its last grid row mixes real and dummy cells inside one 32-token tile; both presets at
128^2 (ppd = 8, seq = 2304, K1 = 65536, 2 S^2 = 32768), B = 1, placement only."""
import functools
import math

import pytest
import torch

import head_layout_cases as H

pytestmark = pytest.mark.gpu

CASES_64 = [("UnrealEgo", 64, 1), ("UnrealEgo", 64, 3), ("UnrealEgo", 64, 5), ("EgoCap", 64, 4)]
CASES = CASES_64 + [("UnrealEgo", 128, 1), ("EgoCap", 128, 1)]
MODES = ("f32", "bf16x3", "bf16")
GUARD = 4096
# bit patterns (as the signed integers of the element's width): a quiet NaN with a payload for "never written", an ordinary number for the guard
UNWRITTEN = {torch.float32: 0x7FC0BEEF, torch.bfloat16: 0x7FC1}
SENTINEL = {torch.float32: 0x4B3C614E, torch.bfloat16: 0x4B3C}
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16}


# ---------------------------------------------------------------------------------------------------- outputs with a guard
def _bits(buf):
    return buf.view(INT[buf.dtype])


def _fresh(shape, dtype):
    """(whole buffer, output view of `shape`): the output prefilled with the NaN pattern, GUARD elements of sentinel behind it"""
    n = math.prod(shape)
    buf = torch.empty(n + GUARD, dtype=dtype, device="cuda")
    _bits(buf)[:n] = UNWRITTEN[dtype]
    _bits(buf)[n:] = SENTINEL[dtype]
    return buf, buf[:n].view(shape)


def _place(run, shape, dtype, ref, mask, what):
    """run(out) once on one prefilled output and twice on another: the guard intact, the elements outside `mask` untouched, the elements
    inside equal to `ref` (float64, host), all three calls the same bits.  Returns the output's bits."""
    n = math.prod(shape)
    a_buf, a = _fresh(shape, dtype)
    run(a)
    b_buf, b = _fresh(shape, dtype)
    run(b)
    run(b)
    torch.cuda.synchronize()
    bits = _bits(a_buf).cpu()
    assert bool((bits[n:] == SENTINEL[dtype]).all()), f"{what}: wrote behind the output"
    left = bits[:n].view(shape)[~mask]
    assert bool((left == UNWRITTEN[dtype]).all()), f"{what}: {int((left != UNWRITTEN[dtype]).sum())} elements written that the contract leaves alone"
    got = a.cpu().double()
    wrong = (got != ref) & mask                      # (a NaN left inside the mask compares unequal: not written)
    assert not bool(wrong.any()), f"{what}: {int(wrong.sum())} of {int(mask.sum())} written elements differ from the reference; first at {wrong.nonzero()[0].tolist()}"
    assert torch.equal(_bits(a_buf), _bits(b_buf)), f"{what}: a second call changed the result"
    return bits


def _handle(preset, side):
    from gpu_util import lift_net
    net, _, p = lift_net(preset, side)
    return net, net._ensure_handle(), p


# ---------------------------------------------------------------------------------------------------- references, computed once
def _gathers(p):
    return {"patch": lambda x: H.patches_of_hm(x, p), "rot": lambda x: H.rot_rows(x, p), "tokens": lambda x: H.cells(x, p)}


def _layout(p, B, which):
    """(gather, shape of the scatter's output, GEMM rows M, GEMM columns N, depth K of the product in front of the scatter)"""
    S2, D = p.hm_size * p.hm_size, p.vit_dim
    if which == "patch":
        return _gathers(p)[which], H.hm_shape(p, B), B * p.seq, 256, D
    if which == "rot":
        return _gathers(p)[which], H.hm_shape(p, B), B * p.tokens, 2 * S2, 2048
    return _gathers(p)[which], (B * p.seq, D), B * p.tokens, p.ppd * p.ppd * D, 2048


@functools.lru_cache(maxsize=None)
def _onehot_reference(preset, side, B, which):
    """(scatter of onehot_rows(M, K) @ coded(N, K)^T, mask of the elements the scatter writes) -- shared by every test of the layout, never modified"""
    from egotap_amd import spec
    p = spec.lift_preset(preset, side)
    gather, shape, M, N, K = _layout(p, B, which)
    return H.scatter(gather, shape, H.onehot_product(M, N, K)), H.written(gather, shape) == 1


def _onehot_operands(p, B, which, dtype):
    """device operands of the exact product: one-hot rows [M, K] and the coded weight [N, K], built on the device"""
    _, _, M, N, K = _layout(p, B, which)
    return H.onehot_rows(M, K, device="cuda").to(dtype), H.coded(N, K, device="cuda").to(dtype)


def _both_depths(run_one):
    """run_one() under the 32-deep bf16 GEMM and under the default choice; the bits must agree"""
    from egotap_amd import lib
    L = lib.load()
    out = {}
    try:
        for bk in (32, 0):
            lib.check(L.egotap_debug_gemm_bk(bk))
            out[bk] = run_one(f"K-tile depth {bk or 'default'}")
    finally:
        lib.check(L.egotap_debug_gemm_bk(0))
    assert torch.equal(out[32], out[0]), "the 32-deep and the default kernel give different bits"


# ---------------------------------------------------------------------------------------------------- placement: bf16-storage scatters
@pytest.mark.parametrize("preset,side,B", CASES)
def test_bf16_fc1_dgrad_tokens_places_every_element(preset, side, B):
    """egotap_bf16_fc1_dgrad_tokens (SEpiScatterTokens): the whole bf16 dtok is written, dummy tokens exactly zero"""
    from egotap_amd import bf16s
    net, h, p = _handle(preset, side)
    ref, mask = _onehot_reference(preset, side, B, "tokens")
    assert int((~mask).sum()) == B * (p.grid ** 2 - p.tokens) * p.ppd ** 2 * p.vit_dim and float(ref[~mask].abs().max()) == 0.0
    dz, wt = _onehot_operands(p, B, "tokens", torch.bfloat16)
    everything = torch.ones_like(mask)
    _both_depths(lambda what: _place(lambda out: bf16s.fc1_dgrad_tokens(h, dz, wt, B, p.seq, p.vit_dim, out=out), ref.shape, torch.bfloat16, ref, everything,
                                     f"fc1_dgrad_tokens, {what}"))


@pytest.mark.parametrize("preset,side,B", CASES)
def test_bf16_fc1_dgrad_rot_places_every_element(preset, side, B):
    """egotap_bf16_fc1_dgrad_rot (SEpiScatterRot): channels [2J, 6J) written once each, [0, 2J) left alone"""
    from egotap_amd import bf16s
    net, h, p = _handle(preset, side)
    ref, mask = _onehot_reference(preset, side, B, "rot")
    assert bool(mask[:, H.rot_channels(p)].all()) and not bool(mask[:, H.pos_channels(p)].any())
    dz, wt = _onehot_operands(p, B, "rot", torch.bfloat16)
    _both_depths(lambda what: _place(lambda out: bf16s.fc1_dgrad_rot(h, dz, wt, out, B), ref.shape, torch.float32, ref, mask, f"fc1_dgrad_rot, {what}"))


@pytest.mark.parametrize("preset,side,B", CASES)
def test_bf16_patch_dgrad_places_every_element(preset, side, B):
    """egotap_bf16_patch_dgrad (SEpiScatterPatch): channels [0, 2J) written once each, [2J, 6J) left alone, rows of dummy tokens stored nowhere"""
    from egotap_amd import bf16s
    net, h, p = _handle(preset, side)
    ref, mask = _onehot_reference(preset, side, B, "patch")
    assert bool(mask[:, H.pos_channels(p)].all()) and not bool(mask[:, H.rot_channels(p)].any())
    dx, wt = _onehot_operands(p, B, "patch", torch.bfloat16)
    _both_depths(lambda what: _place(lambda out: bf16s.patch_dgrad(h, dx, wt, out, B), ref.shape, torch.float32, ref, mask, f"patch_dgrad, {what}"))


# ---------------------------------------------------------------------------------------------------- placement: fp32-tensor scatters
@pytest.mark.parametrize("which", ["patch", "rot"])
@pytest.mark.parametrize("preset,side,B", CASES)
def test_gemm_nt_scatter_epilogues_place_every_element(preset, side, B, which):
    """egotap_train_gemm_nt with TE_SCATTER_PATCH / TE_SCATTER_ROT in fp32, bf16x3 and bf16 arithmetic: the coded product is exact in all three
    (B seq >= 1024 rows: the LDS-DMA / persistent kernels; fewer: the 128 x 128 tiles), so all three give the reference's numbers"""
    from egotap_amd import train_ops as T
    net, h, p = _handle(preset, side)
    ref, mask = _onehot_reference(preset, side, B, which)
    _, _, M, N, K = _layout(p, B, which)
    x, wt = _onehot_operands(p, B, which, torch.float32)
    epi = T.TE_SCATTER_PATCH if which == "patch" else T.TE_SCATTER_ROT
    try:
        for mode in MODES:
            net.set_precision(mode)
            _place(lambda out: T.gemm_nt(h, x, wt, None, M, N, K, epi=epi, out=out), ref.shape, torch.float32, ref, mask, f"{which} scatter epilogue, {mode}")
    finally:
        net.set_precision("f32")


@pytest.mark.parametrize("preset,side,B", CASES)
def test_tokens_scatter_places_every_element(preset, side, B):
    """egotap_train_tokens_scatter: a coded dA [B T, ppd^2 D] to token order, dummy tokens zero, the whole dtok written"""
    from egotap_amd import lib, train_ops as T
    net, h, p = _handle(preset, side)
    gather, shape, M, N, _ = _layout(p, B, "tokens")
    ref = H.scatter(gather, shape, H.coded(M, N).double())
    dummy = H.written(gather, shape) == 0
    assert float(ref[dummy].abs().max()) == 0.0
    dA = H.coded(M, N, device="cuda")
    L = lib.load()
    _place(lambda out: lib.check(L.egotap_train_tokens_scatter(h, T._p(dA), T._p(out), B, T._s())), shape, torch.float32, ref, torch.ones_like(dummy), "tokens_scatter")


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("preset,side", [("UnrealEgo", 64), ("EgoCap", 64), ("UnrealEgo", 128), ("EgoCap", 128)])
def test_patch_split_sums_real_and_dummy_tokens(preset, side, accumulate):
    """egotap_train_patch_split: dbias = the sum of dpos [seq, D] over the tokens of real cells, dmask = over the dummy tokens.  Coded
    integers: every partial sum stays below 2^24 (seq x 125 <= 288000), so the fp32 sums are exact in any order."""
    from egotap_amd import lib, train_ops as T
    net, h, p = _handle(preset, side)
    D = p.vit_dim
    dummy = H.written(_gathers(p)["tokens"], (p.seq, 1)).view(-1) == 0          # (one frame: the tokens fc1 never reads)
    assert int(dummy.sum()) == (p.grid ** 2 - p.tokens) * p.ppd ** 2
    dpos = H.coded(p.seq, D)
    before = H.coded(2, D) * 3.0
    want = torch.stack((dpos[~dummy].double().sum(0), dpos[dummy].double().sum(0)))
    if accumulate:
        want = want + before.double()
    dpos_d = dpos.cuda()
    L = lib.load()

    def run(out):
        if accumulate:
            out.copy_(before)
        lib.check(L.egotap_train_patch_split(h, T._p(dpos_d), T._p(out[0]), T._p(out[1]), int(accumulate), T._s()))
    _place(run, (2, D), torch.float32, want, torch.ones((2, D), dtype=torch.bool), f"patch_split accumulate={accumulate}")


# ---------------------------------------------------------------------------------------------------- numeric: random operands
@functools.lru_cache(maxsize=None)
def _uniform(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


@functools.lru_cache(maxsize=None)
def _normal_bf16(shape, seed, scale):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).bfloat16()


def _close(got, ref64, atol, rtol, what):
    """every element: |got - ref| <= atol + rtol |ref|"""
    err = (got.detach().cpu().double() - ref64).abs()
    bad = err > atol + rtol * ref64.abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside {atol:.2e} + {rtol:.0e} |ref|; max err {float(err.max()):.3e} (max ref {float(ref64.abs().max()):.3e})"


def _f32_sources(p, B):
    """the two tensors the fp32 loaders gather from, operands in [-1, 1] as in test_linear_bias / test_gemm_tn"""
    return _uniform((B * p.seq, p.vit_dim), 101), _uniform(H.hm_shape(p, B), 102)


@pytest.mark.parametrize("which", ["tokens", "rot"])
@pytest.mark.parametrize("preset,side,B", CASES_64)
def test_f32_gemm_nt_gathers_fc1_rows(preset, side, B, which):
    """egotap_train_gemm_nt with LD_TOKENS / LD_ROT (fc1 of the two encoders, N = 2048, TE_BIAS) against float64 on the gathered rows: the rule
    of test_gpu_ops.py::test_linear_bias for the same operand ranges (x in [-1, 1], weights in +-0.1): atol = 2e-6 sqrt(K), rtol = 1e-5"""
    from egotap_amd import train_ops as T
    net, h, p = _handle(preset, side)
    tokens, hm = _f32_sources(p, B)
    gather, _, M, K, N = _layout(p, B, which)          # (the scatter's columns are the gather's depth)
    src = tokens if which == "tokens" else hm
    w, b = _uniform((N, K), 103, -0.1, 0.1), _uniform((N,), 104)
    y = torch.full((M + 2, N), 7.0, device="cuda")
    T.gemm_nt(h, src.cuda(), w.cuda(), b.cuda(), M, N, K, loader=T.LD_TOKENS if which == "tokens" else T.LD_ROT, epi=T.TE_BIAS, out=y[:M])
    torch.cuda.synchronize()
    assert float((y[M:] - 7.0).abs().max()) == 0.0
    ref = gather(src.double()) @ w.double().T + b.double()
    _close(y[:M], ref, 2e-6 * math.sqrt(K), 1e-5, f"gemm_nt LD_{which.upper()}")


@pytest.mark.parametrize("which", ["patch", "tokens", "rot"])
@pytest.mark.parametrize("preset,side,B", CASES_64)
def test_f32_gemm_tn_gathers_weight_gradient_rows(preset, side, B, which):
    """egotap_train_gemm_tn with LD_PATCH (N = D, K = 256), LD_TOKENS and LD_ROT (N = 2048): dw = dy^T gather(x) against float64, the rule of
    test_gpu_train_ops.py::test_gemm_tn (operands in [-1, 1]): atol = 2e-5 sqrt(M), rtol = 1e-4; without accumulate dw is overwritten"""
    from egotap_amd import train_ops as T
    net, h, p = _handle(preset, side)
    tokens, hm = _f32_sources(p, B)
    gather, _, M, K, N = _layout(p, B, which)          # (patch: dy = the patch embedding's output gradient [B seq, D], N = D)
    src = tokens if which == "tokens" else hm
    dy = _uniform((M, N), 105)
    dw = torch.full((N, K), 3.0, device="cuda")
    loader = {"patch": T.LD_PATCH, "tokens": T.LD_TOKENS, "rot": T.LD_ROT}[which]
    T.gemm_tn(h, dy.cuda(), src.cuda(), dw, M, N, K, loader=loader)
    ref = dy.double().T @ gather(src.double())
    _close(dw, ref, 2e-5 * math.sqrt(M), 1e-4, f"gemm_tn LD_{which.upper()}")
    T.gemm_tn(h, dy.cuda(), src.cuda(), dw, M, N, K, loader=loader, accumulate=True)
    _close(dw, 2 * ref, 4e-5 * math.sqrt(M), 1e-4, f"gemm_tn LD_{which.upper()} accumulate")


@pytest.mark.parametrize("preset,side,B", CASES_64)
def test_f32_patch_embedding_forward(preset, side, B):
    """egotap_train_patch_fwd (ALoadPatch + EpiPatch) against oracle.vit_embed in float64: real cells embedded, the mask token on dummy cells,
    position embeddings on both; K = 256 products with weights in +-0.1: test_linear_bias's rule, atol = 2e-6 sqrt(256), rtol = 1e-5"""
    from egotap_amd import lib, train_ops as T
    from oracle import lift_ref as O
    net, h, p = _handle(preset, side)
    D = p.vit_dim
    _, hm = _f32_sources(p, B)
    w, b, mask_tok, pos = _uniform((D, 256), 106, -0.1, 0.1), _uniform((D,), 107), _uniform((D,), 108), _uniform((p.seq, D), 109)
    x = torch.full((B * p.seq + 2, D), 7.0, device="cuda")
    dev = [t.cuda() for t in (hm, w, b, mask_tok, pos)]
    lib.check(lib.load().egotap_train_patch_fwd(h, T._p(dev[0]), B, T._p(dev[1]), T._p(dev[2]), T._p(dev[3]), T._p(dev[4]), T._p(x), T._s()))
    torch.cuda.synchronize()
    assert float((x[B * p.seq:] - 7.0).abs().max()) == 0.0
    e = "pos_heatmap_encoder.vit.embeddings."
    sd = {e + "patch_embeddings.projection.weight": w.double().view(D, 1, 16, 16), e + "patch_embeddings.projection.bias": b.double(),
          e + "mask_token": mask_tok.double().view(1, 1, D), e + "position_embeddings": pos.double().view(1, p.seq, D)}
    ref = O.vit_embed(hm[:, H.pos_channels(p)].double(), sd, p).reshape(B * p.seq, D)
    _close(x[:B * p.seq], ref, 2e-6 * math.sqrt(256), 1e-5, "patch_fwd")


@pytest.mark.parametrize("preset,side,B", CASES_64)
def test_bf16_scatters_on_random_operands(preset, side, B):
    """the three bf16-storage scatters on random bf16 operands (the ranges of test_fc1_weight_gradients_on_gathered_rows) against the autograd
    scatter of the float64 product of the same operands.  fp32 results: err < 2e-5 max|ref| + 1e-5, that test's rule; the bf16 dtok: one bf16
    rounding per element, |err| <= 2^-8 |ref| + 2^-8 1e-3 max|ref|"""
    from egotap_amd import bf16s
    net, h, p = _handle(preset, side)
    D = p.vit_dim
    dz = _normal_bf16((B * p.tokens, 2048), 111, 0.1)
    dx = _normal_bf16((B * p.seq, D), 112, 0.1)
    for which, a in (("tokens", dz), ("rot", dz), ("patch", dx)):
        gather, shape, M, N, K = _layout(p, B, which)
        wt = _normal_bf16((N, K), 113 + len(which), 0.02)
        ref = H.scatter(gather, shape, a.double() @ wt.double().T)
        top = float(ref.abs().max())
        if which == "tokens":
            got = bf16s.fc1_dgrad_tokens(h, a.cuda(), wt.cuda(), B, p.seq, D)
            err = (got.double().cpu() - ref).abs()
            bad = err > 2.0 ** -8 * ref.abs() + 2.0 ** -8 * 1e-3 * top
            assert not bool(bad.any()), f"dtok: {int(bad.sum())} of {bad.numel()} elements outside one bf16 rounding; max err {float(err.max()):.3e}, max ref {top:.3e}"
            continue
        dhm = torch.full(shape, float("nan"), device="cuda")
        (bf16s.fc1_dgrad_rot if which == "rot" else bf16s.patch_dgrad)(h, a.cuda(), wt.cuda(), dhm, B)
        sl = H.rot_channels(p) if which == "rot" else H.pos_channels(p)
        err = float((dhm[:, sl].double().cpu() - ref[:, sl]).abs().max())          # (a NaN left in the channels makes err NaN: the comparison fails)
        assert err < 2e-5 * top + 1e-5, (which, err, top)
