"""The PU chain + pose head of training (egotap_train_pu_fwd, egotap_train_pose_head_fwd / _bwd, egotap_train_pu_bwd) at the batch sizes that take
every kernel the batch can select, against the float64 oracle (tests/pu_train_cases.py).  Each case first asserts, through the routing query
(egotap_debug_pu_train_routes), that its batch still lands in the regime it exists for; then EVERY returned tensor meets its gate, every output
started as NaN, and a second run gives the same bits."""
import pytest
import torch

import pu_train_cases as P

pytestmark = pytest.mark.gpu

_runs = {}


def _run(name, B, mode="f32", accumulate=0, chain=True):
    key = (name, B, mode, accumulate, chain)
    if key not in _runs:
        _runs[key] = P.run_gpu(name, B, mode, accumulate, chain)
    return _runs[key]


def _same_bits(a, b, what):
    assert set(a) == set(b)
    for k in a:
        if k != "prefill":
            assert torch.equal(a[k], b[k]), f"{what}: {k} differs, max |diff| {float((a[k] - b[k]).abs().max()):.3e}"


def _no_nan(got):
    for k, v in got.items():
        if k != "prefill":
            assert bool(torch.isfinite(v).all()), f"{k}: {int((~torch.isfinite(v)).sum())} elements of the NaN prefill survived (nobody wrote them)"


def _regime_ue17(r):
    assert r["chain"] == 1 and r["chunks"] == 1, f"B = 17 no longer runs pu_chain_kernel<1> in one launch (resident workgroups below 2 x 32?): {r}"
    assert (r["row_blocks"], r["last_rows"]) == (2, 1), f"B = 17 is no longer a second row block holding one row (row block size moved): {r}"
    assert set(r["wgrad_family"].values()) == {"f32_big"}, f"a weight gradient of 255 rows left TnBig: {r}"
    assert min(r["wgrad_splits"].values()) >= 2 and (15 * 17) % 16 != 0, f"255 rows no longer split (rows-per-split cap of gemm_tn_f32_launch moved): {r}"
    assert r["colsum_gy"] == 1


def _regime_ec32(r):
    assert r["chain"] == 1 and (r["row_blocks"], r["last_rows"]) == (2, 16), f"B = 32 is no longer two full row blocks on pu_chain_kernel<1>: {r}"
    assert r["colsum_gy"] == 2, f"544 rows are no longer two partial rows of the column sums (rows per block of colsum_f32_launch moved): {r}"
    assert min(r["wgrad_splits"].values()) >= 2


def _regime_ue96(r):
    assert r["chain"] == 1 and r["chunks"] == 1 and r["row_blocks"] == 6, f"B = 96 is no longer six row blocks on pu_chain_kernel<1> (its row-block or residency limit moved): {r}"
    fam = r["wgrad_family"]
    assert [fam[k] for k in ("h2h0", "x2f1", "x2h1", "h2h1")] == ["f32_dma"] * 4, f"1440 plain rows left the DMA-staged weight gradient (its M threshold or M % 32 rule moved): {r}"
    assert [fam[k] for k in ("x2f0", "x2h0", "b2h0")] == ["f32_big"] * 3, f"the stereo loaders left TnBig: {r}"
    assert min(r["wgrad_splits"].values()) >= 2 and r["colsum_gy"] == 3


def _regime_ue290(r):
    assert r["chain"] == 2, f"B = 290 (19 row blocks) no longer runs pu_chain_kernel<2> (the 8-row-block limit of <1> moved, or <2> is not resident): {r}"
    assert (r["row_blocks"], r["last_rows"]) == (19, 2), f"B = 290 no longer ends in a row block of 2 rows: {r}"
    sk = r["dgrad_splitk"]
    assert (sk["x2h1"], sk["b2h0"], sk["x2h0"], sk["step"]) == (0, 1, 1, 1), f"4350 rows: the N = 512 input gradient should leave split-K (136 tiles), the N = 256 ones stay (68 tiles): the 128-tile threshold moved: {r}"
    assert r["wgrad_capped"]["h2h0"] == 1 and r["wgrad_capped"]["h2h1"] == 1, f"the slab scratch no longer caps h2h's split count: {r}"
    assert set(r["wgrad_family"].values()) == {"f32_big"} and r["colsum_gy"] == 9, f"4350 rows (not a multiple of 32) should stay on TnBig with 9 partial rows: {r}"


F32_CASES = [("UnrealEgo", 17, _regime_ue17), ("EgoCap", 32, _regime_ec32), ("UnrealEgo", 96, _regime_ue96), ("UnrealEgo", 290, _regime_ue290)]


@pytest.mark.parametrize("name,B,regime", F32_CASES, ids=[f"{n}-{b}" for n, b, _ in F32_CASES])
def test_every_tensor_against_float64_f32(name, B, regime):
    """fp32 gate per tensor: e(k) = max|got - ref64| / max|ref64| <= 8 * max(e32(k), 2.5e-7), e32 from the float32 oracle inside the test.
    UnrealEgo 17: second row block of one row, 4 weight-gradient splits with a ragged last slab of 15 rows.  EgoCap 32: J = 17, no head joint,
    null dWg / dbg, two partial rows of the column sums.  UnrealEgo 96: DMA-staged weight gradients for the plain operands, TnBig with many
    splits for the stereo ones, three samples per lane in the pose-head weight kernel, six row blocks.  UnrealEgo 290: pu_chain_kernel<2> with
    GP and C, last row block of 2 rows, the N = 512 input gradients off split-K, slab scratch capping the split counts.
    Measured on an MI355X, worst e(k) / max(e32(k), 2.5e-7) over the tensors of a case (8 allowed): UnrealEgo 17: 2.29 (global_mlp weight),
    EgoCap 32: 1.79 (skel), UnrealEgo 96: 1.70 (skel), UnrealEgo 290: 3.04 (layer-0 x2f bias)."""
    regime(P.routes(name, B))
    got = _run(name, B)
    lines = []
    bad = P.f32_gate_failures(got, name, B, report=lines.append)
    print("\n".join(lines))
    _no_nan(got)
    assert not bad, bad
    _same_bits(got, P.run_gpu(name, B), "second run")


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
def test_every_tensor_against_float64_bf16_modes(mode):
    """UnrealEgo, B = 96: gemm_tn_bf16_launch with the ALoadStereo and ALoadStereoGated loaders (1440 rows >= 1024).  bf16x3: ten times the fp32
    bound (the ratio between the fp32 and bf16x3 attention gates); bf16: relative L2 <= 20 %, cosine >= 0.98 per gradient tensor, the forward
    within 3e-2 * max|ref|.  Measured on an MI355X: bf16x3 worst e(k) / max(e32(k), 2.5e-7) = 25.4 (layer-0 b2h weight; 80 allowed), everything but
    the seven PU weight gradients as in fp32 (only they change arithmetic at this batch); bf16 worst relative L2 2.4e-3, cosine 0.999997."""
    from egotap_amd import lib as L
    name, B = "UnrealEgo", 96
    h, net, _ = P.handle(name)
    try:
        net.set_precision(mode)
        r = L.pu_train_routes(h, B)
    finally:
        net.set_precision("f32")
    assert set(r["wgrad_family"].values()) == {mode}, f"a weight gradient of 1440 rows left gemm_tn_bf16_launch in {mode} mode (its M >= 1024 threshold moved): {r}"
    got = _run(name, B, mode)
    lines = []
    bad = P.f32_gate_failures(got, name, B, factor=P.BF16X3_FACTOR, report=lines.append) if mode == "bf16x3" else P.bf16_gate_failures(got, name, B, report=lines.append)
    print("\n".join(lines))
    _no_nan(got)
    assert not bad, bad
    _same_bits(got, P.run_gpu(name, B, mode), "second run")
    assert net.precision == "f32"


def test_per_step_kernels_give_the_chain_bits():
    """UnrealEgo, B = 17, set_pu_chain(False): forward output and EVERY gradient bit-identical to the chain run -- the per-step kernel's gpre_out and
    the cell states it leaves, through their only consumer, the backward."""
    from egotap_amd import lib as L
    name, B = "UnrealEgo", 17
    h, net, _ = P.handle(name)
    try:
        net.set_pu_chain(False)
        assert L.pu_train_routes(h, B)["chain"] == 0
    finally:
        net.set_pu_chain(True)
    assert L.pu_train_routes(h, B)["chain"] == 1
    off = P.run_gpu(name, B, chain=False)
    _no_nan(off)
    _same_bits(_run(name, B), off, "per-step kernels against the chain")
    assert net.pu_chain_status() == (True, 0)


def test_accumulate_adds_to_what_the_buffers_hold():
    """UnrealEgo, B = 17, accumulate = 1: every gradient buffer starts as random values in [-1, 1); result = prefill + reference.  Tolerance per
    tensor: the fp32 gate of the gradient alone (on the gradient's scale) plus the roundings of the additions on the SUM's scale, which is
    some 30 times the gradient's here: reduce_slabs_kernel adds the slabs to the buffer one after the other, so a weight gradient of S splits
    (the routing query's count) rounds S times, a bias gradient (one partial row) and the pose head's once, each by at most 2^-24 of the
    running sum -- itself at most |prefill| plus a partial gradient sum, taken as 4 x max|reference| (a quarter of the rows each)."""
    name, B = "UnrealEgo", 17
    splits = P.routes(name, B)["wgrad_splits"]
    got = P.run_gpu(name, B, accumulate=1)
    _no_nan(got)
    ref, bounds, bad = P.reference(name, B), P.f32_bounds(name, B), []
    for k, pre in got["prefill"].items():
        want = pre.double() + ref[k]
        layer, _, kind = k[len(P.PU_PRE):].rpartition(".") if k.startswith(P.PU_PRE) else ("", "", "")
        adds = splits[layer.split(".")[1] + layer.split(".")[0]] if kind == "weight" else 1
        tol = bounds[k][0] * float(ref[k].abs().max()) + adds * 2.0 ** -24 * (float(pre.abs().max()) + 4.0 * float(ref[k].abs().max()))
        err = float((got[k].double() - want).abs().max())
        print(f"{k}: err {err:.3e} tol {tol:.3e} ({adds} additions)")
        if not err <= tol:
            bad.append((k, err, tol))
    assert not bad, bad
    for k in P.DATA:                      # the data outputs do not depend on the flag
        assert torch.equal(got[k], _run(name, B)[k]), k


def test_pose_head_scalar_path_on_a_four_byte_aligned_view():
    """pose_head_kernel takes its scalar loop for an hseq that is only 4-byte aligned: hs1 copied one float into a larger buffer gives the aligned
    pose within the fp32 bound (another summation order: not the same bits), and the aligned pose is the case's own."""
    name, B = "UnrealEgo", 17
    aligned, unaligned = P.pose_aligned_and_unaligned(name, B)
    assert torch.equal(aligned, _run(name, B)["pose"])
    ref, (bound, _) = P.reference(name, B)["pose"], P.f32_bounds(name, B)["pose"]
    e = P.rel_err(unaligned, ref)
    print(f"pose through the scalar path: e = {e:.3e}, bound {bound:.3e}; aligned e = {P.rel_err(aligned, ref):.3e}")
    assert e <= bound
    assert P.rel_err(unaligned, aligned.double()) <= bound
