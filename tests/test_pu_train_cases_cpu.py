"""The conditions of tests/test_gpu_pu_train_batches.py hold for the reference alone (no GPU): the float32 oracle passes the fp32 gate against the
float64 oracle at every case's batch, three subtly wrong results built from the float64 oracle miss it, and the routing query
(egotap_debug_pu_train_routes_for: host only) puts every case's batch into the regime the case exists for, at stated resident counts."""
import ctypes as C

import pytest
import torch

import pu_train_cases as P

CASES = [("UnrealEgo", 17), ("EgoCap", 32), ("UnrealEgo", 96), ("UnrealEgo", 290)]


@pytest.mark.parametrize("name,B", CASES)
def test_float32_oracle_passes_the_gate_and_wrong_results_miss_it(name, B):
    lines = []
    bad = P.f32_gate_failures(P.reference(name, B, torch.float32), name, B, report=lines.append)
    print("\n".join(lines))
    assert not bad, bad
    worst = max(e32 for _, e32 in P.f32_bounds(name, B).values())
    assert worst < 4e-6, worst                       # (the float32 oracle is itself a sound yardstick: its own error is a few ulp)
    r64 = P.reference(name, B, torch.float64)
    for what, (wrong, must_miss) in P.wrong_results(name, B).items():
        missed = {k for k, _, _ in P.f32_gate_failures(wrong, name, B)}
        assert must_miss <= missed, (what, sorted(must_miss - missed))
        # ... by a wide margin: also at ten times the bound (the bf16x3 gate), and each measured on the tensor's own scale
        assert must_miss <= {k for k, _, _ in P.f32_gate_failures(wrong, name, B, factor=P.BF16X3_FACTOR)}, what
        assert set(wrong) == set(r64)


def test_inputs_give_every_row_its_own_values_and_a_loud_last_sample():
    posz, rotz, dpose = P.inputs("UnrealEgo", 17)
    assert posz.shape == (17 * 30, 128) and torch.unique(posz, dim=0).shape[0] == posz.shape[0]
    assert torch.unique(rotz, dim=0).shape[0] == rotz.shape[0]
    assert float(dpose[-1].abs().max()) > 4.0 and float(dpose[:-1].abs().max()) <= 1.0
    assert P.inputs("EgoCap", 32)[2].shape == (32, 17, 3)
    assert not [k for k in P.weights("EgoCap") if k.startswith("global_mlp.")] and len(P.weights("UnrealEgo")) == 18


def _handle(**kw):
    from egotap_amd import lib as L
    from test_abi_cpu import _cfg
    h = C.c_void_p()
    L.check(L.load().egotap_create(C.byref(_cfg(**kw)), C.byref(h)))
    return h


def test_routing_predicates_at_stated_resident_counts():
    """256 CUs; pu_chain_kernel<1> / <2> with 512 / 256 resident workgroups (two / one per CU)."""
    from egotap_amd import lib as L
    h = _handle()
    r ={B: L.pu_train_routes(h, B, (512, 256), 256) for B in (3, 17, 96, 290)}
    J = 15
    # B = 3: the single branch the suite took before: one row block, one split (a direct store), one partial row, split-K everywhere it can be
    assert (r[3]["chain"], r[3]["chunks"], r[3]["row_blocks"], r[3]["last_rows"], r[3]["colsum_gy"]) == (1, 1, 1, 3, 1)
    assert set(r[3]["wgrad_splits"].values()) == {1} and set(r[3]["wgrad_family"].values()) == {"f32_big"}
    # B = 17: a second row block of one row; J * B = 255 rows in ceil(255 / 64) = 4 splits of 64 rows, the last of 63 (a ragged slab of 15)
    assert (r[17]["chain"], r[17]["chunks"], r[17]["row_blocks"], r[17]["last_rows"], r[17]["colsum_gy"]) == (1, 1, 2, 1, 1)
    assert set(r[17]["wgrad_splits"].values()) == {4} and set(r[17]["wgrad_family"].values()) == {"f32_big"} and (J * 17) % 16 == 15
    # B = 96: 1440 rows = 45 slabs of 32: the plain operands on the DMA-staged kernel, the gathered ones on TnBig; six row blocks on <1>
    assert (r[96]["chain"], r[96]["chunks"], r[96]["row_blocks"], r[96]["last_rows"], r[96]["colsum_gy"]) == (1, 1, 6, 16, 3)
    assert r[96]["wgrad_family"] == {"x2f0": "f32_big", "x2h0": "f32_big", "b2h0": "f32_big", "h2h0": "f32_dma", "x2f1": "f32_dma", "x2h1": "f32_dma",
                                     "h2h1": "f32_dma"}
    assert r[96]["wgrad_splits"]["x2h0"] == (1440 + 63) // 64 and min(r[96]["wgrad_splits"].values()) > 1
    # B = 290: 19 row blocks on <2> in chunks of 256 / 16 = 16, the last of 2 rows; 4350 rows: 34 x 4 = 136 output tiles for N = 512 (no split-K),
    # 34 x 2 = 68 for N = 256 (split-K); the slab scratch caps every split count
    assert (r[290]["chain"], r[290]["chunks"], r[290]["row_blocks"], r[290]["last_rows"], r[290]["colsum_gy"]) == (2, 2, 19, 2, 9)
    assert r[290]["dgrad_splitk"] == {"step": 1, "x2h1": 0, "x2f1": 0, "b2h0": 1, "x2h0": 1, "x2f0": 0}
    assert r[290]["wgrad_capped"]["h2h0"] == 1 and r[290]["wgrad_capped"]["h2h1"] == 1 and set(r[290]["wgrad_family"].values()) == {"f32_big"}
    for B in (3, 17, 96):
        assert r[B]["dgrad_splitk"] == {"step": 1, "x2h1": 1, "x2f1": 0, "b2h0": 1, "x2h0": 1, "x2f0": 0} and not any(r[B]["wgrad_capped"].values())
    # resident counts decide the chain: none -> per step; fewer than 32 per row block -> <2>; <2> in chunks of resident2 / 16 row blocks
    assert L.pu_train_routes(h, 17, (0, 0), 256)["chain"] == 0 and L.pu_train_routes(h, 17, (0, 0), 256)["chunks"] == 0
    assert L.pu_train_routes(h, 17, (32, 256), 256)["chain"] == 2
    assert L.pu_train_routes(h, 290, (512, 512), 256)["chunks"] == 1 and L.pu_train_routes(h, 290, (512, 64), 256)["chunks"] == 5
    # the precision decides the weight-gradient family from 1024 rows on
    lib = L.load()
    try:
        for mode in ("bf16x3", "bf16"):
            L.check(lib.egotap_set_precision(h, L.PRECISIONS[mode]))
            assert set(L.pu_train_routes(h, 96, (512, 256), 256)["wgrad_family"].values()) == {mode}
            assert set(L.pu_train_routes(h, 17, (512, 256), 256)["wgrad_family"].values()) == {"f32_big"}
    finally:
        L.check(lib.egotap_set_precision(h, L.PRECISIONS["f32"]))
    # EgoCap, B = 32: 544 rows, two partial rows of the column sums
    e = L.pu_train_routes(_handle(n_joints_hm=17, estimate_head=0), 32, (512, 256), 256)
    assert (e["chain"], e["row_blocks"], e["last_rows"], e["colsum_gy"]) == (1, 2, 16, 2) and set(e["wgrad_splits"].values()) == {9}
    assert lib.egotap_debug_pu_train_routes_for(h, 17, 512, 256, 256, (C.c_int * 8)(), 8) == 1 and b"32 ints" in lib.egotap_last_error()
