"""The reference layouts of tests/head_layout_cases.py are sound by themselves (no GPU): each gather is a bijection between the (row, column)
pairs of the real cells and the elements it reads, and its shapes and dummy tokens are the ones egotap_amd/spec.py states.  The kernel
tests (test_gpu_head_layouts.py) compare against these functions, so they are checked first, without any kernel."""
import pytest
import torch

import head_layout_cases as H
from egotap_amd import spec

CASES = [(preset, side) for preset in ("UnrealEgo", "EgoCap") for side in (64, 128)]
B = 2


def _layouts(p):
    """(name, gather, shape of what it reads, rows, columns) of the three layouts at batch B"""
    D = p.vit_dim
    return [("patches", lambda x: H.patches_of_hm(x, p), H.hm_shape(p, B), B * p.seq, 256),
            ("cells", lambda x: H.cells(x, p), (B * p.seq, D), B * p.tokens, p.ppd * p.ppd * D),
            ("rot_rows", lambda x: H.rot_rows(x, p), H.hm_shape(p, B), B * p.tokens, 2 * p.hm_size * p.hm_size)]


@pytest.mark.parametrize("preset,side", CASES)
def test_shapes_and_dummy_tokens_are_those_of_the_spec(preset, side):
    p = spec.lift_preset(preset, side)
    assert p.ppd == side // 16 and p.side == p.grid * p.ppd and p.seq == p.side ** 2 and p.tokens == 2 * p.n_joints_hm
    assert (p.grid - 1) ** 2 < p.tokens <= p.grid ** 2
    n_dummy = (p.grid ** 2 - p.tokens) * p.ppd ** 2
    for name, gather, shape, rows, cols in _layouts(p):
        assert tuple(gather(torch.zeros(shape, dtype=torch.float64)).shape) == (rows, cols), name
    rows, dummy = H.patches(torch.ones((B, p.tokens, side, side), dtype=torch.float64), p)
    assert dummy.shape == (p.seq,) and int(dummy.sum()) == n_dummy
    # rows of dummy tokens read no heatmap, every other row reads 256 pixels
    assert torch.equal(rows.view(B, p.seq, 256).sum(-1), (~dummy).double().expand(B, -1) * 256)
    # the tokens fc1 never reads are the same dummy tokens
    unread = H.written(lambda x: H.cells(x, p), (B * p.seq, 8)).view(B, p.seq, 8) == 0
    assert torch.equal(unread, dummy.view(1, -1, 1).expand(B, -1, 8))


@pytest.mark.parametrize("preset,side", CASES)
def test_every_row_and_column_of_a_real_cell_has_exactly_one_destination(preset, side):
    p = spec.lift_preset(preset, side)
    J = p.n_joints_hm
    _, dummy = H.patches(torch.zeros((1, p.tokens, side, side), dtype=torch.float64), p)
    for name, gather, shape, rows, cols in _layouts(p):
        count = H.written(gather, shape)
        want = torch.ones(shape, dtype=torch.long)
        if name == "patches":
            want[:, H.rot_channels(p)] = 0
            real_rows = B * (p.seq - int(dummy.sum()))
        elif name == "rot_rows":
            want[:, H.pos_channels(p)] = 0
            real_rows = rows
        else:
            want.view(B, p.seq, -1)[:, dummy] = 0
            real_rows = rows
        assert torch.equal(count, want), name
        assert int(count.sum()) == real_rows * cols, name
        # a coded matrix scattered and gathered again comes back: no two (row, column) pairs share a destination and none is lost
        Y = H.coded(rows, cols).double()
        if name == "patches":
            Y = Y * (~dummy).double().repeat(B)[:, None]          # rows of dummy tokens have no destination
        back = gather(H.scatter(gather, shape, Y))
        assert torch.equal(back, Y), name
    assert 6 * J == p.in_channels


def test_exact_operands():
    c = H.coded(300, 77)
    assert c.dtype == torch.float32 and float(c.abs().max()) <= 125 and torch.equal(c, c.round())
    assert torch.equal(c.bfloat16().float(), c)                     # exact in bf16
    assert float(c[2, 3]) == (131 * 2 + 71 * 3) % 251 - 125
    x = H.onehot_rows(300, 64)
    assert torch.equal(x.sum(1), torch.ones(300)) and float(x[70, 6]) == 1.0
    assert torch.equal(x.double() @ H.coded(40, 64).double().T, H.onehot_product(300, 40, 64))
