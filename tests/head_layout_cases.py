"""The three operand layouts of the lifting head as plain float64 torch functions, for the tests of the kernels that gather GEMM rows out of
them and scatter gradients back (test_head_layouts_cpu.py, test_gpu_head_layouts.py, test_gpu_bf16_stages.py).

Every gather is the oracle's own view / permute statement (oracle/lift_ref.py: tile_to_patches, tokens_to_cells, rot_relayout); every
scatter is the autograd transpose of its gather.  No index formula is written here, so nothing here can share a mistake with
csrc/head_layout.h or with the loaders and epilogues that keep their own lines.

Exact operands: `coded` weights and `onehot_rows` make a GEMM whose result is known without a product -- integers of magnitude <= 125, exact
in bf16, in the hi + lo split of bf16x3 and in fp32, one non-zero term per sum -- so a placement test can ask for equality."""
import torch

from oracle import lift_ref as O


# ---------------------------------------------------------------------------------------------------- gathers (differentiable)
def patches(pos_hm, p):
    """position heatmaps [B, 2J, S, S] -> (GEMM rows of the patch embedding [B * seq, 256], dummy-token mask [seq]); rows of dummy tokens are zero"""
    rows, dummy = O.tile_to_patches(pos_hm, p)
    return rows.reshape(-1, rows.shape[-1]), dummy


def cells(tokens, p):
    """ViT tokens [B * seq, D] -> GEMM rows of the position encoder's fc1 [B * T, ppd^2 * D]"""
    return O.tokens_to_cells(tokens.view(-1, p.seq, tokens.shape[-1]), p)


def rot_rows(hm, p):
    """the head's input heatmaps [B, 6J, S, S] -> GEMM rows of the rotation encoder's fc1 [B * T, 2 S^2] (from channels [2J, 6J))"""
    return O.rot_relayout(hm[:, 2 * p.n_joints_hm:], p)


def pos_channels(p):
    return slice(0, 2 * p.n_joints_hm)


def rot_channels(p):
    return slice(2 * p.n_joints_hm, 6 * p.n_joints_hm)


def hm_shape(p, B):
    return (B, p.in_channels, p.hm_size, p.hm_size)


def patches_of_hm(hm, p):
    """`patches` on the whole input [B, 6J, S, S] (channels [0, 2J)), rows only: the form `scatter` takes"""
    return patches(hm[:, pos_channels(p)], p)[0]


# ---------------------------------------------------------------------------------------------------- scatters (autograd)
def scatter(gather, x_shape, Y):
    """the transpose of `gather` applied to Y (the shape of gather's result): float64 tensor of x_shape, zero where gather reads nothing"""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(gather(x), x, Y.double())
    return g


def written(gather, x_shape):
    """how many (row, column) pairs of the gathered matrix land on each element of x: the scatter of all ones, as int64"""
    x = torch.zeros(x_shape, dtype=torch.float64, requires_grad=True)
    rows = gather(x)
    (g,) = torch.autograd.grad(rows, x, torch.ones_like(rows))
    return g.round().long()


# ---------------------------------------------------------------------------------------------------- exact operands
def coded_at(r, c):
    """((131 r + 71 c) mod 251) - 125 for integer index tensors (broadcast): int32 arithmetic, float32 result"""
    return ((r.to(torch.int32) * 131 + c.to(torch.int32) * 71) % 251 - 125).float()


def coded(rows, cols, device=None):
    """[rows, cols] float32 with element (r, c) = ((131 r + 71 c) mod 251) - 125: integers in [-125, 125]"""
    return coded_at(torch.arange(rows, device=device)[:, None], torch.arange(cols, device=device)[None, :])


def onehot_rows(M, K, device=None):
    """[M, K] float32, row m is 1 at column m mod K"""
    x = torch.zeros((M, K), dtype=torch.float32, device=device)
    x[torch.arange(M, device=device), torch.arange(M, device=device) % K] = 1.0
    return x


def onehot_product(M, N, K):
    """onehot_rows(M, K) @ coded(N, K)^T without the product: Y[m, n] = coded(N, K)[n, m mod K], float64 on the host"""
    return coded_at(torch.arange(N)[None, :], (torch.arange(M) % K)[:, None]).double()
