// Operand layouts of the lifting head, stated once: how a GEMM row and a GEMM column map to ELEMENT offsets inside the tensor a loader
// gathers from (or a scattering epilogue writes to).  address = base + rowpart(m) + kpart(k); what a loader or epilogue adds is only its
// own packaging: the pointer type, the x 2 / unsigned of the scalar-origin forms, the zero page, + ko / + chunk * 8, the store.
// col(p, k) = p + kpart(k) with the terms added to p one by one, as the per-lane pointer forms compile them.  The structs are nested as the
// int members of the loaders / epilogues, in this order (their kernel-argument offsets).  spec.py states the same layouts in Python.
// A caller that hipcc compiles differently through these functions keeps its own lines and says so (profiles/operand_layout_summary.md).
#pragma once
#include <hip/hip_runtime.h>
// The ViT's input is the heatmaps tiled into one image: grid x grid cells of ppd x ppd patches (ppd = hm_size / 16), side = grid * ppd
// patches per image row, seq = side^2 tokens, token (pr, pc) row-major.  Cell (pr / ppd) * grid + pc / ppd is heatmap `cell`; the cells
// >= T (grid^2 > T) are dummies: no heatmap feeds them, the patch embedding puts the mask token there.  Reference:
// net_architecture.py:375-383 + modeling_vit.py:137-153, 195.
struct CellGrid {
    int seq, side, ppd, grid, T;
    __host__ __device__ __forceinline__ int cell(int tok) const {
        const int pr = tok / side, pc = tok - pr * side;
        return (pr / ppd) * grid + pc / ppd;
    }
    __host__ __device__ __forceinline__ bool dummy(int tok) const { return cell(tok) >= T; }
};
// Patch embedding operand: row m = ViT token (b, tok), column k = pixel (k >> 4, k & 15) of the 16 x 16 patch the token covers, inside the
// heatmaps [B, C, S, S] (position channels first): heatmap `cell`, patch (pr % ppd, pc % ppd) of it.
struct PatchCells {
    int C, S;
    CellGrid g;
    // hm + row part: the origin of row m's patch (AT: its pixel (py, px), for the scattering epilogue); nullptr: a dummy cell
    template <bool AT = false, class P> __host__ __device__ __forceinline__ P pixel(P hm, int m, int py = 0, int px = 0) const {
        const int b = m / g.seq, tok = m - b * g.seq;
        const int pr = tok / g.side, pc = tok - pr * g.side;
        const int cell = g.cell(tok);
        if (cell >= g.T) return nullptr;
        return hm + ((long)(b * C + cell) * S + (pr % g.ppd) * 16 + (AT ? py : 0)) * S + (pc % g.ppd) * 16 + (AT ? px : 0);
    }
    template <class P> __host__ __device__ __forceinline__ P col(P p, int k) const { return p + (k >> 4) * S + (k & 15); }
};
// fc1 of the position encoder: row m = (b, heatmap i) gathers the ppd x ppd patch tokens of cell i from the tokens [B * seq, D];
// column k = (patch row prl, patch col pcl, channel c), k = (prl * ppd + pcl) * D + c: a bijection onto the non-dummy tokens (net_architecture.py:388-406).
struct TokenGather {
    int T, D, seq, side, ppd, grid;
    // column k -> channel c of patch (prl, pcl) of the cell: prl * side + pcl tokens after the row's first
    __host__ __device__ __forceinline__ void patch_of(int k, int& prl, int& pcl, int& c) const {
        const int s = k / D;
        c = k - s * D, prl = s / ppd, pcl = s - prl * ppd;
    }
    __host__ __device__ __forceinline__ long rowpart(int m) const {
        const int b = m / T, i = m - b * T;
        return ((long)b * seq + (long)(ppd * (i / grid)) * side + ppd * (i % grid)) * D;
    }
    template <class O = long> __host__ __device__ __forceinline__ O kpart(int k) const {      // O = int: 32-bit offsets (the scalar-origin forms)
        int prl, pcl, c;
        patch_of(k, prl, pcl, c);
        return (O)(prl * side + pcl) * D + c;
    }
    template <class P> __host__ __device__ __forceinline__ P col(P p, int k) const {
        int prl, pcl, c;
        patch_of(k, prl, pcl, c);
        return p + (long)(prl * side + pcl) * D + c;
    }
};
// fc1 of the rotation encoder: row m = (b, eye * J + j) = [cos map | sin map] of limb j of that eye in the heatmaps [B, C, HW]; column k =
// plane k / HW (0 cos, 1 sin: + J channels) and pixel k % HW.  Channel order after the 2J position maps: L_cos, L_sin, R_cos, R_sin, J maps
// each.  Reference: net_architecture.py:690-694.
__host__ __device__ __forceinline__ int rot_channel(int J, int eye, int j) { return 2 * J + eye * 2 * J + j; }
struct RotRows {
    int C, J, HW;
    __host__ __device__ __forceinline__ int plane(int k) const { return k / HW; }
    // row part; AT: of the row's plane cs (the scattering epilogue, whose column decides the plane)
    template <bool AT = false> __host__ __device__ __forceinline__ long rowpart(int m, int cs = 0) const {
        const int T = 2 * J;
        const int b = m / T, t = m - b * T;
        const int eye = t / J, j = t - eye * J;
        // = b * C + rot_channel(J, eye, j) + cs * J, spelt out: through the call hipcc factors the sum differently
        return (long)(b * C + 2 * J + eye * 2 * J + (AT ? cs * J : 0) + j) * HW;
    }
    template <class P> __host__ __device__ __forceinline__ P col(P p, int k) const {
        const int cs = plane(k);
        return p + (long)cs * J * HW + (k - cs * HW);
    }
    template <class O = long> __host__ __device__ __forceinline__ O kpart(int k) const {
        const int cs = plane(k);
        return (O)cs * J * HW + (k - cs * HW);
    }
};
