// Fused softmax attention with bf16 tensors in HBM (bf16-storage training mode, EGOTAP_PREC_BF16): what the forward
// (attention_bf16s_fwd.h) and the backward (attention_bf16s_bwd.h) share.  Tile staging, LDS images and tile products only: no kernel
// and no launch.
//   forward   ctx = softmax(Q K^T / sqrt(128)) V                                   (model/modeling_vit.py:226-252)
//   backward  flash style, P recomputed from Q, K and the forward's log-sum-exp:
//             dV = P^T dO,  dP = dO V^T,  dS = P * (dP - delta) / sqrt(dh),  dQ = dS K,  dK = dS^T Q,  delta = rowsum(dO * O)
// q | k | v are read in place from the fused bf16 [B*N, 3*heads*128] buffer and the three gradients are written in place into a
// bf16 buffer of the same layout (the operand of the QKV weight-gradient / input-gradient GEMMs).
// Same operand maps as attention_bf16.h / attention_bwd_bf16.h (v_mfma_f32_32x32x16_bf16; scores with the key on the accumulator
// row; probability accumulators used as the next product's B operand where they stand; transposed tiles through
// ds_read_b64_tr_b16) -- what changes: no conversion pass (tiles are staged as they lie, 16-byte loads, half the bytes).
//
// Two ways of staging a 32 x 128 bf16 tile stand here.  Namespace attns: through registers into the padded row / transposed-read
// images of attention_bf16_tiles.h (the register-staged dQ kernel), with the fragment loads and the bf16 row store every kernel uses.
// Namespace att2: by LDS DMA into one swizzled image (the forward, the dK + dV kernel and the DMA-staged dQ kernel):
//   * ONE image per tile serves the row reads (ds_read_b128: S = Q K^T, dP = dO V^T) AND the transposed reads (ds_read_b64_tr_b16:
//     dV^T += dO^T P, dK^T += Q^T dS): cdna_hip_programming.md T10 image (a), 8-row x 32-column subtiles of 512 bytes,
//       off(row, ch) = 2048 (row >> 3) + 512 (ch >> 2) + 64 (row & 7) + 16 ((ch & 3) ^ ((row >> 2) & 3)),
//     conflict-free for both kinds of read with only two base registers each (constant offsets fold into the DS immediates);
//   * the image is filled by the LDS DMA (global_load_lds_dwordx4: 16 wave-instructions per 32-query step and workgroup, no staging
//     registers, no ds_write); the swizzle is applied on the global side -- which 16 bytes a lane fetches -- the DMA writes lane i
//     at base + 16 i (one instruction = 8 rows x two 64-byte column blocks).
#pragma once
#include "common.h"
#include "attention_bf16_tiles.h"      // namespace attnbf
#include "gemm_bf16.h"                 // bf16x8, bf16x4, lds_bf16x4_ptr
#include "gemm_bf16s.h"                // store_bf16x8

namespace attns {
using namespace attnbf;

// a ROWS x 128 bf16 tile in two steps (global -> registers, registers -> LDS images), so that the next tile's global loads are in
// flight during the current tile's MFMAs.  ROWS = 32 * SUB: SUB sub-tiles of 32 rows are staged per barrier pair.
template <int THREADS, int ROWS>
struct TileRegs { bf16x8 v[ROWS * (DH / 8) / THREADS]; };
template <int THREADS, int ROWS>
__device__ __forceinline__ void tile_load(TileRegs<THREADS, ROWS>& t, const __bf16* src, long ld, int tid) {
#pragma unroll
    for (int i = 0; i < ROWS * (DH / 8) / THREADS; ++i) {
        const int idx = tid + i * THREADS, row = idx >> 4, c8 = idx & 15;
        t.v[i] = *(const bf16x8*)(src + (size_t)(unsigned)(row * (int)ld + c8 * 8));
    }
}
template <int THREADS, int ROWS>
__device__ __forceinline__ void tile_store(const TileRegs<THREADS, ROWS>& t, __bf16* rowimg, __bf16* trimg, int tid) {
#pragma unroll
    for (int i = 0; i < ROWS * (DH / 8) / THREADS; ++i) {
        const int idx = tid + i * THREADS, row = idx >> 4, c8 = idx & 15;
        if (rowimg) *(bf16x8*)(rowimg + row * RSTR + c8 * 8) = t.v[i];
        if (trimg) *(bf16x8*)(trimg + row * TSTR + c8 * 8) = t.v[i];
    }
}

// one 128-element bf16 row as 8 k-step fragments: lane half h of step s holds d = 16 s + 8 h + j
__device__ __forceinline__ void load_row_frags(Frags<1>& fr, const __bf16* rowp, int lh) {
#pragma unroll
    for (int s = 0; s < 8; ++s) fr.f[0][s] = *(const bf16x8*)(rowp + 16 * s + 8 * lh);
}

// [r4] "Use" every fragment of a row right after its loads, OUTSIDE the tile loop.  The tile loops below prefetch with LDS DMAs issued from
// inline asm and wait for them with hand-counted s_waitcnt: invisible to hipcc's waitcnt pass, which therefore still counted these plain
// loads as possibly pending at the loop header and put s_waitcnt vmcnt(7) ... vmcnt(0) in front of the first MFMAs of EVERY step (the
// first uses of the fragment registers).  vmcnt is one in-order counter: those waits drained the DMAs of the next tile, issued a few
// instructions earlier -- the double buffering overlapped nothing (all three kernels: MFMA busy 0.37-0.44 in profiles/r04_config3_summary.md).
__device__ __forceinline__ void settle_frags(const Frags<1>& fr) {
#pragma unroll
    for (int s = 0; s < 8; ++s) asm volatile("" ::"v"(fr.f[0][s]));
}

// a wave's [4][32 d x 32 lane-rows] accumulators (times mul) as 32 rows of 128 bf16 (row stride ld) through an fp32 LDS patch.
// [r3] colpart (optional): 128 floats that receive the column sums of the 32 STORED (bf16) rows -- the per-block share of the
// q / k / v bias gradient, so that no kernel has to read the gradient tensor again just to sum its columns.
__device__ __forceinline__ void store_rows_bf16(const f32x16 (&o)[4], float mul, float* patch, __bf16* out, long ld, int lane, float* colpart = nullptr) {
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = o[dt][4 * g + c] * mul;
            *(f32x4*)(patch + l31 * OLD + dt * 32 + 8 * g + 4 * lh) = v;
        }
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int it = 0; it < 8; ++it) {
        const int row = it * 4 + (lane >> 4), c8 = lane & 15;
        const f32x4 a = *(const f32x4*)(patch + row * OLD + c8 * 8), b = *(const f32x4*)(patch + row * OLD + c8 * 8 + 4);
        float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
        store_bf16x8(out + (long)row * ld + c8 * 8, v);
        if (colpart != nullptr) {
#pragma unroll
            for (int i = 0; i < 8; ++i) cs[i] += (float)(__bf16)v[i];
        }
    }
    if (colpart != nullptr) {          // lanes l, l + 16, l + 32, l + 48 hold the same 8 columns for different rows
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            cs[i] += __shfl_xor(cs[i], 16, 64);
            cs[i] += __shfl_xor(cs[i], 32, 64);
        }
        if (lane < 16) {
            *(f32x4*)(colpart + lane * 8) = f32x4{cs[0], cs[1], cs[2], cs[3]};
            *(f32x4*)(colpart + lane * 8 + 4) = f32x4{cs[4], cs[5], cs[6], cs[7]};
        }
    }
}
}  // namespace attns

namespace att2 {
using namespace attnbf;
constexpr int TILEB = 32 * 256;                    // one 32 x 128 bf16 image
constexpr int LSB = 256;                           // 32 log-sum-exp + 32 delta values (fp32)
constexpr int BUF = 2 * TILEB + LSB;               // Q image | dO image | lse, delta

// [r5] the DMAs (lds_dma.h) take their address as a wave-uniform 64-bit base (scalar registers) + a 32-bit byte offset per lane: every tile of these kernels
// is "uniform tile origin + a lane pattern fixed for the whole kernel", so the per-lane 64-bit add (and the 64-bit address operand) of the flat form is dropped.
// The A/B against the per-lane pointer form is recorded in profiles/r05_attention_ab.log.

// element offset (row * ld + column) this lane fetches for DMA piece e (0..7) of a 32 x 128 tile whose rows are ld elements apart:
// piece e covers image bytes [1024 e, 1024 e + 1024) = rows 8 (e >> 1) .. + 7, column blocks 2 (e & 1) and 2 (e & 1) + 1
__device__ __forceinline__ int dma_src(int e, int lane, int ld) {
    const int row = 8 * (e >> 1) + ((lane >> 2) & 7);
    const int ch = 4 * (2 * (e & 1) + (lane >> 5)) + ((lane & 3) ^ ((row >> 2) & 3));
    return row * ld + 8 * ch;
}

struct LaneAddr {
    unsigned row0, row1;     // row read (32x32x16 A / B operand: row lane & 31, chunk 2 t + lane >> 5): t even / odd; + 512 (t >> 1)
    unsigned tr0, tr1;       // transposed read: rows 16 ss + 4 lh + q (tr0) and + 8 (tr1); + 4096 ss + 512 dt
};
__device__ __forceinline__ LaneAddr lane_addr(int lane) {
    const int l31 = lane & 31, lh = lane >> 5;
    const int s2 = (l31 >> 2) & 3;
    const unsigned rb = 2048 * (l31 >> 3) + 64 * (l31 & 7);
    const int tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;
    const unsigned tb = 64 * (4 * lh + tq) + 8 * (tp & 1);
    LaneAddr a;
    a.row0 = rb + 16 * (lh ^ s2);
    a.row1 = rb + 16 * ((lh ^ s2) ^ 2);
    a.tr0 = tb + 16 * ((2 * tg + (tp >> 1)) ^ lh);
    a.tr1 = tb + 2048 + 16 * ((2 * tg + (tp >> 1)) ^ (lh + 2));
    return a;
}

// T[32][32] = A_img[32 rows][128] x B^T, B given as 8 k-step fragments in registers: acc col = B's row (lane), rows = A's rows
__device__ __forceinline__ f32x16 rows_x_frags(const char* img, const LaneAddr& la, const Frags<1>& fr) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const bf16x8 a = *(const bf16x8*)(img + ((t & 1) ? la.row1 : la.row0) + 512 * (t >> 1));
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, fr.f[0][t], s, 0, 0, 0);
    }
    return s;
}
// the same with B read from a second image (same lane pattern): T = A_img x B_img^T
__device__ __forceinline__ f32x16 rows_x_rows(const char* aimg, const char* bimg, const LaneAddr& la) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const unsigned o = ((t & 1) ? la.row1 : la.row0) + 512 * (t >> 1);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(aimg + o), *(const bf16x8*)(bimg + o), s, 0, 0, 0);
    }
    return s;
}
// o^T[4 d-tiles][d][lane col] += sum_rows img[row][d] * p[row][lane col]: p's accumulator registers, rounded to bf16 where they
// stand, are the B operand (k order 16 ss + 8 (j >> 2) + 4 lh + (j & 3)); the image comes back transposed in exactly that order
__device__ __forceinline__ void imgT_x_p(f32x16 (&o)[4], const char* img, const LaneAddr& la, const f32x16& p) {
    bf16x8 ph[2];
#pragma unroll
    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
        for (int e = 0; e < 8; ++e) ph[ss][e] = (__bf16)p[8 * ss + e];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + la.tr0 + 4096 * ss + 512 * dt));
            const bf16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + la.tr1 + 4096 * ss + 512 * dt));
            bf16x8 f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[e] = a[e];
                f[4 + e] = c[e];
            }
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f, ph[ss], o[dt], 0, 0, 0);
        }
}
}  // namespace att2
