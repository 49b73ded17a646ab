// Backward of the fused softmax attention on bf16 tensors (bf16-storage training mode; model/modeling_vit.py:226-252 backward), flash
// style on the forward's log-sum-exp (attention_bf16s_fwd.h).  TWO kernels instead of the three of attention_bwd_bf16.h:
//   dQ       per 32-query block: S, dP, dQ (3 products) + delta.  attn_bwd_dq_bf16s2_kernel (DMA-staged, 64 keys per step) where
//            N % 64 == 0, attn_bwd_dq_bf16s_kernel (register-staged, 32-key tiles) for the other multiples of 32;
//   dK + dV  per 32-key block:   S, dV, dP, dK (4 products): S and dP are shared by the two gradient sums, the block's K rows stay in
//            registers and its V rows in a per-wave LDS image, each gradient owns its accumulator (no float atomics, fixed summation
//            order: bitwise reproducible).  7 products per tile pair instead of 8.  attn_bwd_dkv_bf16s2_kernel.
//
// [r3] The second generation (the two DMA-staged kernels).  Round 2's dK + dV kernel staged each 32-query tile of Q and dO through
// registers into FOUR padded LDS images (a row image and a transposed-read image each) with NO prefetch -- 160 accumulator / fragment
// registers left no room for staging registers -- so every tile paid a global-load round trip between two barriers: MFMA busy 0.295,
// the furthest kernel from its roofline in the whole step.  Here:
//   * ONE image per tile, filled by the LDS DMA (attention_bf16s_tiles.h), serves the row reads and the transposed reads;
//   * double buffered: the DMA of tile t + 1 is issued right after the barrier that opens tile t and lands under tile t's 32 MFMAs;
//     ONE barrier per tile (own DMA retired by s_waitcnt vmcnt(0), then s_barrier: every wave's pieces have landed and every wave
//     is done reading the buffer about to be refilled);
//   * log-sum-exp and delta of the tile's 32 queries ride along as one global_load_lds_dword.
// Arithmetic per (32 queries x 32 keys) pair and wave is round 2's: S, dV, dP, dK = 4 products, P and dS rounded to bf16 where they
// become MFMA operands, fixed summation order, no atomics -> bitwise reproducible.
#pragma once
#include "common.h"
#include "attention_bf16_tiles.h"      // attnbf::Frags, tile_x_frags, acc_tile_t_x_p, the image strides
#include "attention_bf16s_tiles.h"
#include "gemm_bf16.h"                 // bf16x8
#include "lds_dma.h"

// ------------------------------------------------------------------------------------------------- dQ (register-staged; N % 64 != 0)
// SUB sub-tiles of 32 keys per barrier pair.
template <int NW, int SUB>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_dq_bf16s_kernel(const __bf16* __restrict__ QKV, const __bf16* __restrict__ O,
                                                                      const __bf16* __restrict__ dO, const float* __restrict__ LSE,
                                                                      __bf16* __restrict__ dQKV, float* __restrict__ DELTA, int N, int heads,
                                                                      int qgroups, float scale) {
    using namespace attns;
    constexpr int THREADS = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) __bf16 bsm_s[];
    constexpr int ROWS = 32 * SUB;
    __bf16* Krow = bsm_s;
    __bf16* Ktr = Krow + SUB * RIMG;
    __bf16* Vrow = Ktr + SUB * TIMG;
    // XCD-aware block order (as the forward): the workgroups of one (batch, head) stream the same K / V tiles; dealt round-robin over
    // the 8 XCDs each would fetch them into its own L2 (measured: 15 GB of L2-side reads per launch against 6 GB algorithmic)
    const int lin = xcd_lin(blockIdx.x, gridDim.x);
    const int bh = lin / qgroups, qg = lin - bh * qgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const long ld3 = 3L * D;
    const __bf16* qkv = QKV + (long)b * N * ld3 + h * DH;
    const int qb = qg * NW + wid;
    const bool valid = qb * 32 < N;
    const int q0 = min(qb * 32, N - 32);
    const long orow = ((long)b * N + q0 + l31) * D + h * DH;
    Frags<1> qf, dof;
    load_row_frags(qf, qkv + (long)(q0 + l31) * ld3, lh);
    load_row_frags(dof, dO + orow, lh);
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const bf16x8 o8 = *(const bf16x8*)(O + orow + 16 * s + 8 * lh);
#pragma unroll
        for (int u = 0; u < 8; ++u) delta += (float)o8[u] * (float)dof.f[0][s][u];
    }
    delta += __shfl_xor(delta, 32, 64);
    const float lse = LSE[(long)bh * N + q0 + l31];
    if (valid && lh == 0) DELTA[(long)bh * N + q0 + l31] = delta;
    const float c2 = scale * 1.4426950408889634f, lse2 = lse * 1.4426950408889634f;
    f32x16 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
    TileRegs<THREADS, ROWS> tk, tv;
    tile_load(tk, qkv + D, ld3, tid);
    tile_load(tv, qkv + 2 * D, ld3, tid);
    const int ntiles = N / ROWS;
    for (int kt = 0; kt < ntiles; ++kt) {
        __syncthreads();
        tile_store(tk, Krow, Ktr, tid);
        tile_store(tv, Vrow, nullptr, tid);
        __syncthreads();
        if (kt + 1 < ntiles) {
            tile_load(tk, qkv + (long)((kt + 1) * ROWS) * ld3 + D, ld3, tid);
            tile_load(tv, qkv + (long)((kt + 1) * ROWS) * ld3 + 2 * D, ld3, tid);
        }
#pragma unroll
        for (int sub = 0; sub < SUB; ++sub) {
            f32x16 s = tile_x_frags<1>(Krow + sub * RIMG, qf, l31, lh);             // S^T[key][q]
            const f32x16 dp = tile_x_frags<1>(Vrow + sub * RIMG, dof, l31, lh);     // dP^T[key][q]
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lse2)) * (dp[r] - delta) * scale;   // dS^T
            acc_tile_t_x_p<1>(dq, Ktr + sub * TIMG, s, lane);                       // dQ^T[d][q] += K^T dS^T
        }
    }
    __syncthreads();
    if (valid) store_rows_bf16(dq, 1.0f, (float*)bsm_s + wid * 32 * OLD, dQKV + ((long)b * N + q0) * ld3 + h * DH, ld3, lane);
}

// ------------------------------------------------------------------------------------------------- dK and dV
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_dkv_bf16s2_kernel(const __bf16* __restrict__ QKV, const __bf16* __restrict__ dO,
                                                                        const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                                        __bf16* __restrict__ dQKV, int N, int heads, int kgroups, float scale,
                                                                        float* __restrict__ colpart) {
    // colpart (or null): fp32 [B * N / 32][3 * heads * 128]; row (b, key block) receives the column sums of the block's 32 dK rows at
    // columns D + h * 128 .. and of its dV rows at 2 D + h * 128 ..  (the dQ kernel fills columns h * 128 .. of row (b, query block))
    using namespace att2;
    static_assert(NW == 4, "a workgroup's four waves stage the four 8-row groups of a tile");
    extern __shared__ __attribute__((aligned(16))) char sm2[];
    const int lin = xcd_lin(blockIdx.x, gridDim.x);          // the key blocks of one (batch, head) share Q / dO tiles in one L2
    const int bh = lin / kgroups, kg = lin - bh * kgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const int ld3 = 3 * D;
    const __bf16* qkv = QKV + (long)b * N * ld3 + h * DH;
    const __bf16* dob = dO + (long)b * N * D + h * DH;
    const float* lsep = LSE + (long)bh * N;
    const float* delp = DELTA + (long)bh * N;
    const int kb = kg * NW + wid;
    const bool valid = kb * 32 < N;            // invalid waves (last group of a head) redo the last key block and skip the store
    const int k0 = min(kb * 32, N - 32);
    const unsigned lds0 = lds_addr_of(sm2);
    const unsigned vimg = 2 * BUF + wid * TILEB;               // this wave's V rows (dP = dO V^T reads them as the B operand)

    Frags<1> kf;                                               // K rows of this wave's 32 keys, all 128 d: B operand of S = Q K^T
    attns::load_row_frags(kf, qkv + (long)(k0 + l31) * ld3 + D, lh);
#pragma unroll
    for (int e = 0; e < 8; ++e) lds_dma16(qkv + (long)k0 * ld3 + 2 * D + dma_src(e, lane, ld3), lds0 + vimg + 1024 * e);

    // DMA duty per tile: 8-row group `wid` of the Q tile and of the dO tile (two pieces each); wave 0 also fetches lse | delta
    const unsigned oq0 = 2u * dma_src(2 * wid, lane, ld3), oq1 = 2u * dma_src(2 * wid + 1, lane, ld3);      // byte offsets from the tile's first row
    const unsigned od0 = 2u * dma_src(2 * wid, lane, D), od1 = 2u * dma_src(2 * wid + 1, lane, D);
    auto issue = [&](int qt, unsigned boff) __attribute__((always_inline)) {
        const unsigned long long qs = lds_dma_base(qkv + (long)(qt * 32) * ld3);
        const unsigned long long ds = lds_dma_base(dob + (long)(qt * 32) * D);
        const unsigned a = lds0 + boff + 2048 * wid;
        lds_dma16(oq0, qs, a);
        lds_dma16(oq1, qs, a + 1024);
        lds_dma16(od0, ds, a + TILEB);
        lds_dma16(od1, ds, a + TILEB + 1024);
        if (wid == 0) lds_dma4((lane < 32 ? lsep : delp - 32) + qt * 32 + lane, lds0 + boff + 2 * TILEB);
    };
    const LaneAddr la = lane_addr(lane);
    const float c2 = scale * 1.4426950408889634f;
    f32x16 dk[4], dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[dt][r] = dv[dt][r] = 0.f;

    const int ntiles = N / 32;
    issue(0, 0);
    attns::settle_frags(kf);                                    // (the waits for these loads belong here, not inside the tile loop: attention_bf16s_tiles.h)
    auto step = [&](int qt, unsigned boff) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's pieces of tile qt (issued a whole tile ago) have landed ...
        __builtin_amdgcn_s_barrier();                           // ... and so have everyone's; everyone is done with the other buffer
        __builtin_amdgcn_sched_barrier(0);
        if (qt + 1 < ntiles) issue(qt + 1, boff ^ BUF);         // lands under this tile's MFMAs
        if (!valid) return;                                     // (wave-uniform) a wave past the last key block only stages: its SIMD's matrix pipe goes to the CU's other workgroup
        const char* Qi = sm2 + boff;
        const char* Di = sm2 + boff + TILEB;
        const float* Ls = (const float*)(sm2 + boff + 2 * TILEB);
        f32x16 p = rows_x_frags(Qi, la, kf);                   // S[q][key]
        // accumulator register r holds query (r & 3) + 8 (r >> 2) + 4 lh: registers 4 g .. 4 g + 3 are four consecutive queries
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 l4 = *(const f32x4*)(Ls + 8 * g + 4 * lh);
#pragma unroll
            for (int c = 0; c < 4; ++c) p[4 * g + c] = __builtin_amdgcn_exp2f(fmaf(p[4 * g + c], c2, -1.4426950408889634f * l4[c]));
        }
        imgT_x_p(dv, Di, la, p);                                // dV^T[d][key] += dO^T P
        const f32x16 dp = rows_x_rows(Di, sm2 + vimg, la);      // dP[q][key] = dO V^T
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 d4 = *(const f32x4*)(Ls + 32 + 8 * g + 4 * lh);
#pragma unroll
            for (int c = 0; c < 4; ++c) p[4 * g + c] = p[4 * g + c] * (dp[4 * g + c] - d4[c]) * scale;      // dS[q][key]
        }
        imgT_x_p(dk, Qi, la, p);                                // dK^T[d][key] += Q^T dS
    };
    for (int qt = 0; qt < ntiles; qt += 2) {
        step(qt, 0);
        if (qt + 1 < ntiles) step(qt + 1, BUF);
    }
    __syncthreads();                                           // the images are dead: their space becomes the output patches
    if (valid) {
        float* patch = (float*)sm2 + wid * 32 * OLD;
        __bf16* dst = dQKV + ((long)b * N + k0) * ld3 + h * DH;
        float* cp = colpart ? colpart + ((long)b * (N / 32) + kb) * ld3 + h * DH : nullptr;
        attns::store_rows_bf16(dk, 1.0f, patch, dst + D, ld3, lane, cp ? cp + D : nullptr);
        attns::store_rows_bf16(dv, 1.0f, patch, dst + 2 * D, ld3, lane, cp ? cp + 2 * D : nullptr);    // same wave, same patch: program order
    }
}

static hipError_t attention_bf16s2_dkv_launch(const __bf16* QKV, const __bf16* dO, const float* LSE, const float* DELTA, __bf16* dQKV, int B, int N,
                                              int heads, hipStream_t stream, float* colpart) {
    using namespace att2;
    constexpr int NW = 4;
    constexpr size_t img = 2 * BUF + (size_t)NW * TILEB, patch = (size_t)NW * 32 * OLD * 4;
    constexpr size_t lds = img > patch ? img : patch;
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    auto kern = attn_bwd_dkv_bf16s2_kernel<NW>;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    const int groups = (N / 32 + NW - 1) / NW;
    hipLaunchKernelGGL(kern, dim3(B * heads * groups), dim3(64 * NW), lds, stream, QKV, dO, LSE, DELTA, dQKV, N, heads, groups, 1.0f / sqrtf((float)DH),
                       colpart);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- dQ (+ delta), generation 2
// Per 32-query block and wave: S^T = K Q^T, dP^T = V dO^T (A operand = K / V rows from the image, B = Q / dO fragments in
// registers), dQ^T += K^T dS^T (K transposed from the SAME image).  64 keys per step: K and V tiles as 2 + 2 images, DMA-staged and
// double buffered as above (32 pieces per step and workgroup, 8 per wave).
template <int NW>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_dq_bf16s2_kernel(const __bf16* __restrict__ QKV, const __bf16* __restrict__ O,
                                                                       const __bf16* __restrict__ dO, const float* __restrict__ LSE,
                                                                       __bf16* __restrict__ dQKV, float* __restrict__ DELTA, int N, int heads,
                                                                       int qgroups, float scale, float* __restrict__ colpart) {
    using namespace att2;
    static_assert(NW == 4, "four waves share the DMA duty of a 64-key step");
    constexpr unsigned KVBUF = 4 * TILEB;                      // K keys 0-31 | K keys 32-63 | V keys 0-31 | V keys 32-63
    extern __shared__ __attribute__((aligned(16))) char sm2[];
    const int lin = xcd_lin(blockIdx.x, gridDim.x);
    const int bh = lin / qgroups, qg = lin - bh * qgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6), l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const int ld3 = 3 * D;
    const __bf16* qkv = QKV + (long)b * N * ld3 + h * DH;
    const int qb = qg * NW + wid;
    const bool valid = qb * 32 < N;
    const int q0 = min(qb * 32, N - 32);
    const long orow = ((long)b * N + q0 + l31) * D + h * DH;
    const unsigned lds0 = lds_addr_of(sm2);
    unsigned ok[4];                                            // this wave's 4 K pieces of a step, in bytes from the step's first row (the V pieces sit D elements further)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = 4 * wid + i;
        ok[i] = 2u * (unsigned)(32 * (e >> 3) * ld3 + D + dma_src(e & 7, lane, ld3));
    }
    auto issue = [&](int kt, unsigned boff) __attribute__((always_inline)) {
        const unsigned long long src = lds_dma_base(qkv + (long)(kt * 64) * ld3);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned a = lds0 + boff + 1024 * (4 * wid + i);         // piece e of the step: image e >> 3, piece e & 7 = byte 1024 e
            lds_dma16(ok[i], src, a);
            lds_dma16(ok[i], src + 2ull * D, a + 2 * TILEB);
        }
    };
    issue(0, 0);
    Frags<1> qf, dof;
    attns::load_row_frags(qf, qkv + (long)(q0 + l31) * ld3, lh);
    attns::load_row_frags(dof, dO + orow, lh);
    float delta = 0.f;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const bf16x8 o8 = *(const bf16x8*)(O + orow + 16 * s + 8 * lh);
#pragma unroll
        for (int u = 0; u < 8; ++u) delta += (float)o8[u] * (float)dof.f[0][s][u];
    }
    delta += __shfl_xor(delta, 32, 64);
    const float lse = LSE[(long)bh * N + q0 + l31];
    if (valid && lh == 0) DELTA[(long)bh * N + q0 + l31] = delta;
    const float c2 = scale * 1.4426950408889634f, lse2 = lse * 1.4426950408889634f;
    attns::settle_frags(qf);
    attns::settle_frags(dof);
    asm volatile("" ::"v"(lse2), "v"(delta));
    const LaneAddr la = lane_addr(lane);
    f32x16 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dq[dt][r] = 0.f;
    const int ntiles = N / 64;
    auto step = [&](int kt, unsigned boff) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < ntiles) issue(kt + 1, boff ^ KVBUF);
        if (!valid) return;                                     // (wave-uniform) stage only
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const char* Ki = sm2 + boff + sub * TILEB;
            const char* Vi = sm2 + boff + 2 * TILEB + sub * TILEB;
            f32x16 s = rows_x_frags(Ki, la, qf);                 // S^T[key][q]
            const f32x16 dp = rows_x_frags(Vi, la, dof);         // dP^T[key][q]
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], c2, -lse2)) * (dp[r] - delta) * scale;   // dS^T
            imgT_x_p(dq, Ki, la, s);                             // dQ^T[d][q] += K^T dS^T
        }
    };
    for (int kt = 0; kt < ntiles; kt += 2) {
        step(kt, 0);
        if (kt + 1 < ntiles) step(kt + 1, KVBUF);
    }
    __syncthreads();
    if (valid)
        attns::store_rows_bf16(dq, 1.0f, (float*)sm2 + wid * 32 * OLD, dQKV + ((long)b * N + q0) * ld3 + h * DH, ld3, lane,
                               colpart ? colpart + ((long)b * (N / 32) + qb) * ld3 + h * DH : nullptr);
}

static hipError_t attention_bf16s2_dq_launch(const __bf16* QKV, const __bf16* O, const __bf16* dO, const float* LSE, float* DELTA, __bf16* dQKV, int B, int N,
                                             int heads, hipStream_t stream, float* colpart) {
    using namespace att2;
    constexpr int NW = 4;
    constexpr size_t img = 2 * 4 * (size_t)TILEB, patch = (size_t)NW * 32 * OLD * 4;
    constexpr size_t lds = img > patch ? img : patch;
    static_assert(2 * lds <= 160 * 1024, "two workgroups per CU");
    auto kern = attn_bwd_dq_bf16s2_kernel<NW>;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    const int groups = (N / 32 + NW - 1) / NW;
    hipLaunchKernelGGL(kern, dim3(B * heads * groups), dim3(64 * NW), lds, stream, QKV, O, dO, LSE, dQKV, DELTA, N, heads, groups, 1.0f / sqrtf((float)DH),
                       colpart);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------- the backward: dQ (either kernel), then dK + dV
static hipError_t attention_bf16s_bwd_launch(const __bf16* QKV, const __bf16* O, const __bf16* dO, const float* LSE, float* DELTA, __bf16* dQKV, int B, int N,
                                             int heads, hipStream_t stream, float* colpart = nullptr) {
    // colpart (N % 64 == 0 only): fp32 [B * N / 32][3 * heads * 128] partial column sums of dQKV, one row per 32-row block -- summed over
    // the rows they give the q | k | v bias gradients
    using namespace attns;
    if (B <= 0) return hipSuccess;
    if (N % 32 != 0) return hipErrorInvalidValue;
    if (colpart != nullptr && N % 64 != 0) return hipErrorInvalidValue;
    if (N % 64 == 0) {       // the DMA-staged dQ kernel walks the keys 64 at a time
        hipError_t e = attention_bf16s2_dq_launch(QKV, O, dO, LSE, DELTA, dQKV, B, N, heads, stream, colpart);
        if (e != hipSuccess) return e;
    } else {                 // other multiples of 32: the register-staged dQ kernel on 32-key tiles
        constexpr int NW = 4, SUB = 1;
        const int groups = (N / 32 + NW - 1) / NW;
        constexpr size_t patch = (size_t)NW * 32 * OLD * 4, img_q = (size_t)SUB * (2 * RIMG + TIMG) * 2;
        constexpr size_t lds_q = img_q > patch ? img_q : patch;
        static_assert(2 * lds_q <= 160 * 1024, "two workgroups per CU");
        if (hipError_t e = ego_allow_dynamic_lds((const void*)attn_bwd_dq_bf16s_kernel<NW, SUB>, (int)lds_q); e != hipSuccess) return e;
        hipLaunchKernelGGL((attn_bwd_dq_bf16s_kernel<NW, SUB>), dim3(B * heads * groups), dim3(64 * NW), lds_q, stream, QKV, O, dO, LSE, dQKV, DELTA, N, heads, groups,
                           1.0f / sqrtf((float)DH));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return attention_bf16s2_dkv_launch(QKV, dO, LSE, DELTA, dQKV, B, N, heads, stream, colpart);
}
