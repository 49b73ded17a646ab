// Forward of the fused softmax attention on bf16 tensors (bf16-storage training mode and bf16 serving; model/modeling_vit.py:226-252):
//   ctx = softmax(Q K^T / sqrt(128)) V, with the log-sum-exp of every query row kept for the backward (attention_bf16s_bwd.h).
// K and V tiles are DMA-staged into the one-image layout of attention_bf16s_tiles.h, 32 keys per step, three K | V buffers; the DMA of
// tile t + 1 is issued right after the barrier that opens tile t and lands under tile t's MFMAs; ONE barrier per tile (own DMA retired
// by s_waitcnt vmcnt(0), then s_barrier: every wave's pieces have landed and every wave is done reading the buffer about to be refilled).
#pragma once
#include "common.h"
#include "attention_bf16_tiles.h"      // attnbf::Frags, DH
#include "attention_bf16s_tiles.h"
#include "gemm_bf16.h"                 // bf16x8, bf16x4, lds_bf16x4_ptr
#include "gemm_bf16s.h"                // store_bf16x8
#include "lds_dma.h"

// ------------------------------------------------------------------------------------------------- forward, 32-key steps, three workgroups per CU
// [r3] At N = 576 a (batch, head) pair is 4.5 workgroups of 9 steps each and the per-block cost (dispatch, Q load, first tile's round trip,
// output store) is worth 5.4 steps (measured: 0.67 PF at N = 576 against 0.93 PF at N = 2304 on the same kernel).  With two workgroups per
// CU there is one partner to run under it.  The forward needs 160 VGPRs, so three waves per SIMD fit; what held it at two was LDS
// (64 KB of images, a 68 KB output patch).  This variant steps 32 keys at a time (32 KB of images) and stores its output through a
// half-width patch in two passes (35 KB): three workgroups per CU.  Same arithmetic and summation order as the 64-key kernel.
namespace att2 {
__device__ __forceinline__ void store_rows_bf16_2pass(const f32x16 (&o)[4], float mul, float* patch, __bf16* out, long ld, int lane) {
    constexpr int PLD = 68;
    const int l31 = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
#pragma unroll
        for (int dd = 0; dd < 2; ++dd)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = o[2 * half + dd][4 * g + c] * mul;
                *(f32x4*)(patch + l31 * PLD + dd * 32 + 8 * g + 4 * lh) = v;
            }
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int row = it * 8 + (lane >> 3), c8 = lane & 7;
            const f32x4 a = *(const f32x4*)(patch + row * PLD + c8 * 8), b = *(const f32x4*)(patch + row * PLD + c8 * 8 + 4);
            float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
            store_bf16x8(out + (long)row * ld + half * 64 + c8 * 8, v);
        }
    }
}
}  // namespace att2

namespace att2 {
// o^T += V^T P for bf16 P fragments that already exist (the deferred form keeps a tile's P across a step)
__device__ __forceinline__ void imgT_x_ph(f32x16 (&o)[4], const char* img, const LaneAddr& la, const bf16x8 (&ph)[2]) {
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

template <int NW>
__global__ __launch_bounds__(64 * NW, 3) void attention_bf16s3_kernel(const __bf16* __restrict__ QKV, __bf16* __restrict__ CTX, int N, int heads,
                                                                     int qgroups, float scale_log2e, float* __restrict__ LSE) {
    using namespace att2;
    static_assert(NW >= 2 && NW <= 4, "the workgroup's waves share the 8 + 8 DMA pieces of a 32-key step");
    constexpr unsigned KVBUF = 2 * TILEB;                      // K image | V image
    // The running maximum is only raised (and the output accumulators rescaled) when a query's scores exceed it by more than 2^RESC in the
    // softmax's base-2 units (cdna_hip_programming.md T13): probabilities then stay below 2^RESC, harmless in fp32 sums and bf16 operands,
    // and the 64 multiplies per step disappear from almost every tile.
    constexpr float RESC = 6.0f;
    extern __shared__ __attribute__((aligned(16))) char sm3[];
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
    const unsigned lds0 = lds_addr_of(sm3);
    constexpr int PPW = (8 + NW - 1) / NW;                     // pieces per wave: wave w takes pieces w, w + NW, ... < 8 of the K and of the V image
    unsigned ok[PPW];                                          // bytes from the tile's first row
#pragma unroll
    for (int i = 0; i < PPW; ++i) ok[i] = 2u * (unsigned)(D + dma_src(min(wid + i * NW, 7), lane, ld3));
    auto issue = [&](int kt, unsigned boff) __attribute__((always_inline)) {
        const unsigned long long src = lds_dma_base(qkv + (long)(kt * 32) * ld3);
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            if (wid + i * NW < 8) {                             // wave-uniform
                const unsigned a = lds0 + boff + 1024 * (wid + i * NW);
                lds_dma16(ok[i], src, a);
                lds_dma16(ok[i], src + 2ull * D, a + TILEB);
            }
        }
    };
    const int ntiles = N / 32;
    issue(0, 0);
    Frags<1> qf;
    attns::load_row_frags(qf, qkv + (long)(q0 + l31) * ld3, lh);
    attns::settle_frags(qf);
    const LaneAddr la = lane_addr(lane);
    f32x16 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[dt][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;
    // [r5] P V of tile t - 1 runs DURING the softmax of tile t.  Through round 4 a wave's step was the dependent chain  S (8 MFMAs) -> row maximum ->
    // 16 exp2 -> bf16 P -> transposed V reads -> P V (8 MFMAs): its VALU part had no matrix work of its own beside it (round-4 verdict: "the waves
    // run the same chain in phase").  Here the 8 MFMAs and 16 transposed reads of the PREVIOUS tile's P V are interleaved with the exponentials of this
    // tile, group by group (sched_group_barrier): chain per step  S -> {softmax(t) || P V(t - 1)}.  The V image of tile t - 1 lives one step longer:
    // the three K | V buffers hold tiles t - 1, t and (in flight) t + 1 -- ONE tile ahead (round 4 ran two ahead and measured that the DMA was never
    // late), requested right after the barrier that ends every wave's use of tile t - 2.
    // Measured (same-call A/Bs against the round-4 kernel, profiles/r05_attention_ab.log and DESIGN 3.13): 1.704 -> 1.685 ms per layer at B = 1024,
    // N = 576 and 5.36 -> 5.30 ms at N = 2304 in one call, 1.710 / 1.714 and 5.382 / 5.381 in another: at most one per cent, inside the run-to-run
    // spread; bit-identical context and log-sum-exp.  So the chain was NOT what holds the kernel at half the matrix pipe -- with three waves per SIMD
    // the partners already ran under each other's softmax.  What the SIMD runs out of is issue time: per 32 x 32 wave-step 16 MFMAs x 8 cycles of
    // issue, ~60 VALU, 16 transcendentals, 24 LDS reads and 4 LDS-DMA pieces at ~60 cycles each, times three waves, against 1536 matrix cycles.
    // (Also measured: the same deferral left to hipcc's scheduler at two waves per SIMD: 236 VGPRs, 1.98 ms; the next tile's DMA issued from
    // inside the softmax instead of behind the barrier: -0.8 % / -1.9 %.)
    // ONE code path writes O (two paths -- a plain P V before a rescale, an interleaved one otherwise -- made hipcc copy the accumulator tuples
    // between them: 210 spilled registers): the exponentials of tile t are taken against the NEW maximum while P V(t - 1) accumulates at the old
    // scale; O and l are rescaled after it, before P V(t) in the next step.
    bf16x8 ph[2];
    auto softmax_head = [&](const f32x16& s, float& alpha, bool& any) __attribute__((always_inline)) {
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64)) * scale_log2e;
        const bool raise = mx > m_run + RESC;
        any = __builtin_amdgcn_ballot_w64(raise) != 0;
        const float m_new = raise ? mx : m_run;
        alpha = any ? exp2f(m_run - m_new) : 1.f;
        m_run = m_new;
    };
    auto open = [&](int kt, unsigned bnext) __attribute__((always_inline)) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if (kt + 1 < ntiles) issue(kt + 1, bnext);
    };
    auto to_ph = [&](const f32x16& s) __attribute__((always_inline)) {
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
            for (int e = 0; e < 8; ++e) ph[ss][e] = (__bf16)s[8 * ss + e];
    };
    // tile 0: nothing pending (m_run = -inf: alpha = 0 on an O and l of zeros)
    open(0, KVBUF);
    if (valid) {
        f32x16 s = rows_x_frags(sm3, la, qf);
        float alpha;
        bool any;
        softmax_head(s, alpha, any);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -m_run));
            psum += s[r];
        }
        l_run = psum;
        to_ph(s);
    }
    auto step = [&](int kt, unsigned boff, unsigned bnext, unsigned bprev) __attribute__((always_inline)) {
        open(kt, bnext);
        if (!valid) return;
        f32x16 s = rows_x_frags(sm3 + boff, la, qf);
        float alpha;
        bool any;
        softmax_head(s, alpha, any);
        float psum = 0.f;
        // 8 groups of { 1 MFMA of P V(t - 1) on fragments read one group ahead, the next group's 2 transposed reads, 2 exponentials of tile t }
        // (left to itself hipcc hoists all 16 reads and all the exponentials: 236 VGPRs, two waves per SIMD, 1.98 ms)
        const char* img = sm3 + bprev + TILEB;
        auto frag = [&](int g) __attribute__((always_inline)) {
            const int dt = g >> 1, ss = g & 1;
            const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + la.tr0 + 4096 * ss + 512 * dt));
            const bf16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(img + la.tr1 + 4096 * ss + 512 * dt));
            bf16x8 f;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[e] = a[e];
                f[4 + e] = c[e];
            }
            return f;
        };
        bf16x8 fc = frag(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            bf16x8 fn = fc;
            if (g < 7) fn = frag(g + 1);
            o[g >> 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fc, ph[g & 1], o[g >> 1], 0, 0, 0);
#pragma unroll
            for (int r = 2 * g; r < 2 * g + 2; ++r) {
                s[r] = __builtin_amdgcn_exp2f(fmaf(s[r], scale_log2e, -m_run));
                psum += s[r];
            }
            fc = fn;
        }
        // the order above, spelled out for the machine scheduler (the IR optimiser sinks the exponentials below the last MFMA otherwise, and
        // scheduling fences between the groups cannot bring them back): per group 1 MFMA, the next group's 2 reads, 2 fma + 2 exp + 2 add
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (g < 7) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x400, 2, 0);
            __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        }
        l_run = l_run * alpha + psum;
        to_ph(s);                                                // (before the branch below: hipcc's IR passes sink the exponentials to their first use otherwise, out of the scheduled region)
        asm volatile("" : "+v"(ph[0]), "+v"(ph[1]), "+v"(l_run));
        __builtin_amdgcn_sched_barrier(0);
        if (any) {                                               // (wave-uniform, rare: the maximum grew by more than 2^RESC)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[dt][r] *= alpha;
        }
    };
    for (int kt = 1; kt < ntiles; kt += 3) {                 // buffer of tile t: t mod 3; tile t + 1 goes where tile t - 2 was
        step(kt, KVBUF, 2 * KVBUF, 0);
        if (kt + 1 < ntiles) step(kt + 1, 2 * KVBUF, 0, KVBUF);
        if (kt + 2 < ntiles) step(kt + 2, 0, KVBUF, 2 * KVBUF);
    }
    if (valid) imgT_x_ph(o, sm3 + ((ntiles - 1) % 3) * KVBUF + TILEB, la, ph);
    __syncthreads();
    if (valid) {
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        if (LSE != nullptr && lh == 0) LSE[(long)bh * N + q0 + l31] = m_run * 0.6931471805599453f + logf(l_tot);
        store_rows_bf16_2pass(o, 1.0f / l_tot, (float*)sm3 + wid * 32 * 68, CTX + ((long)b * N + q0) * D + h * DH, D, lane);
    }
}

template <int NW>
static hipError_t attention_bf16s3_fwd_launch_t(const __bf16* QKV, __bf16* CTX, float* LSE, int B, int N, int heads, hipStream_t stream) {
    using namespace att2;
    constexpr size_t img = 3 * 2 * (size_t)TILEB, patch = (size_t)NW * 32 * 68 * 4;           // three K | V buffers
    constexpr size_t lds = img > patch ? img : patch;
    static_assert(NW == 2 || (12 / NW) * lds <= 160 * 1024, "twelve waves (three per SIMD) per CU (two-wave workgroups: five per CU, ten waves)");
    auto kern = attention_bf16s3_kernel<NW>;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)kern, (int)lds); e != hipSuccess) return e;
    const int groups = (N / 32 + NW - 1) / NW;
    hipLaunchKernelGGL(kern, dim3(B * heads * groups), dim3(64 * NW), lds, stream, QKV, CTX, N, heads, groups, 1.4426950408889634f / sqrtf(128.0f), LSE);
    return hipGetLastError();
}
static hipError_t attention_bf16s3_fwd_launch(const __bf16* QKV, __bf16* CTX, float* LSE, int B, int N, int heads, hipStream_t stream) {
    // four waves per workgroup: three-wave workgroups (no idle wave at N = 576: 18 query blocks = 6 x 3) measured equal at N = 576 and
    // 7 % slower at N = 2304, two-wave ones 20 % slower (each workgroup streams the pair's whole K and V)
    return attention_bf16s3_fwd_launch_t<4>(QKV, CTX, LSE, B, N, heads, stream);
}

static hipError_t attention_bf16s_fwd_launch(const __bf16* QKV, __bf16* CTX, float* LSE, int B, int N, int heads, hipStream_t stream) {
    if (B <= 0) return hipSuccess;
    if (N % 32 != 0) return hipErrorInvalidValue;
    return attention_bf16s3_fwd_launch(QKV, CTX, LSE, B, N, heads, stream);      // 32-key steps, three workgroups per CU
}
