// Backward of the fused softmax attention on the bf16 matrix cores (opt-in modes of egotap_set_precision), fp32 tensors in HBM.
// Same three kernels, same math and the same fixed summation orders as attention_bwd_f32.h (flash style: P is recomputed from
// Q, K and the forward's log-sum-exp; dQ, dV, dK each own their accumulator, no float atomics):
//   dV = P^T dO,  dP = dO V^T,  dS = P * (dP - delta) / sqrt(dh),  dQ = dS K,  dK = dS^T Q.
// Every product runs on v_mfma_f32_32x32x16_bf16 with operands made in registers (NP = 3 or 1).  The row image, the transposed-read
// image and the tile products are attention_bf16_tiles.h's; K in dQ and Q in dK are used both ways and get both images.
#pragma once
#include "common.h"
#include "attention_bf16_tiles.h"

// ------------------------------------------------------------------------------------------------- dQ (+ delta)
// Invalid waves (query block past N) run the whole loop on clamped rows and skip only the final store: EXEC stays all
// ones around the transposing reads.
template <int NW, int NP>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_dq_bf16_kernel(const float* __restrict__ QKV, const float* __restrict__ O,
                                                                      const float* __restrict__ dO, const float* __restrict__ LSE,
                                                                      float* __restrict__ dQKV, float* __restrict__ DELTA, int N,
                                                                      int heads, int qgroups, float scale) {
    using namespace attnbf;
    extern __shared__ __attribute__((aligned(16))) __bf16 bsm[];
    __bf16* Krow = bsm;
    __bf16* Ktr = Krow + rimg_pair<NP>();
    __bf16* Vrow = Ktr + timg_pair<NP>();
    const int bh = blockIdx.x / qgroups, qg = blockIdx.x - bh * qgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const long ld3 = 3L * D;
    const float* qkv = QKV + (long)b * N * ld3 + h * DH;
    const int qb = qg * NW + wid;
    const bool valid = qb * 32 < N;
    const int q0 = min(qb * 32, N - 32);
    const long orow = ((long)b * N + q0 + l31) * D + h * DH;

    Frags<NP> qf, dof;
    load_row_frags<NP>(qf, qkv + (long)(q0 + l31) * ld3, lh);
    load_row_frags<NP>(dof, dO + orow, lh);
    float delta = 0.f;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const f32x4 o4 = *(const f32x4*)(O + orow + 8 * t + 4 * lh), d4 = *(const f32x4*)(dO + orow + 8 * t + 4 * lh);
#pragma unroll
        for (int u = 0; u < 4; ++u) delta += o4[u] * d4[u];
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
    for (int kt = 0; kt < N / KT; ++kt) {
        __syncthreads();
        stage<64 * NW, NP>(Krow, Ktr, qkv + (long)(kt * KT) * ld3 + D, ld3, tid);
        stage<64 * NW, NP>(Vrow, nullptr, qkv + (long)(kt * KT) * ld3 + 2 * D, ld3, tid);
        __syncthreads();
        f32x16 s = tile_x_frags<NP>(Krow, qf, l31, lh);            // S^T[key][q]
        const f32x16 dp = tile_x_frags<NP>(Vrow, dof, l31, lh);    // dP^T[key][q]
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = exp2f(fmaf(s[r], c2, -lse2)) * (dp[r] - delta) * scale;   // dS^T
        acc_tile_t_x_p<NP>(dq, Ktr, s, lane);                      // dQ^T[d][q] += K^T dS^T
    }
    __syncthreads();
    if (valid) store_rows(dq, (float*)bsm + wid * 32 * OLD, dQKV + ((long)b * N + q0) * ld3 + h * DH, ld3, l31, lh);
}

// ------------------------------------------------------------------------------------------------- dV
template <int NW, int NP>
__global__ __launch_bounds__(64 * NW, 2) void attn_bwd_dv_bf16_kernel(const float* __restrict__ QKV, const float* __restrict__ dO,
                                                                      const float* __restrict__ LSE, float* __restrict__ dQKV, int N,
                                                                      int heads, int kgroups, float scale) {
    using namespace attnbf;
    extern __shared__ __attribute__((aligned(16))) __bf16 bsm[];
    __bf16* Qrow = bsm;
    __bf16* Dtr = Qrow + rimg_pair<NP>();
    float* Ls = (float*)(Dtr + timg_pair<NP>());      // lse of the tile's 32 queries (log2 units)
    const int bh = blockIdx.x / kgroups, kg = blockIdx.x - bh * kgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const long ld3 = 3L * D;
    const float* qkv = QKV + (long)b * N * ld3 + h * DH;
    const int kb = kg * NW + wid;
    const bool valid = kb * 32 < N;
    const int k0 = min(kb * 32, N - 32);
    Frags<NP> kf;
    load_row_frags<NP>(kf, qkv + (long)(k0 + l31) * ld3 + D, lh);
    const float c2 = scale * 1.4426950408889634f;
    f32x16 dv[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dv[dt][r] = 0.f;
    for (int qt = 0; qt < N / KT; ++qt) {
        __syncthreads();
        stage<64 * NW, NP>(Qrow, nullptr, qkv + (long)(qt * KT) * ld3, ld3, tid);
        stage<64 * NW, NP>(nullptr, Dtr, dO + ((long)b * N + qt * KT) * D + h * DH, D, tid);
        if (tid < 32) Ls[tid] = LSE[(long)bh * N + qt * KT + tid] * 1.4426950408889634f;
        __syncthreads();
        f32x16 p = tile_x_frags<NP>(Qrow, kf, l31, lh);             // S[q][key]
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = exp2f(fmaf(p[r], c2, -Ls[(r & 3) + 8 * (r >> 2) + 4 * lh]));
        acc_tile_t_x_p<NP>(dv, Dtr, p, lane);                       // dV^T[d][key] += dO^T P
    }
    __syncthreads();
    if (valid) store_rows(dv, (float*)bsm + wid * 32 * OLD, dQKV + ((long)b * N + k0) * ld3 + 2 * D + h * DH, ld3, l31, lh);
}

// ------------------------------------------------------------------------------------------------- dK
template <int NW, int NP>
__global__ __launch_bounds__(64 * NW, NP == 1 ? 2 : 1) void attn_bwd_dk_bf16_kernel(const float* __restrict__ QKV, const float* __restrict__ dO,
                                                                      const float* __restrict__ LSE, const float* __restrict__ DELTA,
                                                                      float* __restrict__ dQKV, int N, int heads, int kgroups,
                                                                      float scale) {
    using namespace attnbf;
    extern __shared__ __attribute__((aligned(16))) __bf16 bsm[];
    __bf16* Qrow = bsm;
    __bf16* Qtr = Qrow + rimg_pair<NP>();
    __bf16* Drow = Qtr + timg_pair<NP>();
    float* Ls = (float*)(Drow + rimg_pair<NP>());     // [32] lse (log2 units), [32] delta
    __bf16* Vw = (__bf16*)(Ls + 64);                  // per wave: row image (hi [+ lo]) of the V rows of its 32 keys
    const int bh = blockIdx.x / kgroups, kg = blockIdx.x - bh * kgroups;
    const int b = bh / heads, h = bh - b * heads;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int D = heads * DH;
    const long ld3 = 3L * D;
    const float* qkv = QKV + (long)b * N * ld3 + h * DH;
    const int kb = kg * NW + wid;
    const bool valid = kb * 32 < N;
    const int k0 = min(kb * 32, N - 32);
    Frags<NP> kf;
    load_row_frags<NP>(kf, qkv + (long)(k0 + l31) * ld3 + D, lh);
    __bf16* Vmine = Vw + wid * rimg_pair<NP>();
    stage<64, NP>(Vmine, nullptr, qkv + (long)k0 * ld3 + 2 * D, ld3, lane);     // this wave's V rows -> its private row image
    const float c2 = scale * 1.4426950408889634f;
    f32x16 dk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) dk[dt][r] = 0.f;
    for (int qt = 0; qt < N / KT; ++qt) {
        __syncthreads();
        stage<64 * NW, NP>(Qrow, Qtr, qkv + (long)(qt * KT) * ld3, ld3, tid);
        stage<64 * NW, NP>(Drow, nullptr, dO + ((long)b * N + qt * KT) * D + h * DH, D, tid);
        if (tid < 32) Ls[tid] = LSE[(long)bh * N + qt * KT + tid] * 1.4426950408889634f;
        else if (tid < 64) Ls[tid] = DELTA[(long)bh * N + qt * KT + tid - 32];
        __syncthreads();
        f32x16 s = tile_x_frags<NP>(Qrow, kf, l31, lh);              // S[q][key]
        const f32x16 dp = tile_x_tile<NP>(Drow, Vmine, l31, lh);     // dP[q][key] = dO_tile V^T
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int q = (r & 3) + 8 * (r >> 2) + 4 * lh;
            s[r] = exp2f(fmaf(s[r], c2, -Ls[q])) * (dp[r] - Ls[32 + q]) * scale;     // dS[q][key]
        }
        acc_tile_t_x_p<NP>(dk, Qtr, s, lane);                        // dK^T[d][key] += Q^T dS
    }
    __syncthreads();
    // every image is dead after the barrier: the fp32 output patches lie over them from the base (plain bf16: 70 KB of images,
    // 68 KB of patches -- two workgroups per CU instead of one)
    if (valid) store_rows(dk, (float*)bsm + wid * 32 * OLD, dQKV + ((long)b * N + k0) * ld3 + D + h * DH, ld3, l31, lh);
}

template <int NP>
static hipError_t attention_bwd_bf16_launch(const float* QKV, const float* O, const float* dO, const float* LSE, float* DELTA,
                                            float* dQKV, int B, int N, int heads, hipStream_t stream) {
    using namespace attnbf;
    if (B <= 0) return hipSuccess;
    if (N % 32 != 0) return hipErrorInvalidValue;
    const float scale = 1.0f / sqrtf((float)DH);
    constexpr int NW = 4;
    const int groups = (N / 32 + NW - 1) / NW;
    constexpr size_t patch = (size_t)NW * 32 * OLD * 4;
    constexpr size_t img_q = (size_t)(2 * rimg_pair<NP>() + timg_pair<NP>()) * 2;
    constexpr size_t img_v = (size_t)(rimg_pair<NP>() + timg_pair<NP>()) * 2 + 128;
    constexpr size_t lds_q = img_q > patch ? img_q : patch, lds_v = img_v > patch ? img_v : patch;
    constexpr size_t img_k = (size_t)(2 * rimg_pair<NP>() + timg_pair<NP>()) * 2 + 256 + (size_t)NW * rimg_pair<NP>() * 2;
    constexpr size_t lds_k = img_k > patch ? img_k : patch;
    static_assert(lds_k <= 160 * 1024, "LDS budget");
    if (hipError_t e = ego_allow_dynamic_lds((const void*)attn_bwd_dq_bf16_kernel<NW, NP>, (int)lds_q); e != hipSuccess) return e;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)attn_bwd_dv_bf16_kernel<NW, NP>, (int)lds_v); e != hipSuccess) return e;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)attn_bwd_dk_bf16_kernel<NW, NP>, (int)lds_k); e != hipSuccess) return e;
    hipLaunchKernelGGL((attn_bwd_dq_bf16_kernel<NW, NP>), dim3(B * heads * groups), dim3(64 * NW), lds_q, stream, QKV, O, dO, LSE, dQKV,
                       DELTA, N, heads, groups, scale);
    hipLaunchKernelGGL((attn_bwd_dv_bf16_kernel<NW, NP>), dim3(B * heads * groups), dim3(64 * NW), lds_v, stream, QKV, dO, LSE, dQKV, N,
                       heads, groups, scale);
    hipLaunchKernelGGL((attn_bwd_dk_bf16_kernel<NW, NP>), dim3(B * heads * groups), dim3(64 * NW), lds_k, stream, QKV, dO, LSE, DELTA, dQKV,
                       N, heads, groups, scale);
    return hipGetLastError();
}
