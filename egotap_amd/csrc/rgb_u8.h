// [r7] Camera bytes -> the normalised planar fp32 frames the estimators read: uint8 [B, S0, S0, 3] (RGB, contiguous) -> fp32 [B, 3, S0, S0] with
// out[b][c][y][x] = table[c][in[b][y][x][c]], table fp32 [3][256] (egotap_amd/spec.py rgb_u8_table: the reference's
// (float64(float32(v) / 255) - mean[c]) / std[c], rounded to fp32 last -- utils/util.py:188-197 normalize_ImageNet behind the loader's .float()).
// What a caller does today as astype(float32) / 255, normalise, HWC -> CHW: here one pass, 3 bytes in and 12 out per pixel (HBM-bound).
//   * one thread = four pixels of a row: three aligned dwords in (the base is 4-byte aligned, a row is 3 S0 bytes, S0 a multiple of 4), one
//     16-byte store per channel out; consecutive lanes take consecutive groups, so a wave reads 768 contiguous bytes and writes three 1 KB runs.
//   * the table sits in LDS (3 KB per workgroup); workgroups stride over the groups so that it is staged a few times per CU, not once per 1024 pixels.
//   * both eyes in one launch (blockIdx.y).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

static __global__ __launch_bounds__(256) void rgb_u8_to_f32_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                                  const float* __restrict__ table, float* __restrict__ left, float* __restrict__ right,
                                                                  long groups, int S0) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    __shared__ float tab[3 * 256];
    for (int i = threadIdx.x; i < 3 * 256; i += 256) tab[i] = table[i];
    __syncthreads();
    const unsigned char* src = blockIdx.y ? right8 : left8;
    float* dst = blockIdx.y ? right : left;
    const long plane = (long)S0 * S0;
    const int gpr = S0 / 4;                                   // groups per row
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
        const unsigned* rp = (const unsigned*)(src + i * 12);
        const unsigned raw[3] = {rp[0], rp[1], rp[2]};
        const long row = i / gpr;                             // b * S0 + y
        const int x = (int)(i - row * gpr) * 4;
        const long b = row / S0;
        const int y = (int)(row - b * S0);
        float* o = dst + (b * 3) * plane + (long)y * S0 + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            f32x4v v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int bi = 3 * e + c;
                v[e] = tab[c * 256 + ((raw[bi >> 2] >> (8 * (bi & 3))) & 255u)];
            }
            *(f32x4v*)(o + c * plane) = v;
        }
    }
}

// B frames per eye; pointers checked by the caller (left8 / right8 4-byte, left / right 16-byte aligned, S0 a multiple of 4)
static inline hipError_t rgb_u8_to_f32_launch(const unsigned char* left8, const unsigned char* right8, const float* table, float* left, float* right, long B, int S0,
                                              int num_cu, hipStream_t s) {
    if (B <= 0 || S0 <= 0 || S0 % 4 != 0) return hipErrorInvalidValue;
    const long groups = B * S0 * (S0 / 4);
    long grid = (groups + 255) / 256;
    if (grid > 8L * num_cu) grid = 8L * num_cu;
    hipLaunchKernelGGL(rgb_u8_to_f32_kernel, dim3((unsigned)grid, 2), dim3(256), 0, s, left8, right8, table, left, right, groups, S0);
    return hipGetLastError();
}
