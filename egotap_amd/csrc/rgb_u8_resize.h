// [r8] Sensor frames -> the camera bytes the estimators read: per eye a source rectangle of a uint8 [n, H, W, 3] frame, optionally mirrored, resampled
// bilinearly (align_corners = false) to uint8 [n, S0, S0, 3].  What a caller does today on the host as crop, flip, F.interpolate and a second resize
// (reprocess_egocap_data.py:72-88, :100-104; dataloader/data_loader.py:70-74): here one pass in integers, specified in egotap_amd/spec.py
// (resize_taps, resize_u8) and restated below token for token -- host and device agree bit for bit.
//   taps along an axis of source length L, output index X:  n = max((2X + 1) L - S0, 0), i0 = n / 2S0, r = n % 2S0, w1 = (r * 2048 + S0) / 2S0,
//     w0 = 2048 - w1, i1 = min(i0 + 1, L - 1);  byte = (sum wy_a wx_b p[y0 + iy_a][x0 + ix_b][c] + 2^21) >> 22  (<= 2048^2 * 255 + 2^21 < 2^31)
//   mirror: output column X takes the taps of column S0 - 1 - X.
// HBM-bound (at 1024^2 -> 256^2: two of every four source rows are touched, 12 output bytes per thread):
//   * the x-tap table of the eye's S0 columns (byte offset of tap 0 in a row, distance to tap 1, w1) sits in LDS, computed once per workgroup;
//     workgroups stride over the groups so that it is built a few times per CU; a thread reads its four entries as two 16-byte LDS loads.
//   * one thread = four output pixels of a row = three aligned dword stores (S0 a multiple of 4, the output base 4-byte aligned); consecutive
//     lanes take consecutive groups, so a wave writes 768 contiguous bytes and reads two source rows front to back.
//   * W need not be a multiple of 4, so a source row starts at any byte: every source byte is loaded as a byte, at an offset inside the
//     rectangle -- no load touches a byte outside n*H*W*3, the last partial dword of the buffer included.  The frames may sit at any address.
//   * both eyes in one launch (blockIdx.y).  Plain loads and vector stores, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ResizeEye { int x0, y0, w, h, mirror; };      // source rectangle in pixels (inside the H x W frame, w, h >= 1) and the mirror flag

static constexpr int kResizeMaxSide = 4096;          // S0 <= 4096: the table is 8 S0 bytes of LDS (32 KB at most)
static constexpr int kResizeMaxSrc = 16384;          // H, W <= 16384: (2 S0 - 1) L and 3 W stay far inside int32

// the taps of output index X along an axis of source length L (spec.resize_taps)
static __device__ __forceinline__ void resize_tap(int X, int L, int S0, int& i0, int& i1, int& w1) {
    int n = (2 * X + 1) * L - S0;
    n = n < 0 ? 0 : n;
    i0 = n / (2 * S0);
    const int r = n - i0 * (2 * S0);
    w1 = (r * 2048 + S0) / (2 * S0);
    i1 = i0 + 1 < L ? i0 + 1 : L - 1;
}

static __global__ __launch_bounds__(256) void rgb_u8_resize_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                                  unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8,
                                                                  ResizeEye eye_l, ResizeEye eye_r, long groups, int H, int W, int S0) {
    extern __shared__ __attribute__((aligned(16))) int xtab[];          // [S0][2]: {3 (x0 + ix0), (3 (ix1 - ix0)) << 16 | w1}
    const ResizeEye eye = blockIdx.y ? eye_r : eye_l;
    for (int X = threadIdx.x; X < S0; X += 256) {
        int i0, i1, w1;
        resize_tap(eye.mirror ? S0 - 1 - X : X, eye.w, S0, i0, i1, w1);
        xtab[2 * X] = 3 * (eye.x0 + i0);
        xtab[2 * X + 1] = ((3 * (i1 - i0)) << 16) | w1;
    }
    __syncthreads();
    const unsigned char* src = blockIdx.y ? right8 : left8;
    unsigned char* dst = blockIdx.y ? out_right8 : out_left8;
    const int gpr = S0 / 4;                                   // groups per output row
    const long row_bytes = 3L * W;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
        const long row = i / gpr;                             // b * S0 + y
        const int xg = (int)(i - row * gpr) * 4;
        const long b = row / S0;
        const int y = (int)(row - b * S0);
        int iy0, iy1, wy1;
        resize_tap(y, eye.h, S0, iy0, iy1, wy1);
        const unsigned wy0 = 2048u - (unsigned)wy1;
        const unsigned char* r0 = src + (b * H + eye.y0 + iy0) * row_bytes;
        const unsigned char* r1 = src + (b * H + eye.y0 + iy1) * row_bytes;
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        const i32x4v ta = *(const i32x4v*)(xtab + 2 * xg), tb = *(const i32x4v*)(xtab + 2 * xg + 4);
        const int t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int off0 = t[2 * e], off1 = off0 + (t[2 * e + 1] >> 16);
            const unsigned wx1 = (unsigned)(t[2 * e + 1] & 0xffff), wx0 = 2048u - wx1;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned top = wx0 * r0[off0 + c] + wx1 * r0[off1 + c];
                const unsigned bot = wx0 * r1[off0 + c] + wx1 * r1[off1 + c];
                const unsigned v = (wy0 * top + (unsigned)wy1 * bot + (1u << 21)) >> 22;
                const int bi = 3 * e + c;
                o[bi >> 2] |= v << (8 * (bi & 3));
            }
        }
        unsigned* op = (unsigned*)(dst + i * 12);
        op[0] = o[0];
        op[1] = o[1];
        op[2] = o[2];
    }
}

// the one wording of what a rectangle must be, for every entry that takes one
static inline const char* rgb_u8_resize_rect_refusal(const int* r, int H, int W) {
    if (r[2] < 1 || r[3] < 1) return "an empty source rectangle (w and h must be at least 1)";
    if (r[0] < 0 || r[1] < 0 || (long)r[0] + r[2] > W || (long)r[1] + r[3] > H) return "a source rectangle outside the frame (0 <= x0, x0 + w <= W, 0 <= y0, y0 + h <= H)";
    return nullptr;
}

// n frames per eye; pointers and rectangles checked by the caller (outputs 4-byte aligned, rectangles inside the frame)
static inline hipError_t rgb_u8_resize_launch(const unsigned char* left8, const unsigned char* right8, long n, int H, int W, const int* rect_left,
                                              const int* rect_right, int mirror_left, int mirror_right, int S0, unsigned char* out_left8,
                                              unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (n <= 0 || S0 <= 0 || S0 % 4 != 0 || S0 > kResizeMaxSide || H < 1 || W < 1 || H > kResizeMaxSrc || W > kResizeMaxSrc) return hipErrorInvalidValue;
    if (rgb_u8_resize_rect_refusal(rect_left, H, W) || rgb_u8_resize_rect_refusal(rect_right, H, W)) return hipErrorInvalidValue;
    const ResizeEye el{rect_left[0], rect_left[1], rect_left[2], rect_left[3], mirror_left ? 1 : 0};
    const ResizeEye er{rect_right[0], rect_right[1], rect_right[2], rect_right[3], mirror_right ? 1 : 0};
    const long groups = n * S0 * (S0 / 4);
    long grid = (groups + 255) / 256;
    if (grid > 8L * num_cu) grid = 8L * num_cu;
    hipLaunchKernelGGL(rgb_u8_resize_kernel, dim3((unsigned)grid, 2), dim3(256), (size_t)S0 * 8, s, left8, right8, out_left8, out_right8, el, er, groups, H, W, S0);
    return hipGetLastError();
}
