// Sensor frames -> the camera bytes the estimators read: per eye a source rectangle of a frame (FrameSource, frame_source.h: packed RGB8, NV12 or
// YUYV), optionally mirrored, resampled bilinearly (align_corners = false) to uint8 [n, S0, S0, 3].  What a caller does on the host as crop, flip,
// F.interpolate and a second resize (reprocess_egocap_data.py:72-88, :100-104; dataloader/data_loader.py:70-74): here one pass in integers, specified
// in egotap_amd/spec.py (resize_taps, resize_u8; for the YUV fetches resize_u8(yuv_to_rgb_u8(frames)) = yuv_resize_u8).
//   taps along an axis of source length L, output index X:  n = max((2X + 1) L - S0, 0), i0 = n / 2S0, r = n % 2S0, w1 = (r * 2048 + S0) / 2S0,
//     w0 = 2048 - w1, i1 = min(i0 + 1, L - 1);  the four taps are fetched and blended by frame_pixel_rgb and blend_rgb
//   mirror: output column X takes the taps of column S0 - 1 - X.
// HBM-bound (at 1024^2 -> 256^2: two of every four source rows are touched, 12 output bytes per thread):
//   * the x-tap table of the eye's S0 columns (pixel index of tap 0, distance to tap 1, w1 -- pixel indices for every fetch: the RGB8 fetch multiplies
//     by 3, luma and chroma sit at different offsets of one index) sits in LDS, computed once per workgroup with the mirror folded in; workgroups
//     stride over the groups so that it is built a few times per CU; a thread reads its four entries as two 16-byte LDS loads.
//   * one thread = four output pixels of a row (store_rgb4); a wave reads two source rows front to back.
//   * pixel indices come only from inside the rectangle: no load touches a byte outside n * frame_stride, the last partial dword of an RGB8 buffer
//     included (the caller has checked the layout: frame_layout_refusal).  RGB8 frames may sit at any address.
//   * both eyes in one launch (blockIdx.y); the layout and the colour by value.  No LDS beyond the table.
#pragma once
#include "frame_source.h"

struct ResizeEye { int x0, y0, w, h, mirror; };      // source rectangle in pixels (inside the H x W frame, w, h >= 1) and the mirror flag

// the taps of output index X along an axis of source length L (spec.resize_taps)
static __device__ __forceinline__ void resize_tap(int X, int L, int S0, int& i0, int& i1, int& w1) {
    int n = (2 * X + 1) * L - S0;
    n = n < 0 ? 0 : n;
    i0 = n / (2 * S0);
    const int r = n - i0 * (2 * S0);
    w1 = (r * 2048 + S0) / (2 * S0);
    i1 = i0 + 1 < L ? i0 + 1 : L - 1;
}

template <int FETCH>
static __global__ __launch_bounds__(256) void frame_resize_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                                 unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8,
                                                                 ResizeEye eye_l, ResizeEye eye_r, long groups, int pitch, long uv_offset, long frame_stride,
                                                                 YuvCoef coef, int S0) {
    extern __shared__ __attribute__((aligned(16))) int xtab[];          // [S0][2]: {x0 + ix0, (ix1 - ix0) << 16 | w1}
    const ResizeEye eye = blockIdx.y ? eye_r : eye_l;
    for (int X = threadIdx.x; X < S0; X += 256) {
        int i0, i1, w1;
        resize_tap(eye.mirror ? S0 - 1 - X : X, eye.w, S0, i0, i1, w1);
        xtab[2 * X] = eye.x0 + i0;
        xtab[2 * X + 1] = ((i1 - i0) << 16) | w1;
    }
    __syncthreads();
    const unsigned char* src = blockIdx.y ? right8 : left8;
    unsigned char* dst = blockIdx.y ? out_right8 : out_left8;
    const int gpr = S0 / 4;                                   // groups per output row
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
        const long row = i / gpr;                             // b * S0 + y
        const int xg = (int)(i - row * gpr) * 4;
        const long b = row / S0;
        const int y = (int)(row - b * S0);
        int iy0, iy1, wy1;
        resize_tap(y, eye.h, S0, iy0, iy1, wy1);
        const unsigned char* frame = src + b * frame_stride;
        const int ya = eye.y0 + iy0, yb = eye.y0 + iy1;
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        const i32x4v ta = *(const i32x4v*)(xtab + 2 * xg), tb = *(const i32x4v*)(xtab + 2 * xg + 4);
        const int t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
        unsigned px[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xa = t[2 * e], xb = xa + (t[2 * e + 1] >> 16);
            const unsigned p00 = frame_pixel_rgb<FETCH>(frame, ya, xa, pitch, uv_offset, coef), p01 = frame_pixel_rgb<FETCH>(frame, ya, xb, pitch, uv_offset, coef);
            const unsigned p10 = frame_pixel_rgb<FETCH>(frame, yb, xa, pitch, uv_offset, coef), p11 = frame_pixel_rgb<FETCH>(frame, yb, xb, pitch, uv_offset, coef);
            px[e] = blend_rgb(p00, p01, p10, p11, (unsigned)(t[2 * e + 1] & 0xffff), (unsigned)wy1);
        }
        store_rgb4(dst, i, px);
    }
}

// the one wording of what a rectangle must be, for every entry that takes one
static inline const char* resize_rect_refusal(const int* r, int H, int W) {
    if (r[2] < 1 || r[3] < 1) return "an empty source rectangle (w and h must be at least 1)";
    if (r[0] < 0 || r[1] < 0 || (long)r[0] + r[2] > W || (long)r[1] + r[3] > H) return "a source rectangle outside the frame (0 <= x0, x0 + w <= W, 0 <= y0, y0 + h <= H)";
    return nullptr;
}
static inline const char* resize_rects_refusal(const FrameSource& q, const int* rect_left, const int* rect_right) {
    if (const char* why = resize_rect_refusal(rect_left, q.H, q.W)) return why;
    return resize_rect_refusal(rect_right, q.H, q.W);
}

// n frames per eye; pointers, layout and rectangles checked by the caller (outputs 4-byte aligned, the frame bases aligned to frame_base_alignment)
static inline hipError_t frame_resize_launch(const unsigned char* left8, const unsigned char* right8, long n, const FrameSource& q, const int* rect_left,
                                             const int* rect_right, int mirror_left, int mirror_right, int S0, unsigned char* out_left8,
                                             unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (!frame_launch_ok(n, S0, q) || resize_rects_refusal(q, rect_left, rect_right)) return hipErrorInvalidValue;
    const ResizeEye el{rect_left[0], rect_left[1], rect_left[2], rect_left[3], mirror_left ? 1 : 0};
    const ResizeEye er{rect_right[0], rect_right[1], rect_right[2], rect_right[3], mirror_right ? 1 : 0};
    const long groups = n * S0 * (S0 / 4);
    return frame_fetch_dispatch(q.fetch, [&](auto fetch) {
        hipLaunchKernelGGL(frame_resize_kernel<decltype(fetch)::value>, dim3(frame_grid(groups, num_cu), 2), dim3(256), (size_t)S0 * 8, s, left8, right8, out_left8,
                           out_right8, el, er, groups, q.pitch, q.uv_offset, q.frame_stride, q.coef, S0);
    });
}
