// Sensor frames as cameras deliver them -> the camera bytes the estimators read: per eye a source rectangle of an NV12 (4:2:0, a Y plane followed by an
// interleaved UV plane) or YUYV (packed 4:2:2) frame, optionally mirrored, converted to RGB bytes and resampled bilinearly (align_corners = false) to
// uint8 [n, S0, S0, 3].  The sibling of rgb_u8_resize_kernel (rgb_u8_resize.h): the same taps (resize_tap), the same bilinear formula, on the bytes
//   R = clip((CY (Y - y_off) + RV (V - 128) + 2^13) >> 14, 0, 255)
//   G = clip((CY (Y - y_off) - GU (U - 128) - GV (V - 128) + 2^13) >> 14, 0, 255)
//   B = clip((CY (Y - y_off) + BU (U - 128) + 2^13) >> 14, 0, 255)          (arithmetic shift, one rounding, every intermediate below 2^24)
// of each of the four taps: by definition spec.resize_u8(spec.yuv_to_rgb_u8(frames)), restated here token for token -- host and device agree bit for
// bit, nothing is interpolated in YUV.  Chroma is replicated: a pixel takes the U, V of its 2 x 2 block (NV12) or of its pair (YUYV).
//   NV12: Y(y, x) at y * pitch + x; the chroma pair at uv_offset + (y >> 1) * pitch + 2 * (x >> 1), U then V, read as ONE aligned 16-bit load
//   YUYV: the pixel pair x >> 1 of row y is Y0 U Y1 V at y * pitch + 4 * (x >> 1), read as ONE aligned dword
// HBM-bound, the shape of the sibling:
//   * the x-tap table of the eye's S0 columns (pixel index of tap 0, distance to tap 1, w1 -- pixel indices, not byte offsets: luma and chroma sit at
//     different offsets of one index) sits in LDS, computed once per workgroup with the mirror folded in; workgroups stride over the groups
//   * one thread = four output pixels of a row = three aligned dword stores; consecutive lanes take consecutive groups
//   * pixel indices come only from inside the rectangle; W (and for NV12 H) is even, so a pixel's block lies inside the frame: no load touches a byte
//     outside n * frame_stride or a byte of a row past pitch (the caller has checked the layout: yuv_layout_refusal)
//   * both eyes in one launch (blockIdx.y); the five coefficients and y_off by value.  Plain loads and vector stores, no atomics, no scratch, no LDS
//     beyond the table.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "rgb_u8_resize.h"

enum { YUV_NV12 = 0, YUV_YUYV = 1 };                 // egotap.h EGOTAP_YUV_NV12 / _YUYV
enum { YUV_BT601 = 0, YUV_BT709 = 1 };               // egotap.h EGOTAP_YUV_BT601 / _BT709
enum { YUV_LIMITED = 0, YUV_FULL = 1 };              // egotap.h EGOTAP_YUV_LIMITED / _FULL

struct YuvCoef { int cy, rv, gu, gv, bu, y_off; };   // round(real * 2^14) each, and the luma offset
// one frame's layout in bytes (spec.YuvLayout), and the colour as the kernel takes it
struct YuvSource {
    int format, H, W, pitch;
    long uv_offset, frame_stride;
    YuvCoef coef;
};

// (spec.YuvColour.coefficients) with Kg = 1 - Kr - Kb, limited: cy = 255/219, cc = 255/224, y_off = 16; full: cy = cc = 1, y_off = 0
static inline YuvCoef yuv_coefficients(int matrix, int range) {
    const double kr = matrix == YUV_BT709 ? 0.2126 : 0.299, kb = matrix == YUV_BT709 ? 0.0722 : 0.114, kg = 1.0 - kr - kb;
    const bool limited = range == YUV_LIMITED;
    const double cy = limited ? 255.0 / 219.0 : 1.0, cc = limited ? 255.0 / 224.0 : 1.0;
    const double real[5] = {cy, 2.0 * (1.0 - kr) * cc, 2.0 * kb * (1.0 - kb) / kg * cc, 2.0 * kr * (1.0 - kr) / kg * cc, 2.0 * (1.0 - kb) * cc};
    int q[5];
    for (int k = 0; k < 5; ++k) q[k] = (int)floor(real[k] * 16384.0 + 0.5);
    return YuvCoef{q[0], q[1], q[2], q[3], q[4], limited ? 16 : 0};
}

// the one wording of what a layout must be (spec.YuvLayout), for every entry that takes one
static inline const char* yuv_layout_refusal(int format, int H, int W, int pitch, long uv_offset, long frame_stride) {
    if (format != YUV_NV12 && format != YUV_YUYV) return "unknown format (EGOTAP_YUV_NV12 or EGOTAP_YUV_YUYV)";
    if (H < 1 || W < 1 || H > kResizeMaxSrc || W > kResizeMaxSrc) return "the frame height and width must be between 1 and 16384";
    if (format == YUV_NV12) {
        if (H % 2 || W % 2) return "NV12 needs an even H and W (4:2:0 chroma covers 2 x 2 blocks)";
        if (pitch < W) return "pitch is too small (NV12: pitch >= W)";
        if (uv_offset < (long)pitch * (H - 1) + W) return "the planes overlap (NV12: uv_offset >= pitch * (H - 1) + W)";
        if (uv_offset + (long)(H / 2 - 1) * pitch + W > frame_stride) return "the last chroma byte is past frame_stride";
        if (pitch % 2 || uv_offset % 2 || frame_stride % 2) return "NV12 needs an even pitch, uv_offset and frame_stride (the chroma pair is one aligned 16-bit load)";
    } else {
        if (W % 2) return "YUYV needs an even W (4:2:2 chroma covers pixel pairs)";
        if (pitch < 2L * W) return "pitch is too small (YUYV: pitch >= 2 W)";
        if ((long)(H - 1) * pitch + 2L * W > frame_stride) return "the last byte is past frame_stride";
        if (pitch % 4 || frame_stride % 4) return "YUYV needs pitch and frame_stride to be multiples of 4 (the pixel pair is one aligned dword)";
    }
    return nullptr;
}
static inline int yuv_base_alignment(int format) { return format == YUV_NV12 ? 2 : 4; }

// the RGB bytes of pixel (y, x) of a frame, packed R | G << 8 | B << 16
template <int FORMAT>
static __device__ __forceinline__ unsigned yuv_pixel_rgb(const unsigned char* __restrict__ frame, int y, int x, int pitch, long uv_offset, const YuvCoef& k) {
    int Y, U, V;
    if (FORMAT == YUV_NV12) {
        Y = frame[(long)y * pitch + x];
        const unsigned uv = *(const unsigned short*)(frame + uv_offset + (long)(y >> 1) * pitch + 2 * (x >> 1));
        U = (int)(uv & 0xffu);
        V = (int)(uv >> 8);
    } else {
        const unsigned d = *(const unsigned*)(frame + (long)y * pitch + 4 * (x >> 1));
        Y = (int)((x & 1 ? d >> 16 : d) & 0xffu);
        U = (int)((d >> 8) & 0xffu);
        V = (int)(d >> 24);
    }
    const int c = k.cy * (Y - k.y_off) + (1 << 13), u = U - 128, v = V - 128;
    int r = (c + k.rv * v) >> 14, g = (c - k.gu * u - k.gv * v) >> 14, b = (c + k.bu * u) >> 14;
    r = r < 0 ? 0 : r > 255 ? 255 : r;
    g = g < 0 ? 0 : g > 255 ? 255 : g;
    b = b < 0 ? 0 : b > 255 ? 255 : b;
    return (unsigned)r | (unsigned)g << 8 | (unsigned)b << 16;
}

template <int FORMAT>
static __global__ __launch_bounds__(256) void yuv_u8_resize_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
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
        const unsigned wy0 = 2048u - (unsigned)wy1;
        const unsigned char* frame = src + b * frame_stride;
        const int ya = eye.y0 + iy0, yb = eye.y0 + iy1;
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        const i32x4v ta = *(const i32x4v*)(xtab + 2 * xg), tb = *(const i32x4v*)(xtab + 2 * xg + 4);
        const int t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int xa = t[2 * e], xb = xa + (t[2 * e + 1] >> 16);
            const unsigned wx1 = (unsigned)(t[2 * e + 1] & 0xffff), wx0 = 2048u - wx1;
            const unsigned p00 = yuv_pixel_rgb<FORMAT>(frame, ya, xa, pitch, uv_offset, coef), p01 = yuv_pixel_rgb<FORMAT>(frame, ya, xb, pitch, uv_offset, coef);
            const unsigned p10 = yuv_pixel_rgb<FORMAT>(frame, yb, xa, pitch, uv_offset, coef), p11 = yuv_pixel_rgb<FORMAT>(frame, yb, xb, pitch, uv_offset, coef);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const unsigned top = wx0 * ((p00 >> (8 * c)) & 0xffu) + wx1 * ((p01 >> (8 * c)) & 0xffu);
                const unsigned bot = wx0 * ((p10 >> (8 * c)) & 0xffu) + wx1 * ((p11 >> (8 * c)) & 0xffu);
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

// n frames per eye; pointers, layout and rectangles checked by the caller (outputs 4-byte aligned, the frame bases aligned to yuv_base_alignment)
static inline hipError_t yuv_u8_resize_launch(const unsigned char* left8, const unsigned char* right8, long n, const YuvSource& q, const int* rect_left,
                                              const int* rect_right, int mirror_left, int mirror_right, int S0, unsigned char* out_left8,
                                              unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (n <= 0 || S0 <= 0 || S0 % 4 != 0 || S0 > kResizeMaxSide) return hipErrorInvalidValue;
    if (yuv_layout_refusal(q.format, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride)) return hipErrorInvalidValue;
    if (rgb_u8_resize_rect_refusal(rect_left, q.H, q.W) || rgb_u8_resize_rect_refusal(rect_right, q.H, q.W)) return hipErrorInvalidValue;
    const ResizeEye el{rect_left[0], rect_left[1], rect_left[2], rect_left[3], mirror_left ? 1 : 0};
    const ResizeEye er{rect_right[0], rect_right[1], rect_right[2], rect_right[3], mirror_right ? 1 : 0};
    const long groups = n * S0 * (S0 / 4);
    long grid = (groups + 255) / 256;
    if (grid > 8L * num_cu) grid = 8L * num_cu;
    if (q.format == YUV_NV12)
        hipLaunchKernelGGL(yuv_u8_resize_kernel<YUV_NV12>, dim3((unsigned)grid, 2), dim3(256), (size_t)S0 * 8, s, left8, right8, out_left8, out_right8, el, er,
                           groups, q.pitch, q.uv_offset, q.frame_stride, q.coef, S0);
    else
        hipLaunchKernelGGL(yuv_u8_resize_kernel<YUV_YUYV>, dim3((unsigned)grid, 2), dim3(256), (size_t)S0 * 8, s, left8, right8, out_left8, out_right8, el, er,
                           groups, q.pitch, q.uv_offset, q.frame_stride, q.coef, S0);
    return hipGetLastError();
}
