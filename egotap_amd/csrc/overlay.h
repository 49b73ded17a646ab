// What the estimators saw and found, drawn onto the frames (egotap.h: egotap_heat_u8, egotap_overlay_u8).  Two kernels, both specified in integers or
// single float32 roundings in egotap_amd/spec.py (heat_u8, overlay_taps, overlay_u8) and restated token for token -- host and device agree bit for bit.
//   heat_u8_kernel<T>   the reference's picture of a heatmap stack (utils/util.py:160-175 tensor2im(is_heatmap=True)) per group of channels: uint8
//                       [B, G, S, S] from channels c0 .. c0 + n - 1 of [B, C, S, S] maps (fp32 or bf16, element (b, c, y, x) at b * image_stride +
//                       c * S*S + y * S + x).  Per pixel in fp32, nothing to contract: v = the group's channels added in ascending order,
//                       v = v > 0 ? (v < 1 ? v : 1) : 0 (a NaN gives 0), byte = (uint8)(int)(v * 255.0f).  One thread = one 16-byte vector of every
//                       channel of its group (heatmap_peaks.h's load) = 4 or 8 pixels = ONE 4- or 8-byte store; consecutive lanes take consecutive
//                       vectors.  S*S is a multiple of 256, so a vector lies inside one map.  HBM-bound: every element is read once.
//   overlay_u8_kernel   three layers blended onto packed RGB8 canvases [B, Hc, Wc, 3], both eyes in one launch (blockIdx.z), a frame per blockIdx.y, the
//                       frame's store groups strided over by blockIdx.x.  One thread = four pixels of a row: three aligned dword loads, the layers in
//                       registers, store_rgb4 (frame_source.h).  Every layer is c = (c (65536 - t) + colour t + 32768) >> 16 per channel with
//                       t = coverage (0 .. 256) * alpha; t = 0 returns c, so a pixel a layer does not reach keeps its bits whether the layer is
//                       evaluated there or culled.
//       heat    a byte of heat8 [B, E, S, S] blended over four taps (blend_rgb on one byte) from the eye's tap tables (spec.overlay_taps: entry
//               i0 | w1 << 16, -1 outside the map; four x entries are one 16-byte load); the device never sees the affine.  t = A * heat alpha.
//       bones   in ascending index, then
//       marks   in ascending index.  Sixteenths of a pixel, int64 products (all below 2^42): a mark is mx = rint(16 x), a pixel centre 16 X + 8,
//               d = isqrt(dx^2 + dy^2), coverage = clamp(r16 + 8 - d, 0, 16) * 16.  A bone: e = b - a, dd = e . e, s = (p - a) . e; dd == 0 or s <= 0:
//               the distance to a; s >= dd: to b; otherwise |cross(p - a, e)| div isqrt(dd); w16 in place of r16.  isqrt is the float64 square root
//               truncated plus one integer correction step each way; the floor division is the float64 quotient truncated plus the same correction.
//     Prepared ONCE per workgroup in LDS (4.4 KB) by its first wave: per mark the eligibility, the sixteenths and a box of canvas pixels outside of
//     which its coverage is provably 0; per bone the same with isqrt(dd); the union of all boxes.  A thread outside the union box pays one compare for
//     all marks and bones, one inside pays one box compare per mark and bone it is far from.  The style (palettes, bone table) travels by value.
// Plain loads and vector stores, no atomics, no scratch, no workspace.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "egotap.h"
#include "frame_source.h"
#include "heatmap_peaks.h"

static constexpr int kOverlayMaxSide = 16384;          // Hc, Wc: 16 X + 8 < 2^18
static constexpr int kOverlayMaxHeatSide = 4096;       // S: a tap index fits 16 bits, S*S an int
static constexpr int kOverlayMaxR16 = 16384;           // r16, w16: a box stays inside int32

template <typename T>
static __global__ __launch_bounds__(256) void heat_u8_kernel(const T* __restrict__ hm, long image_stride, int S, int c0, int per, int G, long vecs,
                                                            unsigned char* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int V = 16 / sizeof(T);
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= vecs) return;
    const int HW = S * S, vpm = HW / V;                      // vectors per map
    const long map = i / vpm;                                // b * G + g
    const int e = (int)(i - map * vpm) * V;
    const long b = map / G;
    const int g = (int)(map - b * G);
    const T* __restrict__ p = hm + b * image_stride + ((long)c0 + (long)g * per) * HW + e;
    float v[V];
    peaks_load16(p, v);
    for (int k = 1; k < per; ++k) {
        float x[V];
        peaks_load16(p + (long)k * HW, x);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = v[j] + x[j];
    }
    unsigned w[V / 4];
#pragma unroll
    for (int q = 0; q < V / 4; ++q) w[q] = 0u;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float c = v[j] > 0.f ? (v[j] < 1.f ? v[j] : 1.f) : 0.f;
        w[j / 4] |= (unsigned)(int)(c * 255.0f) << (8 * (j % 4));
    }
    unsigned char* o = out + map * HW + e;
    if (V == 4) {
        *(unsigned*)o = w[0];
    } else {
        typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
        u32x2v r;
        r[0] = w[0];
        r[1] = w[V / 4 - 1];
        *(u32x2v*)o = r;
    }
}

// hm 16-byte aligned, out 8-byte aligned, image_stride a multiple of 16 bytes, S a multiple of 16 up to kOverlayMaxHeatSide, groups dividing n: checked by the caller
template <typename T>
static inline hipError_t heat_u8_launch(const T* hm, long B, int S, long image_stride, int c0, int n, int groups, unsigned char* out, hipStream_t s) {
    if (B <= 0 || n <= 0 || groups <= 0 || n % groups || S < 16 || S > kOverlayMaxHeatSide || S % 16) return hipErrorInvalidValue;
    const long vecs = B * groups * ((long)S * S / (16 / (long)sizeof(T))), blocks = (vecs + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(heat_u8_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, hm, image_stride, S, c0, n / groups, groups, vecs, out);
    return hipGetLastError();
}

// floor(sqrt(n)), 0 <= n < 2^52 (spec.overlay_isqrt)
static __device__ __forceinline__ long overlay_isqrt(long n) {
    long r = (long)sqrt((double)n);
    r -= (r * r > n);
    r += ((r + 1) * (r + 1) <= n);
    return r;
}
// clamp(R - isqrt(dx^2 + dy^2), 0, 16) * 16 with R = the half-size in sixteenths + 8
static __device__ __forceinline__ int overlay_cover_point(int dx, int dy, int R) {
    const long n = (long)dx * dx + (long)dy * dy;
    if (n >= (long)R * R) return 0;                          // isqrt(n) >= R
    const int c = R - (int)overlay_isqrt(n);
    return (c > 16 ? 16 : c) * 16;
}
// the same against the segment a .. a + e, (dx, dy) = p - a, isq = isqrt(e . e)
static __device__ __forceinline__ int overlay_cover_bone(int dx, int dy, int ex, int ey, int isq, int R) {
    const long dd = (long)ex * ex + (long)ey * ey, s = (long)dx * ex + (long)dy * ey;
    if (dd == 0 || s <= 0) return overlay_cover_point(dx, dy, R);
    if (s >= dd) return overlay_cover_point(dx - ex, dy - ey, R);
    long cr = (long)dx * ey - (long)dy * ex;
    cr = cr < 0 ? -cr : cr;
    if (cr >= (long)R * isq) return 0;                       // cr div isq >= R
    long d = (long)((double)cr / (double)isq);
    d -= (d * isq > cr);
    d += ((d + 1) * isq <= cr);
    const int c = R - (int)d;
    return (c > 16 ? 16 : c) * 16;
}
// one layer on one pixel's three channels; rgba packed R | G << 8 | B << 16 | alpha << 24, t = coverage * alpha
static __device__ __forceinline__ void overlay_blend(unsigned (&c)[3], unsigned rgba, unsigned t) {
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (c[k] * (65536u - t) + ((rgba >> (8 * k)) & 0xffu) * t + 32768u) >> 16;
}
static __device__ __forceinline__ unsigned overlay_rgba(const uint8_t (&c)[4]) { return (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | (unsigned)c[3] << 24; }

struct OverlayBox { int x0, x1, y0, y1; };                   // canvas pixels, inclusive; x0 > x1: empty
struct OverlayEye {
    const unsigned char* in;
    unsigned char* out;                                      // may be `in` itself: a thread reads its twelve bytes, then writes them
    const int* tx;
    const int* ty;
};
// the pixels whose centre can lie within R sixteenths of the span lo .. hi (conservative by up to a pixel; an empty box for a thing not drawn)
static __device__ __forceinline__ OverlayBox overlay_box(bool drawn, int xlo, int xhi, int ylo, int yhi, int R) {
    if (!drawn) return OverlayBox{1, 0, 1, 0};
    return OverlayBox{(xlo - R - 8) >> 4, ((xhi + R - 8) >> 4) + 1, (ylo - R - 8) >> 4, ((yhi + R - 8) >> 4) + 1};
}
static __device__ __forceinline__ bool overlay_box_misses(const OverlayBox& b, int X0, int Y) { return Y < b.y0 || Y > b.y1 || X0 + 3 < b.x0 || X0 > b.x1; }

static __global__ __launch_bounds__(256) void overlay_u8_kernel(OverlayEye eye_l, OverlayEye eye_r, const unsigned char* __restrict__ heat8,
                                                               const float* __restrict__ marks, egotap_overlay_style st, int E, int Hc, int Wc, int S) {
#pragma clang fp contract(off)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    typedef int i32x4v __attribute__((ext_vector_type(4)));
    __shared__ OverlayBox s_mbox[EGOTAP_OVERLAY_MAX], s_bbox[EGOTAP_OVERLAY_MAX], s_union;
    __shared__ int s_mx[EGOTAP_OVERLAY_MAX], s_my[EGOTAP_OVERLAY_MAX], s_ok[EGOTAP_OVERLAY_MAX];
    __shared__ int s_ba[EGOTAP_OVERLAY_MAX][2], s_be[EGOTAP_OVERLAY_MAX][2], s_bisq[EGOTAP_OVERLAY_MAX];
    __shared__ unsigned s_mrgba[EGOTAP_OVERLAY_MAX], s_brgba[EGOTAP_OVERLAY_MAX];
    const int e = blockIdx.z, tid = threadIdx.x;
    const long b = blockIdx.y;
    const OverlayEye eye = e ? eye_r : eye_l;
    const int M = marks ? st.n_marks : 0, L = marks ? st.n_bones : 0;
    const int Rm = st.r16 + 8, Rb = st.w16 + 8;
    // ---- the frame's marks and bones, once per workgroup, by the first wave
    if (tid < EGOTAP_OVERLAY_MAX) {
        int ok = 0, mx = 0, my = 0;
        unsigned rgba = 0u;
        if (tid < M) {
            const f32x4v rec = *(const f32x4v*)(marks + ((b * E + e) * M + tid) * 4);
            ok = rec[2] >= st.min_score && fabsf(rec[0]) < 32768.f && fabsf(rec[1]) < 32768.f;      // (every comparison is false on a NaN)
            if (ok) {
                mx = (int)rintf(16.f * rec[0]);
                my = (int)rintf(16.f * rec[1]);
            }
            rgba = overlay_rgba(st.mark_rgba[tid]);
        }
        s_ok[tid] = ok;
        s_mx[tid] = mx;
        s_my[tid] = my;
        s_mrgba[tid] = rgba;
        s_mbox[tid] = overlay_box(ok && (rgba >> 24) != 0u, mx, mx, my, my, Rm);
    }
    __syncthreads();
    if (tid < EGOTAP_OVERLAY_MAX) {
        OverlayBox box = overlay_box(false, 0, 0, 0, 0, 0);
        if (tid < L) {
            const int i = st.bones[tid][0], j = st.bones[tid][1];      // (< M: checked by the caller)
            const unsigned rgba = overlay_rgba(st.bone_rgba[tid]);
            const int ax = s_mx[i], ay = s_my[i], bx = s_mx[j], by = s_my[j], ex = bx - ax, ey = by - ay;
            s_ba[tid][0] = ax;
            s_ba[tid][1] = ay;
            s_be[tid][0] = ex;
            s_be[tid][1] = ey;
            s_bisq[tid] = (int)overlay_isqrt((long)ex * ex + (long)ey * ey);
            s_brgba[tid] = rgba;
            box = overlay_box(s_ok[i] && s_ok[j] && (rgba >> 24) != 0u, ax < bx ? ax : bx, ax < bx ? bx : ax, ay < by ? ay : by, ay < by ? by : ay, Rb);
        }
        s_bbox[tid] = box;
        // the union of the 128 boxes over the wave's 64 lanes (an empty box is (1, 0, 1, 0): it must not widen the union)
        const OverlayBox mb = s_mbox[tid];
        const int big = 0x7fffffff;
        int x0 = big, x1 = -big, y0 = big, y1 = -big;
        if (mb.x0 <= mb.x1) { x0 = mb.x0; x1 = mb.x1; y0 = mb.y0; y1 = mb.y1; }
        if (box.x0 <= box.x1) {
            x0 = box.x0 < x0 ? box.x0 : x0;
            x1 = box.x1 > x1 ? box.x1 : x1;
            y0 = box.y0 < y0 ? box.y0 : y0;
            y1 = box.y1 > y1 ? box.y1 : y1;
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const int ox0 = __shfl_xor(x0, m), ox1 = __shfl_xor(x1, m), oy0 = __shfl_xor(y0, m), oy1 = __shfl_xor(y1, m);
            x0 = ox0 < x0 ? ox0 : x0;
            x1 = ox1 > x1 ? ox1 : x1;
            y0 = oy0 < y0 ? oy0 : y0;
            y1 = oy1 > y1 ? oy1 : y1;
        }
        if (tid == 0) s_union = OverlayBox{x0, x1, y0, y1};
    }
    __syncthreads();
    const OverlayBox un = s_union;
    const int gpr = Wc / 4;                                  // store groups per row
    const long groups = (long)Hc * gpr;                      // of this frame
    const unsigned char* src = eye.in + b * groups * 12;
    unsigned char* dst = eye.out + b * groups * 12;
    const unsigned char* heat = heat8 ? heat8 + (b * E + e) * ((long)S * S) : nullptr;
    const unsigned heat_rgba = overlay_rgba(st.heat_rgba), heat_alpha = heat_rgba >> 24;
    for (long i = (long)blockIdx.x * 256 + tid; i < groups; i += (long)gridDim.x * 256) {
        const int Y = (int)(i / gpr), X0 = (int)(i - (long)Y * gpr) * 4;
        const unsigned* ip = (const unsigned*)(src + i * 12);
        const unsigned w[3] = {ip[0], ip[1], ip[2]};
        unsigned c[4][3];
#pragma unroll
        for (int k = 0; k < 12; ++k) c[k / 3][k % 3] = (w[k / 4] >> (8 * (k % 4))) & 0xffu;
        if (heat) {
            const int ty = eye.ty[Y];
            const i32x4v tx = *(const i32x4v*)(eye.tx + X0);
            if (ty >= 0) {
                int iy0 = ty & 0xffff;
                iy0 = iy0 < S ? iy0 : S - 1;                 // (a table of spec.overlay_taps never needs it: no entry may lead a load outside the map)
                const int iy1 = iy0 + 1 < S ? iy0 + 1 : S - 1;
                const unsigned char* r0 = heat + (long)iy0 * S;
                const unsigned char* r1 = heat + (long)iy1 * S;
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    if (tx[p] < 0) continue;
                    int ix0 = tx[p] & 0xffff;
                    ix0 = ix0 < S ? ix0 : S - 1;
                    const int ix1 = ix0 + 1 < S ? ix0 + 1 : S - 1;
                    const unsigned A = blend_rgb(r0[ix0], r0[ix1], r1[ix0], r1[ix1], (unsigned)(tx[p] >> 16), (unsigned)(ty >> 16)) & 0xffu;
                    overlay_blend(c[p], heat_rgba, A * heat_alpha);
                }
            }
        }
        if (!overlay_box_misses(un, X0, Y)) {
            const int py = 16 * Y + 8, px0 = 16 * X0 + 8;
            for (int l = 0; l < L; ++l) {
                if (overlay_box_misses(s_bbox[l], X0, Y)) continue;
                const int ax = s_ba[l][0], ay = s_ba[l][1], ex = s_be[l][0], ey = s_be[l][1], isq = s_bisq[l];
                const unsigned rgba = s_brgba[l];
#pragma unroll
                for (int p = 0; p < 4; ++p)
                    overlay_blend(c[p], rgba, (unsigned)overlay_cover_bone(px0 + 16 * p - ax, py - ay, ex, ey, isq, Rb) * (rgba >> 24));
            }
            for (int j = 0; j < M; ++j) {
                if (overlay_box_misses(s_mbox[j], X0, Y)) continue;
                const int mx = s_mx[j], my = s_my[j];
                const unsigned rgba = s_mrgba[j];
#pragma unroll
                for (int p = 0; p < 4; ++p) overlay_blend(c[p], rgba, (unsigned)overlay_cover_point(px0 + 16 * p - mx, py - my, Rm) * (rgba >> 24));
            }
        }
        const unsigned px[4] = {c[0][0] | c[0][1] << 8 | c[0][2] << 16, c[1][0] | c[1][1] << 8 | c[1][2] << 16, c[2][0] | c[2][1] << 8 | c[2][2] << 16,
                                c[3][0] | c[3][1] << 8 | c[3][2] << 16};
        store_rgb4(dst, i, px);
    }
}

// workgroups of one frame of one eye: they stride over the frame's store groups, at most eight workgroups per compute unit over all frames and eyes
static inline unsigned overlay_grid_x(long groups, long frames, int num_cu) {
    long cap = 8L * num_cu / frames, grid = (groups + 255) / 256;
    cap = cap < 1 ? 1 : cap;
    return (unsigned)(grid > cap ? cap : grid);
}

// canvases [B, Hc, Wc, 3] with Wc % 4 == 0 and 4-byte aligned bases, eye_r all NULL for one eye; heat8 NULL: no heat layer (S and the tables are not read);
// marks NULL: no marks and no bones.  Sizes, alignments, the style's ranges and indices: checked by the caller.
static inline hipError_t overlay_u8_launch(const OverlayEye& eye_l, const OverlayEye& eye_r, int E, long B, int Hc, int Wc, const unsigned char* heat8, int S,
                                           const float* marks, const egotap_overlay_style& st, int num_cu, hipStream_t s) {
    if (B <= 0 || B > 65535 || E < 1 || E > 2 || Hc < 1 || Wc < 4 || Wc % 4 || Hc > kOverlayMaxSide || Wc > kOverlayMaxSide) return hipErrorInvalidValue;
    if (heat8 && (S < 1 || S > kOverlayMaxHeatSide)) return hipErrorInvalidValue;
    if (st.n_marks < 0 || st.n_marks > EGOTAP_OVERLAY_MAX || st.n_bones < 0 || st.n_bones > EGOTAP_OVERLAY_MAX) return hipErrorInvalidValue;
    const long groups = (long)Hc * (Wc / 4);
    hipLaunchKernelGGL(overlay_u8_kernel, dim3(overlay_grid_x(groups, B * E, num_cu), (unsigned)B, (unsigned)E), dim3(256), 0, s, eye_l, eye_r, heat8, marks, st, E,
                       Hc, Wc, S);
    return hipGetLastError();
}
