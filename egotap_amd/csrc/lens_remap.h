// Frames from another lens -> the camera bytes the estimators read: per eye a LENS MAP (spec.lens_map: int32 [S0 * S0][2], for every pixel of the
// S0 x S0 frame the stems read the Q11 pixel coordinates (fx, fy) in the sensor's H x W frame it is sampled at, or (-1, -1) where the sensor does not
// see it), applied as a bilinear gather to uint8 [n, S0, S0, 3].  The map is built once per rig on the host in float64 from two OCamCalib models and a
// rotation (ocam.h holds the same model behind the network); the kernel sees integers only.  The sibling of rgb_u8_resize_kernel and
// yuv_u8_resize_kernel: the same bilinear formula on the same bytes, specified in egotap_amd/spec.py (lens_taps, lens_remap_u8) and restated here
// token for token -- host and device agree bit for bit.
//   taps of an entry: ix0 = fx >> 11, wx1 = fx & 2047, wx0 = 2048 - wx1, ix1 = min(ix0 + 1, W - 1); likewise iy0, wy1, wy0, iy1 from fy
//   byte = (wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) + 2^21) >> 22          (<= 2048^2 * 255 + 2^21 < 2^31: resize_u8's formula)
//   an invalid entry (either half negative) gives the eye's fill bytes and loads nothing
// FETCH says what a tap is: three bytes of a packed RGB8 frame, or the pixel of an NV12 / YUYV frame converted to RGB bytes by yuv_pixel_rgb
// (yuv_u8_resize.h, as it stands: one byte and one aligned 16-bit load, or one aligned dword) -- by definition lens_remap_u8(yuv_to_rgb_u8(frames)),
// nothing is interpolated in YUV.
// Bound by gather latency and HBM, not by arithmetic.  Bytes per output pixel: 8 map bytes (both eyes' maps are 2 * 8 * S0^2 = 1 MB at S0 = 256:
// read from HBM for the first frame of a batch, from L2 for every other), up to 12 source bytes (four taps x three bytes; neighbouring pixels share
// taps, and a lens map is smooth, so a wave's taps fall into a few runs of source rows and what HBM delivers is the touched rows, as for the resize),
// 3 output bytes.  Hence the shape:
//   * NO tap table in LDS: the taps differ for every pixel, so a thread reads its four entries straight from the map as two 16-byte loads (the
//     maps are 16-byte aligned, a group of four pixels never crosses a row: S0 is a multiple of 4).
//   * one thread = four output pixels of a row = three aligned dword stores (the output base 4-byte aligned); consecutive lanes take consecutive
//     groups, so a wave reads 2 KB of map and writes 768 bytes, both contiguous, and its 16 x 64 taps are neighbours in the source.
//   * the four taps of a pixel are independent loads issued before the first is used; a pixel is skipped as a whole where its entry is invalid (the
//     branch keeps the pixels of a thread apart, so latency is hidden by occupancy -- about 40 VGPRs, eight waves per SIMD -- and not by one thread's
//     queue depth); workgroups stride over the groups under the siblings' 8 * num_cu grid cap.
//   * every tap index comes from a valid entry and is clamped to the frame on BOTH sides (ix0 <= W - 1 as well: a no-op for a map built for this
//     H x W, which the library cannot inspect on the device) -- no load touches a byte outside n * frame bytes whatever the map holds; W (and for
//     NV12 H) is even, so a pixel's chroma block lies inside the frame.  RGB8 frames may sit at any address.
//   * both eyes in one launch (blockIdx.y), each with its own map and fill.  Plain loads and vector stores, no atomics, no scratch, no LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "yuv_u8_resize.h"

enum { LENS_RGB8 = 0, LENS_NV12 = 1, LENS_YUYV = 2 };            // egotap.h EGOTAP_LENS_RGB8 / _NV12 / _YUYV
static constexpr int kLensFracBits = 11;                         // spec.LENS_FRAC_BITS

// one frame's layout in bytes and what a tap is: RGB8 has pitch = 3 W and frame_stride = 3 H W; the YUV fetches take theirs from the YuvSource
struct LensSource {
    int fetch, H, W, pitch;
    long uv_offset, frame_stride;
    YuvCoef coef;
};
static inline LensSource lens_source_rgb8(int H, int W) { return LensSource{LENS_RGB8, H, W, 3 * W, 0L, 3L * H * W, YuvCoef{}}; }
static inline LensSource lens_source_yuv(const YuvSource& q) {
    return LensSource{q.format == YUV_NV12 ? LENS_NV12 : LENS_YUYV, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride, q.coef};
}
static inline unsigned lens_fill(const uint8_t* rgb) { return (unsigned)rgb[0] | (unsigned)rgb[1] << 8 | (unsigned)rgb[2] << 16; }

// the RGB bytes of pixel (y, x) of a frame, packed R | G << 8 | B << 16
template <int FETCH>
static __device__ __forceinline__ unsigned lens_pixel_rgb(const unsigned char* __restrict__ frame, int y, int x, int pitch, long uv_offset, const YuvCoef& k) {
    if (FETCH == LENS_RGB8) {
        const unsigned char* p = frame + (long)y * pitch + 3 * x;
        return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
    return yuv_pixel_rgb<FETCH == LENS_NV12 ? YUV_NV12 : YUV_YUYV>(frame, y, x, pitch, uv_offset, k);
}

template <int FETCH>
static __global__ __launch_bounds__(256) void lens_remap_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                               const int* __restrict__ map_left, const int* __restrict__ map_right,
                                                               unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8, long groups,
                                                               int H, int W, int pitch, long uv_offset, long frame_stride, YuvCoef coef, unsigned fill_l,
                                                               unsigned fill_r, int S0) {
    const unsigned char* src = blockIdx.y ? right8 : left8;
    const int* map = blockIdx.y ? map_right : map_left;
    unsigned char* dst = blockIdx.y ? out_right8 : out_left8;
    const unsigned fill = blockIdx.y ? fill_r : fill_l;
    const long gpf = (long)S0 * (S0 / 4);                     // groups per frame
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
        const long b = i / gpf, g = i - b * gpf;              // the group's four pixels are entries 4 g .. 4 g + 3 of the eye's map
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        const i32x4v ta = *(const i32x4v*)(map + 8 * g), tb = *(const i32x4v*)(map + 8 * g + 4);
        const int t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
        const unsigned char* frame = src + b * frame_stride;
        unsigned o[3] = {0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int fx = t[2 * e], fy = t[2 * e + 1];
            unsigned px = fill;
            if (fx >= 0 && fy >= 0) {
                int ix0 = fx >> kLensFracBits, iy0 = fy >> kLensFracBits;
                ix0 = ix0 < W - 1 ? ix0 : W - 1;
                iy0 = iy0 < H - 1 ? iy0 : H - 1;
                const int ix1 = ix0 + 1 < W ? ix0 + 1 : W - 1, iy1 = iy0 + 1 < H ? iy0 + 1 : H - 1;
                const unsigned wx1 = (unsigned)(fx & 2047), wx0 = 2048u - wx1, wy1 = (unsigned)(fy & 2047), wy0 = 2048u - wy1;
                const unsigned p00 = lens_pixel_rgb<FETCH>(frame, iy0, ix0, pitch, uv_offset, coef), p01 = lens_pixel_rgb<FETCH>(frame, iy0, ix1, pitch, uv_offset, coef);
                const unsigned p10 = lens_pixel_rgb<FETCH>(frame, iy1, ix0, pitch, uv_offset, coef), p11 = lens_pixel_rgb<FETCH>(frame, iy1, ix1, pitch, uv_offset, coef);
                px = 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned top = wx0 * ((p00 >> (8 * c)) & 0xffu) + wx1 * ((p01 >> (8 * c)) & 0xffu);
                    const unsigned bot = wx0 * ((p10 >> (8 * c)) & 0xffu) + wx1 * ((p11 >> (8 * c)) & 0xffu);
                    px |= ((wy0 * top + wy1 * bot + (1u << 21)) >> 22) << (8 * c);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int bi = 3 * e + c;
                o[bi >> 2] |= ((px >> (8 * c)) & 0xffu) << (8 * (bi & 3));
            }
        }
        unsigned* op = (unsigned*)(dst + i * 12);
        op[0] = o[0];
        op[1] = o[1];
        op[2] = o[2];
    }
}

// n frames per eye; pointers and the layout checked by the caller (maps 16-byte aligned, outputs 4-byte aligned, YUV frame bases aligned to
// yuv_base_alignment and the layout passed by yuv_layout_refusal)
static inline hipError_t lens_remap_launch(const unsigned char* left8, const unsigned char* right8, long n, const LensSource& q, const int* map_left,
                                           const int* map_right, unsigned fill_left, unsigned fill_right, int S0, unsigned char* out_left8,
                                           unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (n <= 0 || S0 <= 0 || S0 % 4 != 0 || S0 > kResizeMaxSide || q.H < 1 || q.W < 1 || q.H > kResizeMaxSrc || q.W > kResizeMaxSrc) return hipErrorInvalidValue;
    if (!left8 || !right8 || !map_left || !map_right || !out_left8 || !out_right8) return hipErrorInvalidValue;
    if ((((uintptr_t)map_left | (uintptr_t)map_right) & 15) != 0 || (((uintptr_t)out_left8 | (uintptr_t)out_right8) & 3) != 0) return hipErrorInvalidValue;
    if (q.fetch != LENS_RGB8 && yuv_layout_refusal(q.fetch == LENS_NV12 ? YUV_NV12 : YUV_YUYV, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride))
        return hipErrorInvalidValue;
    const long groups = n * S0 * (S0 / 4);
    long grid = (groups + 255) / 256;
    if (grid > 8L * num_cu) grid = 8L * num_cu;
    const dim3 g((unsigned)grid, 2), blk(256);
    if (q.fetch == LENS_RGB8)
        hipLaunchKernelGGL(lens_remap_kernel<LENS_RGB8>, g, blk, 0, s, left8, right8, map_left, map_right, out_left8, out_right8, groups, q.H, q.W, q.pitch,
                           q.uv_offset, q.frame_stride, q.coef, fill_left, fill_right, S0);
    else if (q.fetch == LENS_NV12)
        hipLaunchKernelGGL(lens_remap_kernel<LENS_NV12>, g, blk, 0, s, left8, right8, map_left, map_right, out_left8, out_right8, groups, q.H, q.W, q.pitch,
                           q.uv_offset, q.frame_stride, q.coef, fill_left, fill_right, S0);
    else if (q.fetch == LENS_YUYV)
        hipLaunchKernelGGL(lens_remap_kernel<LENS_YUYV>, g, blk, 0, s, left8, right8, map_left, map_right, out_left8, out_right8, groups, q.H, q.W, q.pitch,
                           q.uv_offset, q.frame_stride, q.coef, fill_left, fill_right, S0);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
