// Frames from another lens -> the camera bytes the estimators read: per eye a LENS MAP (spec.lens_map: int32 [S0 * S0][2], for every pixel of the
// S0 x S0 frame the stems read the Q11 pixel coordinates (fx, fy) in the sensor's H x W frame it is sampled at, or (-1, -1) where the sensor does not
// see it), applied as a bilinear gather to uint8 [n, S0, S0, 3].  The map is built once per rig on the host in float64 from two OCamCalib models and a
// rotation (ocam.h holds the same model behind the network); the kernel sees integers only, specified in egotap_amd/spec.py (lens_taps,
// lens_remap_u8; for the YUV fetches lens_remap_u8(yuv_to_rgb_u8(frames))).  The fetch, the blend and the store are frame_source.h's.
//   taps of an entry: ix0 = fx >> 11, wx1 = fx & 2047, ix1 = min(ix0 + 1, W - 1); likewise iy0, wy1, iy1 from fy
//   an invalid entry (either half negative) gives the eye's fill bytes and loads nothing
// Bound by gather latency and HBM, not by arithmetic.  Bytes per output pixel: 8 map bytes (both eyes' maps are 2 * 8 * S0^2 = 1 MB at S0 = 256:
// read from HBM for the first frame of a batch, from L2 for every other), up to 12 source bytes (four taps x three bytes; neighbouring pixels share
// taps, and a lens map is smooth, so a wave's taps fall into a few runs of source rows and what HBM delivers is the touched rows, as for the resize),
// 3 output bytes.  Hence the shape:
//   * NO tap table in LDS: the taps differ for every pixel, so a thread reads its four entries straight from the map as two 16-byte loads (the
//     maps are 16-byte aligned, a group of four pixels never crosses a row: S0 is a multiple of 4).
//   * one thread = four output pixels of a row (store_rgb4); a wave reads 2 KB of map, contiguous, and its 16 x 64 taps are neighbours in the source.
//   * the four taps of a pixel are independent loads issued before the first is used; a pixel is skipped as a whole where its entry is invalid (the
//     branch keeps the pixels of a thread apart, so latency is hidden by occupancy -- about 40 VGPRs, eight waves per SIMD -- and not by one thread's
//     queue depth).
//   * every tap index comes from a valid entry and is clamped to the frame on BOTH sides (ix0 <= W - 1 as well: a no-op for a map built for this
//     H x W, which the library cannot inspect on the device) -- no load touches a byte outside n * frame bytes whatever the map holds.
//   * both eyes in one launch (blockIdx.y), each with its own map and fill.  No LDS.
//   * a map PER STREAM (lens_remap_streams_kernel, egotap_lens_remap_streams): each eye's pointer is int32 [S][S0 * S0][2] and frame b of the caller's
//     batch reads map b % S -- one more term in the map address, everything else the same body.  A launch that gathers a piece of a batch is told the
//     piece's first frame, so the index is the frame's place in the WHOLE batch.  Every stream's map is 16-byte aligned where the first is.
#pragma once
#include "frame_source.h"

static constexpr int kLensFracBits = 11;                         // spec.LENS_FRAC_BITS
static inline unsigned lens_fill(const uint8_t* rgb) { return (unsigned)rgb[0] | (unsigned)rgb[1] << 8 | (unsigned)rgb[2] << 16; }

// The kernel's body.  STREAMS false: one map per eye for the whole batch.  STREAMS true: each eye's pointer is a table of S maps, int32 [S][S0 * S0][2],
// and frame b of the launch reads map (frame0 + b) % S -- frame0 is the launch's first frame in the caller's whole batch, so a piece of a batch walked
// in pieces still reads each frame's own map.  One more term in the map address, nothing else.
template <int FETCH, bool STREAMS>
static __device__ __forceinline__ void lens_remap_body(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                       const int* __restrict__ map_left, const int* __restrict__ map_right,
                                                       unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8, long groups, int H, int W,
                                                       int pitch, long uv_offset, long frame_stride, const YuvCoef& coef, unsigned fill_l, unsigned fill_r, int S0,
                                                       int S, long frame0) {
    const unsigned char* src = blockIdx.y ? right8 : left8;
    const int* map = blockIdx.y ? map_right : map_left;
    unsigned char* dst = blockIdx.y ? out_right8 : out_left8;
    const unsigned fill = blockIdx.y ? fill_r : fill_l;
    const long gpf = (long)S0 * (S0 / 4);                     // groups per frame
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < groups; i += (long)gridDim.x * 256) {
        const long b = i / gpf, g = i - b * gpf;              // the group's four pixels are entries 4 g .. 4 g + 3 of the eye's map
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        const int* entry = map + 8 * g;
        if (STREAMS) entry += (long)((unsigned)(frame0 + b) % (unsigned)S) * (8 * gpf);      // (the batch is an int: 32-bit division; 8 gpf = 2 S0^2 ints, one map)
        const i32x4v ta = *(const i32x4v*)entry, tb = *(const i32x4v*)(entry + 4);
        const int t[8] = {ta[0], ta[1], ta[2], ta[3], tb[0], tb[1], tb[2], tb[3]};
        const unsigned char* frame = src + b * frame_stride;
        unsigned px[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int fx = t[2 * e], fy = t[2 * e + 1];
            px[e] = fill;
            if (fx >= 0 && fy >= 0) {
                int ix0 = fx >> kLensFracBits, iy0 = fy >> kLensFracBits;
                ix0 = ix0 < W - 1 ? ix0 : W - 1;
                iy0 = iy0 < H - 1 ? iy0 : H - 1;
                const int ix1 = ix0 + 1 < W ? ix0 + 1 : W - 1, iy1 = iy0 + 1 < H ? iy0 + 1 : H - 1;
                const unsigned p00 = frame_pixel_rgb<FETCH>(frame, iy0, ix0, pitch, uv_offset, coef), p01 = frame_pixel_rgb<FETCH>(frame, iy0, ix1, pitch, uv_offset, coef);
                const unsigned p10 = frame_pixel_rgb<FETCH>(frame, iy1, ix0, pitch, uv_offset, coef), p11 = frame_pixel_rgb<FETCH>(frame, iy1, ix1, pitch, uv_offset, coef);
                px[e] = blend_rgb(p00, p01, p10, p11, (unsigned)(fx & 2047), (unsigned)(fy & 2047));
            }
        }
        store_rgb4(dst, i, px);
    }
}

template <int FETCH>
static __global__ __launch_bounds__(256) void lens_remap_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                               const int* __restrict__ map_left, const int* __restrict__ map_right,
                                                               unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8, long groups,
                                                               int H, int W, int pitch, long uv_offset, long frame_stride, YuvCoef coef, unsigned fill_l,
                                                               unsigned fill_r, int S0) {
    lens_remap_body<FETCH, false>(left8, right8, map_left, map_right, out_left8, out_right8, groups, H, W, pitch, uv_offset, frame_stride, coef, fill_l, fill_r, S0,
                                  1, 0L);
}

template <int FETCH>
static __global__ __launch_bounds__(256) void lens_remap_streams_kernel(const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8,
                                                                       const int* __restrict__ map_left, const int* __restrict__ map_right,
                                                                       unsigned char* __restrict__ out_left8, unsigned char* __restrict__ out_right8, long groups,
                                                                       int H, int W, int pitch, long uv_offset, long frame_stride, YuvCoef coef, unsigned fill_l,
                                                                       unsigned fill_r, int S0, int S, long frame0) {
    lens_remap_body<FETCH, true>(left8, right8, map_left, map_right, out_left8, out_right8, groups, H, W, pitch, uv_offset, frame_stride, coef, fill_l, fill_r, S0,
                                 S, frame0);
}

// n frames per eye; pointers and the layout checked by the caller (maps 16-byte aligned, outputs 4-byte aligned, the frame bases aligned to
// frame_base_alignment and the layout passed by frame_layout_refusal)
static inline hipError_t lens_remap_launch(const unsigned char* left8, const unsigned char* right8, long n, const FrameSource& q, const int* map_left,
                                           const int* map_right, unsigned fill_left, unsigned fill_right, int S0, unsigned char* out_left8,
                                           unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (!frame_launch_ok(n, S0, q)) return hipErrorInvalidValue;
    if (!left8 || !right8 || !map_left || !map_right || !out_left8 || !out_right8) return hipErrorInvalidValue;
    if ((((uintptr_t)map_left | (uintptr_t)map_right) & 15) != 0 || (((uintptr_t)out_left8 | (uintptr_t)out_right8) & 3) != 0) return hipErrorInvalidValue;
    const long groups = n * S0 * (S0 / 4);
    return frame_fetch_dispatch(q.fetch, [&](auto fetch) {
        hipLaunchKernelGGL(lens_remap_kernel<decltype(fetch)::value>, dim3(frame_grid(groups, num_cu), 2), dim3(256), 0, s, left8, right8, map_left, map_right,
                           out_left8, out_right8, groups, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride, q.coef, fill_left, fill_right, S0);
    });
}
// the same through S maps per eye (int32 [S][S0 * S0][2]: every stream's map is 16-byte aligned where the first is); the launch's first frame is
// frame `frame0` of the caller's batch: frame b of the launch reads map (frame0 + b) % S.  S >= 1 and frame0 >= 0 checked by the caller.
static inline hipError_t lens_remap_streams_launch(const unsigned char* left8, const unsigned char* right8, long n, const FrameSource& q, const int* map_left,
                                                   const int* map_right, int S, long frame0, unsigned fill_left, unsigned fill_right, int S0,
                                                   unsigned char* out_left8, unsigned char* out_right8, int num_cu, hipStream_t s) {
    if (!frame_launch_ok(n, S0, q) || S < 1 || frame0 < 0) return hipErrorInvalidValue;
    if (!left8 || !right8 || !map_left || !map_right || !out_left8 || !out_right8) return hipErrorInvalidValue;
    if ((((uintptr_t)map_left | (uintptr_t)map_right) & 15) != 0 || (((uintptr_t)out_left8 | (uintptr_t)out_right8) & 3) != 0) return hipErrorInvalidValue;
    const long groups = n * S0 * (S0 / 4);
    return frame_fetch_dispatch(q.fetch, [&](auto fetch) {
        hipLaunchKernelGGL(lens_remap_streams_kernel<decltype(fetch)::value>, dim3(frame_grid(groups, num_cu), 2), dim3(256), 0, s, left8, right8, map_left,
                           map_right, out_left8, out_right8, groups, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride, q.coef, fill_left, fill_right, S0, S, frame0);
    });
}
