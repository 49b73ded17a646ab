// What the sensor front ends share (frame_resize.h: a rectangle of the sensor's frame cropped, mirrored and resized; lens_remap.h: another lens's
// frame gathered through a map).  Both turn the sensor's own frames into the camera bytes the estimators read, uint8 [n, S0, S0, 3], in one pass in
// integers specified in egotap_amd/spec.py (resize_u8, yuv_to_rgb_u8, yuv_resize_u8, lens_remap_u8) and restated token for token -- host and device
// agree bit for bit.  Stated here once, no kernel in this file:
//   FrameSource      one frame's layout in bytes and what a tap is (FETCH): three bytes of a packed RGB8 frame, or the pixel of an NV12 (4:2:0, a Y
//                    plane followed by an interleaved UV plane) or YUYV (packed 4:2:2) frame converted to RGB bytes
//   frame_pixel_rgb  the fetch.  RGB8: three byte loads, at any address (W need not be a multiple of 4, a row starts at any byte)
//                    NV12: Y(y, x) at y * pitch + x; the chroma pair at uv_offset + (y >> 1) * pitch + 2 * (x >> 1), U then V, ONE aligned 16-bit load
//                    YUYV: the pixel pair x >> 1 of row y is Y0 U Y1 V at y * pitch + 4 * (x >> 1), ONE aligned dword
//                      R = clip((CY (Y - y_off) + RV (V - 128) + 2^13) >> 14, 0, 255)
//                      G = clip((CY (Y - y_off) - GU (U - 128) - GV (V - 128) + 2^13) >> 14, 0, 255)
//                      B = clip((CY (Y - y_off) + BU (U - 128) + 2^13) >> 14, 0, 255)      (arithmetic shift, one rounding, all below 2^24)
//                    Chroma is replicated (a pixel takes the U, V of its 2 x 2 block or of its pair); nothing is interpolated in YUV: the kernels
//                    are by definition resize_u8 / lens_remap_u8 of yuv_to_rgb_u8(frames).  W (and for NV12 H) is even, so a pixel's block lies
//                    inside the frame: a fetch at a pixel inside H x W touches no byte outside frame_stride or of a row past pitch.
//   blend_rgb        byte = (wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) + 2^21) >> 22, weights Q11 (<= 2048^2 * 255 + 2^21 < 2^31)
//   store_rgb4       one thread = four output pixels of a row = three aligned dword stores (S0 a multiple of 4, the output base 4-byte aligned);
//                    consecutive lanes take consecutive groups, so a wave writes 768 contiguous bytes
//   frame_grid       workgroups stride over the groups, at most eight per compute unit; both eyes in one launch (blockIdx.y)
//   frame_fetch_dispatch   the run-time fetch -> the kernel's template argument, so that a launcher writes its argument list once
// Plain loads and vector stores, no atomics, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

enum { FETCH_RGB8 = 0, FETCH_NV12 = 1, FETCH_YUYV = 2 };      // internal: the ABI's format codes are mapped to it where a descriptor is checked
enum { YUV_BT601 = 0, YUV_BT709 = 1 };                         // egotap.h EGOTAP_YUV_BT601 / _BT709
enum { YUV_LIMITED = 0, YUV_FULL = 1 };                        // egotap.h EGOTAP_YUV_LIMITED / _FULL

static constexpr int kResizeMaxSide = 4096;          // S0 <= 4096: the resize's tap table is 8 S0 bytes of LDS (32 KB at most)
static constexpr int kResizeMaxSrc = 16384;          // H, W <= 16384: (2 S0 - 1) L and 3 W stay far inside int32

struct YuvCoef { int cy, rv, gu, gv, bu, y_off; };   // round(real * 2^14) each, and the luma offset
// one frame's layout in bytes (spec.YuvLayout) and the colour as the kernels take it; RGB8 has pitch = 3 W and frame_stride = 3 H W
struct FrameSource {
    int fetch, H, W, pitch;
    long uv_offset, frame_stride;
    YuvCoef coef;
};
static inline FrameSource frame_source_rgb8(int H, int W) { return FrameSource{FETCH_RGB8, H, W, 3 * W, 0L, 3L * H * W, YuvCoef{}}; }

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
static inline const char* frame_layout_refusal(int fetch, int H, int W, int pitch, long uv_offset, long frame_stride) {
    if (H < 1 || W < 1 || H > kResizeMaxSrc || W > kResizeMaxSrc) return "the frame height and width must be between 1 and 16384";
    if (fetch == FETCH_NV12) {
        if (H % 2 || W % 2) return "NV12 needs an even H and W (4:2:0 chroma covers 2 x 2 blocks)";
        if (pitch < W) return "pitch is too small (NV12: pitch >= W)";
        if (uv_offset < (long)pitch * (H - 1) + W) return "the planes overlap (NV12: uv_offset >= pitch * (H - 1) + W)";
        if (uv_offset + (long)(H / 2 - 1) * pitch + W > frame_stride) return "the last chroma byte is past frame_stride";
        if (pitch % 2 || uv_offset % 2 || frame_stride % 2) return "NV12 needs an even pitch, uv_offset and frame_stride (the chroma pair is one aligned 16-bit load)";
    } else if (fetch == FETCH_YUYV) {
        if (W % 2) return "YUYV needs an even W (4:2:2 chroma covers pixel pairs)";
        if (pitch < 2L * W) return "pitch is too small (YUYV: pitch >= 2 W)";
        if ((long)(H - 1) * pitch + 2L * W > frame_stride) return "the last byte is past frame_stride";
        if (pitch % 4 || frame_stride % 4) return "YUYV needs pitch and frame_stride to be multiples of 4 (the pixel pair is one aligned dword)";
    }
    return nullptr;
}
static inline const char* frame_layout_refusal(const FrameSource& q) { return frame_layout_refusal(q.fetch, q.H, q.W, q.pitch, q.uv_offset, q.frame_stride); }
static inline int frame_base_alignment(int fetch) { return fetch == FETCH_NV12 ? 2 : fetch == FETCH_YUYV ? 4 : 1; }

// what a launcher refuses about the batch, the output side and the layout (the entries have said it by name before)
static inline bool frame_launch_ok(long n, int S0, const FrameSource& q) {
    return n > 0 && S0 > 0 && S0 % 4 == 0 && S0 <= kResizeMaxSide && q.fetch >= FETCH_RGB8 && q.fetch <= FETCH_YUYV && !frame_layout_refusal(q);
}
static inline unsigned frame_grid(long groups, int num_cu) {
    const long grid = (groups + 255) / 256;
    return (unsigned)(grid > 8L * num_cu ? 8L * num_cu : grid);
}
// launch(std::integral_constant<int, FETCH>) for the fetch at hand (checked by frame_launch_ok)
template <class Launch>
static inline hipError_t frame_fetch_dispatch(int fetch, Launch&& launch) {
    if (fetch == FETCH_RGB8) launch(std::integral_constant<int, FETCH_RGB8>{});
    else if (fetch == FETCH_NV12) launch(std::integral_constant<int, FETCH_NV12>{});
    else launch(std::integral_constant<int, FETCH_YUYV>{});
    return hipGetLastError();
}

// the RGB bytes of pixel (y, x) of a frame, packed R | G << 8 | B << 16
template <int FETCH>
static __device__ __forceinline__ unsigned frame_pixel_rgb(const unsigned char* __restrict__ frame, int y, int x, int pitch, long uv_offset, const YuvCoef& k) {
    if (FETCH == FETCH_RGB8) {
        const unsigned char* p = frame + (long)y * pitch + 3 * x;
        return (unsigned)p[0] | (unsigned)p[1] << 8 | (unsigned)p[2] << 16;
    }
    int Y, U, V;
    if (FETCH == FETCH_NV12) {
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

// the four taps of a pixel blended, packed as they are; wx1, wy1 in 0 .. 2047
static __device__ __forceinline__ unsigned blend_rgb(unsigned p00, unsigned p01, unsigned p10, unsigned p11, unsigned wx1, unsigned wy1) {
    const unsigned wx0 = 2048u - wx1, wy0 = 2048u - wy1;
    unsigned px = 0u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const unsigned top = wx0 * ((p00 >> (8 * c)) & 0xffu) + wx1 * ((p01 >> (8 * c)) & 0xffu);
        const unsigned bot = wx0 * ((p10 >> (8 * c)) & 0xffu) + wx1 * ((p11 >> (8 * c)) & 0xffu);
        px |= ((wy0 * top + wy1 * bot + (1u << 21)) >> 22) << (8 * c);
    }
    return px;
}

// group i of an eye's output: pixels 4 i .. 4 i + 3, twelve bytes
static __device__ __forceinline__ void store_rgb4(unsigned char* __restrict__ dst, long i, const unsigned (&px)[4]) {
    unsigned* op = (unsigned*)(dst + i * 12);
    op[0] = px[0] | px[1] << 24;
    op[1] = px[1] >> 8 | px[2] << 16;
    op[2] = px[2] >> 16 | px[3] << 8;
}
