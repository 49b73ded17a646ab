// The 3x3 taps (pad 1) of the convolution loaders on channels-last bf16 maps (conv_bf16s.h: 32-deep K-tiles, gemm_bf16s64.h: 64-deep,
// pointer and scalar-origin forms), stated once.  k = (channel slab, tap, channel in slab): a K-tile is ONE tap of one slab, the nine
// taps of a slab are consecutive K-tiles, tap t = (dy + 1) * 3 + (dx + 1).
#pragma once
#include <hip/hip_runtime.h>
// Output row m = (image n, yo, xo) of So x So maps, So = 1 << log2So; its centre tap is pixel (y, x) = (yo, xo) * stride of image n's S x S input
// map, S = So * stride (STRIDED: a run-time stride; else stride 1).  Bit t of mask set: tap t lies inside the map (else the loader reads its
// page of zeros: F.conv2d's padding).
struct Conv3Px { int n, y, x, S; unsigned mask; };
template <bool STRIDED = false> __device__ __forceinline__ Conv3Px conv3_pixel(int m, int log2So, int stride = 1) {
    const int So = 1 << log2So, xo = m & (So - 1), yo = (m >> log2So) & (So - 1), n = m >> (2 * log2So);
    const int S = STRIDED ? So * stride : So, y = STRIDED ? yo * stride : yo, x = STRIDED ? xo * stride : xo;
    unsigned mask = 0;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if (y + dy >= 0 && y + dy < S && x + dx >= 0 && x + dx < S) mask |= 1u << t;
    }
    return Conv3Px{n, y, x, S, mask};
}
// K-tile kt -> (slab, tap, dy, dx) without a division: kt / 9 = (kt * 7282) >> 16 exactly for kt < 7000, tap / 3 = (tap * 11) >> 5 for tap < 9
struct Conv3Tap {
    int slab, tap;
    __device__ __forceinline__ explicit Conv3Tap(int kt) : slab((kt * 7282) >> 16), tap(kt - 9 * slab) {}
    __device__ __forceinline__ int pixels(int rowstride) const {
        const int dy = ((tap * 11) >> 5) - 1, dx = tap - 3 * (dy + 1) - 1;      // distance from the centre pixel
        return dy * rowstride + dx;
    }
};
