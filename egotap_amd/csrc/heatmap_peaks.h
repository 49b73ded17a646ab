// Heatmap peaks: each S x S map of a [B, C, S, S] tensor (fp32 or bf16, the lifting head's input layout: element (b, c, y, x) at
// b * image_stride + c * S*S + y * S + x) reduced to ONE 16-byte record (x, y, score, index) -- where the joint is and how sure the estimator is.
// The ground-truth maps (utils/projection.py:263-279) are unit-peak Gaussians for a joint in view and all zero for one out of view, so the peak's
// value gates the joint and its position is the joint's pixel.
//   index  = iy * S + ix of the maximum.  Values are compared as fp32 (bf16 upcast exactly); a larger value wins, among equal values the smallest
//            linear index; a NaN never beats a number; the running maximum starts at -inf (a map may be all negative); a map of only NaNs gives 0.
//   score  = the element at index, as fp32.
//   x      = ix + 0.5 + 0.25 * sgn(h[iy][ix + 1] - h[iy][ix - 1]) (the quarter-pixel step towards the higher neighbour; 0 when a neighbour lies
//            outside the map or the difference is zero or NaN), y the same from the rows above and below: exact in fp32.
//   affine per group of n / G consecutive channels, by value in the kernel arguments: x_out = fmaf(ax, x, bx), y_out = fmaf(ay, y, by).
// (value, index) pairs have a total order, so the result does not depend on how the map is split over lanes and waves:
//   * 16-byte loads, consecutive lanes consecutive vectors (a wave reads 1 KB runs); every lane keeps the best pair of its vectors,
//   * a butterfly over the wave's 64 lanes (__shfl_xor), then -- W = 4: one workgroup per map, maps of 4096 elements and more -- four (value, index) pairs in LDS
//     across the waves; W = 1: one WAVE per map, four maps per workgroup (sides 16 .. 48: no barrier, no idle waves),
//   * one lane reads the four neighbours again (they are in L2) and stores the record: one vector store, no atomics, no workspace.
// S*S is a multiple of 256 (S a multiple of 16), so a 16-byte vector lies inside the map or outside it as a whole.  HBM-bound: every element is read once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int kPeaksMaxGroups = 32;
struct PeaksAffine { float g[kPeaksMaxGroups][4]; };          // per group (ax, bx, ay, by)

// the total order of the reduction: does (v, i) beat (bv, bi)?  (bv is never NaN; a NaN v beats nothing)
static __device__ __forceinline__ bool peaks_beats(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

static __device__ __forceinline__ float peaks_f32(float v) { return v; }
static __device__ __forceinline__ float peaks_f32(__bf16 v) { return __uint_as_float((unsigned)__builtin_bit_cast(unsigned short, v) << 16); }

static __device__ __forceinline__ void peaks_load16(const float* p, float (&v)[4]) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    const f32x4v r = *(const f32x4v*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = r[k];
}
static __device__ __forceinline__ void peaks_load16(const __bf16* p, float (&v)[8]) {
    typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
    const u32x4v r = *(const u32x4v*)p;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[2 * k] = __uint_as_float(r[k] << 16);
        v[2 * k + 1] = __uint_as_float(r[k] & 0xffff0000u);
    }
}

// +-0.25 towards the higher of two neighbours, 0 where they are equal or the difference is NaN
static __device__ __forceinline__ float peaks_quarter(float lo, float hi) {
    const float d = hi - lo;
    return d > 0.f ? 0.25f : (d < 0.f ? -0.25f : 0.f);
}

template <typename T, int W>
static __global__ __launch_bounds__(256) void heatmap_peaks_kernel(const T* __restrict__ hm, long image_stride, int S, int c0, int n, long maps, int per_group,
                                                                  PeaksAffine aff, float* __restrict__ out) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    constexpr int V = 16 / sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long map = W == 1 ? (long)blockIdx.x * 4 + wave : (long)blockIdx.x;
    if (W == 1 && map >= maps) return;                       // a whole wave leaves; this path has no barrier
    const int HW = S * S;
    const long b = map / n;
    const int ch = (int)(map - b * n);
    const T* __restrict__ p = hm + b * image_stride + (long)(c0 + ch) * HW;
    float best = -INFINITY;
    int at = HW;                                             // "nothing yet": behind every index, so the first -inf element still takes it
    for (int e = (W == 1 ? lane : (int)threadIdx.x) * V; e < HW; e += 64 * W * V) {
        float v[V];
        peaks_load16(p + e, v);
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (peaks_beats(v[k], e + k, best, at)) { best = v[k]; at = e + k; }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float ov = __shfl_xor(best, m);
        const int oi = __shfl_xor(at, m);
        if (peaks_beats(ov, oi, best, at)) { best = ov; at = oi; }
    }
    if (W > 1) {
        __shared__ float sv[W];
        __shared__ int si[W];
        if (lane == 0) { sv[wave] = best; si[wave] = at; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < W; ++w)
                if (peaks_beats(sv[w], si[w], best, at)) { best = sv[w]; at = si[w]; }
    }
    if ((W == 1 ? lane : (int)threadIdx.x) != 0) return;
    if (at >= HW) at = 0;                                    // only NaNs
    const int iy = at / S, ix = at - iy * S;
    const float score = peaks_f32(p[at]);
    const float dx = ix > 0 && ix < S - 1 ? peaks_quarter(peaks_f32(p[at - 1]), peaks_f32(p[at + 1])) : 0.f;
    const float dy = iy > 0 && iy < S - 1 ? peaks_quarter(peaks_f32(p[at - S]), peaks_f32(p[at + S])) : 0.f;
    const float* a = aff.g[ch / per_group];
    f32x4v rec;
    rec[0] = fmaf(a[0], (float)ix + 0.5f + dx, a[1]);
    rec[1] = fmaf(a[2], (float)iy + 0.5f + dy, a[3]);
    rec[2] = score;
    rec[3] = (float)at;
    *(f32x4v*)(out + map * 4) = rec;
}

// hm, out 16-byte aligned, image_stride a multiple of 16 bytes, S a multiple of 16 in 16 .. 128, 1 <= groups <= kPeaksMaxGroups dividing n:
// checked by the caller.  affine: host, groups x 4 (ax, bx, ay, by), or NULL = identity.
template <typename T>
static inline hipError_t heatmap_peaks_launch(const T* hm, long B, int S, long image_stride, int c0, int n, int groups, const float* affine, float* out,
                                              hipStream_t s) {
    if (B <= 0 || n <= 0 || groups <= 0 || groups > kPeaksMaxGroups || n % groups || S < 16 || S > 128 || S % 16) return hipErrorInvalidValue;
    PeaksAffine aff;
    for (int g = 0; g < kPeaksMaxGroups; ++g)
        for (int k = 0; k < 4; ++k) aff.g[g][k] = affine && g < groups ? affine[4 * g + k] : (k & 1 ? 0.f : 1.f);
    const long maps = B * n;
    if (S * S >= 4096)
        hipLaunchKernelGGL((heatmap_peaks_kernel<T, 4>), dim3((unsigned)maps), dim3(256), 0, s, hm, image_stride, S, c0, n, maps, n / groups, aff, out);
    else
        hipLaunchKernelGGL((heatmap_peaks_kernel<T, 1>), dim3((unsigned)((maps + 3) / 4)), dim3(256), 0, s, hm, image_stride, S, c0, n, maps, n / groups, aff, out);
    return hipGetLastError();
}
