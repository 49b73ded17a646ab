// Limb decode: each (cos, sin) PAIR of S x S limb maps of a [B, C, S, S] tensor (fp32 or bf16, the layout of heatmap_peaks.h) reduced to ONE 32-byte
// record (theta, coherence, x, y, phi, length, peak, mass).  The reference draws a target limb map as the anti-aliased segment parent -> joint,
// Gaussian-blurred and doubled, and multiplies it by cos(theta) and by sin(theta), theta = arctan(dz / |dxy|) the limb's elevation out of the image plane
// (utils/data.py:197-252, dataloader/data_loader.py:193-199): a pair carries the angle, the segment, how much of it was seen and whether the pixels agree.
// For eye e and limb l of n the cos map is channel c0 + e * 2n + l, the sin map channel c0 + e * 2n + n + l (cat(cos, sin) per eye).
// Every sum runs over all S*S pixels in float64, pixel centres at ix + 0.5, iy + 0.5:
//   m = sqrt(c^2 + s^2)   M = sum m   C = sum c   Sn = sum s   X = sum m x   Y = sum m y   XX = sum m x^2   YY = sum m y^2   XY = sum m x y
//   peak      = max m (a NaN never wins; starts at 0)           mass = M
//   theta     = atan2(Sn, C)           exact for a target pair (both are the same non-negative map times sin / cos theta); the affine does not touch it
//   coherence = hypot(C, Sn) / M       in [0, 1]; 1 when every pixel votes for the same angle
//   x, y      = ax * X/M + bx, ay * Y/M + by                    the eye's affine (ax, bx, ay, by), by value in the kernel arguments
//   central moments mu20 = XX/M - (X/M)^2, mu02, mu11, scaled by ax^2, ay^2, ax ay;   D = (mu20' - mu02')^2 + 4 mu11'^2
//   phi       = atan2(2 mu11', mu20' - mu02') / 2               the segment's orientation in the output frame, in (-pi/2, pi/2]
//   length    = sqrt(12 sqrt(D))       a uniform segment of length l blurred by an isotropic sigma has variance l^2/12 + sigma^2 along its axis and
//                                      sigma^2 across it: the difference of the eigenvalues is sqrt(D) and the blur drops out.  Exact when |ax| = |ay|;
//                                      a non-uniform sensor crop (|ax| != |ay|) makes the blur anisotropic and bends phi and length.
//   The segment's ends are (x, y) +- length / 2 * (cos phi, sin phi).
//   Empty rule, when !(M > 0) or M is not finite (an all-zero pair, a NaN or inf inside): theta = coherence = phi = length = 0, (x, y) the affine of
//   the map centre (S/2, S/2), peak as computed, mass = (float)M.
// Each of the eight values is rounded ONCE from float64.  The sums' order differs from the host's, so they agree to S*S * 2^-53 relative, not in bits.
//   * 16-byte loads, consecutive lanes consecutive vectors; a vector lies inside one row (S is a multiple of 16); every lane keeps its eight float64
//     sums and its running maximum,
//   * a butterfly over the wave's 64 lanes (__shfl_xor, a double moved as two 32-bit halves), then -- W = 4: one workgroup per pair, maps of 4096
//     elements and more -- 4 x 9 doubles in LDS across the waves; W = 1: one WAVE per pair, four pairs per workgroup (sides 16 .. 48: no barrier),
//   * one lane finishes the arithmetic and stores the record: two 16-byte vector stores, no atomics, no workspace.
// HBM-bound: every element of the 2n maps per eye is read once.
#pragma once
#include "heatmap_peaks.h"

constexpr int kLimbSums = 9;                                 // M, C, Sn, X, Y, XX, YY, XY and the maximum

static __device__ __forceinline__ double limb_shfl_xor(double v, int mask) {
    return __hiloint2double(__shfl_xor(__double2hiint(v), mask), __shfl_xor(__double2loint(v), mask));
}

// the record of one pair from its sums (a[]: the eye's affine); products and sums are kept apart as the host definition writes them
static __device__ __forceinline__ void limb_finish(const double (&r)[kLimbSums], const float* a, int S, float* out) {
#pragma clang fp contract(off)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    const double M = r[0], C = r[1], Sn = r[2], ax = a[0], bx = a[1], ay = a[2], by = a[3];
    double theta = 0.0, coh = 0.0, x = 0.5 * S, y = 0.5 * S, phi = 0.0, len = 0.0;
    if (M > 0.0 && M <= 1.7976931348623157e308) {
        x = r[3] / M;
        y = r[4] / M;
        const double m20 = (r[5] / M - x * x) * (ax * ax), m02 = (r[6] / M - y * y) * (ay * ay), m11 = (r[7] / M - x * y) * (ax * ay);
        const double d = m20 - m02, D = d * d + 4.0 * (m11 * m11);
        theta = atan2(Sn, C);
        coh = hypot(C, Sn) / M;
        phi = 0.5 * atan2(2.0 * m11 + 0.0, d);               // (+ 0.0: a -0 numerator would turn a vertical segment's pi/2 into -pi/2)
        len = sqrt(12.0 * sqrt(D));
    }
    f32x4v lo, hi;
    lo[0] = (float)theta;
    lo[1] = (float)coh;
    lo[2] = (float)(ax * x + bx);
    lo[3] = (float)(ay * y + by);
    hi[0] = (float)phi;
    hi[1] = (float)len;
    hi[2] = (float)r[8];
    hi[3] = (float)M;
    *(f32x4v*)out = lo;
    *(f32x4v*)(out + 4) = hi;
}

template <typename T, int W>
static __global__ __launch_bounds__(256) void limb_decode_kernel(const T* __restrict__ hm, long image_stride, int S, int c0, int n, int eyes, long pairs,
                                                                PeaksAffine aff, float* __restrict__ out) {
    constexpr int V = 16 / sizeof(T);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long pair = W == 1 ? (long)blockIdx.x * 4 + wave : (long)blockIdx.x;
    if (W == 1 && pair >= pairs) return;                     // a whole wave leaves; this path has no barrier
    const int HW = S * S;
    const long be = pair / n;                                // frame * eyes + eye
    const int limb = (int)(pair - be * n), eye = (int)(be % eyes);
    const T* __restrict__ pc = hm + (be / eyes) * image_stride + (long)(c0 + eye * 2 * n + limb) * HW;
    const T* __restrict__ ps = pc + (long)n * HW;
    double r[kLimbSums];
#pragma unroll
    for (int k = 0; k < kLimbSums; ++k) r[k] = 0.0;
    for (int e = (W == 1 ? lane : (int)threadIdx.x) * V; e < HW; e += 64 * W * V) {
        float c[V], s[V];
        peaks_load16(pc + e, c);
        peaks_load16(ps + e, s);
        const int iy = e / S;
        const double y = iy + 0.5, x0 = (e - iy * S) + 0.5;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const double cd = c[k], sd = s[k], x = x0 + k;
            const double m = sqrt(cd * cd + sd * sd), mx = m * x, my = m * y;
            r[0] += m;
            r[1] += cd;
            r[2] += sd;
            r[3] += mx;
            r[4] += my;
            r[5] += mx * x;
            r[6] += my * y;
            r[7] += mx * y;
            if (m > r[8]) r[8] = m;                          // (a NaN m beats nothing)
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < kLimbSums - 1; ++k) r[k] += limb_shfl_xor(r[k], m);
        const double o = limb_shfl_xor(r[8], m);
        if (o > r[8]) r[8] = o;
    }
    if (W > 1) {
        __shared__ double sr[W][kLimbSums];
        if (lane == 0)
#pragma unroll
            for (int k = 0; k < kLimbSums; ++k) sr[wave][k] = r[k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (int w = 1; w < W; ++w) {
#pragma unroll
                for (int k = 0; k < kLimbSums - 1; ++k) r[k] += sr[w][k];
                if (sr[w][8] > r[8]) r[8] = sr[w][8];
            }
    }
    if ((W == 1 ? lane : (int)threadIdx.x) != 0) return;
    limb_finish(r, aff.g[eye], S, out + pair * 8);
}

// hm, out 16-byte aligned, image_stride a multiple of 16 bytes and at least (c0 + 2 * eyes * n) * S*S, S a multiple of 16 in 16 .. 128,
// 1 <= eyes <= kPeaksMaxGroups: checked by the caller.  affine: host, eyes x 4 (ax, bx, ay, by), or NULL = identity.  out: [B, eyes, n, 8].
template <typename T>
static inline hipError_t limb_decode_launch(const T* hm, long B, int S, long image_stride, int c0, int n, int eyes, const float* affine, float* out, hipStream_t s) {
    if (B <= 0 || n <= 0 || eyes <= 0 || eyes > kPeaksMaxGroups || S < 16 || S > 128 || S % 16) return hipErrorInvalidValue;
    PeaksAffine aff;
    for (int g = 0; g < kPeaksMaxGroups; ++g)
        for (int k = 0; k < 4; ++k) aff.g[g][k] = affine && g < eyes ? affine[4 * g + k] : (k & 1 ? 0.f : 1.f);
    const long pairs = B * eyes * n;
    if (S * S >= 4096)
        hipLaunchKernelGGL((limb_decode_kernel<T, 4>), dim3((unsigned)pairs), dim3(256), 0, s, hm, image_stride, S, c0, n, eyes, pairs, aff, out);
    else
        hipLaunchKernelGGL((limb_decode_kernel<T, 1>), dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, s, hm, image_stride, S, c0, n, eyes, pairs, aff, out);
    return hipGetLastError();
}
