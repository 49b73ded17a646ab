// The fisheye camera model (OCamCalib, utils/projection.py:55-144) and the stereo triangulation of the serving entries' keypoints.  Three kernels, each
// one launch, float64 inside (a few KB of work per call: bound by latency, not by the float64 rate), fp32 in and out, every output rounded once:
//   ocam_project_kernel    world2cam, one thread per point: [N, 3] -> pixels [N, 2]
//   ocam_unproject_kernel  cam2world, one thread per point: pixels [N, 2] -> unit rays [N, 3]
//   stereo_triangulate_kernel  keypoints [B, 2, J, 4] -> joints3d [B, J, 8] + frame [B, 8]: one WAVE per frame, lane = joint (J <= 64), four frames per
//       workgroup.  Each lane unprojects its joint through both cameras, intersects the two rays (closest approach) and leaves (valid, X, pose row, gap)
//       in LDS; every lane then adds the frame's sums from LDS in ASCENDING joint order (same address for all lanes: a broadcast read), so the host
//       restatement, which adds in that order, gets the same bits.  Lane = joint writes its record as two 16-byte stores, lane 0 the frame record.
//   stereo_triangulate_streams_kernel  the same body with a rig PER STREAM: a table of S StereoRig in device memory (egotap.h egotap_stereo_rig), the
//       wave of frame b reads rig b % S -- a wave-uniform index, so the rig's doubles are plain uniform loads, fetched once per wave -- and n_pol is
//       clamped to the array's length: whatever the table holds, no load leaves it.  Same records in the same bits as the by-value kernel with that rig.
// The models, R, t and the affines travel by value in the kernel arguments (uniform indices: scalar loads).  Contraction is off in every function here:
// the definitions (egotap.h, spec.py ocam_world2cam_ref / ocam_cam2world_ref / stereo_triangulate_ref) keep products and sums apart, and each polynomial is
// the reference's running-power sum (r_i *= r; z += r_i * pol[i]), not Horner.  sqrt and the divisions are correctly rounded; atan is the library's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "egotap.h"

constexpr int kStereoMaxJoints = 64;
constexpr int kStereoFramesPerBlock = 4;

struct StereoRig {
    egotap_ocam cam[2];
    double R[9], t[3], aff[2][4], min_score;
};
static_assert(sizeof(StereoRig) == sizeof(egotap_stereo_rig) && alignof(StereoRig) == alignof(egotap_stereo_rig),
              "a row of the caller's rig table (egotap.h egotap_stereo_rig) is read as a StereoRig");

static __device__ __forceinline__ double ocam_poly(const double* coef, int n, double r) {
#pragma clang fp contract(off)
    double z = coef[0], ri = 1.0;
    for (int k = 1; k < n; ++k) {
        ri = ri * r;
        z = z + ri * coef[k];
    }
    return z;
}

static __device__ __forceinline__ void ocam_project_one(const egotap_ocam& m, double x, double y, double z, double& u, double& v) {
#pragma clang fp contract(off)
    const bool flip = m.ue_flip != 0.0;
    if (flip) {
        y = y * -1.0;
        z = z * -1.0;
    }
    const double norm = sqrt(x * x + y * y);
    if (norm <= 1e-8) {                                      // isclose(norm, 0); a NaN norm takes the other branch, as in the reference
        u = m.xc;
        v = m.yc;
    } else {
        const double theta = atan(z / norm), invnorm = 1.0 / norm;
        const double rho = ocam_poly(m.invpol, m.n_invpol, theta);
        const double xs = x * invnorm * rho, ys = y * invnorm * rho;
        u = xs * m.c + ys * m.d + m.xc;
        v = xs * m.e + ys + m.yc;
    }
    if (flip) v = m.yc * 2.0 - v;
}

// CLAMP: the model was read from device memory the library cannot inspect (a rig table): n_pol is held to the array's length, so whatever the table
// holds no load leaves the model.  A model passed by value was checked on the host and is read as it stands.
template <bool CLAMP = false>
static __device__ __forceinline__ void ocam_unproject_one(const egotap_ocam& m, double u, double v, double (&ray)[3]) {
#pragma clang fp contract(off)
    const bool flip = m.ue_flip != 0.0;
    if (flip) v = m.yc * 2.0 - v;
    const double invdet = 1.0 / (m.c - m.d * m.e);
    const double du = u - m.xc, dv = v - m.yc;
    const double xp = invdet * (du - m.d * dv);
    const double yp = invdet * (-m.e * du + m.c * dv);
    const double r = sqrt(xp * xp + yp * yp);
    const double zp = ocam_poly(m.pol, CLAMP && m.n_pol > EGOTAP_OCAM_MAX_POL ? EGOTAP_OCAM_MAX_POL : m.n_pol, r);
    const double invnorm = 1.0 / sqrt(xp * xp + yp * yp + zp * zp);
    ray[0] = invnorm * xp;
    ray[1] = invnorm * yp;
    ray[2] = invnorm * zp;
    if (flip) {
        ray[1] = ray[1] * -1.0;
        ray[2] = ray[2] * -1.0;
    }
}

static __global__ __launch_bounds__(256) void ocam_project_kernel(const float* __restrict__ p3, int N, egotap_ocam m, float* __restrict__ p2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double u, v;
    ocam_project_one(m, (double)p3[3 * i], (double)p3[3 * i + 1], (double)p3[3 * i + 2], u, v);
    p2[2 * i] = (float)u;
    p2[2 * i + 1] = (float)v;
}

static __global__ __launch_bounds__(256) void ocam_unproject_kernel(const float* __restrict__ p2, int N, egotap_ocam m, float* __restrict__ rays) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    double ray[3];
    ocam_unproject_one(m, (double)p2[2 * i], (double)p2[2 * i + 1], ray);
    rays[3 * i] = (float)ray[0];
    rays[3 * i + 1] = (float)ray[1];
    rays[3 * i + 2] = (float)ray[2];
}

static __device__ __forceinline__ double stereo_dot(const double (&p)[3], const double (&q)[3]) {
#pragma clang fp contract(off)
    return p[0] * q[0] + p[1] * q[1] + p[2] * q[2];
}
static __device__ __forceinline__ bool stereo_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-inf

// The kernel's body, shared by the two places a rig comes from.  TABLE false: `rig` is the kernel's by-value argument.  TABLE true: `rig` is one row of
// a table in device memory, picked by a wave-uniform index -- plain uniform loads of doubles, and the polynomial lengths clamped.  Where a value of the
// rig was loaded from does not enter the arithmetic: both kernels return the same bits for the same rig.
template <bool TABLE>
static __device__ __forceinline__ void stereo_triangulate_body(const float* __restrict__ kp, int B, int J, const StereoRig& rig, const float* __restrict__ pose,
                                                               int P, int row0, float* __restrict__ joints3d, float* __restrict__ frame) {
#pragma clang fp contract(off)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    __shared__ double sj[kStereoFramesPerBlock][kStereoMaxJoints][8];      // per joint: valid, X (3), pose row (3), gap
    __shared__ double sd[kStereoFramesPerBlock][kStereoMaxJoints];         // per joint: disagree
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * kStereoFramesPerBlock + wave;
    const bool live = f < B && lane < J;                     // no wave leaves early: the two barriers below are the workgroup's
    double X[3] = {0.0, 0.0, 0.0}, q[3] = {0.0, 0.0, 0.0}, gap = 0.0, den = 0.0, s = 0.0;
    bool valid = false;
    if (live) {
        const f32x4v kl = *(const f32x4v*)(kp + ((f * 2 + 0) * J + lane) * 4);
        const f32x4v kr = *(const f32x4v*)(kp + ((f * 2 + 1) * J + lane) * 4);
        const double xl = kl[0], yl = kl[1], xr = kr[0], yr = kr[1];
        const bool seen = (double)kl[2] >= rig.min_score && (double)kr[2] >= rig.min_score && stereo_finite(xl) && stereo_finite(yl) && stereo_finite(xr) &&
                          stereo_finite(yr);
        double dL[3], r[3], dR[3], w0[3];
        ocam_unproject_one<TABLE>(rig.cam[0], rig.aff[0][0] * xl + rig.aff[0][1], rig.aff[0][2] * yl + rig.aff[0][3], dL);
        ocam_unproject_one<TABLE>(rig.cam[1], rig.aff[1][0] * xr + rig.aff[1][1], rig.aff[1][2] * yr + rig.aff[1][3], r);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            dR[k] = rig.R[3 * k] * r[0] + rig.R[3 * k + 1] * r[1] + rig.R[3 * k + 2] * r[2];
            w0[k] = -rig.t[k];
        }
        const double b = stereo_dot(dL, dR), d = stereo_dot(dL, w0), e = stereo_dot(dR, w0);
        den = 1.0 - b * b;
        s = (b * e - d) / den;
        const double u = (e - b * d) / den;
        double df[3];
        bool fin = stereo_finite(den) && stereo_finite(s) && stereo_finite(u);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double pl = s * dL[k], pr = rig.t[k] + u * dR[k];
            X[k] = (pl + pr) * 0.5;
            df[k] = pl - pr;
            fin = fin && stereo_finite(X[k]);
        }
        gap = sqrt(df[0] * df[0] + df[1] * df[1] + df[2] * df[2]);
        valid = seen && den > 0.0 && s > 0.0 && u > 0.0 && fin && stereo_finite(gap);
        if (pose) {
            const float* pr = pose + (f * P + row0 + lane) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                q[k] = (double)pr[k];
                valid = valid && stereo_finite(q[k]);
            }
        }
    }
    double(*mine)[8] = sj[wave];
    mine[lane][0] = valid ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        mine[lane][1 + k] = X[k];
        mine[lane][4 + k] = q[k];
    }
    mine[lane][7] = gap;
    __syncthreads();
    // the frame's sums, by every lane for itself, in ascending joint order
    double n = 0.0, sx[3] = {0.0, 0.0, 0.0}, sp[3] = {0.0, 0.0, 0.0};
    for (int j = 0; j < J; ++j) {
        if (mine[j][0] != 0.0) {                             // (the same for all lanes of the wave)
            n = n + 1.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                sx[k] = sx[k] + mine[j][1 + k];
                sp[k] = sp[k] + mine[j][4 + k];
            }
        }
    }
    const double nn = n > 0.0 ? n : 1.0;
    double that[3] = {0.0, 0.0, 0.0}, dis = 0.0;
    if (pose) {
        double g[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            that[k] = sx[k] / nn - sp[k] / nn;
            g[k] = X[k] - q[k] - that[k];
        }
        dis = sqrt(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    }
    sd[wave][lane] = dis;
    __syncthreads();
    if (live) {
        f32x4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
        if (valid) {
            lo[0] = (float)X[0];
            lo[1] = (float)X[1];
            lo[2] = (float)X[2];
            lo[3] = (float)gap;
            hi[0] = (float)den;
            hi[1] = (float)s;
            hi[2] = (float)dis;
            hi[3] = 1.f;
        }
        float* out = joints3d + (f * J + lane) * 8;
        *(f32x4v*)out = lo;
        *(f32x4v*)(out + 4) = hi;
    }
    if (lane != 0 || f >= B) return;
    double s2d = 0.0, s2g = 0.0, mxd = 0.0, mxg = 0.0;
    for (int j = 0; j < J; ++j) {
        if (mine[j][0] != 0.0) {
            const double dj = sd[wave][j], gj = mine[j][7];
            s2d = s2d + dj * dj;
            s2g = s2g + gj * gj;
            if (dj > mxd) mxd = dj;
            if (gj > mxg) mxg = gj;
        }
    }
    f32x4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (n > 0.0) {
        lo[0] = (float)that[0];
        lo[1] = (float)that[1];
        lo[2] = (float)that[2];
        lo[3] = (float)n;
        hi[0] = (float)sqrt(s2d / nn);
        hi[1] = (float)mxd;
        hi[2] = (float)sqrt(s2g / nn);
        hi[3] = (float)mxg;
    }
    float* out = frame + f * 8;
    *(f32x4v*)out = lo;
    *(f32x4v*)(out + 4) = hi;
}

static __global__ __launch_bounds__(256) void stereo_triangulate_kernel(const float* __restrict__ kp, int B, int J, StereoRig rig, const float* __restrict__ pose,
                                                                       int P, int row0, float* __restrict__ joints3d, float* __restrict__ frame) {
    stereo_triangulate_body<false>(kp, B, J, rig, pose, P, row0, joints3d, frame);
}

// the rig of a wave's frame in a table of S rigs (frame b uses rig b % S; time-major batches, b = t * S + s): the index made uniform, so the rig's
// values are fetched once per wave.  A wave past the batch still picks a row inside the table.
static __device__ __forceinline__ const StereoRig& stereo_stream_rig(const StereoRig* __restrict__ rigs, int S) {
    const unsigned f = blockIdx.x * (unsigned)kStereoFramesPerBlock + (threadIdx.x >> 6);
    return rigs[__builtin_amdgcn_readfirstlane((int)(f % (unsigned)S))];
}

static __global__ __launch_bounds__(256) void stereo_triangulate_streams_kernel(const float* __restrict__ kp, int B, int J, const StereoRig* __restrict__ rigs, int S,
                                                                               const float* __restrict__ pose, int P, int row0, float* __restrict__ joints3d,
                                                                               float* __restrict__ frame) {
    stereo_triangulate_body<true>(kp, B, J, stereo_stream_rig(rigs, S), pose, P, row0, joints3d, frame);
}

// N > 0 and the pointers checked by the caller.
static inline hipError_t ocam_project_launch(const float* p3, int N, const egotap_ocam& m, float* p2, hipStream_t s) {
    if (N <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ocam_project_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, p3, N, m, p2);
    return hipGetLastError();
}
static inline hipError_t ocam_unproject_launch(const float* p2, int N, const egotap_ocam& m, float* rays, hipStream_t s) {
    if (N <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ocam_unproject_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, p2, N, m, rays);
    return hipGetLastError();
}
// keypoints, joints3d, frame 16-byte aligned, 1 <= J <= kStereoMaxJoints, pose == NULL or 0 <= row0 and row0 + J <= P: checked by the caller.
static inline hipError_t stereo_triangulate_launch(const float* kp, int B, int J, const StereoRig& rig, const float* pose, int P, int row0, float* joints3d,
                                                   float* frame, hipStream_t s) {
    if (B <= 0 || J <= 0 || J > kStereoMaxJoints || (pose && (row0 < 0 || row0 + J > P))) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)B + kStereoFramesPerBlock - 1) / kStereoFramesPerBlock);
    hipLaunchKernelGGL(stereo_triangulate_kernel, dim3(blocks), dim3(64 * kStereoFramesPerBlock), 0, s, kp, B, J, rig, pose, P, row0, joints3d, frame);
    return hipGetLastError();
}
// the same with a table of S rigs in device memory (8-byte aligned, S >= 1, B a multiple of S: checked by the caller)
static inline hipError_t stereo_triangulate_streams_launch(const float* kp, int B, int J, const StereoRig* rigs, int S, const float* pose, int P, int row0,
                                                           float* joints3d, float* frame, hipStream_t s) {
    if (B <= 0 || J <= 0 || J > kStereoMaxJoints || (pose && (row0 < 0 || row0 + J > P)) || !rigs || S < 1 || B % S != 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)B + kStereoFramesPerBlock - 1) / kStereoFramesPerBlock);
    hipLaunchKernelGGL(stereo_triangulate_streams_kernel, dim3(blocks), dim3(64 * kStereoFramesPerBlock), 0, s, kp, B, J, rigs, S, pose, P, row0, joints3d, frame);
    return hipGetLastError();
}
