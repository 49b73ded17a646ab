// The lifted joints fused with the keypoint rays (egotap.h egotap_stereo_fuse, spec.py stereo_fuse_ref): one launch, float64 inside, fp32 in and out, every
// output rounded once.
//   stereo_fuse_kernel  keypoints [B, 2, J, 4] + pose [B, P, 3] + frame [B, 8] -> fused [B, J, 8] + pose_fused [B, P, 3] + stats [B, 8]: stereo_triangulate_kernel's
//       shape, one WAVE per frame, lane = joint (J <= 64), four frames per workgroup.  Each lane places its prior, unprojects its joint through both
//       cameras (ocam.h ocam_unproject_one), gates each eye, solves the 3 x 3 system by LDL^T, checks the fit and leaves (mode, move, res left, res right) in
//       LDS; after the workgroup's one barrier lane 0 adds the frame's statistics from LDS in ASCENDING joint order, so the host restatement, which adds in
//       that order, gets the same bits.  Lane = joint writes its record as two 16-byte stores and its pose_fused row; the wave copies the rows outside the
//       joint rows.  pose_fused may be pose: every element is read and written by the same thread, and neither pointer is __restrict__.
//   stereo_fuse_streams_kernel  the same body with a rig per stream: frame b reads rig b % S of a table in device memory (ocam.h
//       stereo_triangulate_streams_kernel); the parameters stay by value, one set for all streams.
// The rig and the parameters travel by value in the kernel arguments (uniform indices: scalar loads).  Contraction is off in every function here: the
// definition keeps products and sums apart.  sqrt and the divisions are correctly rounded; the six divisions of the solve form two short chains
// (l10, l20 | D1 -> l21 -> D2 -> y2), latency the one wave per frame cannot hide and does not need to: a call is a few KB of work.
#pragma once
#include "ocam.h"

struct FuseEye {
    bool used;
    double d[3], w, sr;
};

// one eye against the prior x0: the gate, the weight and the eye's mode bits (shift 0: left, 1: right)
static __device__ __forceinline__ int fuse_gate_eye(bool seen, double score, const double (&d)[3], const double (&o)[3], const double (&x0)[3],
                                                    const egotap_fuse_params& prm, int shift, FuseEye& eye) {
#pragma clang fp contract(off)
    double y0[3], r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) y0[k] = x0[k] - o[k];
    const double a = stereo_dot(d, y0), rho = sqrt(stereo_dot(y0, y0));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r[k] = y0[k] - a * d[k];
        eye.d[k] = d[k];
    }
    const double sr = prm.sigma_ray * rho, sr2 = sr * sr;
    const double g = sqrt(stereo_dot(r, r)) / sqrt(sr2 + prm.sigma_prior * prm.sigma_prior);
    eye.sr = sr;
    eye.w = score / sr2;
    eye.used = false;
    if (!seen) return 0;
    if (!(a > 0.0) || !stereo_finite(g)) return 32 << shift;
    if (!(g <= prm.max_sigma)) return 8 << shift;
    eye.used = true;
    return 2 << shift;
}

// a used eye's I - d d^T, weighted, into the upper triangle A = (A00, A01, A02, A11, A12, A22); the right eye's origin into b
static __device__ __forceinline__ void fuse_add_eye(const FuseEye& eye, const double* o, double (&A)[6], double (&b)[3]) {
#pragma clang fp contract(off)
    const double(&d)[3] = eye.d;
    const double m00 = 1.0 - d[0] * d[0], m01 = -(d[0] * d[1]), m02 = -(d[0] * d[2]), m11 = 1.0 - d[1] * d[1], m12 = -(d[1] * d[2]), m22 = 1.0 - d[2] * d[2];
    A[0] = A[0] + eye.w * m00;
    A[1] = A[1] + eye.w * m01;
    A[2] = A[2] + eye.w * m02;
    A[3] = A[3] + eye.w * m11;
    A[4] = A[4] + eye.w * m12;
    A[5] = A[5] + eye.w * m22;
    if (o) {
        b[0] = b[0] + eye.w * ((m00 * o[0] + m01 * o[1]) + m02 * o[2]);
        b[1] = b[1] + eye.w * ((m01 * o[0] + m11 * o[1]) + m12 * o[2]);
        b[2] = b[2] + eye.w * ((m02 * o[0] + m12 * o[1]) + m22 * o[2]);
    }
}

// a used eye against the fit: its residual in standard deviations, and whether it passes
static __device__ __forceinline__ bool fuse_check_eye(const FuseEye& eye, const double (&o)[3], const double (&x)[3], double max_sigma, double& res) {
#pragma clang fp contract(off)
    double v[3], p[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = x[k] - o[k];
    const double c = stereo_dot(v, eye.d);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = v[k] - c * eye.d[k];
    res = sqrt(stereo_dot(p, p)) / eye.sr;
    return res <= max_sigma && c > 0.0;
}

// the kernel's body, shared by the two places a rig comes from (ocam.h stereo_triangulate_body: TABLE false the by-value argument, true a row of a table)
template <bool TABLE>
static __device__ __forceinline__ void stereo_fuse_body(const float* __restrict__ kp, int B, int J, const StereoRig& rig, const float* pose, int P, int row0,
                                                        const float* __restrict__ frame, const egotap_fuse_params& prm, float* __restrict__ fused, float* pose_fused,
                                                        float* __restrict__ stats) {
#pragma clang fp contract(off)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    __shared__ double sj[kStereoFramesPerBlock][kStereoMaxJoints][4];      // per joint: mode, move, res left, res right
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long f = (long)blockIdx.x * kStereoFramesPerBlock + wave;
    const bool live = f < B && lane < J;                     // no wave leaves early: the barrier below is the workgroup's
    int mode = 0;
    double x[3] = {0.0, 0.0, 0.0}, move = 0.0, res[2] = {0.0, 0.0}, share = 0.0;
    if (f < B) {                                             // the rows outside the joint rows: the input's bits
        const float* src = pose + f * P * 3;
        float* dst = pose_fused + f * P * 3;
        for (int r = lane; r < P; r += 64) {
            if (r >= row0 && r < row0 + J) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[3 * r + k] = src[3 * r + k];
        }
    }
    if (live) {
        const f32x4v fr = *(const f32x4v*)(frame + f * 8);  // (the same address for the wave's lanes)
        const double that[3] = {(double)fr[0], (double)fr[1], (double)fr[2]};
        const bool root_ok = (double)fr[3] >= (double)prm.min_joints && stereo_finite(that[0]) && stereo_finite(that[1]) && stereo_finite(that[2]);
        const float* qr = pose + (f * P + row0 + lane) * 3;
        const float q32[3] = {qr[0], qr[1], qr[2]};
        const double q[3] = {(double)q32[0], (double)q32[1], (double)q32[2]};
        float out_row[3] = {q32[0], q32[1], q32[2]};
        if (root_ok && stereo_finite(q[0]) && stereo_finite(q[1]) && stereo_finite(q[2])) {
            mode = 1;
            const f32x4v kl = *(const f32x4v*)(kp + ((f * 2 + 0) * J + lane) * 4);
            const f32x4v kr = *(const f32x4v*)(kp + ((f * 2 + 1) * J + lane) * 4);
            const double xl = kl[0], yl = kl[1], xr = kr[0], yr = kr[1];
            const bool seenL = (double)kl[2] >= rig.min_score && stereo_finite(xl) && stereo_finite(yl);
            const bool seenR = (double)kr[2] >= rig.min_score && stereo_finite(xr) && stereo_finite(yr);
            double dL[3], r[3], dR[3], x0[3];
            ocam_unproject_one<TABLE>(rig.cam[0], rig.aff[0][0] * xl + rig.aff[0][1], rig.aff[0][2] * yl + rig.aff[0][3], dL);
            ocam_unproject_one<TABLE>(rig.cam[1], rig.aff[1][0] * xr + rig.aff[1][1], rig.aff[1][2] * yr + rig.aff[1][3], r);
            const double zero[3] = {0.0, 0.0, 0.0}, wp = 1.0 / (prm.sigma_prior * prm.sigma_prior);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                dR[k] = rig.R[3 * k] * r[0] + rig.R[3 * k + 1] * r[1] + rig.R[3 * k + 2] * r[2];
                x0[k] = q[k] + that[k];
                x[k] = x0[k];
            }
            FuseEye eL, eR;
            mode |= fuse_gate_eye(seenL, (double)kl[2], dL, zero, x0, prm, 0, eL);
            mode |= fuse_gate_eye(seenR, (double)kr[2], dR, rig.t, x0, prm, 1, eR);
            if (eL.used || eR.used) {
                double A[6] = {wp, 0.0, 0.0, wp, 0.0, wp}, b[3] = {wp * x0[0], wp * x0[1], wp * x0[2]}, sw = 0.0;
                if (eL.used) {
                    fuse_add_eye(eL, nullptr, A, b);
                    sw = sw + eL.w;
                }
                if (eR.used) {
                    fuse_add_eye(eR, rig.t, A, b);
                    sw = sw + eR.w;
                }
                const double l10 = A[1] / A[0], l20 = A[2] / A[0];
                const double D1 = A[3] - l10 * A[1], c21 = A[4] - l20 * A[1];
                const double l21 = c21 / D1;
                const double D2 = (A[5] - l20 * A[2]) - l21 * c21;
                const double z1 = b[1] - l10 * b[0], z2 = (b[2] - l20 * b[0]) - l21 * z1;
                const double y0 = b[0] / A[0], y1 = z1 / D1, y2 = z2 / D2;
                double xs[3];
                xs[2] = y2;
                xs[1] = y1 - l21 * xs[2];
                xs[0] = (y0 - l10 * xs[1]) - l20 * xs[2];
                bool keep = stereo_finite(xs[0]) && stereo_finite(xs[1]) && stereo_finite(xs[2]);
                double rs[2] = {0.0, 0.0};
                if (eL.used) keep = fuse_check_eye(eL, zero, xs, prm.max_sigma, rs[0]) && keep;
                if (eR.used) keep = fuse_check_eye(eR, rig.t, xs, prm.max_sigma, rs[1]) && keep;
                res[0] = stereo_finite(rs[0]) ? rs[0] : 0.0;
                res[1] = stereo_finite(rs[1]) ? rs[1] : 0.0;
                if (keep) {
                    double dx[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        x[k] = xs[k];
                        dx[k] = xs[k] - x0[k];
                        out_row[k] = (float)(xs[k] - that[k]);
                    }
                    move = sqrt(stereo_dot(dx, dx));
                    share = sw / (wp + sw);
                } else {
                    mode |= 128;
                }
            }
        }
        float* pr = pose_fused + (f * P + row0 + lane) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) pr[k] = out_row[k];
        f32x4v lo = {(float)x[0], (float)x[1], (float)x[2], (float)move}, hi = {(float)res[0], (float)res[1], (float)share, (float)mode};
        float* out = fused + (f * J + lane) * 8;
        *(f32x4v*)out = lo;
        *(f32x4v*)(out + 4) = hi;
    }
    double(*mine)[4] = sj[wave];
    mine[lane][0] = (double)mode;
    mine[lane][1] = move;
    mine[lane][2] = res[0];
    mine[lane][3] = res[1];
    __syncthreads();
    if (lane != 0 || f >= B) return;
    // the frame's statistics, in ascending joint order, left before right
    double n_prior = 0.0, n_both = 0.0, n_one = 0.0, n_rej = 0.0, n_res = 0.0, s2m = 0.0, mxm = 0.0, s2r = 0.0, mxr = 0.0;
    for (int j = 0; j < J; ++j) {
        const int m = (int)mine[j][0];
        if (!(m & 1)) continue;
        n_prior = n_prior + 1.0;
        const double mv = mine[j][1];
        s2m = s2m + mv * mv;
        if (mv > mxm) mxm = mv;
        const int tried = ((m >> 1) & 1) + ((m >> 2) & 1);
        n_rej = n_rej + (double)(((m >> 3) & 1) + ((m >> 4) & 1) + ((m >> 5) & 1) + ((m >> 6) & 1));
        if (m & 128) {
            n_rej = n_rej + (double)tried;
            continue;
        }
        if (tried == 2) n_both = n_both + 1.0;
        if (tried == 1) n_one = n_one + 1.0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!(m & (2 << e))) continue;
            const double rv = mine[j][2 + e];
            n_res = n_res + 1.0;
            s2r = s2r + rv * rv;
            if (rv > mxr) mxr = rv;
        }
    }
    f32x4v lo = {(float)n_prior, (float)n_both, (float)n_one, (float)n_rej}, hi = {0.f, 0.f, 0.f, 0.f};
    if (n_prior > 0.0) {
        hi[0] = (float)sqrt(s2m / n_prior);
        hi[1] = (float)mxm;
    }
    if (n_res > 0.0) {
        hi[2] = (float)sqrt(s2r / n_res);
        hi[3] = (float)mxr;
    }
    float* out = stats + f * 8;
    *(f32x4v*)out = lo;
    *(f32x4v*)(out + 4) = hi;
}

static __global__ __launch_bounds__(256) void stereo_fuse_kernel(const float* __restrict__ kp, int B, int J, StereoRig rig, const float* pose, int P, int row0,
                                                                const float* __restrict__ frame, egotap_fuse_params prm, float* __restrict__ fused, float* pose_fused,
                                                                float* __restrict__ stats) {
    stereo_fuse_body<false>(kp, B, J, rig, pose, P, row0, frame, prm, fused, pose_fused, stats);
}

// frame b fused with rig b % S of a table in device memory (ocam.h stereo_stream_rig); one set of parameters serves all streams
static __global__ __launch_bounds__(256) void stereo_fuse_streams_kernel(const float* __restrict__ kp, int B, int J, const StereoRig* __restrict__ rigs, int S,
                                                                        const float* pose, int P, int row0, const float* __restrict__ frame, egotap_fuse_params prm,
                                                                        float* __restrict__ fused, float* pose_fused, float* __restrict__ stats) {
    stereo_fuse_body<true>(kp, B, J, stereo_stream_rig(rigs, S), pose, P, row0, frame, prm, fused, pose_fused, stats);
}

// keypoints, frame, fused, stats 16-byte aligned, 1 <= J <= kStereoMaxJoints, 0 <= row0 and row0 + J <= P: checked by the caller.
static inline hipError_t stereo_fuse_launch(const float* kp, int B, int J, const StereoRig& rig, const float* pose, int P, int row0, const float* frame,
                                            const egotap_fuse_params& prm, float* fused, float* pose_fused, float* stats, hipStream_t s) {
    if (B <= 0 || J <= 0 || J > kStereoMaxJoints || row0 < 0 || row0 + J > P) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)B + kStereoFramesPerBlock - 1) / kStereoFramesPerBlock);
    hipLaunchKernelGGL(stereo_fuse_kernel, dim3(blocks), dim3(64 * kStereoFramesPerBlock), 0, s, kp, B, J, rig, pose, P, row0, frame, prm, fused, pose_fused, stats);
    return hipGetLastError();
}
// the same with a table of S rigs in device memory (8-byte aligned, S >= 1, B a multiple of S: checked by the caller)
static inline hipError_t stereo_fuse_streams_launch(const float* kp, int B, int J, const StereoRig* rigs, int S, const float* pose, int P, int row0, const float* frame,
                                                    const egotap_fuse_params& prm, float* fused, float* pose_fused, float* stats, hipStream_t s) {
    if (B <= 0 || J <= 0 || J > kStereoMaxJoints || row0 < 0 || row0 + J > P || !rigs || S < 1 || B % S != 0) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)B + kStereoFramesPerBlock - 1) / kStereoFramesPerBlock);
    hipLaunchKernelGGL(stereo_fuse_streams_kernel, dim3(blocks), dim3(64 * kStereoFramesPerBlock), 0, s, kp, B, J, rigs, S, pose, P, row0, frame, prm, fused,
                       pose_fused, stats);
    return hipGetLastError();
}
