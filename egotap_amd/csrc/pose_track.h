// The temporal filter of the serving outputs: a One-Euro filter (Casiez et al. 2012) on 3-vectors, a missing sample taken as irregular sampling
// (egotap.h egotap_pose_track; spec.py pose_track_ref restates it in float64 numpy, operation for operation).
//   pose_track_kernel  T frames of S streams, time-major (frame b = t * S + s): one WAVE per stream, four streams per workgroup.  A stream has
//       K = P + 1 + J tracks (pose rows, the root, the triangulated joints); lane l owns tracks l, l + 64 and l + 128 (P, J <= 64: K <= 129).  The
//       state (12 doubles per track) is read once before the loop over the T steps, lives in registers, and is written once after it.  Tracks are
//       independent but for the root's x^, which `placed` adds to every pose row: EVERY lane runs the root track for itself from the frame record
//       (a uniform address), so all lanes hold the same bits and the lane that owns track P writes them.  Step t + 1's measurements are requested
//       before step t's arithmetic.  No LDS, no barrier, no atomics, no workspace; plain vector stores, the 32-byte track records as two 16-byte ones.
//       A wave whose stream lies past S loads and stores nothing.
//   pose_track_world_kernel  the same walk in a WORLD frame (egotap.h egotap_pose_track_world; spec.py pose_track_world_ref): each step carries the
//       left camera's pose in the world, 12 doubles (R | t) that every lane reads from the same address (why not into SGPRs: at the kernel).  A rig
//       pose that is finite, orthonormal within ortho_tol and right-handed moves the step's measurements into the world before track_step (points
//       R m + t, the pose rows R m); any other one accepts no track, so the step is a missing sample.  placed_world as placed; placed_cam the same
//       float64 value brought back through this step's rig pose.  A sibling of pose_track_kernel, whose text and code stay as they are.
// Bound by LATENCY, not by any rate: per step a serial chain of float64 divisions (dx / te, two alphas) and a square root per track, on a few KB of
// data; a call of T steps costs T times that chain whatever S is, up to 4 streams per workgroup and one workgroup per CU.
// Compiler's resource summary for gfx950 (-Rpass-analysis=kernel-resource-usage): see the numbers at the kernel.
// Contraction is off in every function here: the definition keeps products and sums apart.  sqrt and the divisions are correctly rounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "egotap.h"

constexpr int kTrackMaxRows = 64;             // P and J: one lane each
constexpr int kTrackStreamsPerBlock = 4;
constexpr int kTrackState = 12;               // x^ (3), v^ (3), m_prev (3), gap_t, age, live

struct TrackState {
    double x[3], v[3], mp[3], gap_t, age, live;
};
struct TrackClass {
    double min_cutoff, beta, d_cutoff;
};
// one step's measurement of one track as it lies in memory: (m, the joint's gap, the joint's valid flag); a pose row has gap 0 and valid 1
struct TrackRaw {
    float m[3], gap, valid;
};

static __device__ __forceinline__ bool track_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }      // false for NaN and +-inf
static __device__ __forceinline__ double track_alpha(double fc, double te) {
#pragma clang fp contract(off)
    const double r = (6.283185307179586 * fc) * te;
    return r / (r + 1.0);
}

// one step of one track (egotap.h); returns the status, sets the cutoff.  m is read only where a is set.
static __device__ __forceinline__ int track_step(TrackState& s, const double (&m)[3], bool a, double dt, bool ok, const TrackClass& c, double max_hold,
                                                 double& cutoff) {
#pragma clang fp contract(off)
    cutoff = 0.0;
    if (s.live == 0.0) {
        if (!a) return 0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.x[k] = m[k];
            s.mp[k] = m[k];
            s.v[k] = 0.0;
        }
        s.gap_t = 0.0;
        s.age = 0.0;
        s.live = 1.0;
        cutoff = c.min_cutoff;
        return 1;
    }
    if (a && ok) {
        const double te = s.gap_t + dt, ad = track_alpha(c.d_cutoff, te);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double dx = (m[k] - s.mp[k]) / te;
            s.v[k] = s.v[k] + ad * (dx - s.v[k]);
        }
        const double speed = sqrt(s.v[0] * s.v[0] + s.v[1] * s.v[1] + s.v[2] * s.v[2]);
        const double fc = c.min_cutoff + c.beta * speed, ax = track_alpha(fc, te);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s.x[k] = s.x[k] + ax * (m[k] - s.x[k]);
            s.mp[k] = m[k];
        }
        s.gap_t = 0.0;
        s.age = 0.0;
        cutoff = fc;
        return 1;
    }
    s.age = s.age + 1.0;
    if (ok) s.gap_t = s.gap_t + dt;
    if (s.age > max_hold) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.x[k] = s.v[k] = s.mp[k] = 0.0;
        s.gap_t = s.age = s.live = 0.0;
        return 0;
    }
    return 2;
}

static __device__ __forceinline__ void track_load(TrackState& s, const double* p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s.x[k] = p[k];
        s.v[k] = p[3 + k];
        s.mp[k] = p[6 + k];
    }
    s.gap_t = p[9];
    s.age = p[10];
    s.live = p[11];
}
static __device__ __forceinline__ void track_store(const TrackState& s, double* p) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        p[k] = s.x[k];
        p[3 + k] = s.v[k];
        p[6 + k] = s.mp[k];
    }
    p[9] = s.gap_t;
    p[10] = s.age;
    p[11] = s.live;
}
// the record of one track at one step: (x^, v^, cutoff, status), each rounded once; status 0 is all zeros
static __device__ __forceinline__ void track_record(const TrackState& s, int status, double cutoff, float* out) {
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    f32x4v lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
    if (status != 0) {
        lo[0] = (float)s.x[0];
        lo[1] = (float)s.x[1];
        lo[2] = (float)s.x[2];
        lo[3] = (float)s.v[0];
        hi[0] = (float)s.v[1];
        hi[1] = (float)s.v[2];
        hi[2] = (float)cutoff;
        hi[3] = (float)status;
    }
    *(f32x4v*)out = lo;
    *(f32x4v*)(out + 4) = hi;
}

// ---- the world frame: one step's rig pose g = the row-major 3 x 4 (R | t) of the left camera in the world, x_w = R x_c + t; wave-uniform
// finite, every |E_ij| <= tol with E = R R^T - 1 (symmetric in bits: six entries), det R > 0 by cofactors along row 0; every comparison false on a NaN
static __device__ __forceinline__ bool rig_seen(const double (&g)[12], double tol) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 12; ++k) ok = ok && track_finite(g[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double e = ((g[4 * i] * g[4 * j] + g[4 * i + 1] * g[4 * j + 1]) + g[4 * i + 2] * g[4 * j + 2]) - (i == j ? 1.0 : 0.0);
            ok = ok && fabs(e) <= tol;
        }
    const double c0 = g[5] * g[10] - g[6] * g[9], c1 = g[4] * g[10] - g[6] * g[8], c2 = g[4] * g[9] - g[5] * g[8];
    const double det = (g[0] * c0 - g[1] * c1) + g[2] * c2;
    return ok && det > 0.0;
}
// a camera-frame measurement in the world: a point gets R m + t, a pelvis-relative offset (a pose row) R m
static __device__ __forceinline__ void rig_to_world(const double (&g)[12], const double (&m)[3], bool point, double (&w)[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double rot = (g[4 * r] * m[0] + g[4 * r + 1] * m[1]) + g[4 * r + 2] * m[2];
        w[r] = point ? rot + g[4 * r + 3] : rot;
    }
}
// a world value back in this step's camera: R^T (p - t) for a point, R^T p for an offset
static __device__ __forceinline__ void rig_to_camera(const double (&g)[12], const double (&p)[3], bool point, double (&o)[3]) {
#pragma clang fp contract(off)
    double d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = point ? p[r] - g[4 * r + 3] : p[r];
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (g[c] * d[0] + g[4 + c] * d[1]) + g[8 + c] * d[2];
}

// gfx950, -O3: 220 VGPRs (four track states of 12 doubles and the next step's measurements), 0 AGPRs, 96 SGPRs, scratch 0 bytes, no spills, LDS 0
// bytes, 2 waves per SIMD (a workgroup puts one on each).
// state_in and state_out may be the same array (each lane reads its tracks before the loop and writes them after it): not __restrict__.
static __global__ __launch_bounds__(64 * kTrackStreamsPerBlock) void pose_track_kernel(const float* __restrict__ pose, const float* __restrict__ frame,
                                                                                       const float* __restrict__ joints3d, int T, int S, int P, int J,
                                                                                       const float* __restrict__ dts, double dt_host, egotap_track_params prm,
                                                                                       const double* state_in, double* state_out, float* __restrict__ tracks,
                                                                                       float* __restrict__ placed) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long s = (long)blockIdx.x * kTrackStreamsPerBlock + wave;
    if (s >= S) return;                                      // (no barrier anywhere: a wave may leave)
    const int K = P + 1 + J;
    const TrackClass cls_pose = {prm.pose_min_cutoff, prm.pose_beta, prm.pose_d_cutoff}, cls_root = {prm.root_min_cutoff, prm.root_beta, prm.root_d_cutoff},
                     cls_joint = {prm.joints_min_cutoff, prm.joints_beta, prm.joints_d_cutoff};
    const double max_hold = (double)prm.max_hold, min_joints = (double)prm.min_joints;
    // slot i of this lane is track lane + 64 i; the root (track P) is run by every lane below and skipped as a slot
    bool on[3], is_pose[3];
    TrackState st[3], root;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = lane + 64 * i;
        on[i] = k < K && k != P;
        is_pose[i] = k < P;
        st[i] = TrackState{};
        if (on[i]) track_load(st[i], state_in + (s * K + k) * kTrackState);
    }
    track_load(root, state_in + (s * K + P) * kTrackState);
    const bool owns_root = lane == (P & 63);

    TrackRaw nxt[3] = {};
    float nfr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ndt = 0.f;
    auto fetch = [&](int t) {
        const long b = (long)t * S + s;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!on[i]) continue;
            const int k = lane + 64 * i;
            if (is_pose[i]) {
                const float* p = pose + (b * P + k) * 3;
                nxt[i].m[0] = p[0];
                nxt[i].m[1] = p[1];
                nxt[i].m[2] = p[2];
                nxt[i].gap = 0.f;
                nxt[i].valid = 1.f;
            } else {
                const float* q = joints3d + (b * J + (k - P - 1)) * 8;
                nxt[i].m[0] = q[0];
                nxt[i].m[1] = q[1];
                nxt[i].m[2] = q[2];
                nxt[i].gap = q[3];
                nxt[i].valid = q[7];
            }
        }
        if (frame) {
            const float* f = frame + b * 8;
            nfr[0] = f[0];
            nfr[1] = f[1];
            nfr[2] = f[2];
            nfr[3] = f[3];
            nfr[4] = f[4];
            nfr[5] = f[6];
        }
        if (dts) ndt = dts[t];
    };
    fetch(0);
    for (int t = 0; t < T; ++t) {
        TrackRaw cur[3];
        float fr[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) cur[i] = nxt[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) fr[i] = nfr[i];
        const double dt = dts ? (double)ndt : dt_host;
        if (t + 1 < T) fetch(t + 1);                         // the next step's measurements travel during this step's chain
        const bool ok = track_finite(dt) && dt > 0.0;
        const long b = (long)t * S + s;
        // the root, by every lane for itself: (t^, n, rms disagree, rms gap) of the frame record
        const double mr[3] = {(double)fr[0], (double)fr[1], (double)fr[2]};
        const bool ar = frame != nullptr && (double)fr[3] >= min_joints && track_finite(mr[0]) && track_finite(mr[1]) && track_finite(mr[2]) &&
                        (double)fr[4] <= prm.max_disagree && (double)fr[5] <= prm.max_gap;
        double cutoff;
        const int root_status = track_step(root, mr, ar, dt, ok, cls_root, max_hold, cutoff);
        if (owns_root) track_record(root, root_status, cutoff, tracks + (b * K + P) * 8);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!on[i]) continue;
            const int k = lane + 64 * i;
            const double m[3] = {(double)cur[i].m[0], (double)cur[i].m[1], (double)cur[i].m[2]};
            const bool a = cur[i].valid == 1.f && track_finite(m[0]) && track_finite(m[1]) && track_finite(m[2]) &&
                           (is_pose[i] || (double)cur[i].gap <= prm.max_joint_gap);
            const int status = track_step(st[i], m, a, dt, ok, is_pose[i] ? cls_pose : cls_joint, max_hold, cutoff);
            track_record(st[i], status, cutoff, tracks + (b * K + k) * 8);
            if (i == 0 && is_pose[0]) {                      // (P <= 64: every pose row is a slot-0 track)
                float* o = placed + (b * P + k) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = status == 0 ? 0.f : (float)(root_status != 0 ? st[0].x[c] + root.x[c] : st[0].x[c]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (on[i]) track_store(st[i], state_out + (s * K + lane + 64 * i) * kTrackState);
    if (owns_root) track_store(root, state_out + (s * K + P) * kTrackState);
}

// T, S, P > 0, P, J <= kTrackMaxRows, the pointers and the parameters checked by the caller.
static inline hipError_t pose_track_launch(const float* pose, const float* frame, const float* joints3d, int T, int S, int P, int J, const float* dts, double dt,
                                           const egotap_track_params& prm, const double* state_in, double* state_out, float* tracks, float* placed, hipStream_t s) {
    if (T <= 0 || S <= 0 || P <= 0 || P > kTrackMaxRows || J < 0 || J > kTrackMaxRows || (J > 0) != (joints3d != nullptr)) return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)S + kTrackStreamsPerBlock - 1) / kTrackStreamsPerBlock);
    hipLaunchKernelGGL(pose_track_kernel, dim3(blocks), dim3(64 * kTrackStreamsPerBlock), 0, s, pose, frame, joints3d, T, S, P, J, dts, dt, prm, state_in, state_out,
                       tracks, placed);
    return hipGetLastError();
}

// The camera-frame kernel's walk with a rig pose per step; the step itself, the loads, the stores and the records are the shared functions above.
// The 12 rig values are wave-uniform but live in VGPRs: the 96 SGPRs of the walk leave no room for 24 more (the scalar-load form spills 15 of
// them), and a copy of the NEXT step's rig pose in flight would take the kernel to 256 VGPRs + 6 AGPRs and one wave per SIMD, so this step's
// rig pose is asked for at the top of the step and not a step ahead; the measurements still travel a step ahead.
// gfx950, -O3: 248 VGPRs (the camera-frame walk's 220, this step's rig pose and the transform's temporaries), 0 AGPRs, 104 SGPRs, scratch 0 bytes, no
// spills, LDS 0 bytes, 2 waves per SIMD.
// state_in and state_out may be the same array, as above: not __restrict__.
static __global__ __launch_bounds__(64 * kTrackStreamsPerBlock) void pose_track_world_kernel(const float* __restrict__ pose, const float* __restrict__ frame,
                                                                                             const float* __restrict__ joints3d, const double* __restrict__ rig_pose,
                                                                                             int T, int S, int P, int J, const float* __restrict__ dts, double dt_host,
                                                                                             egotap_track_params prm, double ortho_tol, const double* state_in,
                                                                                             double* state_out, float* __restrict__ tracks,
                                                                                             float* __restrict__ placed_world, float* __restrict__ placed_cam) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long s = (long)blockIdx.x * kTrackStreamsPerBlock + wave;
    if (s >= S) return;                                      // (no barrier anywhere: a wave may leave)
    const int K = P + 1 + J;
    const TrackClass cls_pose = {prm.pose_min_cutoff, prm.pose_beta, prm.pose_d_cutoff}, cls_root = {prm.root_min_cutoff, prm.root_beta, prm.root_d_cutoff},
                     cls_joint = {prm.joints_min_cutoff, prm.joints_beta, prm.joints_d_cutoff};
    const double max_hold = (double)prm.max_hold, min_joints = (double)prm.min_joints;
    // slot i of this lane is track lane + 64 i; the root (track P) is run by every lane below and skipped as a slot
    bool on[3], is_pose[3];
    TrackState st[3], root;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int k = lane + 64 * i;
        on[i] = k < K && k != P;
        is_pose[i] = k < P;
        st[i] = TrackState{};
        if (on[i]) track_load(st[i], state_in + (s * K + k) * kTrackState);
    }
    track_load(root, state_in + (s * K + P) * kTrackState);
    const bool owns_root = lane == (P & 63);

    TrackRaw nxt[3] = {};
    float nfr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ndt = 0.f;
    auto fetch = [&](int t) {
        const long b = (long)t * S + s;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!on[i]) continue;
            const int k = lane + 64 * i;
            if (is_pose[i]) {
                const float* p = pose + (b * P + k) * 3;
                nxt[i].m[0] = p[0];
                nxt[i].m[1] = p[1];
                nxt[i].m[2] = p[2];
                nxt[i].gap = 0.f;
                nxt[i].valid = 1.f;
            } else {
                const float* q = joints3d + (b * J + (k - P - 1)) * 8;
                nxt[i].m[0] = q[0];
                nxt[i].m[1] = q[1];
                nxt[i].m[2] = q[2];
                nxt[i].gap = q[3];
                nxt[i].valid = q[7];
            }
        }
        if (frame) {
            const float* f = frame + b * 8;
            nfr[0] = f[0];
            nfr[1] = f[1];
            nfr[2] = f[2];
            nfr[3] = f[3];
            nfr[4] = f[4];
            nfr[5] = f[6];
        }
        if (dts) ndt = dts[t];
    };
    fetch(0);
    for (int t = 0; t < T; ++t) {
        TrackRaw cur[3];
        float fr[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) cur[i] = nxt[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) fr[i] = nfr[i];
        const double dt = dts ? (double)ndt : dt_host;
        const long b = (long)t * S + s;
        double rig[12];                                      // asked for first: everything below waits for it
#pragma unroll
        for (int k = 0; k < 12; ++k) rig[k] = rig_pose[b * 12 + k];
        if (t + 1 < T) fetch(t + 1);                         // the next step's measurements travel during this step's chain
        const bool ok = track_finite(dt) && dt > 0.0;
        const bool seen = rig_seen(rig, ortho_tol);          // not seen: no track accepts, the step is a missing sample
        // the root, by every lane for itself: (t^, n, rms disagree, rms gap) of the frame record
        const double mr[3] = {(double)fr[0], (double)fr[1], (double)fr[2]};
        const bool ar = frame != nullptr && (double)fr[3] >= min_joints && track_finite(mr[0]) && track_finite(mr[1]) && track_finite(mr[2]) &&
                        (double)fr[4] <= prm.max_disagree && (double)fr[5] <= prm.max_gap;
        double cutoff, wr[3];
        rig_to_world(rig, mr, true, wr);
        const int root_status = track_step(root, wr, ar && seen, dt, ok, cls_root, max_hold, cutoff);
        if (owns_root) track_record(root, root_status, cutoff, tracks + (b * K + P) * 8);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            if (!on[i]) continue;
            const int k = lane + 64 * i;
            const double m[3] = {(double)cur[i].m[0], (double)cur[i].m[1], (double)cur[i].m[2]};
            const bool a = cur[i].valid == 1.f && track_finite(m[0]) && track_finite(m[1]) && track_finite(m[2]) &&
                           (is_pose[i] || (double)cur[i].gap <= prm.max_joint_gap);
            double w[3];
            rig_to_world(rig, m, !is_pose[i], w);
            const int status = track_step(st[i], w, a && seen, dt, ok, is_pose[i] ? cls_pose : cls_joint, max_hold, cutoff);
            track_record(st[i], status, cutoff, tracks + (b * K + k) * 8);
            if (i == 0 && is_pose[0]) {                      // (P <= 64: every pose row is a slot-0 track)
                const bool with_root = root_status != 0;
                double pw[3], pc[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) pw[c] = with_root ? st[0].x[c] + root.x[c] : st[0].x[c];
                rig_to_camera(rig, pw, with_root, pc);       // the same float64 value, back through this step's rig pose
                float *o = placed_world + (b * P + k) * 3, *oc = placed_cam + (b * P + k) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    o[c] = status == 0 ? 0.f : (float)pw[c];
                    oc[c] = status == 0 || !seen ? 0.f : (float)pc[c];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        if (on[i]) track_store(st[i], state_out + (s * K + lane + 64 * i) * kTrackState);
    if (owns_root) track_store(root, state_out + (s * K + P) * kTrackState);
}

// the same checks; rig_pose, placed_world and placed_cam checked by the caller.
static inline hipError_t pose_track_world_launch(const float* pose, const float* frame, const float* joints3d, const double* rig_pose, int T, int S, int P, int J,
                                                 const float* dts, double dt, const egotap_track_params& prm, double ortho_tol, const double* state_in,
                                                 double* state_out, float* tracks, float* placed_world, float* placed_cam, hipStream_t s) {
    if (T <= 0 || S <= 0 || P <= 0 || P > kTrackMaxRows || J < 0 || J > kTrackMaxRows || (J > 0) != (joints3d != nullptr) || !rig_pose || !placed_cam)
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)S + kTrackStreamsPerBlock - 1) / kTrackStreamsPerBlock);
    hipLaunchKernelGGL(pose_track_world_kernel, dim3(blocks), dim3(64 * kTrackStreamsPerBlock), 0, s, pose, frame, joints3d, rig_pose, T, S, P, J, dts, dt, prm,
                       ortho_tol, state_in, state_out, tracks, placed_world, placed_cam);
    return hipGetLastError();
}
