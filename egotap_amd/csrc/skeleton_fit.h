// A rigid skeleton and a rotation per bone from tracked joint positions (egotap.h egotap_skeleton_fit; spec.py skeleton_fit_ref restates it in float64,
// operation for operation).
//   skeleton_fit_kernel  T frames of S streams, time-major (frame b = t * S + s): one WAVE per stream, four streams per workgroup, lane j owns pose
//       row j (P <= 64).  The (L^, n) of the lane's bone is read once before the loop over the T steps, lives in registers, and is written once after
//       it.  Per step: the lane takes its parent's input position from the parent's lane (the bone sample), updates its length, takes its mirror's
//       (L^, n) from the mirror's lane, then the tree is walked LEVEL BY LEVEL, serial in depth and not in rows: at level d every lane of depth d takes
//       its parent's rigid position r (3 doubles), rotation Q (4 doubles) and the two ok flags from the parent's lane.  The root rows' rotation comes
//       from the three frame rows, which every lane reads for itself (three cross-lane reads with a uniform source), so all lanes hold the same bits.
//       Step t + 1's inputs are requested before step t's arithmetic.  A wave whose stream lies past S loads and stores nothing.
//   skeleton_fit_kernel<true>  the same walk with the TWIST of egotap_skeleton_fit_twist (spec.py skeleton_fit_twist_ref): next to the bone sample lane j
//       takes its pole child's input position from the child's lane (one more per-lane-constant source; three fp32 reads and the seen flag), repeats the
//       child's own sample arithmetic on it (the same operations, hence the child's bits), and has the bend normal n and the weight w before the walk;
//       at its level it rolls Q_s about its bone so that the rotated hinge g meets n.  <false> is egotap_skeleton_fit's kernel, operation for operation.
// Cross-lane reads, not LDS: __shfl on a double is two ds_bpermute_b32, which go through the LDS crossbar but allocate no LDS and need no barrier or
// fence -- the exchange is inside one wave, all 64 lanes take part in every one (no lane leaves the loop early, rows past P are idle root rows), and
// the parent's lane is a per-lane constant.  The LDS form (7 doubles + flags per row, ~4 KB a workgroup) would need a fence between a level's
// writes and the next level's reads for the compiler's sake and saves nothing: a level costs 15 bpermutes against a chain of ~10 dependent float64
// divisions and square roots.
// Bound by LATENCY, not by any rate: per level rotate, shortest arc (sqrt, 4 divisions), product, normalise (sqrt, 4 divisions), each waiting for the
// one before; a call costs T x (depth of the tree) such chains whatever S is, up to 4 streams per workgroup and one workgroup per CU.
// Compiler's resource summary for gfx950 (-Rpass-analysis=kernel-resource-usage): see the numbers at the kernel.
// Contraction is off in every function here: the definition keeps products and sums apart.  sqrt and the divisions are correctly rounded.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "egotap.h"

constexpr int kSkelMaxRows = EGOTAP_SKELETON_MAX_ROWS;      // P: one lane each
constexpr int kSkelStreamsPerBlock = 4;

// what the entry derives from an egotap_skeleton_rig and the kernel takes by value: 2344 bytes of the 4 KB kernel-argument segment
struct SkelRigDev {
    double rest_dir[kSkelMaxRows][3];      // unit, zeros for root rows
    double rest_frame[3][3];               // rows e0, e1, e2 of the rest pose's triangle
    double fixed_length[kSkelMaxRows];
    int8_t parent[kSkelMaxRows], mirror[kSkelMaxRows], depth[kSkelMaxRows];      // -1: a root row / no mirror
    int32_t P, fa, fb, fc, max_depth, has_fixed, pad_;
};
static_assert(sizeof(SkelRigDev) == 2344 && sizeof(egotap_skeleton_rig) == 2584, "egotap.h states both sizes");
struct SkelParamsDev {
    double window, min_samples, max_dev;
    int32_t freeze, track_rows;
};

// what the entry derives from an egotap_skeleton_twist and the twist instantiation takes by value: 1616 bytes; with the rest of the block (two
// pointers, T and S, the rig, the parameters, five pointers: 2440 bytes) 4056 of the 4 KB kernel-argument segment
struct SkelTwistDev {
    double g[kSkelMaxRows][3];             // the rest hinge made orthogonal to rest_dir and normalised; zeros where the row has no pole
    double bend_lo, bend_hi;
    int8_t pole[kSkelMaxRows];             // the row whose bone bends against this row's, or -1
};
struct SkelNoTwist {};                     // egotap_skeleton_fit's instantiation takes nothing more
static_assert(sizeof(SkelTwistDev) == 1616 && sizeof(egotap_skeleton_twist) == 1808, "egotap.h states both sizes");
static_assert(2 * sizeof(void*) + 2 * sizeof(int) + sizeof(SkelRigDev) + sizeof(SkelParamsDev) + 5 * sizeof(void*) + sizeof(SkelTwistDev) <= 4096,
              "the twist instantiation's argument block fits the 4 KB kernel-argument segment");

struct SkelQuat {
    double w, x, y, z;
};
struct SkelVec {
    double v[3];
};

static __host__ __device__ __forceinline__ bool skel_pos_finite(double n) { return n > 0.0 && n <= 1.7976931348623157e308; }      // false for NaN, +-inf, <= 0
static __host__ __device__ __forceinline__ double skel_norm3(const SkelVec& d) {
#pragma clang fp contract(off)
    return sqrt((d.v[0] * d.v[0] + d.v[1] * d.v[1]) + d.v[2] * d.v[2]);
}
static __host__ __device__ __forceinline__ SkelVec skel_cross(const SkelVec& a, const SkelVec& b) {
#pragma clang fp contract(off)
    return SkelVec{{a.v[1] * b.v[2] - a.v[2] * b.v[1], a.v[2] * b.v[0] - a.v[0] * b.v[2], a.v[0] * b.v[1] - a.v[1] * b.v[0]}};
}
// the frame of three points, rows (e0, e1, e2) into f; false where a norm is zero or not finite (egotap.h)
static __host__ __device__ __forceinline__ bool skel_frame(const SkelVec& xa, const SkelVec& xb, const SkelVec& xc, SkelVec (&f)[3]) {
#pragma clang fp contract(off)
    SkelVec d, w, g;
    for (int i = 0; i < 3; ++i) d.v[i] = xb.v[i] - xc.v[i];
    const double n0 = skel_norm3(d);
    for (int i = 0; i < 3; ++i) f[0].v[i] = d.v[i] / n0;
    for (int i = 0; i < 3; ++i) w.v[i] = xa.v[i] - 0.5 * (xb.v[i] + xc.v[i]);
    const double p = (w.v[0] * f[0].v[0] + w.v[1] * f[0].v[1]) + w.v[2] * f[0].v[2];
    for (int i = 0; i < 3; ++i) g.v[i] = w.v[i] - p * f[0].v[i];
    const double n1 = skel_norm3(g);
    for (int i = 0; i < 3; ++i) f[1].v[i] = g.v[i] / n1;
    f[2] = skel_cross(f[0], f[1]);
    return skel_pos_finite(n0) && skel_pos_finite(n1);
}
static __device__ __forceinline__ SkelQuat skel_sign(const SkelQuat& q) {
    const bool neg = q.w < 0.0 || (q.w == 0.0 && (q.x < 0.0 || (q.x == 0.0 && (q.y < 0.0 || (q.y == 0.0 && q.z < 0.0)))));
    return neg ? SkelQuat{-q.w, -q.x, -q.y, -q.z} : q;
}
static __device__ __forceinline__ SkelQuat skel_normalize(const SkelQuat& q) {
#pragma clang fp contract(off)
    const double n = sqrt(((q.w * q.w + q.x * q.x) + q.y * q.y) + q.z * q.z);
    return SkelQuat{q.w / n, q.x / n, q.y / n, q.z / n};
}
static __device__ __forceinline__ SkelQuat skel_mul(const SkelQuat& a, const SkelQuat& b) {
#pragma clang fp contract(off)
    return SkelQuat{((a.w * b.w - a.x * b.x) - a.y * b.y) - a.z * b.z, ((a.w * b.x + a.x * b.w) + a.y * b.z) - a.z * b.y,
                    ((a.w * b.y - a.x * b.z) + a.y * b.w) + a.z * b.x, ((a.w * b.z + a.x * b.y) - a.y * b.x) + a.z * b.w};
}
static __device__ __forceinline__ SkelVec skel_rotate(const SkelQuat& q, const SkelVec& v) {
#pragma clang fp contract(off)
    const SkelVec qv = {{q.x, q.y, q.z}}, c = skel_cross(qv, v), t = {{2.0 * c.v[0], 2.0 * c.v[1], 2.0 * c.v[2]}}, k = skel_cross(qv, t);
    return SkelVec{{(v.v[0] + q.w * t.v[0]) + k.v[0], (v.v[1] + q.w * t.v[1]) + k.v[1], (v.v[2] + q.w * t.v[2]) + k.v[2]}};
}
// quat(M_cur M_rest^T) of two frames given as rows (e0, e1, e2), Shepperd's rule (spec.quat_from_frames)
static __device__ __forceinline__ SkelQuat skel_quat_from_frames(const SkelVec (&cur)[3], const double (&rest)[3][3]) {
#pragma clang fp contract(off)
    double R[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[i][j] = (cur[0].v[i] * rest[0][j] + cur[1].v[i] * rest[1][j]) + cur[2].v[i] * rest[2][j];
    const double t = (R[0][0] + R[1][1]) + R[2][2];
    SkelQuat q;
    if (t > 0.0) {
        const double s = sqrt(t + 1.0) * 2.0;
        q = SkelQuat{0.25 * s, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s};
    } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
        const double s = sqrt(fmax(((1.0 + R[0][0]) - R[1][1]) - R[2][2], 0.0)) * 2.0;
        q = SkelQuat{(R[2][1] - R[1][2]) / s, 0.25 * s, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s};
    } else if (R[1][1] >= R[2][2]) {
        const double s = sqrt(fmax(((1.0 + R[1][1]) - R[0][0]) - R[2][2], 0.0)) * 2.0;
        q = SkelQuat{(R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, 0.25 * s, (R[1][2] + R[2][1]) / s};
    } else {
        const double s = sqrt(fmax(((1.0 + R[2][2]) - R[0][0]) - R[1][1], 0.0)) * 2.0;
        q = SkelQuat{(R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, 0.25 * s};
    }
    return skel_sign(skel_normalize(q));
}
// the swing v -> u by the shortest arc (egotap.h step 6); not given a sign
static __device__ __forceinline__ SkelQuat skel_shortest_arc(const SkelVec& v, const SkelVec& u) {
#pragma clang fp contract(off)
    const double c = (v.v[0] * u.v[0] + v.v[1] * u.v[1]) + v.v[2] * u.v[2];
    if (c > -1.0 + 1e-12) {
        const SkelVec x = skel_cross(v, u);
        return skel_normalize(SkelQuat{1.0 + c, x.v[0], x.v[1], x.v[2]});
    }
    int k = 0;
    if (fabs(v.v[1]) < fabs(v.v[k])) k = 1;
    if (fabs(v.v[2]) < fabs(v.v[k])) k = 2;
    const SkelVec e = {{k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0}}, x = skel_cross(v, e);
    const double n = skel_norm3(x);
    return SkelQuat{0.0, x.v[0] / n, x.v[1] / n, x.v[2] / n};
}
// the twist (egotap.h egotap_skeleton_fit_twist): Q = Q_s rolled about the bone u so that the rotated hinge g, made orthogonal to u, moves the share w of
// the way to the bend normal n; false, and Q as it was, where a norm is zero or not finite
static __device__ __forceinline__ bool skel_twist(SkelQuat& Q, const SkelVec& g, const SkelVec& u, const SkelVec& n, double w) {
#pragma clang fp contract(off)
    const SkelVec h = skel_rotate(Q, g);
    const double p = (h.v[0] * u.v[0] + h.v[1] * u.v[1]) + h.v[2] * u.v[2];
    const SkelVec hr = {{h.v[0] - p * u.v[0], h.v[1] - p * u.v[1], h.v[2] - p * u.v[2]}};
    const double nh = skel_norm3(hr);
    const SkelVec hp = {{hr.v[0] / nh, hr.v[1] / nh, hr.v[2] / nh}};
    const double w1 = 1.0 - w;
    const SkelVec br = {{w1 * hp.v[0] + w * n.v[0], w1 * hp.v[1] + w * n.v[1], w1 * hp.v[2] + w * n.v[2]}};
    const double nb = skel_norm3(br);
    if (!(skel_pos_finite(nh) && skel_pos_finite(nb))) return false;
    const SkelVec b = {{br.v[0] / nb, br.v[1] / nb, br.v[2] / nb}};
    const double k = (hp.v[0] * b.v[0] + hp.v[1] * b.v[1]) + hp.v[2] * b.v[2];
    SkelQuat tw = {0.0, u.v[0], u.v[1], u.v[2]};             // h' = -b: the half turn about the bone
    if (k > -1.0 + 1e-12) {
        const SkelVec x = skel_cross(hp, b);
        tw = skel_normalize(SkelQuat{1.0 + k, x.v[0], x.v[1], x.v[2]});
    }
    Q = skel_normalize(skel_mul(tw, Q));
    return true;
}
static __device__ __forceinline__ bool skel_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // false for NaN and +-inf

// gfx950, -O3: 92 VGPRs (the row's sample, r, Q, local, the parent's r and Q in flight, the next step's inputs), 0 AGPRs, 106 SGPRs (the rest frame, the
// parameters and the frame rows are uniform; 14 of them parked in VGPR lanes), scratch 0 bytes, LDS 0 bytes, 5 waves per SIMD (a workgroup puts one on each).
// <false> is the kernel above (the same 1673 instructions as before it became a template; the empty SkelNoTwist makes its argument block 2444 bytes for
// 2440).  <true>, gfx950, -O3: 117 VGPRs (the hinge, the bend normal and its weight, the child's position in flight), 0 AGPRs, 106 SGPRs (27 of them
// parked in VGPR lanes), scratch 0 bytes, LDS 0 bytes, 4 waves per SIMD; 4056 bytes of arguments.
// state_in and state_out may be the same array (each lane reads its row before the loop and writes it after it): not __restrict__.
template <bool TWIST>
static __global__ __launch_bounds__(64 * kSkelStreamsPerBlock) void skeleton_fit_kernel(const float* __restrict__ points, const float* __restrict__ tracks, int T,
                                                                                        int S, SkelRigDev rig, SkelParamsDev prm, const double* state_in,
                                                                                        double* state_out, float* __restrict__ rigid,
                                                                                        float* __restrict__ rotations, float* __restrict__ lengths,
                                                                                        std::conditional_t<TWIST, SkelTwistDev, SkelNoTwist> tw) {
#pragma clang fp contract(off)
    typedef float f32x4v __attribute__((ext_vector_type(4)));
    typedef float f32x2v __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long s = (long)blockIdx.x * kSkelStreamsPerBlock + wave;
    if (s >= S) return;                                      // (no barrier anywhere: a wave may leave)
    const int P = rig.P, K = prm.track_rows;
    const bool row = lane < P;                               // lanes past P: idle root rows that take part in every cross-lane read and store nothing
    const int par = row ? rig.parent[lane] : -1, mir = row ? rig.mirror[lane] : -1, depth = row ? rig.depth[lane] : 0;
    const bool bone = par >= 0, fixed = rig.has_fixed != 0, calibrate = bone && !fixed;
    const int src_p = bone ? par : lane, src_m = mir >= 0 ? mir : lane;
    SkelVec rest = {{0.0, 0.0, 0.0}};
    double L_hat = 0.0, n_hat = 0.0, L_fixed = 0.0;
    if (bone) {
#pragma unroll
        for (int c = 0; c < 3; ++c) rest.v[c] = rig.rest_dir[lane][c];
        if (fixed) L_fixed = rig.fixed_length[lane];
    }
    int src_c = lane;                                        // (twist) the pole child's lane, and the hinge of the lane's own bone
    bool poled = false;
    SkelVec hinge = {{0.0, 0.0, 0.0}};
    if constexpr (TWIST) {
        const int pol = row ? tw.pole[lane] : -1;
        poled = pol >= 0;
        if (poled) {
            src_c = pol;
#pragma unroll
            for (int c = 0; c < 3; ++c) hinge.v[c] = tw.g[lane][c];
        }
    }
    const bool stateful = row && !fixed;                     // a root row's (L^, n) passes through: state_out is a whole state
    if (stateful) {
        L_hat = state_in[(s * P + lane) * 2];
        n_hat = state_in[(s * P + lane) * 2 + 1];
    }

    float nx[3] = {0.f, 0.f, 0.f}, nst = 1.f;
    auto fetch = [&](int t) {
        if (!row) return;
        const long b = (long)t * S + s;
        const float* p = points + (b * P + lane) * 3;
        nx[0] = p[0];
        nx[1] = p[1];
        nx[2] = p[2];
        if (tracks) nst = tracks[(b * K + lane) * 8 + 7];
    };
    fetch(0);
    for (int t = 0; t < T; ++t) {
        const float x0 = nx[0], x1 = nx[1], x2 = nx[2], st = nst;
        if (t + 1 < T) fetch(t + 1);                         // the next step's inputs travel during this step's chain
        const long b = (long)t * S + s;
        // 1 seen
        const bool seen = row && skel_finite(x0) && skel_finite(x1) && skel_finite(x2) && (st == 1.f || st == 2.f);
        // 2 the bone sample, against the parent's input position
        const float px0 = __shfl(x0, src_p), px1 = __shfl(x1, src_p), px2 = __shfl(x2, src_p);
        const bool pseen = __shfl((int)seen, src_p) != 0;
        const SkelVec d = {{(double)x0 - (double)px0, (double)x1 - (double)px1, (double)x2 - (double)px2}};
        const double ell = skel_norm3(d);
        const bool valid = bone && seen && pseen && skel_pos_finite(ell);
        const SkelVec u = {{d.v[0] / ell, d.v[1] / ell, d.v[2] / ell}};      // read only where valid
        // (twist) the pole child's sample from its input position, as the child's own lane takes it; the bend normal and its weight
        double bend_w = 0.0;
        SkelVec bend_n = {{0.0, 0.0, 0.0}};
        if constexpr (TWIST) {
            const float cx0 = __shfl(x0, src_c), cx1 = __shfl(x1, src_c), cx2 = __shfl(x2, src_c);
            const bool cseen = __shfl((int)seen, src_c) != 0;
            const SkelVec dc = {{(double)cx0 - (double)x0, (double)cx1 - (double)x1, (double)cx2 - (double)x2}};
            const double ellc = skel_norm3(dc);
            const SkelVec uc = {{dc.v[0] / ellc, dc.v[1] / ellc, dc.v[2] / ellc}};
            const SkelVec m = skel_cross(u, uc);
            const double sigma = skel_norm3(m);
            if (valid && poled && seen && cseen && skel_pos_finite(ellc) && sigma > tw.bend_lo && skel_pos_finite(sigma)) {
                if (sigma >= tw.bend_hi) {
                    bend_w = 1.0;
                } else {
                    const double ramp = (sigma - tw.bend_lo) / (tw.bend_hi - tw.bend_lo);
                    bend_w = (ramp * ramp) * (3.0 - 2.0 * ramp);
                }
                bend_n = SkelVec{{m.v[0] / sigma, m.v[1] / sigma, m.v[2] / sigma}};
            }
        }
        // 3 the length
        if (valid && calibrate && !prm.freeze && (n_hat < prm.min_samples || fabs(ell - L_hat) <= prm.max_dev * L_hat)) {
            n_hat = n_hat + 1.0 < prm.window ? n_hat + 1.0 : prm.window;
            L_hat = L_hat + (ell - L_hat) / n_hat;
        }
        // 4 the length used, after every row's update: the mirror's is one more cross-lane read
        const double L_m = __shfl(L_hat, src_m), n_m = __shfl(n_hat, src_m);
        const bool have = bone && (fixed || n_hat >= 1.0);
        double L = fixed ? L_fixed : L_hat;
        if (calibrate && mir >= 0 && n_hat >= 1.0 && n_m >= 1.0) L = 0.5 * (L_hat + L_m);
        // 6 the root rows' rotation: every lane for itself from the three frame rows (uniform sources: the same bits in all lanes)
        SkelVec fx[3], cur[3];
        const int fsrc[3] = {rig.fa, rig.fb, rig.fc};
        bool fseen = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            fx[k].v[0] = (double)__shfl(x0, fsrc[k]);
            fx[k].v[1] = (double)__shfl(x1, fsrc[k]);
            fx[k].v[2] = (double)__shfl(x2, fsrc[k]);
            fseen = fseen && __shfl((int)seen, fsrc[k]) != 0;
        }
        const bool frame_ok = skel_frame(fx[0], fx[1], fx[2], cur) && fseen;
        SkelQuat Q = {1.0, 0.0, 0.0, 0.0}, loc = {1.0, 0.0, 0.0, 0.0};
        SkelVec r = {{0.0, 0.0, 0.0}};
        bool r_ok = false, q_ok = false, t_ok = false;
        if (!bone) {
            r_ok = seen;
            r = SkelVec{{(double)x0, (double)x1, (double)x2}};
            if (frame_ok) {
                Q = skel_quat_from_frames(cur, rig.rest_frame);
                loc = Q;
                q_ok = true;
            }
        }
        // 5 and 6, level by level: a lane of depth lv takes r, Q and the flags of its parent, which level lv - 1 finished
        for (int lv = 1; lv <= rig.max_depth; ++lv) {
            SkelVec pr;
            SkelQuat pq;
#pragma unroll
            for (int c = 0; c < 3; ++c) pr.v[c] = __shfl(r.v[c], src_p);
            pq.w = __shfl(Q.w, src_p);
            pq.x = __shfl(Q.x, src_p);
            pq.y = __shfl(Q.y, src_p);
            pq.z = __shfl(Q.z, src_p);
            const int pflags = __shfl((int)r_ok | ((int)q_ok << 1), src_p);
            if (depth == lv) {
                if (valid && have && (pflags & 1)) {
                    r_ok = true;
#pragma unroll
                    for (int c = 0; c < 3; ++c) r.v[c] = pr.v[c] + L * u.v[c];
                }
                if (valid && (pflags & 2)) {
                    const SkelVec v = skel_rotate(pq, rest);
                    SkelQuat Qs = skel_normalize(skel_mul(skel_shortest_arc(v, u), pq));
                    if constexpr (TWIST)
                        if (bend_w > 0.0) t_ok = skel_twist(Qs, hinge, u, bend_n, bend_w);
                    Q = skel_sign(Qs);
                    loc = skel_sign(skel_mul(SkelQuat{pq.w, -pq.x, -pq.y, -pq.z}, Q));
                    q_ok = true;
                }
            }
        }
        if (row) {
            const f32x4v rec = {r_ok ? (float)r.v[0] : 0.f, r_ok ? (float)r.v[1] : 0.f, r_ok ? (float)r.v[2] : 0.f, (float)((int)r_ok + 2 * (int)q_ok + 4 * (int)t_ok)};
            const f32x4v glob = {(float)Q.w, (float)Q.x, (float)Q.y, (float)Q.z}, locl = {(float)loc.w, (float)loc.x, (float)loc.y, (float)loc.z};
            const f32x2v len = {bone && have ? (float)L : 0.f, bone ? (float)n_hat : 0.f};
            *(f32x4v*)(rigid + (b * P + lane) * 4) = rec;
            *(f32x4v*)(rotations + (b * P + lane) * 8) = glob;
            *(f32x4v*)(rotations + (b * P + lane) * 8 + 4) = locl;
            *(f32x2v*)(lengths + (b * P + lane) * 2) = len;
        }
    }
    if (stateful) {
        state_out[(s * P + lane) * 2] = L_hat;
        state_out[(s * P + lane) * 2 + 1] = n_hat;
    }
}

// T, S > 0, the rig, the table, the pointers and the parameters checked by the caller.  tw a SkelTwistDev: the twist instantiation; a SkelNoTwist:
// egotap_skeleton_fit's.
template <class Twist>
static inline hipError_t skeleton_fit_launch(const float* points, const float* tracks, int T, int S, const SkelRigDev& rig, const Twist& tw, const SkelParamsDev& prm,
                                             const double* state_in, double* state_out, float* rigid, float* rotations, float* lengths, hipStream_t s) {
    if (T <= 0 || S <= 0 || rig.P <= 0 || rig.P > kSkelMaxRows || !points || !rigid || !rotations || !lengths || (!rig.has_fixed && (!state_in || !state_out)))
        return hipErrorInvalidValue;
    const unsigned blocks = (unsigned)(((long)S + kSkelStreamsPerBlock - 1) / kSkelStreamsPerBlock);
    constexpr bool with_twist = std::is_same<Twist, SkelTwistDev>::value;
    hipLaunchKernelGGL(skeleton_fit_kernel<with_twist>, dim3(blocks), dim3(64 * kSkelStreamsPerBlock), 0, s, points, tracks, T, S, rig, prm, state_in, state_out,
                       rigid, rotations, lengths, tw);
    return hipGetLastError();
}
