// 32 x 128 tiles of the attention backward on v_mfma_f32_32x32x16_bf16, shared by three kernel families: the fp32-tensor backward
// (attention_bwd_bf16.h) and, through attention_bf16s_tiles.h, the bf16-storage forward and backward.  Types, LDS images and tile
// products only: no kernel and no launch.
// Operands are made in registers (NP = 3: hi + lo split, three MFMAs per product; NP = 1: bf16 rounding).  A 32 x 128 tile that is
// contracted over d ("T x regs^T": scores, dP) is staged as a ROW image (272-byte rows, one ds_read_b128 per 16-d step); a tile that
// is contracted over its rows ("T^T x P": the gradient accumulations) is staged as a TRANSPOSED-READ image (320-byte rows,
// ds_read_b64_tr_b16 blocks in the key order of the probability accumulator: 16s + 8(j>>2) + 4h + (j&3)).
#pragma once
#include "common.h"
#include "gemm_bf16.h"      // bf16x8, bf16x4, lds_bf16x4_ptr, bf16_split8, bf16_round8

namespace attnbf {
constexpr int DH = 128, KT = 32, RSTR = 136, TSTR = 160;      // image row strides in bf16
constexpr int RIMG = KT * RSTR, TIMG = KT * TSTR;              // bf16 per image
constexpr int OLD = DH + 4;                                    // fp32 output patch row

template <int NP> struct Frags { bf16x8 f[NP == 3 ? 2 : 1][8]; };

// stage a 32 x 128 fp32 tile (row stride ld) as bf16 images: row image (or nullptr) and transposed-read image (or nullptr);
// each is [hi][lo] for NP = 3
template <int THREADS, int NP>
__device__ __forceinline__ void stage(__bf16* rowimg, __bf16* trimg, const float* src, long ld, int tid) {
    constexpr int PER = KT * (DH / 4) / THREADS;
    f32x4 st[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int idx = tid + i * THREADS, row = idx >> 5, c4 = idx & 31;
        st[i] = *(const f32x4*)(src + (long)row * ld + c4 * 4);
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int idx = tid + i * THREADS, row = idx >> 5, c4 = idx & 31;
        bf16x4 hi, lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            hi[e] = (__bf16)st[i][e];
            lo[e] = (__bf16)(st[i][e] - (float)hi[e]);
        }
        if (rowimg) {
            *(bf16x4*)(rowimg + row * RSTR + c4 * 4) = hi;
            if (NP == 3) *(bf16x4*)(rowimg + RIMG + row * RSTR + c4 * 4) = lo;
        }
        if (trimg) {
            *(bf16x4*)(trimg + row * TSTR + c4 * 4) = hi;
            if (NP == 3) *(bf16x4*)(trimg + TIMG + row * TSTR + c4 * 4) = lo;
        }
    }
}

// one 128-float row as 8 k-step fragments: lane half h of step s holds d = 16 s + 8 h + j
template <int NP>
__device__ __forceinline__ void load_row_frags(Frags<NP>& fr, const float* rowp, int lh) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const f32x4 v0 = *(const f32x4*)(rowp + 16 * s + 8 * lh), v1 = *(const f32x4*)(rowp + 16 * s + 8 * lh + 4);
        if (NP == 3) bf16_split8(v0, v1, fr.f[0][s], fr.f[NP == 3 ? 1 : 0][s]);
        else fr.f[0][s] = bf16_round8(v0, v1);
    }
}

// T[32 x 32] = rowimg (rows on the accumulator row) x frags^T (the lane's fixed row on the accumulator column)
template <int NP>
__device__ __forceinline__ f32x16 tile_x_frags(const __bf16* rowimg, const Frags<NP>& fr, int l31, int lh) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const __bf16* p = rowimg + l31 * RSTR + 8 * lh;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const bf16x8 ah = *(const bf16x8*)(p + 16 * t);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, fr.f[0][t], s, 0, 0, 0);
        if (NP == 3) {
            const bf16x8 al = *(const bf16x8*)(p + RIMG + 16 * t);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, fr.f[NP == 3 ? 1 : 0][t], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, fr.f[0][t], s, 0, 0, 0);
        }
    }
    return s;
}

// same with the second operand read from a (per-wave) row image instead of registers: T = A_img x B_img^T
template <int NP>
__device__ __forceinline__ f32x16 tile_x_tile(const __bf16* aimg, const __bf16* bimg, int l31, int lh) {
    f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
    const __bf16* pa = aimg + l31 * RSTR + 8 * lh;
    const __bf16* pb = bimg + l31 * RSTR + 8 * lh;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const bf16x8 ah = *(const bf16x8*)(pa + 16 * t), bh = *(const bf16x8*)(pb + 16 * t);
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, s, 0, 0, 0);
        if (NP == 3) {
            const bf16x8 al = *(const bf16x8*)(pa + RIMG + 16 * t), bl = *(const bf16x8*)(pb + RIMG + 16 * t);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, s, 0, 0, 0);
        }
    }
    return s;
}

// acc^T[4 d-tiles] += sum_rows tile[row][d] * p[row][lane]: p's accumulator registers (split in place) are the B operand,
// the tile comes back transposed from its row-major image through ds_read_b64_tr_b16
template <int NP>
__device__ __forceinline__ void acc_tile_t_x_p(f32x16 (&o)[4], const __bf16* trimg, const f32x16& p, int lane) {
    const int lh = lane >> 5, tq = (lane & 15) >> 2, tp = lane & 3, tg = (lane >> 4) & 1;
    const __bf16* base = trimg + (4 * lh + tq) * TSTR + 16 * tg + 4 * tp;
    bf16x8 ph[2], pl[2];
#pragma unroll
    for (int ss = 0; ss < 2; ++ss)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float pv = p[8 * ss + e];
            const __bf16 h = (__bf16)pv;
            ph[ss][e] = h;
            pl[ss][e] = (__bf16)(pv - (float)h);
        }
    auto frag = [&](const __bf16* q) __attribute__((always_inline)) {
        const bf16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(q));
        const bf16x4 c = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_ptr)(q + 8 * TSTR));
        bf16x8 f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            f[e] = a[e];
            f[4 + e] = c[e];
        }
        return f;
    };
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const bf16x8 th = frag(base + 16 * ss * TSTR + 32 * dt);
            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, ph[ss], o[dt], 0, 0, 0);
            if (NP == 3) {
                const bf16x8 tl = frag(base + TIMG + 16 * ss * TSTR + 32 * dt);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(th, pl[ss], o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tl, ph[ss], o[dt], 0, 0, 0);
            }
        }
}

// write a wave's [4][32 d x 32 lane-rows] accumulators as 32 rows of 128 floats (row stride ld) through an fp32 LDS patch
__device__ __forceinline__ void store_rows(const f32x16 (&o)[4], float* patch, float* out, long ld, int l31, int lh) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = o[dt][4 * g + c];
            *(f32x4*)(patch + l31 * OLD + dt * 32 + 8 * g + 4 * lh) = v;
        }
#pragma unroll
    for (int it = 0; it < 16; ++it) {
        const int row = it * 2 + lh;
        *(f32x4*)(out + (long)row * ld + l31 * 4) = *(const f32x4*)(patch + row * OLD + l31 * 4);
    }
}
template <int NP> constexpr int rimg_pair() { return (NP == 3 ? 2 : 1) * RIMG; }
template <int NP> constexpr int timg_pair() { return (NP == 3 ? 2 : 1) * TIMG; }
}  // namespace attnbf
