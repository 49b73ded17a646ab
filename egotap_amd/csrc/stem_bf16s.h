// [r3] The ResNet stem of the bf16 estimators as ONE kernel on the bf16 matrix cores:
//     conv 7x7 / 2 pad 3 (3 -> 64) + BatchNorm(eval) + ReLU + MaxPool2d(3, 2, 1)      (torchvision resnet18.conv1 / bn1 / relu / maxpool
// via net_architecture.py:69-70), fp32 NCHW RGB in, bf16 channels-last eye-interleaved out ([B * HP * HP, 2 x 64], HP = S0 / 4: the
// layout conv_bf16s.h's stages read).  It replaces stem_conv7_mfma_kernel<true> (fp32 MFMA at 1/16 of the bf16 rate; wrote the
// 128 x 128 x 64 map, 1.07 GB per 256 stereo frames) + maxpool3s2_nhwc_bf16s_kernel (read it back): the stem's output feeds nothing
// but the max-pool (AfterBackbone never uses layer0, net_architecture.py:146-171), so it never has to reach HBM.
//
//   * Implicit GEMM on v_mfma_f32_32x32x16_bf16 with A = weights (row = output channel), B = input patch (column = stem pixel).  K is
//     ordered (c, ky, kx) with kx padded from 7 to 8, so the 8 k of a lane's B fragment are 8 CONSECUTIVE input pixels of one
//     (channel, row) of the patch: four ds_read_b32 at 4-byte alignment, consecutive lanes on consecutive dwords (conflict-free).
//     21 (c, ky) rows pad to 22 = 11 MFMA steps of two rows (lane half h takes row 2 step + h); the padded taps carry zero weights.
//     All A fragments (64 channels x 176 k) live in registers for the whole kernel: 88 VGPRs, no LDS traffic for weights.
//   * A workgroup (4 waves, 74 KB of LDS: two per CU, one stages while the other multiplies) is persistent over runs (image, group of
//     R = 8 pooled rows) and walks a run in 64-column segments of the stem map; per segment the input patch (39 rows x 136 columns x 3
//     channels, zero halo, converted to bf16 on the way) sits in LDS.  A segment walks 17 stem rows in pairs (waves 0-1 / 2-3 take
//     the two rows, one 32-pixel tile each): 22 MFMAs per wave and row, BatchNorm + ReLU on the accumulators, bf16 rows into a four-slot
//     LDS ring; after every pair the whole workgroup pools one output row out of three ring rows (one thread = 8 channels of one pooled
//     pixel, nine 16-byte LDS reads, unsigned 16-bit max: post-ReLU bf16 values are ordered like their bit patterns) and stores it.
//   * Max-pool padding: post-ReLU values are >= 0 and every window holds a valid element, so a zero column / row stands in for -inf.
//     The last stem column of a segment is the left neighbour of the next one's first pooling window: carried in LDS.
#pragma once
#include "common.h"
#include "gemm_bf16.h"       // bf16x8
#include "gemm_bf16s.h"      // bf16x4s

struct StemPoolCfg {
    static constexpr int R = 8, SR = 2 * R + 1, PR = 2 * SR + 5;       // pooled rows per item, stem rows, patch rows (39)
    static constexpr int XS = 64, PCOLS = 136, PITCH = 320;            // stem columns per segment, staged patch columns, bytes per patch row
    static constexpr int PATCH_BYTES = 3 * PR * PITCH;                  // 37 440
    static constexpr int RING_ROW = (XS + 1) * 128, RING_BYTES = 4 * RING_ROW;      // [slot][1 + 64 columns][64 channels] bf16
    static constexpr int CARRY_BYTES = 2 * SR * 128;
    static constexpr int OFF_RING = PATCH_BYTES, OFF_CARRY = OFF_RING + RING_BYTES, OFF_BN = OFF_CARRY + CARRY_BYTES;
    static constexpr int LDS_BYTES = OFF_BN + 2 * 128 * 4;            // scale | shift, 64 channels x 2 eyes (MODE 2: per-eye batch statistics)
    static constexpr int THREADS = 256;
    static constexpr int NPRE = (3 * PR * (PCOLS / 2) + THREADS - 1) / THREADS;      // column pairs per thread: 32
    static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU");
};

typedef unsigned short u16x8s __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4s __attribute__((ext_vector_type(4)));

// [r5] MODE 0: BatchNorm folded from the running statistics (gamma, beta, mean, var: eval mode).
// MODE 1: STATISTICS ONLY -- the same staging and MFMAs, no BatchNorm / pool / store: every lane sums its 32 (channel, pixel-column) accumulators and
//         their squares over the stem rows its workgroup OWNS (ys >= 1: row ys = 0 of a run is the row group above's last row, computed again only as
//         pooling halo), and the workgroup writes one partial row part[block][eye * 64 + c][2] (`out`, as floats; the other eye's 64 columns zero).
//         The launcher makes the grid a multiple of 2 x (row groups per image), so every run of a workgroup belongs to the same eye.
// MODE 2: BatchNorm with per-eye scale / shift tables (gamma = scale[2][64], beta = shift[2][64], from bn_finish_bf16s_kernel over MODE 1's partials):
//         batch-statistics BatchNorm of the frozen estimators under train.py:91 (bn_bf16s.h).
template <int MODE>
static __global__ __launch_bounds__(StemPoolCfg::THREADS, 2) void stem_pool_bf16s_kernel(
    const float* __restrict__ left, const float* __restrict__ right, const float* __restrict__ w, const float* __restrict__ gamma,
    const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var, __bf16* __restrict__ out, int HIN, int nimg) {
#include "stem_bf16s_body.inc"
}

// [r7] MODE 0 from camera bytes (egotap_hm_forward_u8 / egotap_predict_pose_rgb_u8): the same body behind a byte-source staging.
// Camera bytes: uint8 [B, HIN, HIN, 3] (RGB, contiguous, 4-byte aligned base; a row is 3 HIN bytes, a multiple of 4).  `table` is fp32 [3][256],
// the normalised value per (channel, byte); it sits in LDS as bf16 (the rounding the fp32 staging applies to the fp32 pixel).  An item is four
// pixels of one row = three aligned dwords = 12 table values; the groups are aligned to four pixels in the IMAGE, so a group is inside the image
// or outside it as a whole (HIN is a multiple of 4) and no load touches a byte outside the frame.  Pixels outside the image are 0.0 -- not
// table[c][0]: byte 0 maps to about -2.1 and the halo must stay zero.  Patch column of pixel e of group gg: 4 gg - 1 + e (the patch starts
// three pixels left of a group boundary): 35 groups cover the 136 columns.
struct StemPoolU8 { static constexpr int NG = 35, LDS_EXTRA = 3 * 256 * 2; };
static_assert(2 * (StemPoolCfg::LDS_BYTES + StemPoolU8::LDS_EXTRA) <= 160 * 1024, "two workgroups per CU with the byte source's value table");
static __global__ __launch_bounds__(StemPoolCfg::THREADS, 2) void stem_pool_bf16s_u8_kernel(
    const unsigned char* __restrict__ left8, const unsigned char* __restrict__ right8, const float* __restrict__ table, const float* __restrict__ w,
    const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean, const float* __restrict__ var,
    __bf16* __restrict__ out, int HIN, int nimg) {
    constexpr int MODE = 0;
#define STEM_SRC_U8 1
#include "stem_bf16s_body.inc"
#undef STEM_SRC_U8
}

template <int MODE>
static inline hipError_t stem_pool_bf16s_launch_mode(const float* left, const float* right, const float* w, const float* gamma, const float* beta,
                                                     const float* mean, const float* var, __bf16* out, int HIN, int nimg, int num_cu, hipStream_t s, int* grid_out = nullptr) {
    using Cfg = StemPoolCfg;
    const int HO = HIN / 2, HP = HIN / 4;
    if (HO % Cfg::XS != 0 || HP % Cfg::R != 0 || nimg <= 0) return hipErrorInvalidValue;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)stem_pool_bf16s_kernel<MODE>, Cfg::LDS_BYTES); e != hipSuccess) return e;
    const int groups = HP / Cfg::R;
    const long runs = (long)nimg * groups;
    long grid = runs < 2L * num_cu ? runs : 2L * num_cu;
    if (MODE == 1) {           // every run of a workgroup in ONE eye: run = block + k * grid, image = run / groups -> the grid a multiple of 2 * groups
        if (nimg % 2 != 0) return hipErrorInvalidValue;
        grid = grid / (2 * groups) * (2 * groups);
        if (grid <= 0) return hipErrorInvalidValue;
    }
    if (grid_out) *grid_out = (int)grid;
    hipLaunchKernelGGL(stem_pool_bf16s_kernel<MODE>, dim3((unsigned)grid), dim3(Cfg::THREADS), Cfg::LDS_BYTES, s, left, right, w, gamma, beta, mean, var, out, HIN, nimg);
    return hipGetLastError();
}
static inline hipError_t stem_pool_bf16s_launch(const float* left, const float* right, const float* w, const float* gamma, const float* beta,
                                                const float* mean, const float* var, __bf16* out, int HIN, int nimg, int num_cu, hipStream_t s) {
    return stem_pool_bf16s_launch_mode<0>(left, right, w, gamma, beta, mean, var, out, HIN, nimg, num_cu, s);
}
// the byte source: the same grid rule; frames uint8 [nimg / 2, HIN, HIN, 3] per eye, table fp32 [3][256]
static inline hipError_t stem_pool_bf16s_u8_launch(const unsigned char* left, const unsigned char* right, const float* table, const float* w, const float* gamma,
                                                   const float* beta, const float* mean, const float* var, __bf16* out, int HIN, int nimg, int num_cu, hipStream_t s) {
    using Cfg = StemPoolCfg;
    constexpr int LDS = Cfg::LDS_BYTES + StemPoolU8::LDS_EXTRA;
    const int HO = HIN / 2, HP = HIN / 4;
    if (HO % Cfg::XS != 0 || HP % Cfg::R != 0 || nimg <= 0) return hipErrorInvalidValue;
    if (hipError_t e = ego_allow_dynamic_lds((const void*)stem_pool_bf16s_u8_kernel, LDS); e != hipSuccess) return e;
    const long runs = (long)nimg * (HP / Cfg::R);
    const long grid = runs < 2L * num_cu ? runs : 2L * num_cu;
    hipLaunchKernelGGL(stem_pool_bf16s_u8_kernel, dim3((unsigned)grid), dim3(Cfg::THREADS), LDS, s, left, right, table, w, gamma, beta, mean, var, out, HIN, nimg);
    return hipGetLastError();
}
