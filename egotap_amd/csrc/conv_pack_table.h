// The segment table of conv_bf16s.h's one-launch weight repack (pack_all_bf16s_kernel; the story is told there): types only, no kernel and
// no launcher.  The handle keeps the K-slab depth of PackTable::MAXW packed weights per estimator, so every part of the library sees this
// file; only the part that launches the repack includes conv_bf16s.h.
#pragma once

struct PackSeg {
    const float *w, *b;              // [Cout][Cin][taps] weights, bias (1x1 with bias) or null
    unsigned dst_w, dst_b;           // byte offsets into the region: packed bf16 weights, padded fp32 bias
    unsigned short Cout, Cin, Cp, Np;
    short taps, slab;                // slab: input channels per K slab of a 3x3 weight: 32 (gemm_bf16s.h's XConv3 / XConvE) or 64 (gemm_bf16s64.h's X64Conv3)
    int first_block;
};
struct BnSeg {
    const float *g, *b, *m, *v;
    unsigned dst_sc, dst_sh;
    unsigned short C, Np;
    int first_block;
};
struct PackTable {
    static constexpr int MAXW = 44, MAXB = 36;        // resnet34: 32 + 3 + 8 convolutions, 35 BatchNorms
    PackSeg w[MAXW];
    BnSeg bn[MAXB];
    int nw, nb, blocks_w, blocks;
};
static_assert(sizeof(PackTable) <= 4000, "the table is a kernel argument");
