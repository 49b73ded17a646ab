// Fragment of egotap_abi.hip, included there exactly once; it includes nothing.  The order of the fragments there fixes hipcc's schedules.
// The encoders' fc1 on the bf16-storage GEMMs.
// fc1 of an encoder (rows gathered from the ViT tokens / the limb heatmaps) as an NT product: [r5] on the 64-deep kernel where its shape rules hold
// (D, HW multiples of 64: a K-tile inside one token / map), the 32-deep kernel otherwise or when egotap_debug_gemm_bk pins it; same k order per
// output element: same bits
template <class Epi>
static hipError_t fc1_nt(Handle* h, int which, const __bf16* src, const __bf16* w, long K, const Epi& ep, int BT, int cus, hipStream_t s) {
    const int HW = h->cfg.hm_size * h->cfg.hm_size;
    const bool deep = g_gemm_bf16s_bk != 32 && K % 64 == 0 && K >= 128 && (which == 0 ? h->D % 64 == 0 : HW % 64 == 0) && (long)256 * K * 2 < (1L << 31);
    if (which == 0) {
        // [r5] tensors under 4 GB (every shipped batch): scalar origin + 32-bit lane offsets (X64TokensS / X64RotS); the pointer loaders otherwise
        const size_t tok_bytes = (size_t)(BT / h->T) * h->seq * h->D * 2;
        if (deep && g_conv_addressing == 0 && tok_bytes < ((size_t)1 << 32) - 4096)
            return gemm_bf16s64_launch_x(X64TokensS{src, 0u, h->tokens()}, w, K, ep, BT, 2048, (int)K, cus, s);
        if (deep) return gemm_bf16s64_launch_x(X64Tokens{src, h->tokens()}, w, K, ep, BT, 2048, (int)K, cus, s);
        return gemm_bf16s_launch(XTokens{src, h->tokens()}, w, K, ep, BT, 2048, (int)K, cus, s);
    }
    const size_t hm_bytes = (size_t)(BT / (2 * h->J)) * h->C * HW * 2;
    if (deep && g_conv_addressing == 0 && hm_bytes < ((size_t)1 << 32) - 4096) return gemm_bf16s64_launch_x(X64RotS{src, 0u, h->rots()}, w, K, ep, BT, 2048, (int)K, cus, s);
    if (deep) return gemm_bf16s64_launch_x(X64Rot{src, h->rots()}, w, K, ep, BT, 2048, (int)K, cus, s);
    return gemm_bf16s_launch(XRot{src, h->rots()}, w, K, ep, BT, 2048, (int)K, cus, s);
}
