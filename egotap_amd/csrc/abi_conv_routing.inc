// Fragment of egotap_abi.hip, included there exactly once; it includes nothing.  The order of the fragments there fixes hipcc's schedules.
// The fp32-tensor convolution routing of the estimators' forward and training: the convolution tiles and conv_any.
//                      taps stride log2W CO_T WCO WPX CI_S
using C3s1_128_co64 = ConvCfg<9, 1, 7,  64, 2, 4, 8>;    // 128-wide maps: 512x512 RGB (BASELINE config 5)
using C3s1_128      = ConvCfg<9, 1, 7, 128, 2, 4, 8>;
using C3s2_64       = ConvCfg<9, 2, 6,  64, 2, 4, 8>;
using C1s1_128      = ConvCfg<1, 1, 7,  64, 2, 4, 32>;
using C1s2_64       = ConvCfg<1, 2, 6,  64, 2, 4, 8>;
using C3s1_64_co64  = ConvCfg<9, 1, 6,  64, 2, 4, 8>;
using C3s1_64       = ConvCfg<9, 1, 6, 128, 2, 4, 8>;
using C3s1_32       = ConvCfg<9, 1, 5, 128, 2, 4, 8>;
using C3s1_16       = ConvCfg<9, 1, 4, 128, 2, 4, 8>;
using C3s1_8        = ConvCfg<9, 1, 3, 128, 2, 4, 8>;
using C3s1_16_co64  = ConvCfg<9, 1, 4,  64, 2, 4, 8>;    // [r3] the same two widths with 64-channel tiles: twice the workgroups where 128-channel
using C3s1_8_co64   = ConvCfg<9, 1, 3,  64, 2, 4, 8>;    // tiles leave CUs without one (training batches, serving batches); same bits (k order unchanged)
using C3s2_32       = ConvCfg<9, 2, 5,  64, 2, 4, 8>;
using C3s2_16       = ConvCfg<9, 2, 4,  64, 2, 4, 8>;
using C3s2_8        = ConvCfg<9, 2, 3,  64, 2, 4, 8>;
using C1s1_64       = ConvCfg<1, 1, 6,  64, 2, 4, 32>;
using C1s1_32       = ConvCfg<1, 1, 5, 128, 2, 4, 32>;
using C1s1_16       = ConvCfg<1, 1, 4, 128, 2, 4, 32>;
using C1s1_8        = ConvCfg<1, 1, 3, 128, 2, 4, 32>;
using C1s2_32       = ConvCfg<1, 2, 5,  64, 2, 4, 8>;
using C1s2_16       = ConvCfg<1, 2, 4,  64, 2, 4, 8>;
using C1s2_8        = ConvCfg<1, 2, 3,  64, 2, 4, 8>;

template <class Cfg>
static hipError_t conv(Handle* h, const char* role, const ConvArgs& a, hipStream_t s) {
    static const std::string kname = std::string("conv_f32_kernel<") + (Cfg::TAPS == 9 ? "3x3" : "1x1") + ",s" +
                                     std::to_string(Cfg::STRIDE) + ",W" + std::to_string(Cfg::W) + ",co" +
                                     std::to_string(Cfg::CO_T) + ">";
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * a.Cout * a.Cin * Cfg::TAPS * (double)a.Nimg * Cfg::W * Cfg::W);
    ConvArgs b = a;
    b.part = h->conv_part;
    b.part_floats = h->conv_part_floats;
    return conv_f32_launch<Cfg>(b, s, device_cu_count());
}

// any other output width (conv_f32_any_kernel: pixel tiles over the flattened (image, y, x) map)
template <int TAPS, int STRIDE, int CO_T, int PX_T>
static hipError_t conv_gen(Handle* h, const char* role, int wout, const ConvArgs& a, hipStream_t s) {
    using Cfg = ConvAnyCfg<TAPS, STRIDE, CO_T, PX_T>;
    static const std::string kname = std::string("conv_f32_any_kernel<") + (TAPS == 9 ? "3x3" : "1x1") + ",s" + std::to_string(STRIDE) +
                                     ",co" + std::to_string(CO_T) + ",px" + std::to_string(PX_T) + ">";
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * a.Cout * a.Cin * TAPS * (double)a.Nimg * wout * wout);
    return conv_f32_any_launch<Cfg>(a, wout, s);
}
// tile shape by grid size: 128 x 256 (64 x 256 for Cout <= 64) while that fills the CUs, then 64 x 256, then 64 x 64 (same bits: same k order)
template <int TAPS, int STRIDE>
static hipError_t conv_gen_co(Handle* h, const char* role, int wout, const ConvArgs& a, hipStream_t s) {
    const long t256 = ((long)a.Nimg * wout * wout + 255) / 256, cus = device_cu_count();
    if (a.Cout > 64 && t256 * ((a.Cout + 127) / 128) >= cus) return conv_gen<TAPS, STRIDE, 128, 256>(h, role, wout, a, s);
    if (t256 * ((a.Cout + 63) / 64) >= cus) return conv_gen<TAPS, STRIDE, 64, 256>(h, role, wout, a, s);
    return conv_gen<TAPS, STRIDE, 64, 64>(h, role, wout, a, s);
}

template <class Cfg>
static hipError_t conv_bf(Handle* h, const char* role, const ConvArgs& a, hipStream_t s) {
    static const std::string kname = std::string("conv_bf16_kernel<3x3,s1,W") + std::to_string(Cfg::W) + (Cfg::NP == 3 ? ",bf16x3>" : ",bf16>");
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * a.Cout * a.Cin * 9 * (double)a.Nimg * Cfg::W * Cfg::W);
    return conv_bf16_launch<Cfg>(a, h->conv_pack, s);
}

// dispatch on (taps, stride, output width): the power-of-two instantiations at wout in {128, 64, 32, 16, 8} (where they exist), every
// other width >= 1 on conv_f32_any_kernel (exact fp32 in every precision mode)
static hipError_t conv_any(Handle* h, const char* role, int taps, int stride, int wout, const ConvArgs& a, hipStream_t s) {
    // opt-in modes: 3x3 stride-1 convs with a multiple of 128 output channels at widths 64 / 32 / 16 run on the bf16 matrix cores
    if (h->precision != EGOTAP_PREC_F32 && h->conv_pack && taps == 9 && stride == 1 && a.Cout >= 128) {
        const bool x3 = h->precision == EGOTAP_PREC_BF16X3;
        if (wout == 64) return x3 ? conv_bf<ConvBfCfg<6, 3>>(h, role, a, s) : conv_bf<ConvBfCfg<6, 1>>(h, role, a, s);
        if (wout == 32) return x3 ? conv_bf<ConvBfCfg<5, 3>>(h, role, a, s) : conv_bf<ConvBfCfg<5, 1>>(h, role, a, s);
        if (wout == 16) return x3 ? conv_bf<ConvBfCfg<4, 3>>(h, role, a, s) : conv_bf<ConvBfCfg<4, 1>>(h, role, a, s);
        if (wout == 8) return x3 ? conv_bf<ConvBfCfg<3, 3>>(h, role, a, s) : conv_bf<ConvBfCfg<3, 1>>(h, role, a, s);
    }
    if (h->precision != EGOTAP_PREC_F32 && h->conv_pack && taps == 9 && stride == 1 && a.Cout == 64 && wout == 64)   // ResNet layer1
        return h->precision == EGOTAP_PREC_BF16X3 ? conv_bf<ConvBfCfg<6, 3, 64>>(h, role, a, s) : conv_bf<ConvBfCfg<6, 1, 64>>(h, role, a, s);
    if (h->precision == EGOTAP_PREC_BF16 && h->conv_pack && taps == 9 && stride == 1 && a.Cout == 64 && wout == 128)   // layer1 at 512x512 RGB
        return conv_bf<ConvBfCfg<7, 1, 64>>(h, role, a, s);
    if (taps == 9 && stride == 1) {
        if (wout == 128) return a.Cout <= 64 ? conv<C3s1_128_co64>(h, role, a, s) : conv<C3s1_128>(h, role, a, s);
        if (wout == 64) return a.Cout <= 64 ? conv<C3s1_64_co64>(h, role, a, s) : conv<C3s1_64>(h, role, a, s);
        if (wout == 32) return conv<C3s1_32>(h, role, a, s);
        // layer3 / layer4 at a 32-frame training batch: 128 / 64 workgroups of 128-channel tiles for 256 CUs (MFMA busy 0.21 on the 8 x 8 maps)
        const long co128 = (a.Cout + 127) / 128;
        if (wout == 16) return (long)a.Nimg * co128 < device_cu_count() ? conv<C3s1_16_co64>(h, role, a, s) : conv<C3s1_16>(h, role, a, s);
        if (wout == 8) return (long)((a.Nimg + 3) / 4) * co128 < device_cu_count() ? conv<C3s1_8_co64>(h, role, a, s) : conv<C3s1_8>(h, role, a, s);
    } else if (taps == 9 && stride == 2) {
        if (wout == 64) return conv<C3s2_64>(h, role, a, s);
        if (wout == 32) return conv<C3s2_32>(h, role, a, s);
        if (wout == 16) return conv<C3s2_16>(h, role, a, s);
        if (wout == 8) return conv<C3s2_8>(h, role, a, s);
    } else if (taps == 1 && stride == 1) {
        if (wout == 128) return conv<C1s1_128>(h, role, a, s);
        if (wout == 64) return conv<C1s1_64>(h, role, a, s);
        if (wout == 32) return conv<C1s1_32>(h, role, a, s);
        if (wout == 16) return conv<C1s1_16>(h, role, a, s);
        if (wout == 8) return conv<C1s1_8>(h, role, a, s);
    } else if (taps == 1 && stride == 2) {
        if (wout == 64) return conv<C1s2_64>(h, role, a, s);
        if (wout == 32) return conv<C1s2_32>(h, role, a, s);
        if (wout == 16) return conv<C1s2_16>(h, role, a, s);
        if (wout == 8) return conv<C1s2_8>(h, role, a, s);
    }
    if (wout < 1) return hipErrorInvalidValue;
    if (taps == 9 && stride == 1) return conv_gen_co<9, 1>(h, role, wout, a, s);
    if (taps == 9 && stride == 2) return conv_gen_co<9, 2>(h, role, wout, a, s);
    if (taps == 1 && stride == 1) return conv_gen_co<1, 1>(h, role, wout, a, s);
    if (taps == 1 && stride == 2) return conv_gen_co<1, 2>(h, role, wout, a, s);
    return hipErrorInvalidValue;
}
