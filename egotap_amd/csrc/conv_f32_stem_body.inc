// The body of stem_conv7_mfma_kernel<BF16OUT> (conv_f32.h), included once per patch SOURCE: as it stands it reads the normalised fp32 planar frames (`left`,
// `right`); with STEM_SRC_U8 defined it reads the camera's bytes (`left8`, `right8`: uint8 [B, HIN, HIN, 3]; `table` fp32 [3][256]) and BF16OUT is false.
// A textual include on purpose: the fp32-source kernels are token for token what they were before the byte source existed, so their code objects are too.
    using Cfg = StemCfg;
    constexpr int RG = Cfg::RG, XT = Cfg::XT, PR = Cfg::PR, PC = Cfg::PC, PLD = Cfg::PLD, KP = Cfg::KP, THREADS = Cfg::THREADS;
    extern __shared__ __attribute__((aligned(16))) float stem_sm[];
    float* xs = stem_sm;                          // [3][PR][PLD]
    float* ws = stem_sm + Cfg::XS_FLOATS;         // [KP][64]
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, lh = lane >> 5;
    const int HO = HIN / 2, xsegs = HO / XT, ygroups = HO / RG;
    const long items = (long)nimg * ygroups * xsegs;
    for (int i = tid; i < KP * 64; i += THREADS) {
        const int k = i >> 6, co = i & 63;
        ws[i] = k < 147 ? w[co * 147 + k] : 0.f;
    }
#ifdef STEM_SRC_U8
    for (int i = tid; i < 3 * 256; i += THREADS) stem_sm[Cfg::XS_FLOATS + Cfg::WS_FLOATS + i] = table[i];      // the value table, behind the weights
#endif
    // per-lane BatchNorm constants of its two output channels (eval mode); gamma == nullptr: raw convolution output (training)
    float sc[2] = {1.f, 1.f}, sh[2] = {0.f, 0.f};
    if (gamma != nullptr) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            const int co = nt * 32 + l31;
            sc[nt] = gamma[co] / sqrtf(var[co] + 1e-5f);
            sh[nt] = beta[co] - mean[co] * sc[nt];
        }
    }
#ifdef STEM_SRC_U8
    // the byte source: an item of a thread is four pixels of one row = three aligned dwords (groups aligned to four pixels in the image, so a group is
    // inside the frame or outside it as a whole); pixel e of group gg is patch column 4 gg - 1 + e.  Nine registers cross the MFMAs instead of 33;
    // publish() looks every byte up in the fp32 table behind the weights, pixels outside the image are 0.0 (not table[c][0]).
    constexpr int NG = StemU8::NG, ITEMS = PR * NG, NIT = (ITEMS + THREADS - 1) / THREADS;      // 66 groups, 1386 items, 3 per thread
    const float* tab = stem_sm + Cfg::XS_FLOATS + Cfg::WS_FLOATS;
    unsigned raw[NIT][3], okmask = 0u;
    auto request = [&](long item) __attribute__((always_inline)) {
        const int xseg_ = (int)(item % xsegs), yg_ = (int)((item / xsegs) % ygroups);
        const int n_ = (int)(item / ((long)xsegs * ygroups));
        const unsigned char* src = ((n_ & 1) ? right8 : left8) + (long)(n_ >> 1) * 3 * HIN * HIN;
        const int iy0 = yg_ * RG * 2 - 3, gx0 = xseg_ * XT * 2 - 4;
        okmask = 0u;
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int i = tid + j * THREADS;
            const int yy = i / NG, gg = i - yy * NG;
            const int y = iy0 + yy, x = gx0 + 4 * gg;
            const bool ok = i < ITEMS && y >= 0 && y < HIN && x >= 0 && x + 3 < HIN;
            const unsigned* rp = (const unsigned*)(src + ((long)y * HIN + x) * 3);
#pragma unroll
            for (int k = 0; k < 3; ++k) raw[j][k] = ok ? rp[k] : 0u;
            okmask |= ok ? (1u << j) : 0u;
        }
    };
    auto publish = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NIT; ++j) {
            const int i = tid + j * THREADS;
            const int yy = i / NG, gg = i - yy * NG;
            if (i >= ITEMS) continue;
            const bool ok = (okmask >> j) & 1u;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int bi = 3 * e + c, xx = 4 * gg - 1 + e;
                    const unsigned b = (raw[j][bi >> 2] >> (8 * (bi & 3))) & 255u;
                    if (xx >= 0 && xx < PC) xs[(c * PR + yy) * PLD + xx] = ok ? tab[c * 256 + b] : 0.f;
                }
        }
    };
#else
    // the patch of the NEXT item is requested into registers before the MFMAs of the current one and written to LDS behind them
    constexpr int NPRE = (3 * PR * PC + THREADS - 1) / THREADS;
    float pre[NPRE];
    auto request = [&](long item) __attribute__((always_inline)) {
        const int xseg_ = (int)(item % xsegs), yg_ = (int)((item / xsegs) % ygroups);
        const int n_ = (int)(item / ((long)xsegs * ygroups));
        const float* src = ((n_ & 1) ? right : left) + (long)(n_ >> 1) * 3 * HIN * HIN;
        const int iy0 = yg_ * RG * 2 - 3, ix0 = xseg_ * XT * 2 - 3;
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int i = tid + j * THREADS;
            const int c = i / (PR * PC), rem = i - c * PR * PC, yy = rem / PC, xx = rem - yy * PC;
            const int y = iy0 + yy, x = ix0 + xx;
            pre[j] = (i < 3 * PR * PC && y >= 0 && y < HIN && x >= 0 && x < HIN) ? src[((long)c * HIN + y) * HIN + x] : 0.f;
        }
    };
    auto publish = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NPRE; ++j) {
            const int i = tid + j * THREADS;
            const int c = i / (PR * PC), rem = i - c * PR * PC, yy = rem / PC, xx = rem - yy * PC;
            if (i < 3 * PR * PC) xs[(c * PR + yy) * PLD + xx] = pre[j];
        }
    };
#endif
    if ((long)blockIdx.x < items) request(blockIdx.x);
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const int xseg = (int)(it % xsegs), yg = (int)((it / xsegs) % ygroups);
        const int n = (int)(it / ((long)xsegs * ygroups));
        __syncthreads();                          // everyone is done with the previous patch (and the weights are staged)
        publish();
        __syncthreads();
        if (it + gridDim.x < items) request(it + gridDim.x);
        f32x16 acc[4][2];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;
        const float* ap = xs + (2 * wid) * PLD + 2 * l31;        // output row wid, pixel l31 of row tile 0
        const float* bp = ws + lh * 64 + l31;
#pragma unroll
        for (int s2 = 0; s2 < KP / 2; ++s2) {
            constexpr int dummy = 0; (void)dummy;
            const int k0 = 2 * s2, k1 = 2 * s2 + 1;              // this lane half multiplies k = k0 + lh
            const int o0 = ((k0 / 49) * PR + (k0 % 49) / 7) * PLD + (k0 % 7);
            const int o1 = k1 < 147 ? ((k1 / 49) * PR + (k1 % 49) / 7) * PLD + (k1 % 7) : 0;
            const int ko = lh ? o1 : o0;
            float a[4], b[2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[mt] = ap[ko + 64 * mt];
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) b[nt] = bp[k0 * 64 + nt * 32];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt], b[nt], acc[mt][nt], 0, 0, 0);
        }
        const int y = yg * RG + wid;
        if constexpr (BF16OUT) {
            // lane = channel: 32 lanes write the 64 contiguous bytes of 32 channels of one pixel (the lane halves: two pixels)
            __bf16* ob = (__bf16*)out + ((((long)(n >> 1) * HO + y) * HO + xseg * XT) * 2 + (n & 1)) * 64 + l31;
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int x = mt * 32 + 8 * (r >> 2) + 4 * lh + (r & 3);
                        const float t = acc[mt][nt][r] * sc[nt] + sh[nt];
                        ob[(long)x * 128 + nt * 32] = (__bf16)(gamma != nullptr ? fmaxf(t, 0.f) : t);
                    }
            continue;
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
            float* dst = out + ((long)n * 64 + nt * 32 + l31) * HO * HO + (long)y * HO + xseg * XT;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v;
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const float t = acc[mt][nt][4 * g + c] * sc[nt] + sh[nt];
                        v[c] = gamma != nullptr ? fmaxf(t, 0.f) : t;
                    }
                    *(f32x4*)(dst + mt * 32 + 8 * g + 4 * lh) = v;
                }
        }
    }
