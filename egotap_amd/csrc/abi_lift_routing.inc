// Fragment of egotap_abi.hip, included there exactly once; it includes nothing.  The order of the fragments there fixes hipcc's schedules.
// What the lifting head's forward and its training operators share: GEMM tiles and routing, parameter resolver, the propagation units' residency probe.
// ------------------------------------------------------------------------------------------------ tiles
using TileA = GemmCfg<128, 128, 32, 2, 2, 2>;   // 4 waves, 64x64 per wave, 2 blocks/CU
using TileB = GemmCfg<256, 128, 32, 4, 2, 2>;   // 8 waves, 64x64 per wave, 1 block/CU
using TileC = GemmCfg<128, 256, 32, 2, 4, 2>;   // 8 waves, 64x64 per wave, 1 block/CU
using TileD = GemmCfg<256, 256, 16, 4, 2, 2>;   // 8 waves, 64x128 per wave, 1 block/CU
using TileE = GemmCfg<256, 128, 16, 2, 2, 2>;   // 4 waves, 128x64 per wave, 2 blocks/CU
using TileF = GemmCfg<64, 64, 32, 2, 2, 2>;     // 4 waves, 32x32 per wave (small problems)
using TileG = GemmCfg<256, 128, 32, 2, 2, 1>;   // 4 waves, 128x64 per wave, 1 block/CU
using TileS = GemmCfg<64, 128, 32, 2, 4, 1>;    // [r4] 8 waves, 32x32 per wave (two waves per SIMD when the workgroup is alone on its CU: -1.8 % on a B = 1 forward against 4 waves): GEMMs of at most 64 rows (the encoders' fc layers and the PU projections at B <= 2-4) --
                                                // on the 128-row tile a 30-row product is paced by its MFMAs on 98 rows of zeros (fc1 at B = 1: 1.7 TB/s of weights)
using PipeA = PipeCfg<128, 128, 16, 2, 2, 2>;   // pipelined: 3 x 20 KiB slabs, 2 blocks/CU
using PipeB = PipeCfg<128, 128, 32, 2, 2, 1>;   // pipelined: 3 x 36 KiB slabs, 1 block/CU
using PipeC = PipeCfg<256, 128, 16, 4, 2, 2>;   // pipelined, 8 waves: 3 x 30 KiB slabs, 1 block/CU
using PipeD = PipeCfg<256, 256, 16, 4, 2, 2>;   // pipelined, 8 waves 64x128 per wave: 3 x 40 KiB slabs

typedef std::unordered_map<std::string, Param> ParamMap;
static const float* P(Handle*, const ParamMap& m, const std::string& key, bool& ok) {
    auto it = m.find(key);
    if (it == m.end()) {
        if (ok) egotap_set_error("'%s' is not bound", key.c_str());
        ok = false;
        return nullptr;
    }
    return (const float*)it->second.ptr;
}

// fills a LiftParams from a key -> pointer map: the parameters (with_stats: and the BatchNorm running statistics) or their gradients
static int lift_resolve_into(Handle* h, const ParamMap& N, LiftParams& p, bool with_stats) {
    bool ok = true;
    const std::string v = "pos_heatmap_encoder.vit.";
    p.mask_tok = P(h, N, v + "embeddings.mask_token", ok);
    p.pos_emb = P(h, N, v + "embeddings.position_embeddings", ok);
    p.patch_w = P(h, N, v + "embeddings.patch_embeddings.projection.weight", ok);
    p.patch_b = P(h, N, v + "embeddings.patch_embeddings.projection.bias", ok);
    for (int i = 0; i < h->cfg.vit_layers; ++i) {
        const std::string l = v + "encoder.layer." + std::to_string(i) + ".";
        auto& L = p.layer[i];
        L.q_w = P(h, N, l + "attention.attention.query.weight", ok); L.q_b = P(h, N, l + "attention.attention.query.bias", ok);
        L.k_w = P(h, N, l + "attention.attention.key.weight", ok);   L.k_b = P(h, N, l + "attention.attention.key.bias", ok);
        L.v_w = P(h, N, l + "attention.attention.value.weight", ok); L.v_b = P(h, N, l + "attention.attention.value.bias", ok);
        L.o_w = P(h, N, l + "attention.output.dense.weight", ok);    L.o_b = P(h, N, l + "attention.output.dense.bias", ok);
        L.up_w = P(h, N, l + "intermediate.dense.weight", ok);       L.up_b = P(h, N, l + "intermediate.dense.bias", ok);
        L.dn_w = P(h, N, l + "output.dense.weight", ok);             L.dn_b = P(h, N, l + "output.dense.bias", ok);
        L.ln1_g = P(h, N, l + "layernorm_before.weight", ok);        L.ln1_b = P(h, N, l + "layernorm_before.bias", ok);
        L.ln2_g = P(h, N, l + "layernorm_after.weight", ok);         L.ln2_b = P(h, N, l + "layernorm_after.bias", ok);
    }
    p.lnf_g = P(h, N, v + "layernorm.weight", ok);
    p.lnf_b = P(h, N, v + "layernorm.bias", ok);
    const char* encs[2] = {"pos_heatmap_encoder", "rot_heatmap_encoder"};
    for (int e = 0; e < 2; ++e)
        for (int i = 0; i < 3; ++i) {
            const std::string f = std::string(encs[e]) + ".fc" + std::to_string(i + 1);
            LiftParams::Fc& fc = e == 0 ? p.pos_fc[i] : p.rot_fc[i];
            fc.w = P(h, N, f + ".fc.weight", ok);        fc.b = P(h, N, f + ".fc.bias", ok);
            fc.g = P(h, N, f + ".bn.weight", ok);        fc.beta = P(h, N, f + ".bn.bias", ok);
            fc.mean = fc.var = nullptr;
            if (with_stats) { fc.mean = P(h, N, f + ".bn.running_mean", ok); fc.var = P(h, N, f + ".bn.running_var", ok); }
        }
    const std::string c = "skel_sequential_layer.lstm_custom.layers.";
    p.x2f0_w = P(h, N, c + "0.x2f.weight", ok); p.x2f0_b = P(h, N, c + "0.x2f.bias", ok);
    p.x2h0_w = P(h, N, c + "0.x2h.weight", ok); p.x2h0_b = P(h, N, c + "0.x2h.bias", ok);
    p.b2h0_w = P(h, N, c + "0.b2h.weight", ok); p.b2h0_b = P(h, N, c + "0.b2h.bias", ok);
    p.h2h0_w = P(h, N, c + "0.h2h.weight", ok); p.h2h0_b = P(h, N, c + "0.h2h.bias", ok);
    p.x2f1_w = P(h, N, c + "1.x2f.weight", ok); p.x2f1_b = P(h, N, c + "1.x2f.bias", ok);
    p.x2h1_w = P(h, N, c + "1.x2h.weight", ok); p.x2h1_b = P(h, N, c + "1.x2h.bias", ok);
    p.h2h1_w = P(h, N, c + "1.h2h.weight", ok); p.h2h1_b = P(h, N, c + "1.h2h.bias", ok);
    p.pose_w = P(h, N, "pose_mlp.pose_fcs.0.weight", ok); p.pose_b = P(h, N, "pose_mlp.pose_fcs.0.bias", ok);
    p.glob_w = p.glob_b = nullptr;
    if (h->cfg.estimate_head) {
        p.glob_w = P(h, N, "global_mlp.pose_fcs.0.weight", ok);
        p.glob_b = P(h, N, "global_mlp.pose_fcs.0.bias", ok);
    }
    return ok ? EGOTAP_OK : EGOTAP_ERR_UNBOUND;
}

static int lift_resolve(Handle* h) {
    if (h->lift_resolved) return EGOTAP_OK;
    const int rc = lift_resolve_into(h, h->bound[EGOTAP_NET_LIFT], h->lp, true);
    if (rc != EGOTAP_OK) return rc;
    h->lift_resolved = true;
    return EGOTAP_OK;
}

template <class AL> struct AlName;
template <> struct AlName<ALoadPlain> { static constexpr const char* v = "ALoadPlain"; };
template <> struct AlName<ALoadPatch> { static constexpr const char* v = "ALoadPatch"; };
template <> struct AlName<ALoadTokens> { static constexpr const char* v = "ALoadTokens"; };
template <> struct AlName<ALoadLive> { static constexpr const char* v = "ALoadLive"; };
template <> struct AlName<ALoadHead> { static constexpr const char* v = "ALoadHead"; };
template <> struct AlName<ALoadRot> { static constexpr const char* v = "ALoadRot"; };
template <> struct AlName<ALoadStereo> { static constexpr const char* v = "ALoadStereo"; };
template <> struct AlName<ALoadStereoGated> { static constexpr const char* v = "ALoadStereoGated"; };
template <class E> struct EpiName;
template <> struct EpiName<EpiBias> { static constexpr const char* v = "EpiBias"; };
template <> struct EpiName<EpiBiasRes> { static constexpr const char* v = "EpiBiasRes"; };
template <> struct EpiName<EpiBiasResLive> { static constexpr const char* v = "EpiBiasResLive"; };
template <> struct EpiName<EpiBiasHead> { static constexpr const char* v = "EpiBiasHead"; };
template <> struct EpiName<EpiBiasGelu> { static constexpr const char* v = "EpiBiasGelu"; };
template <> struct EpiName<EpiBnLrelu> { static constexpr const char* v = "EpiBnLrelu"; };
template <> struct EpiName<EpiPatch> { static constexpr const char* v = "EpiPatch"; };

template <class Cfg, class AL, class Epi>
static hipError_t gemm(Handle* h, const char* role, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc,
                       int M, int N, int K, hipStream_t s) {
    static const std::string kname = std::string("gemm_f32_kernel<") + std::to_string(Cfg::BM) + "x" +
                                     std::to_string(Cfg::BN) + "x" + std::to_string(Cfg::BK) + "," + AlName<AL>::v + "," +
                                     EpiName<Epi>::v + ">";
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * M * N * K);
    return gemm_f32_launch<Cfg, AL, Epi>(al, W, epi, C, ldc, M, N, K, s);
}

// rows of an fp32 matrix (row stride lda) -> dense bf16 [M, K]
static __global__ __launch_bounds__(256) void f32_to_bf16_rows_kernel(const float* __restrict__ src, long lda, __bf16* __restrict__ dst, int k8, long n8) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    const long row = i / k8;
    const float* p = src + row * lda + (i - row * k8) * 8;
    *(bf16x8*)(dst + i * 8) = bf16_round8(*(const f32x4*)p, *(const f32x4*)(p + 4));
}
// plain-bf16 GEMM: W rounded to bf16 into the handle's scratch right before the launch (stream ordered), so the W operand costs
// half the vector-memory bytes; without a scratch (or if it is too small) the kernel converts fp32 weights on the fly.
// A plain row-major activation operand is rounded to bf16 the same way (egotap_set_act_scratch; skipped when the scratch is
// absent or too small) and the product runs on the
// LDS-DMA kernel (gemm_bf16_dma.h): same rounding of both operands, same fp32 accumulation order per output element.
template <class AL, class Epi>
static hipError_t gemm_bf16_plain(Handle* h, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc, int M, int N, int K, hipStream_t s) {
    const int nseg = N / W.seg;
    if (h && h->wscratch && (size_t)N * K * 2 <= h->wscratch_bytes && K % 8 == 0 && W.ld == K && nseg >= 1 && nseg <= 3 && nseg * W.seg == N) {
        SegMatB B;
        for (int i = 0; i < 3; ++i) B.p[i] = h->wscratch + (size_t)(i < nseg ? i : 0) * W.seg * K;
        B.seg = W.seg; B.ld = K;
        const long n8 = (long)W.seg * K / 8;
        for (int i = 0; i < nseg; ++i)
            hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, W.p[i], h->wscratch + (size_t)i * W.seg * K, n8);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if constexpr (std::is_same<AL, ALoadPlain>::value) {
            if (K % DmaCfg::BK == 0 && N % DmaCfg::BN == 0 && W.seg % DmaCfg::BN == 0 && al.lda % 4 == 0 && M >= 1024) {
                __bf16* a = (size_t)M * K * 2 <= h->ascratch_bytes ? h->ascratch : nullptr;
                if (a) {
                    const long a8 = (long)M * K / 8;
                    hipLaunchKernelGGL(f32_to_bf16_rows_kernel, dim3((unsigned)((a8 + 255) / 256)), dim3(256), 0, s, al.A, al.lda, a, K / 8, a8);
                    e = hipGetLastError();
                    if (e != hipSuccess) return e;
                    return gemm_bf16_dma_launch(a, (long)K, B, epi, C, ldc, M, N, K, device_cu_count(), s);
                }
            }
        }
        return gemm_bf16_persist_launch<BfCfg<1, 1>, AL, Epi, SegMatB>(al, B, epi, C, ldc, M, N, K, device_cu_count(), s);
    }
    return gemm_bf16_persist_launch<BfCfg<1, 1>, AL, Epi>(al, W, epi, C, ldc, M, N, K, device_cu_count(), s);
}

// large GEMMs (ViT projections, fc1): 256x256 tile, 3-stage pipelined kernel -- fewest global-load
// instructions per MFMA (each costs the matrix pipe ~56 cycles, tools/mfma_probe.hip), DESIGN.md section 4
template <class AL, class Epi>
static hipError_t gemm_big(Handle* h, const char* role, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc,
                           int M, int N, int K, hipStream_t s) {
    using Cfg = PipeD;
    if (h && h->precision == EGOTAP_PREC_BF16X3) {
        static const std::string kname3 = std::string("gemm_bf16_persist_kernel<256x256x16,bf16x3,") + AlName<AL>::v + "," + EpiName<Epi>::v + ">";
        GemmTimer t(h, s, role, kname3.c_str(), 2.0 * M * N * K);
        return gemm_bf16_persist_launch<BfCfg<3, 1>, AL, Epi>(al, W, epi, C, ldc, M, N, K, device_cu_count(), s);
    }
    if (h && h->precision == EGOTAP_PREC_BF16) {
        static const std::string kname1 = std::string("gemm_bf16_persist_kernel<256x256x32,bf16,") + AlName<AL>::v + "," + EpiName<Epi>::v + ">";
        GemmTimer t(h, s, role, kname1.c_str(), 2.0 * M * N * K);
        return gemm_bf16_plain(h, al, W, epi, C, ldc, M, N, K, s);
    }
    if constexpr (AL::HAS_PTR) {
        // loaders that are pure address math: same tile, same k order (bit-identical), slabs staged global -> LDS by DMA (gemm_f32_dma.h)
        if (N % DmaF32Cfg::BN == 0 && K % DmaF32Cfg::BK == 0 && W.seg % DmaF32Cfg::BN == 0 && W.ld % 4 == 0 && al.dma_ok()) {
            static const std::string kdma = std::string("gemm_f32_dma_kernel<256x256x16,") + AlName<AL>::v + "," + EpiName<Epi>::v + ">";
            GemmTimer t(h, s, role, kdma.c_str(), 2.0 * M * N * K);
            return gemm_f32_dma_launch(al, W, epi, C, ldc, M, N, K, device_cu_count(), s);
        }
    }
    static const std::string kname = std::string("gemm_f32_persist_kernel<256x256x16,") + AlName<AL>::v + "," + EpiName<Epi>::v + ">";
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * M * N * K);
    return gemm_f32_persist_launch<Cfg, AL, Epi>(al, W, epi, C, ldc, M, N, K, device_cu_count(), s);
}

// ------------------------------------------------------------------------------------------------ workspace
// asks the device once how many workgroups of the one-launch PU chain it keeps resident (pu_chain.h)
static void pu_chain_probe(Handle* h) {
    // A chain launch of an EARLIER call whose row blocks were not co-resident (shared device) was redone on the device by
    // pu_solo_kernel -- the results were right, but it cost a ~0.1 s stall: from now on this handle walks the steps with the per-step
    // kernels (same bits).  Read without synchronising: the word is host memory the device writes through.
    if (h->pu_fault_host && __atomic_load_n(h->pu_fault_host, __ATOMIC_RELAXED) != 0u) {
        __atomic_store_n(h->pu_fault_host, 0u, __ATOMIC_RELAXED);
        h->pu_faults++;
        h->pu_chain = false;
    }
    if (!h->pu_chain) { h->pu_resident[0] = h->pu_resident[1] = 0; return; }      // 0 resident workgroups: pu_chain_launch declines
    if (!h->pu_fault_host) {           // once per handle, at its first forward (never inside a stream capture: wrappers run eagerly first)
        void* hp = nullptr; void* dp = nullptr;
        if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
            h->pu_fault_host = (unsigned*)hp; h->pu_fault_dev = (unsigned*)dp;
            *h->pu_fault_host = 0u;
        } else {
            if (hp) (void)hipHostFree(hp);
            (void)hipGetLastError();
        }
    }
    if (h->pu_resident[0] <= 0) {
        h->pu_resident[0] = pu_chain_resident<1>();
        h->pu_resident[1] = pu_chain_resident<2>();
    }
}
static size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
enum { TE_NONE = 0, TE_BIAS = 1, TE_BIAS_RES = 2, TE_BIAS_GELU_SAVE = 3, TE_ACCUM = 4, TE_GELU_GRAD = 5, TE_PATCH = 6, TE_SCATTER_PATCH = 7, TE_SCATTER_ROT = 8 };
