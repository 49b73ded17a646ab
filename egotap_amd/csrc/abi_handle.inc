// Fragment of egotap_abi.hip, included there exactly once; it includes nothing.  The order of the fragments there fixes hipcc's schedules.
// The bound parameters, the handle, the GEMM timing bracket, the device's CU count.
// ------------------------------------------------------------------------------------------------ handle
struct Param {
    void* ptr = nullptr;
    int64_t numel = 0;
    int dtype = EGOTAP_F32;
};

struct LiftParams {   // resolved raw pointers of net_AutoEncoder
    const float *mask_tok, *pos_emb, *patch_w, *patch_b;
    struct Layer {
        const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b, *up_w, *up_b, *dn_w, *dn_b;
        const float *ln1_g, *ln1_b, *ln2_g, *ln2_b;
    } layer[8];
    const float *lnf_g, *lnf_b;
    struct Fc { const float *w, *b, *g, *beta, *mean, *var; } pos_fc[3], rot_fc[3];
    const float *x2f0_w, *x2f0_b, *x2h0_w, *x2h0_b, *b2h0_w, *b2h0_b, *h2h0_w, *h2h0_b;
    const float *x2f1_w, *x2f1_b, *x2h1_w, *x2h1_b, *h2h1_w, *h2h1_b;
    const float *pose_w, *pose_b, *glob_w, *glob_b;
};

struct HmParams {   // resolved raw pointers of one heatmap estimator (net_HeatMap / net_RotHeatMap)
    struct Bn { const float *g, *b, *m, *v; long long* nbt; };      // nbt: num_batches_tracked where bound (EGOTAP_I64), else null; m / v are written by the batch-statistics forward
    const float* stem_w; Bn stem_bn;
    struct Block { const float *w1, *w2, *wd; Bn bn1, bn2, bnd; } blk[4][6];
    int nblk[4];        // BasicBlocks per stage (resnet18: 2,2,2,2; resnet34: 3,4,6,3)
    struct Cv { const float *w, *b; } l1x1[4], up[3], head;   // layerK_1x1 (K=1..4), conv_up1..3, conv_heatmap
    int n_out;   // output channels of conv_heatmap (2 * heatmaps per eye)
};

struct egotap_handle_s {
    egotap_config cfg;
    // derived (spec.py LiftPreset)
    int J, T, grid, ppd, side, seq, C, D, H, hid, out_joints;
    CellGrid cells() const { return CellGrid{seq, side, ppd, grid, T}; }
    PatchCells patches() const { return PatchCells{C, cfg.hm_size, cells()}; }
    TokenGather tokens() const { return TokenGather{T, D, seq, side, ppd, grid}; }
    RotRows rots() const { return RotRows{C, J, cfg.hm_size * cfg.hm_size}; }      // the head's operand layouts (head_layout.h) of this preset
    std::unordered_map<std::string, int64_t> expect[EGOTAP_NET_COUNT];   // key -> numel (forward-needed keys)
    std::unordered_map<std::string, Param> bound[EGOTAP_NET_COUNT];
    bool lift_resolved = false;
    LiftParams lp;
    std::unordered_map<std::string, Param> bound_grad;                   // egotap_bind_grad: where egotap_lift_backward writes
    bool grad_resolved = false;
    LiftParams lg;                                                       // the same tensors' gradient buffers (running stats unused)
    bool hm_resolved[EGOTAP_NET_COUNT] = {false, false, false};
    HmParams hp[EGOTAP_NET_COUNT];
    int debug_stop = 0;
    int pu_resident[2] = {-1, -1};     // workgroups of pu_chain_kernel<1> / <2> the device keeps resident (-1: not asked yet)
    bool pu_chain = true;              // egotap_set_pu_chain: one-launch recurrence (needs the device to itself) or per-step kernels
    unsigned* pu_fault_host = nullptr; // pinned, device-mapped word: set by pu_solo_kernel when a chain launch had to be redone (pu_chain.h)
    unsigned* pu_fault_dev = nullptr;  // the same word as the device sees it
    int pu_faults = 0;                 // chain launches found faulted so far (the chain is switched off for the handle at the first)
    int pu_debug_drop = 0;             // egotap_debug_pu_drop_workgroups
    int precision = EGOTAP_PREC_F32;   // arithmetic of the large GEMMs (egotap_set_precision)
    __bf16* wscratch = nullptr;        // scratch for the bf16 copy of a GEMM's weight matrix (plain-bf16 mode), caller-owned
    size_t wscratch_bytes = 0;
    __bf16* ascratch = nullptr;        // scratch for the bf16 copy of a GEMM's activation operand (plain-bf16 mode, gemm_bf16_dma_kernel), caller-owned
    size_t ascratch_bytes = 0;
    __bf16* conv_pack = nullptr;       // scratch for repacked conv weights (set per egotap_hm_forward call from the workspace)
    float* conv_part = nullptr;        // [r4] fp32 egotap_hm_forward only (null outside it): scratch for the input-channel-split partials of conv_f32.h
    size_t conv_part_floats = 0;
    // frozen-weight serving (egotap_lift_freeze / egotap_hm_freeze): caller-owned arenas of prepared weights, null = not frozen
    char* lift_arena = nullptr;                          // lift_frozen_plan's layout; read by the bf16-storage inference forward only
    char* hm_arena[EGOTAP_NET_COUNT] = {nullptr, nullptr, nullptr};       // pack_all_bf16s_kernel's region of one estimator
    short hm_arena_slab[EGOTAP_NET_COUNT][PackTable::MAXW] = {};          // ... and the K-slab depth of every packed weight in it: the part of the
    int hm_arena_nw[EGOTAP_NET_COUNT] = {0, 0, 0};                        // layout that depends on the batch (hm_pack_plan)
    int rgb_form = 0;                  // EGOTAP_RGB_FORM_*: how the last egotap_predict_pose_rgb handed the heatmaps to the head (egotap_debug.h)
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;   // start/stop pairs
    struct Rec { const char* role; const char* kernel; double flops; };
    std::vector<Rec> rec;         // one per recorded pair
    size_t ev_used = 0;
    std::string detail;           // JSON written by egotap_timing_read
};
typedef egotap_handle_s Handle;

struct GemmTimer {   // brackets one GEMM launch when the handle's timing hook is on
    Handle* h;
    hipStream_t s;
    bool on;
    GemmTimer(Handle* h_, hipStream_t s_, const char* role, const char* kernel, double flops)
        : h(h_), s(s_), on(h_ && h_->timing) {
        if (!on) return;
        if (h->ev_used + 2 > h->ev.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            h->ev.push_back(a);
            h->ev.push_back(b);
        }
        (void)hipEventRecord(h->ev[h->ev_used], s);
        h->rec.push_back({role, kernel, flops});
    }
    ~GemmTimer() {
        if (!on) return;
        (void)hipEventRecord(h->ev[h->ev_used + 1], s);
        h->ev_used += 2;
    }
};

static int device_cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) n = v;
        else n = 256;
    }
    return n;
}
