// C ABI of libegotap_hip.so (include/egotap.h, include/egotap_debug.h): the one file build.py compiles.  It holds the part switch, each
// part's list of kernel headers and, below them, the host code.  What more than one part compiles stands in area files, one #include each
// (abi_*.inc: the handle, the zero fill, the lifting head's and the convolutions' routing, fc1 on the bf16-storage GEMMs).  What a single
// part compiles is one guarded run per part (core and inference, the three families of training operators, the one-call training step):
// part 1's run stands in an area file too (abi_train_lift.inc), the other four stand here (profiles/abi_runs_summary.md).
//
// The order of the #include lines and of the text is part of the build: it fixes the order in which host code first references kernel
// templates, clang emits device helpers in that order, and so it decides the schedules hipcc produces (profiles/abi_parts_summary.md
// section 2, profiles/abi_areas_summary.md).  The fragments are included exactly once, from here, and include nothing themselves.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <cmath>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

// The library is ONE source compiled as four translation units in parallel (egotap_amd/build.py: -DEGOTAP_PART=0 core and
// inference, 1 lifting-head training operators, 2 heatmap-estimator training operators, 3 bf16-storage operators); every exported function belongs to one
// part.  Without EGOTAP_PART the file is a single translation unit.
//
// A part sees only what it launches.  A static launcher or kernel a part can see is compiled into that part's code object whether the part
// launches it or not, so each part includes only the kernel headers it launches from, and the code below stands in sections: what all four parts use, what two or
// three share (one guarded section per set of parts), then each part's own code with the helpers only it uses.  `hipcc -DEGOTAP_PART=n --cuda-host-only -fsyntax-only -Wunused-function` names what a part sees
// and does not use (tests/test_abi_cpu.py runs it); a helper withheld from a part that needs it does not compile.
#ifndef EGOTAP_PART
#define EGOTAP_PART -1
#endif
#define EGOTAP_IN(n) (EGOTAP_PART < 0 || EGOTAP_PART == (n))

#if EGOTAP_IN(0)
#include "lds_opt_in.h"
#include "attention_f32.h"
#include "conv_f32.h"
#include "conv_bf16.h"
#include "gemm_f32.h"
#include "gemm_bf16.h"
#include "gemm_bf16_dma.h"
#include "gemm_f32_dma.h"
#include "attention_bf16.h"
#include "layernorm.h"
#include "metrics.h"
#include "heatmap_synth.h"
#include "pu_chain.h"
#include "gemm_bf16s.h"
#include "gemm_bf16s64.h"
#include "bf16s_ops.h"
#include "attention_bf16s_fwd.h"
#include "attention_bf16s_bwd.h"   // not launched from part 0: without it attention_bf16s3_kernel<4>, the serving forward, comes out in another schedule (profiles/kernel_headers_summary.md)
#include "conv_bf16s.h"
#include "stem_bf16s.h"
#include "conv64_bf16s.h"
#include "bn_bf16s.h"
#include "rgb_u8.h"
#include "frame_source.h"          // the fetch, the blend and the store that frame_resize.h and lens_remap.h share
#include "frame_resize.h"
#include "lens_remap.h"
#include "heatmap_peaks.h"
#include "limb_decode.h"
#include "ocam.h"
#include "pose_track.h"
#include "skeleton_fit.h"
#include "stereo_fuse.h"
#include "overlay.h"               // last: its entries stand at the end of part 0's text, so no other kernel is referenced later than before
#endif
#if EGOTAP_IN(1)
#include "attention_f32.h"
#include "gemm_f32.h"
#include "gemm_bf16.h"
#include "gemm_bf16_dma.h"
#include "gemm_f32_dma.h"
#include "attention_bf16.h"
#include "pu_chain.h"
#include "gemm_tn_bf16.h"
#include "train_ops.h"
#include "attention_bwd_f32.h"
#include "attention_bwd_bf16.h"
#include "gemm_tn_f32.h"
// Not launched from part 1, kept for the device code of attn_bwd_dq / _dk / _dv_bf16_kernel<4, 1> (attention_bwd_bf16.h), which it does launch:
// attention_bf16s_bwd.h instantiates attn_bwd_dq_bf16s_kernel<4, 1>, and clang emits the inline helpers the two share (attnbf::tile_x_frags<1>,
// attnbf::acc_tile_t_x_p<1> of attention_bf16_tiles.h) in order of first reference.  Without the two headers they are emitted, and inlined, later, and the three kernels
// come out with the same instructions in another schedule (profiles/abi_parts_summary.md section 2).  Costs this part four kernels it does not launch.
#include "attention_bf16s_fwd.h"
#include "attention_bf16s_bwd.h"
#endif
#if EGOTAP_IN(2)
#include "conv_f32.h"
#include "conv_bf16.h"
#include "hm_train.h"
#endif
#if EGOTAP_IN(3)
#include "gemm_bf16.h"
#include "gemm_bf16s.h"
#include "gemm_bf16s64.h"
#include "gemm_tn_bf16s.h"
#include "bf16s_ops.h"
#include "attention_bf16s_fwd.h"
#include "attention_bf16s_bwd.h"
#include "gemm_tn_f32.h"
#endif
#include "head_layout.h"      // the head's operand layouts the handle hands out
#include "conv_pack_table.h"  // PackTable::MAXW sizes a member of the handle: types only (the kernels that read the table are conv_bf16s.h's, in part 0's list)

// ================================================================================================ all four parts: the handle, the bound parameters, the timing bracket
#include "abi_handle.inc"

// ================================================================================================ parts 0, 1 and 3: the zero fill
#if EGOTAP_IN(0) || EGOTAP_IN(1) || EGOTAP_IN(3)
#include "abi_zero_fill.inc"
#endif

// ================================================================================================ parts 0 and 1: what the lifting head's forward and its training operators share
// (GEMM tiles and routing, parameter resolver, the propagation units' residency probe)
#if EGOTAP_IN(0) || EGOTAP_IN(1)
#include "abi_lift_routing.inc"
#endif

// ================================================================================================ parts 0 and 2: the fp32-tensor convolution routing (estimator forward and training)
#if EGOTAP_IN(0) || EGOTAP_IN(2)
#include "abi_conv_routing.inc"
#endif

// ================================================================================================ parts 0 and 3: fc1 of the encoders on the bf16-storage GEMMs
#if EGOTAP_IN(0) || EGOTAP_IN(3)
#include "abi_fc1_bf16s.inc"
#endif

// ================================================================================================ one part each, in the order 0 (core and inference), 1, 2, 3, 0 (the one-call training step)
#if EGOTAP_IN(0)
// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[1024] = "";
void egotap_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
hipError_t ego_allow_dynamic_lds(const void* kernel, int bytes) {
    static LdsOptIn seen;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev); e != hipSuccess) return e;
    return seen.ensure(kernel, dev, bytes, [kernel](int b) { return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, b); });
}
extern "C" const char* egotap_last_error(void) { return g_err; }
extern "C" int egotap_abi_version(void) { return EGOTAP_ABI_VERSION; }

extern "C" const char* egotap_gemm_tile_name(int tile) {
    switch (tile) {
        case 0: case 1: return "128x128x32/4w";
        case 2: return "256x128x32/8w";
        case 3: return "128x256x32/8w";
        case 4: return "256x256x16/8w";
        case 5: return "256x128x16/4w";
        case 6: return "64x64x32/4w";
        case 7: return "256x128x32/4w";
        case 8: return "pipe128x128x16/4w";
        case 9: return "pipe128x128x32/4w";
        case 10: return "pipe256x128x16/8w";
        case 11: return "pipe256x256x16/8w";
        case 12: return "persist256x256x16/8w";
        case 13: return "persist256x256x16/8w/bf16x3";
        case 14: return "persist256x256x32/8w/bf16";
        case 15: return "persist256x256x16/8w/bf16x3/interleaved";
        case 16: return "persist256x256x32/8w/bf16/interleaved";
        case 19: return "dma256x256x16/8w (exact fp32, LDS-DMA staging)";
        default: return nullptr;
    }
}
// the handle whose timing hook was enabled last: where the operators that take no handle (ocam.h) record their launches; cleared when that handle's hook is
// switched off or the handle is destroyed
[[maybe_unused]] static Handle* g_timing_handle = nullptr;

static int isqrt_floor(int v) {
    int r = 0;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

static void lift_expect(Handle* h) {
    auto& e = h->expect[EGOTAP_NET_LIFT];
    const int64_t D = h->D, H = h->H, hid = h->hid, x = 2 * hid;
    const std::string v = "pos_heatmap_encoder.vit.";
    e[v + "embeddings.mask_token"] = D;
    e[v + "embeddings.position_embeddings"] = (int64_t)h->seq * D;
    e[v + "embeddings.patch_embeddings.projection.weight"] = D * h->cfg.patch * h->cfg.patch;
    e[v + "embeddings.patch_embeddings.projection.bias"] = D;
    auto lin = [&](const std::string& p, int64_t n_out, int64_t n_in) {
        e[p + ".weight"] = n_out * n_in;
        e[p + ".bias"] = n_out;
    };
    for (int i = 0; i < h->cfg.vit_layers; ++i) {
        const std::string l = v + "encoder.layer." + std::to_string(i) + ".";
        lin(l + "attention.attention.query", D, D);
        lin(l + "attention.attention.key", D, D);
        lin(l + "attention.attention.value", D, D);
        lin(l + "attention.output.dense", D, D);
        lin(l + "intermediate.dense", 4 * D, D);
        lin(l + "output.dense", D, 4 * D);
        e[l + "layernorm_before.weight"] = D; e[l + "layernorm_before.bias"] = D;
        e[l + "layernorm_after.weight"] = D;  e[l + "layernorm_after.bias"] = D;
    }
    e[v + "layernorm.weight"] = D; e[v + "layernorm.bias"] = D;
    auto fcb = [&](const std::string& p, int64_t n_in, int64_t n_out) {
        lin(p + ".fc", n_out, n_in);
        e[p + ".bn.weight"] = n_out; e[p + ".bn.bias"] = n_out;
        e[p + ".bn.running_mean"] = n_out; e[p + ".bn.running_var"] = n_out;
    };
    const int64_t k_pos = (int64_t)h->ppd * h->ppd * D, k_rot = 2LL * h->cfg.hm_size * h->cfg.hm_size;
    fcb("pos_heatmap_encoder.fc1", k_pos, 2048); fcb("pos_heatmap_encoder.fc2", 2048, 512); fcb("pos_heatmap_encoder.fc3", 512, hid);
    fcb("rot_heatmap_encoder.fc1", k_rot, 2048); fcb("rot_heatmap_encoder.fc2", 2048, 512); fcb("rot_heatmap_encoder.fc3", 512, hid);
    const std::string c = "skel_sequential_layer.lstm_custom.layers.";
    lin(c + "0.x2f", H + x, x); lin(c + "0.x2h", 4 * H, x); lin(c + "0.b2h", 4 * H, x); lin(c + "0.h2h", 4 * H, H);
    lin(c + "1.x2f", H, H); lin(c + "1.x2h", 4 * H, H); lin(c + "1.h2h", 4 * H, H);
    lin("pose_mlp.pose_fcs.0", 3, x + H);
    if (h->cfg.estimate_head) lin("global_mlp.pose_fcs.0", 6, (int64_t)h->J * H);
}

static const int HM_CH[4] = {64, 128, 256, 512};
// timing-hook role names of the backbone convolutions (static strings: the hook keeps the pointers)
#define HM_ROLE_ROW(L, S) {"hm.l" #L ".0." S, "hm.l" #L ".1." S, "hm.l" #L ".2." S, "hm.l" #L ".3." S, "hm.l" #L ".4." S, "hm.l" #L ".5." S}
static const char* const HM_R1[4][6] = {HM_ROLE_ROW(1, "conv1"), HM_ROLE_ROW(2, "conv1"), HM_ROLE_ROW(3, "conv1"), HM_ROLE_ROW(4, "conv1")};
static const char* const HM_R2[4][6] = {HM_ROLE_ROW(1, "conv2"), HM_ROLE_ROW(2, "conv2"), HM_ROLE_ROW(3, "conv2"), HM_ROLE_ROW(4, "conv2")};
static const char* const HM_RD[4] = {"", "hm.l2.down", "hm.l3.down", "hm.l4.down"};
static inline int hm_nblk(const Handle* h, int i) { return h->cfg.hm_blocks[i] > 0 ? h->cfg.hm_blocks[i] : 2; }

static void hm_expect(Handle* h, int net, int n_out) {
    auto& e = h->expect[net];
    const std::string bb = "backbone.backbone.backbone.";
    auto bn = [&](const std::string& p, int64_t c) {
        e[p + ".weight"] = c; e[p + ".bias"] = c; e[p + ".running_mean"] = c; e[p + ".running_var"] = c;
    };
    e[bb + "conv1.weight"] = 64 * 3 * 49;
    bn(bb + "bn1", 64);
    int cin = 64;
    for (int i = 0; i < 4; ++i) {
        const int c = HM_CH[i];
        for (int b = 0; b < hm_nblk(h, i); ++b) {
            const std::string p = bb + "layer" + std::to_string(i + 1) + "." + std::to_string(b);
            const int bc = b == 0 ? cin : c;
            e[p + ".conv1.weight"] = (int64_t)c * bc * 9; bn(p + ".bn1", c);
            e[p + ".conv2.weight"] = (int64_t)c * c * 9;  bn(p + ".bn2", c);
            if (b == 0 && i > 0) { e[p + ".downsample.0.weight"] = (int64_t)c * bc; bn(p + ".downsample.1", c); }
        }
        cin = c;
    }
    const std::string a = "after_backbone.";
    auto cv = [&](const std::string& n, int64_t co, int64_t ci, int k) { e[a + n + ".weight"] = co * ci * k * k; e[a + n + ".bias"] = co; };
    cv("layer1_1x1.0", 128, 128, 1); cv("layer2_1x1.0", 256, 256, 1); cv("layer3_1x1.0", 516, 512, 1); cv("layer4_1x1.0", 1024, 1024, 1);
    cv("conv_up3.0", 1024, 1540, 3); cv("conv_up2.0", 512, 1280, 3); cv("conv_up1.0", 512, 640, 3);
    cv("conv_heatmap", n_out, 512, 1);
}

// whether a prepared copy of this forward-needed tensor is kept while the net is frozen (egotap_lift_freeze / egotap_hm_freeze).  Lifting head: the
// weights of the patch projection, of the ViT's six Linear layers per block and of the two fc1, and the q / k / v biases (fused into one vector).
// Estimators: everything the pack holds -- every convolution weight and bias and every BatchNorm tensor except the stem's, which the fused
// stem kernel reads live.
static bool frozen_key(int net, const char* key) {
    const std::string k(key);
    auto ends = [&](const char* t) { const size_t n = strlen(t); return k.size() >= n && k.compare(k.size() - n, n, t) == 0; };
    if (net == EGOTAP_NET_LIFT) {
        if (k.find(".attention.attention.") != std::string::npos) return true;
        if (k.find(".encoder.layer.") != std::string::npos) return ends("dense.weight");
        return ends("patch_embeddings.projection.weight") || ends("_heatmap_encoder.fc1.fc.weight");
    }
    const std::string bb = "backbone.backbone.backbone.";
    return k.compare(0, bb.size() + 6, bb + "conv1.") != 0 && k.compare(0, bb.size() + 4, bb + "bn1.") != 0;
}

extern "C" int egotap_create(const egotap_config* cfg, egotap_handle* out) {
    EGO_CHECK(cfg && out, "egotap_create: null argument");
    EGO_CHECK(cfg->struct_bytes == (int32_t)sizeof(egotap_config), "egotap_create: egotap_config is %d bytes, library expects %d",
              cfg->struct_bytes, (int)sizeof(egotap_config));
    EGO_CHECK(cfg->n_joints_hm >= 1 && cfg->n_joints_hm <= 64, "n_joints_hm out of range");
    EGO_CHECK(cfg->patch == 16, "patch size must be 16 (net_architecture.py:326)");
    EGO_CHECK(cfg->hm_size > 0 && cfg->hm_size % 16 == 0, "hm_size must be a positive multiple of 16 (net_architecture.py:327)");
    EGO_CHECK(cfg->vit_dim == 1024 && cfg->vit_heads == 8, "ViT hidden size / heads are fixed at 1024 / 8 (net_architecture.py:340-348)");
    EGO_CHECK(cfg->vit_layers >= 1 && cfg->vit_layers <= 8, "vit_layers out of range");
    EGO_CHECK(cfg->pu_hidden == 512 && cfg->hidden == 128, "hidden sizes are fixed at ae_hidden_size 128 / PU 512 in this build");
    for (int i = 0; i < 4; ++i) EGO_CHECK(cfg->hm_blocks[i] >= 0 && cfg->hm_blocks[i] <= 6, "hm_blocks: at most 6 BasicBlocks per ResNet stage (resnet18 / resnet34)");
    Handle* h = new Handle();
    h->cfg = *cfg;
    h->J = cfg->n_joints_hm;
    h->T = 2 * h->J;
    h->grid = isqrt_floor(h->T - 1) + 1;
    h->ppd = cfg->hm_size / cfg->patch;
    h->side = h->grid * h->ppd;
    h->seq = h->side * h->side;
    h->C = 6 * h->J;
    h->D = cfg->vit_dim;
    h->H = cfg->pu_hidden;
    h->hid = cfg->hidden;
    h->out_joints = h->J + (cfg->estimate_head ? 1 : 0);
    lift_expect(h);
    hm_expect(h, EGOTAP_NET_HM_POS, 2 * h->J);        // num_heatmap per eye, stereo
    hm_expect(h, EGOTAP_NET_HM_ROT, 4 * h->J);        // cos + sin per limb per eye
    h->hp[EGOTAP_NET_HM_POS].n_out = 2 * h->J;
    h->hp[EGOTAP_NET_HM_ROT].n_out = 4 * h->J;
    *out = h;
    return EGOTAP_OK;
}

extern "C" void egotap_destroy(egotap_handle h) {
    if (!h) return;
    if (g_timing_handle == h) g_timing_handle = nullptr;
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->pu_fault_host) (void)hipHostFree(h->pu_fault_host);
    delete h;
}

extern "C" int egotap_bind_param(egotap_handle h, int net, const char* key, void* dev_ptr, int64_t numel, int dtype) {
    EGO_CHECK(h && key, "egotap_bind_param: null argument");
    EGO_CHECK(net >= 0 && net < EGOTAP_NET_COUNT, "egotap_bind_param: bad net id %d", net);
    EGO_CHECK(dev_ptr != nullptr || numel == 0, "egotap_bind_param(%s): null device pointer", key);
    auto it = h->expect[net].find(key);
    if (it != h->expect[net].end()) {
        EGO_CHECK(dtype == EGOTAP_F32, "egotap_bind_param(%s): expected f32", key);
        EGO_CHECK(it->second == numel, "egotap_bind_param(%s): %lld elements, expected %lld", key, (long long)numel,
                  (long long)it->second);
        EGO_CHECK(((uintptr_t)dev_ptr & 15) == 0, "egotap_bind_param(%s): pointer must be 16-byte aligned", key);
    }
    Param p;
    p.ptr = dev_ptr; p.numel = numel; p.dtype = dtype;
    // a tensor whose prepared copy sits in a frozen arena moved: the arena is stale and must never be read silently
    if (it != h->expect[net].end() && frozen_key(net, key)) {
        auto was = h->bound[net].find(key);
        if (was != h->bound[net].end() && was->second.ptr != dev_ptr) {
            if (net == EGOTAP_NET_LIFT) h->lift_arena = nullptr;
            else h->hm_arena[net] = nullptr;
        }
    }
    h->bound[net][key] = p;   // keys the forward never reads (pooler, cls_token, num_batches_tracked) are kept but unused
    if (net == EGOTAP_NET_LIFT) h->lift_resolved = false;
    else h->hm_resolved[net] = false;
    return EGOTAP_OK;
}

extern "C" int egotap_unbound_count(egotap_handle h, int net, int* count) {
    EGO_CHECK(h && count, "egotap_unbound_count: null argument");
    EGO_CHECK(net >= 0 && net < EGOTAP_NET_COUNT, "bad net id %d", net);
    int n = 0;
    for (auto& kv : h->expect[net])
        if (!h->bound[net].count(kv.first)) ++n;
    *count = n;
    return EGOTAP_OK;
}
static const float* P(Handle* h, int net, const std::string& key, bool& ok) { return P(h, h->bound[net], key, ok); }

// ------------------------------------------------------------------------------------------------ timing
extern "C" int egotap_timing_enable(egotap_handle h, int enable) {
    EGO_CHECK(h, "null handle");
    h->timing = enable != 0;
    if (h->timing) g_timing_handle = h;
    else if (g_timing_handle == h) g_timing_handle = nullptr;
    return EGOTAP_OK;
}
extern "C" int egotap_timing_read(egotap_handle h, int* launches, double* total_ms, double* total_flops) {
    EGO_CHECK(h && launches && total_ms && total_flops, "null argument");
    struct Agg { std::string role, kernel; int n = 0; double ms = 0, flops = 0; };
    std::vector<Agg> aggs;
    double ms = 0.0, fl = 0.0;
    const size_t pairs = h->ev_used / 2;
    for (size_t i = 0; i < pairs; ++i) {
        EGO_HIP(hipEventSynchronize(h->ev[2 * i + 1]));
        float t = 0.f;
        EGO_HIP(hipEventElapsedTime(&t, h->ev[2 * i], h->ev[2 * i + 1]));
        ms += t;
        fl += h->rec[i].flops;
        Agg* a = nullptr;
        for (auto& x : aggs)
            if (x.role == h->rec[i].role) { a = &x; break; }
        if (!a) { aggs.emplace_back(); a = &aggs.back(); a->role = h->rec[i].role; a->kernel = h->rec[i].kernel; }
        a->n += 1; a->ms += t; a->flops += h->rec[i].flops;
    }
    std::string js = "[";
    for (size_t i = 0; i < aggs.size(); ++i) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s{\"role\": \"%s\", \"kernel\": \"%s\", \"launches\": %d, \"ms\": %.6f, \"flops\": %.6e}",
                 i ? ", " : "", aggs[i].role.c_str(), aggs[i].kernel.c_str(), aggs[i].n, aggs[i].ms, aggs[i].flops);
        js += buf;
    }
    js += "]";
    h->detail = js;
    *launches = (int)pairs;
    *total_ms = ms;
    *total_flops = fl;
    h->ev_used = 0;
    h->rec.clear();
    return EGOTAP_OK;
}
extern "C" const char* egotap_timing_detail(egotap_handle h) { return h ? h->detail.c_str() : ""; }

// out[0:n | n:2n | 2n:3n] = a | b | c  (the fused q|k|v bias of the bf16-storage forward)
static __global__ __launch_bounds__(256) void concat3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                             float* __restrict__ out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { out[i] = a[i]; out[n + i] = b[i]; out[2 * n + i] = c[i]; }
}

// Small batches (serving): the 256x256 persistent tiling leaves most CUs idle (B = 1: 12 tiles for attn_out / mlp_down, one
// tile row for fc1).  Below `fill` tiles the GEMM runs as exact-fp32 128x128 tiles with K split over blockIdx.y
// (gemm_f32_splitk_launch) in every precision mode; at and above it gemm_big as before, so large-batch results do not change.
static constexpr size_t SPLITK_FLOATS = (size_t)1 << 24;
// ONE routing decision for an fp32-tensor NT product, used by gemm_small (which launches it) and by gemm_res_ln (which fuses the reduce of a split
// product with the LayerNorm behind it and therefore must see exactly the split layout gemm_small would produce).
// The fitted constants below (0.2319 us per 16-deep K step of a 256 x 256 tile = 0.92 x 157.3 TF over 256 CUs, 5 us per round; the per-slab times inside
// gemm_f32_splitk_plan / gemm_f32_direct_estimate_us) were measured on the 256-CU MI355X; `cus` only scales the round counts.  On another part they
// would still pick a CORRECT kernel, not necessarily the faster one.
enum { GS_BIG = 0, GS_DIRECT_A, GS_DIRECT_S, GS_SPLIT_S, GS_SPLIT_A, GS_HYBRID };
struct SmallRoute { int kind, splits, head_rows; };
// epilogues that do not index their operands by the output ROW: a product may be cut into row ranges without touching the functor (GS_HYBRID)
template <class E> struct epi_row_free : std::false_type {};
template <> struct epi_row_free<EpiBias> : std::true_type {};
template <> struct epi_row_free<EpiBiasGelu> : std::true_type {};
template <> struct epi_row_free<EpiBnLrelu> : std::true_type {};
template <> struct epi_row_free<EpiNone> : std::true_type {};
static SmallRoute gemm_small_route(const Handle* h, bool plain_loader, int M, int N, int K, int wseg, int cus, bool row_free = false) {
    const long tiles256 = (long)((M + 255) / 256) * ((N + 255) / 256);
    const long fill = (h && h->precision != EGOTAP_PREC_F32) ? 64 : 160;
    if (N % 128 != 0 || K % 32 != 0 || wseg % 128 != 0) return SmallRoute{GS_BIG, 1, 0};
    if (tiles256 >= fill) {
        // [r4] fp32, plain operands, fewer than four rounds of 256 x 256 tiles: the 256 x 256 kernel runs WHOLE rounds at 0.92 of the matrix
        // pipe (B = 8, N = 4096: 288 tiles = two rounds for 1.1 rounds of work, 484 us) -- the 128 x 128 kernel with its epilogue inside takes
        // 415 us there.  Both estimates are fitted to tools/gemm_small_vs_big_probe.py and name the faster kernel at 46 of its 48 points.
        if (plain_loader && h && h->precision == EGOTAP_PREC_F32 && tiles256 < 4L * cus) {
            const double t_round = K * 0.2319 + 5.0;
            const double t_big = (double)((tiles256 + cus - 1) / cus) * t_round;
            const double t_direct = gemm_f32_direct_estimate_us<TileA>(M, N, K, cus);
            // [r5] GS_HYBRID: the tile rows that fill WHOLE rounds of the 256 x 256 kernel run there, the rows past them as a product of their own
            // (a few tiles: K split over the idle CUs) -- B = 8, N = 4096: one round of 256 tiles + 32 tiles split two ways, ~290 us for the 375 the
            // 128 x 128 kernel took.  Only for epilogues that do not index by row (the functor is passed on unchanged).
            if (row_free && N % 256 == 0 && tiles256 > cus) {
                const int tn = N / 256, mh = (int)((tiles256 / cus) * cus / tn);      // whole tile rows inside the whole rounds
                const int Mt = M - mh * 256;
                if (mh >= 1 && Mt > 0) {
                    const long tt = (long)((Mt + 255) / 256) * tn;
                    const double t_head = (double)(((long)mh * tn + cus - 1) / cus) * t_round;
                    const double t_tail = 4.0 + (tt >= fill ? std::min((double)((tt + cus - 1) / cus) * t_round, gemm_f32_direct_estimate_us<TileA>(Mt, N, K, cus))
                                                            : gemm_f32_splitk_plan<TileA>(Mt, N, K, SPLITK_FLOATS, cus).us);
                    if (t_head + t_tail < std::min(t_big, t_direct)) return SmallRoute{GS_HYBRID, 1, mh * 256};
                }
            }
            if (t_direct < t_big) return SmallRoute{GS_DIRECT_A, 1, 0};
        }
        return SmallRoute{GS_BIG, 1, 0};
    }
    const SplitPlan pa = gemm_f32_splitk_plan<TileA>(M, N, K, SPLITK_FLOATS, cus);
    if (M <= 640) {   // [r4] one frame (576 rows = 4.5 tiles of 128 rows): the 64-row tile when its plan is estimated faster -- nine row tiles exactly, up
        // to one workgroup per CU without a split (qkv: 216 tiles, epilogue in the kernel: no partials, no reduce launch).  Measured: B = 1 forward
        // -33 us; from two frames on the 64-row tile loses what it gains (its slab is shorter than a load's round trip), so the rule stops here.
        const SplitPlan ps = gemm_f32_splitk_plan<TileS>(M, N, K, SPLITK_FLOATS, cus);
        if (ps.us < pa.us) return SmallRoute{ps.splits == 1 ? GS_DIRECT_S : GS_SPLIT_S, ps.splits, 0};
    }
    return SmallRoute{GS_SPLIT_A, pa.splits, 0};
}
template <class AL, class Epi>
static hipError_t gemm_small(Handle* h, const char* role, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc,
                             int M, int N, int K, float* P, hipStream_t s) {
    const int cus = device_cu_count();
    const SmallRoute r = gemm_small_route(h, std::is_same<AL, ALoadPlain>::value, M, N, K, W.seg, cus, epi_row_free<Epi>::value);
    if constexpr (std::is_same<AL, ALoadPlain>::value && epi_row_free<Epi>::value) {
        if (r.kind == GS_HYBRID) {      // whole rounds of 256 x 256 tiles, then the remaining rows routed as a product of their own (never GS_HYBRID again: fewer tiles than CUs)
            hipError_t e = gemm_big(h, role, al, W, epi, C, ldc, r.head_rows, N, K, s);
            if (e != hipSuccess) return e;
            return gemm_small(h, role, ALoadPlain{al.A + (long)r.head_rows * al.lda, al.lda}, W, epi, C + (long)r.head_rows * ldc, ldc, M - r.head_rows, N, K, P, s);
        }
    }
    switch (r.kind) {
        case GS_BIG: case GS_HYBRID: return gemm_big(h, role, al, W, epi, C, ldc, M, N, K, s);
        case GS_DIRECT_A: return gemm<TileA>(h, role, al, W, epi, C, ldc, M, N, K, s);
        case GS_DIRECT_S: return gemm<TileS>(h, role, al, W, epi, C, ldc, M, N, K, s);
        case GS_SPLIT_S: {
            static const std::string kname64 = std::string("gemm_f32_splitk_kernel<64x128x32,") + AlName<AL>::v + ">+splitk_reduce_kernel<" + EpiName<Epi>::v + ">";
            GemmTimer t(h, s, role, kname64.c_str(), 2.0 * M * N * K);
            return gemm_f32_splitk_launch<TileS>(al, W, epi, C, ldc, P, SPLITK_FLOATS, M, N, K, s, cus, r.splits);
        }
        default: {
            static const std::string kname = std::string("gemm_f32_splitk_kernel<128x128x32,") + AlName<AL>::v + ">+splitk_reduce_kernel<" + EpiName<Epi>::v + ">";
            GemmTimer t(h, s, role, kname.c_str(), 2.0 * M * N * K);
            return gemm_f32_splitk_launch<TileA>(al, W, epi, C, ldc, P, SPLITK_FLOATS, M, N, K, s, cus, r.splits);
        }
    }
}

// fc2 / fc3 of the two encoders: one or two 128-row tiles at small batch -> split K as fc1 does (same row threshold)
static constexpr int SKINNY_ROWS = 1024;       // encoder rows (30 or 34 per frame) below which the fc GEMMs run split-K: B <= 34 / 30
template <class AL, class Epi>
static hipError_t fc_gemm(Handle* h, const char* role, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc, int M, int N, int K,
                          float* P, hipStream_t s) {
    // [r3] bf16 mode only (the fp32 routing, and with it the fp32 bits per batch size, stays as it was): also above the row threshold
    // while the 128 x 128 tiles fill less than half the chip (EgoCap at 128 x 128 heatmaps, B = 32 / 64: 36 / 68 tiles of fc2)
    const bool few_tiles = h && h->precision == EGOTAP_PREC_BF16 && 2L * ((M + 127) / 128) * (N / 128) <= device_cu_count() &&
                           (size_t)M * N * 8 <= SPLITK_FLOATS;
    if ((M >= SKINNY_ROWS && !few_tiles) || N % 128 != 0 || K % 32 != 0) return gemm<TileA>(h, role, al, W, epi, C, ldc, M, N, K, s);
    if (M <= 64) {
        static const std::string kname64 = std::string("gemm_f32_splitk_kernel<64x128x32,") + AlName<AL>::v + ">+splitk_reduce_kernel<" + EpiName<Epi>::v + ">";
        GemmTimer t(h, s, role, kname64.c_str(), 2.0 * M * N * K);
        return gemm_f32_splitk_launch<TileS>(al, W, epi, C, ldc, P, SPLITK_FLOATS, M, N, K, s, device_cu_count());
    }
    static const std::string kname = std::string("gemm_f32_splitk_kernel<128x128x32,") + AlName<AL>::v + ">+splitk_reduce_kernel<" + EpiName<Epi>::v + ">";
    GemmTimer t(h, s, role, kname.c_str(), 2.0 * M * N * K);
    return gemm_f32_splitk_launch<TileA>(al, W, epi, C, ldc, P, SPLITK_FLOATS, M, N, K, s);
}

struct LiftWs {
    size_t X, Y, QKV, CTX, HID, Z1, Z2, POSZ, ROTZ, F0, G0, HS0, F1, G1, HS1, C0, C1, ZERO, HPA, HPB, FAULT, SPLITK, total;
};
static LiftWs lift_ws(const Handle* h, int B) {
    LiftWs w;
    const size_t M = (size_t)B * h->seq, D = h->D, BT = (size_t)B * h->T, JB = (size_t)h->J * B, H = h->H;
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o = al256(o + floats * 4); return r; };
    w.X = take(M * D); w.Y = take(M * D); w.QKV = take(M * 3 * D); w.CTX = take(M * D); w.HID = take(M * 4 * D);
    w.Z1 = take(BT * 2048); w.Z2 = take(BT * 512); w.POSZ = take(BT * h->hid); w.ROTZ = take(BT * h->hid);
    w.F0 = take(JB * (H + 2 * h->hid)); w.G0 = take(JB * 4 * H); w.HS0 = take(JB * H);
    w.F1 = take(JB * H); w.G1 = take(JB * 4 * H); w.HS1 = take(JB * H);
    w.C0 = take((size_t)B * H); w.C1 = take((size_t)B * H); w.ZERO = take((size_t)B * H);
    w.HPA = take((size_t)h->J * B * H);                            // the propagation units' gated state: one [B, H] buffer per step
    w.HPB = w.HPA + al256((size_t)B * H * 4);                      // (the per-step fallback kernels ping-pong between the first two)
    w.FAULT = take(64);                                            // fault word of the one-launch recurrence (pu_chain.h)
    w.SPLITK = take(SPLITK_FLOATS);       // split-K partial sums of the small-batch GEMMs (gemm_small)
    w.total = o;
    return w;
}

extern "C" int egotap_lift_workspace_bytes(egotap_handle h, int B, size_t* bytes) {
    EGO_CHECK(h && bytes, "null argument");
    EGO_CHECK(B >= 0, "negative batch");
    *bytes = lift_ws(h, B > 0 ? B : 1).total;
    return EGOTAP_OK;
}

extern "C" int egotap_lift_intermediate(egotap_handle h, int B, const char* name, size_t* offset, int64_t* numel) {
    EGO_CHECK(h && name && offset && numel, "null argument");
    const LiftWs w = lift_ws(h, B > 0 ? B : 1);
    const int64_t M = (int64_t)B * h->seq;
    if (!strcmp(name, "tokens")) { *offset = w.Y; *numel = M * h->D; }
    else if (!strcmp(name, "x")) { *offset = w.X; *numel = M * h->D; }
    else if (!strcmp(name, "pos_embed")) { *offset = w.POSZ; *numel = (int64_t)B * h->T * h->hid; }
    else if (!strcmp(name, "rot_embed")) { *offset = w.ROTZ; *numel = (int64_t)B * h->T * h->hid; }
    else if (!strcmp(name, "skel_embed")) { *offset = w.HS1; *numel = (int64_t)h->J * B * h->H; }
    else { egotap_set_error("unknown intermediate '%s'", name); return EGOTAP_ERR_INVALID; }
    return EGOTAP_OK;
}

extern "C" int egotap_set_pu_chain(egotap_handle h, int enable) {
    EGO_CHECK(h, "null handle");
    h->pu_chain = enable != 0;
    h->pu_resident[0] = h->pu_resident[1] = -1;
    return EGOTAP_OK;
}
extern "C" int egotap_debug_pu_drop_workgroups(egotap_handle h, int n) {
    EGO_CHECK(h && n >= 0 && n < 16, "egotap_debug_pu_drop_workgroups: n in [0, 16)");
    h->pu_debug_drop = n;
    return EGOTAP_OK;
}
extern "C" int egotap_pu_chain_status(egotap_handle h, int* enabled, int* faults) {
    EGO_CHECK(h, "null handle");
    // meaningful after the caller has synchronised the stream of the call it asks about (the word is written by the device)
    if (h->pu_fault_host && __atomic_load_n(h->pu_fault_host, __ATOMIC_RELAXED) != 0u) {
        __atomic_store_n(h->pu_fault_host, 0u, __ATOMIC_RELAXED);
        h->pu_faults++;
        h->pu_chain = false;
        h->pu_resident[0] = h->pu_resident[1] = -1;
    }
    if (enabled) *enabled = h->pu_chain ? 1 : 0;
    if (faults) *faults = h->pu_faults;
    return EGOTAP_OK;
}
extern "C" int egotap_set_precision(egotap_handle h, int mode) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(mode == EGOTAP_PREC_F32 || mode == EGOTAP_PREC_BF16X3 || mode == EGOTAP_PREC_BF16, "egotap_set_precision: unknown mode %d", mode);
    h->precision = mode;
    h->lift_arena = nullptr;         // the prepared weights belong to a precision mode: a mode change unfreezes the handle
    for (int n = 0; n < EGOTAP_NET_COUNT; ++n) h->hm_arena[n] = nullptr;
    return EGOTAP_OK;
}

extern "C" int egotap_set_weight_scratch(egotap_handle h, void* buf, size_t bytes) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(((uintptr_t)buf & 15) == 0, "egotap_set_weight_scratch: 16-byte alignment");
    h->wscratch = (__bf16*)buf;
    h->wscratch_bytes = buf ? bytes : 0;
    return EGOTAP_OK;
}

extern "C" int egotap_set_act_scratch(egotap_handle h, void* buf, size_t bytes) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(((uintptr_t)buf & 15) == 0, "egotap_set_act_scratch: 16-byte alignment");
    h->ascratch = (__bf16*)buf;
    h->ascratch_bytes = buf ? bytes : 0;
    return EGOTAP_OK;
}

extern "C" int egotap_lift_debug_stop(egotap_handle h, int stage) {
    EGO_CHECK(h, "null handle");
    h->debug_stop = stage;   // 0: full forward; 1: after embeddings; 2+i: after ViT layer i  ("x" holds the state)
    return EGOTAP_OK;
}

// ------------------------------------------------------------------------------------------------ forward
static hipError_t launch_ln(const float* x, float* y, const float* g, const float* b, int rows, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    const int blocks = min((rows + 3) / 4, 256 * 8);
    hipLaunchKernelGGL(layernorm_f32_kernel<1024>, dim3(blocks), dim3(256), 0, s, x, y, g, b, rows, eps);
    return hipGetLastError();
}

// [r4] x = x + ctx W^T + bias, y = LayerNorm(x): at serving batches (the product is split over K) the reduce of the partials and the LayerNorm
// that follows are ONE launch (splitk_reduce_res_ln_kernel: same bits as the two); otherwise gemm_small + launch_ln as before.
static hipError_t gemm_res_ln(Handle* h, const char* role, const float* A, long lda, const float* Wp, const float* bias, float* X, int M, int D, int K,
                              const float* ln_g, const float* ln_b, float* Y, float* P, hipStream_t s) {
    if (D == 1024) {
        const SmallRoute r = gemm_small_route(h, true, M, D, K, D, device_cu_count());      // gemm_small's own decision, not a copy of its rule
        if ((r.kind == GS_SPLIT_S || r.kind == GS_SPLIT_A) && r.splits > 1) {
            static const std::string kname = "gemm_f32_splitk_kernel<ALoadPlain>+splitk_reduce_res_ln_kernel";
            GemmTimer t(h, s, role, kname.c_str(), 2.0 * M * D * K);
            hipError_t e = r.kind == GS_SPLIT_S ? gemm_f32_splitk_partials<TileS>(ALoadPlain{A, lda}, segmat1(Wp, D, K), P, SPLITK_FLOATS, M, D, K, s, r.splits)
                                                : gemm_f32_splitk_partials<TileA>(ALoadPlain{A, lda}, segmat1(Wp, D, K), P, SPLITK_FLOATS, M, D, K, s, r.splits);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(splitk_reduce_res_ln_kernel<1024>, dim3(min((M + 3) / 4, 256 * 8)), dim3(256), 0, s, (const float*)P, bias, (const float*)X, X, ln_g,
                               ln_b, Y, M, r.splits, 1e-12f);
            return hipGetLastError();
        }
    }
    hipError_t e = gemm_small(h, role, ALoadPlain{A, lda}, segmat1(Wp, D, K), EpiBiasRes{segvec1(bias, D), X, D}, X, D, M, D, K, P, s);
    if (e != hipSuccess) return e;
    return launch_ln(X, Y, ln_g, ln_b, M, 1e-12f, s);
}

// [r6] A compact product of the pose-only forward (M = B T ppd^2: at B = 256 and N = 1024, 1 920 tiles of 256 x 256 = 7.5 rounds on 256 CUs):
// the tile rows that fill WHOLE rounds on the 256 x 256 kernel, and the rows past them as unsplit 128 x 128 tiles when that is estimated faster
// than one more half-empty round (the constants of gemm_small_route).  Same k order per output element in both kernels: same bits.
// rebase(x, m0): the loader / epilogue of the same product seen from compact row m0 on.
static ALoadPlain rebase(const ALoadPlain& a, int m0) { return ALoadPlain{a.A + (long)m0 * a.lda, a.lda}; }
static ALoadLive rebase(ALoadLive a, int m0) { a.lr.m0 += m0; return a; }
static EpiBias rebase(const EpiBias& e, int) { return e; }
static EpiBiasGelu rebase(const EpiBiasGelu& e, int) { return e; }
static EpiBiasRes rebase(EpiBiasRes e, int m0) { e.R += (long)m0 * e.ldr; return e; }
static EpiBiasResLive rebase(EpiBiasResLive e, int m0) { e.lr.m0 += m0; return e; }
template <class AL, class Epi>
static hipError_t gemm_rounds(Handle* h, const char* role, const AL& al, const SegMat& W, const Epi& epi, float* C, long ldc, int M, int N, int K,
                              hipStream_t s) {
    const int cus = device_cu_count(), tn = N / 256;
    const long tiles = (long)((M + 255) / 256) * tn;
    const int mh = (int)((tiles / cus) * cus / tn) * 256;          // rows of the whole rounds
    if (N % 256 == 0 && K % 32 == 0 && mh > 0 && mh < M) {
        const double t_round = K * 0.2319 + 5.0;
        const double t_big = (double)((tiles + cus - 1) / cus) * t_round;
        const double t_split = (double)(((long)(mh / 256) * tn + cus - 1) / cus) * t_round + 4.0 + gemm_f32_direct_estimate_us<TileA>(M - mh, N, K, cus);
        if (t_split < t_big) {
            hipError_t e = gemm_big(h, role, al, W, epi, C, ldc, mh, N, K, s);
            if (e != hipSuccess) return e;
            return gemm<TileA>(h, role, rebase(al, mh), W, rebase(epi, mh), C + (long)mh * ldc, ldc, M - mh, N, K, s);
        }
    }
    return gemm_big(h, role, al, W, epi, C, ldc, M, N, K, s);
}

// [r6] Whether the pose-only forward runs the last ViT layer on the live rows alone (egotap_lift_predict_pose): fc1 reads only the first T
// cells of the grid, so the dummy cells' queries, attention rows, projections, MLP and final LayerNorm in that layer are never used -- only
// their K and V feed the live rows.  Every product involved is row-independent and the pruned launches run the same kernels with the same
// k order, so the pose keeps its bits -- provided nothing SPLITS: exact fp32 only, every last-layer product of the full problem on the
// 256 x 256 kernel (GS_BIG: the large batches) and its attention unsplit.  Anything else takes the full path.
static bool lift_prune_last(Handle* h, int B) {
    const int D = h->D, M = B * h->seq, Nq = h->T * h->ppd * h->ppd;
    if (h->precision != EGOTAP_PREC_F32 || h->debug_stop != 0 || h->cfg.vit_layers < 1 || Nq < 32 || Nq >= h->seq || D % 256 != 0) return false;
    const int cus = device_cu_count();
    if (gemm_small_route(h, true, M, 3 * D, D, D, cus, true).kind != GS_BIG || gemm_small_route(h, true, M, D, D, D, cus).kind != GS_BIG ||
        gemm_small_route(h, true, M, 4 * D, D, 4 * D, cus, true).kind != GS_BIG || gemm_small_route(h, true, M, D, 4 * D, D, cus).kind != GS_BIG)
        return false;
    return attention_f32_ksplit(B, h->seq, h->cfg.vit_heads, SPLITK_FLOATS, cus) == 1;
}

// Whether the pose-only forward projects layer 0's frame-invariant rows once per call.  The grid's dummy cells hold mask_token + position embedding
// in every image, so their LayerNorm-1 rows and their layer-0 q | k | v are those of image 0.  Where the dummy cells are whole trailing grid rows the
// shared tokens are the contiguous tail [n0, seq) of every image: layer 0 then projects the B * n0 live rows as ONE compact product (ALoadHead /
// EpiBiasHead, the 256 x 256 kernel) and image 0's tail as a second, small one, and its attention reads the tail's Q / K / V from image 0
// (attention_f32_shared_launch).  Every product involved is row-independent and runs unsplit with the k order of the full forward's, so the pose
// keeps its bits -- provided the full product is unsplit too (GS_BIG, as is the live one) and the attention is; the seam must fall between whole
// 32-token attention tiles.  Returns n0, or 0: layer 0 as in the full forward.
static int lift_share_layer0(Handle* h, int B, bool pose_only) {
    const int D = h->D, seq = h->seq, rows = h->T / h->grid;
    if (!pose_only || h->precision != EGOTAP_PREC_F32 || h->debug_stop != 0 || h->cfg.vit_layers < 2) return 0;
    if (h->T >= h->grid * h->grid || h->T % h->grid != 0 || rows < 1) return 0;
    const int n0 = rows * h->ppd * h->side;
    if (n0 % 32 != 0 || seq % 32 != 0 || D % DmaF32Cfg::BN != 0 || D % DmaF32Cfg::BK != 0) return 0;
    if ((long)B * seq >= (1L << 31) || !HeadRows::make(n0, seq).exact((long)B * n0)) return 0;
    const int cus = device_cu_count();
    if (gemm_small_route(h, true, B * seq, 3 * D, D, D, cus, true).kind != GS_BIG || gemm_small_route(h, true, B * n0, 3 * D, D, D, cus, true).kind != GS_BIG) return 0;
    return attention_f32_ksplit(B, seq, h->cfg.vit_heads, SPLITK_FLOATS, cus) == 1 ? n0 : 0;
}

// ---- frozen-weight serving: the arena of egotap_lift_freeze.  Every bf16 weight copy the bf16-storage inference forward multiplies by, in the layout
// its GEMMs read (row-major [N][K]; q | k | v stacked as one [3D][D] block), and per layer the fused q | k | v bias (fp32); 256-byte aligned slices.
// p != nullptr: fills T, the segment table of prep_weights_all_kernel (bf16s_ops.h).
struct LiftFrozen {
    size_t patch, qkv[8], o[8], up[8], dn[8], bias3[8], fc1p, fc1r, total;
};
// the geometry / precision for which the lifting head has prepared weights at all (the bf16-storage route; whether a given call takes it also
// depends on its batch and on the weight scratch, as before)
static bool lift_frozen_route(const Handle* h) { return h->precision == EGOTAP_PREC_BF16 && h->D == 1024 && h->seq % 32 == 0; }
static LiftFrozen lift_frozen_plan(const Handle* h, const LiftParams* p, PrepTable* T) {
    LiftFrozen f{};
    const size_t D = h->D, K1 = (size_t)h->ppd * h->ppd * D, K1r = 2 * (size_t)h->cfg.hm_size * h->cfg.hm_size;
    const int NL = h->cfg.vit_layers;
    size_t o = 0;
    int ns = 0;
    unsigned chunk = 0;
    auto seg = [&](const float* src, size_t elems, size_t elem_bytes, size_t at) {      // at: (size_t)-1 = a slice of its own
        const size_t dst = at == (size_t)-1 ? o : at;
        if (at == (size_t)-1) o = al256(o + elems * elem_bytes);
        if (T && ns < PrepTable::MAXS) {
            T->s[ns] = PrepSeg{src, (unsigned long long)dst, (unsigned)(elems / 8), chunk};
            chunk += (unsigned)((elems / 8 + PrepTable::CHUNK8 - 1) / PrepTable::CHUNK8);
        }
        ++ns;
        return dst;
    };
    const size_t own = (size_t)-1;
    f.patch = seg(p ? p->patch_w : nullptr, D * 256, 2, own);
    for (int i = 0; i < NL; ++i) {
        const LiftParams::Layer* L = p ? &p->layer[i] : nullptr;
        f.qkv[i] = o;
        o = al256(o + 3 * D * D * 2);
        seg(L ? L->q_w : nullptr, D * D, 2, f.qkv[i]);
        seg(L ? L->k_w : nullptr, D * D, 2, f.qkv[i] + D * D * 2);
        seg(L ? L->v_w : nullptr, D * D, 2, f.qkv[i] + 2 * D * D * 2);
        f.o[i] = seg(L ? L->o_w : nullptr, D * D, 2, own);
        f.up[i] = seg(L ? L->up_w : nullptr, 4 * D * D, 2, own);
        f.dn[i] = seg(L ? L->dn_w : nullptr, 4 * D * D, 2, own);
    }
    f.fc1p = seg(p ? p->pos_fc[0].w : nullptr, 2048 * K1, 2, own);
    f.fc1r = seg(p ? p->rot_fc[0].w : nullptr, 2048 * K1r, 2, own);
    if (T) T->nround = ns;
    for (int i = 0; i < NL; ++i) {
        const LiftParams::Layer* L = p ? &p->layer[i] : nullptr;
        f.bias3[i] = o;
        o = al256(o + 3 * D * 4);
        seg(L ? L->q_b : nullptr, D, 4, f.bias3[i]);
        seg(L ? L->k_b : nullptr, D, 4, f.bias3[i] + D * 4);
        seg(L ? L->v_b : nullptr, D, 4, f.bias3[i] + 2 * D * 4);
    }
    if (T) { T->nseg = ns; T->chunks = (int)chunk; }
    f.total = o;
    return f;
}

// EGOTAP_PREC_BF16 at a batch that fills the chip: whether the forward keeps its activations in bf16 (below).  One rule for the forward and for
// egotap_predict_pose_rgb, which asks it whether the head will read a bf16 copy of the heatmaps.
static constexpr int BF16S_MIN_ROWS = 512;      // [r4] 4096 before: a B = 4 forward (2304 rows) took 2.1 ms on the fp32-tensor path, 1.5 ms on this one (B = 1: 1.46 -> 1.38)
static bool lift_bf16s_route(const Handle* h, int B) {
    // (sequence lengths that are not a multiple of 32 -- heatmap sides 32, 48, 96 ...: the bf16-storage attention tiles whole 32-key blocks -- stay on
    // fp32 tensors with bf16 products in the GEMMs and the exact-fp32 attention kernel, which masks a ragged last key tile)
    return h->precision == EGOTAP_PREC_BF16 && h->D == 1024 && (long)B * h->seq >= BF16S_MIN_ROWS && h->wscratch != nullptr && h->seq % 32 == 0 &&
           h->wscratch_bytes >= (size_t)2 * 2048 * (size_t)(h->ppd * h->ppd * h->D);
}

// hmb_ready != nullptr (egotap_predict_pose_rgb's hand-off; the bf16-storage route only): the heatmaps as bf16 [B, 6J, S, S] already, exactly what
// f32_to_bf16_kernel would make of `hm`; hm is then not read and may be null
static int lift_forward_impl(Handle* h, const float* hm, int B, float* pose, void* ws, size_t ws_bytes, void* stream, bool pose_only,
                             const char* who, const __bf16* hmb_ready = nullptr) {
    EGO_CHECK(h, "null handle");
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(B > 0 && (hm || hmb_ready) && pose && ws, "%s: null argument or negative batch", who);
    EGO_CHECK((((uintptr_t)hm | (uintptr_t)hmb_ready) & 15) == 0 && ((uintptr_t)ws & 255) == 0, "hm must be 16-byte and ws 256-byte aligned");
    int rc = lift_resolve(h);
    if (rc != EGOTAP_OK) return rc;
    const LiftWs w = lift_ws(h, B);
    if (ws_bytes < w.total) {
        egotap_set_error("workspace too small: %zu bytes given, %zu needed for B=%d", ws_bytes, w.total, B);
        return EGOTAP_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    const LiftParams& p = h->lp;
    char* base = (char*)ws;
    auto F = [&](size_t off) { return (float*)(base + off); };
    float *X = F(w.X), *Y = F(w.Y), *QKV = F(w.QKV), *CTX = F(w.CTX), *HID = F(w.HID);
    float* SPK = F(w.SPLITK);
    float *Z1 = F(w.Z1), *Z2 = F(w.Z2), *POSZ = F(w.POSZ), *ROTZ = F(w.ROTZ);
    float *F0 = F(w.F0), *G0 = F(w.G0), *HS0 = F(w.HS0), *F1 = F(w.F1), *G1 = F(w.G1), *HS1 = F(w.HS1);
    float *C0 = F(w.C0), *C1 = F(w.C1), *ZERO = F(w.ZERO), *HPA = F(w.HPA), *HPB = F(w.HPB);
    const int D = h->D, M = B * h->seq, BT = B * h->T, J = h->J, H = h->H, hid = h->hid, JB = J * B;
    const int S = h->cfg.hm_size, HW = S * S;
    using Tile = TileA;

    // EGOTAP_PREC_BF16 at a batch that fills the chip: bf16 ACTIVATION STORAGE (the same workspace slices hold bf16): LayerNorm, the
    // GEMM epilogues and attention write bf16, every GEMM reads bf16 operands through the LDS DMA (gemm_bf16s.h); weights are rounded
    // into the caller's weight scratch right before each launch (nothing cached: the fp32 parameters stay the source of truth)
    const bool bf16s = lift_bf16s_route(h, B);
    EGO_CHECK(bf16s || hmb_ready == nullptr, "%s: a bf16 heatmap operand was handed to a route that reads fp32 heatmaps", who);
    // frozen (egotap_lift_freeze): the same GEMMs read the arena's copies -- the same bits the per-call preparation would write -- and no
    // prep_weight_kernel / concat3_kernel is launched.  Every other route ignores the arena.
    const bool frozen = bf16s && h->lift_arena != nullptr;
    const LiftFrozen fz = frozen ? lift_frozen_plan(h, nullptr, nullptr) : LiftFrozen{};
    auto FW = [&](size_t off) { return (const __bf16*)(h->lift_arena + off); };
    // H1+H2: tile -> patch embed -> mask token -> + position embeddings
    if (bf16s) {
        // [r3] on the bf16-storage GEMM: the heatmaps' bf16 copy in the (still free) MLP buffer, by LDS DMA; zeros for the dummy cells in SPK
        const __bf16* hmb0 = hmb_ready ? hmb_ready : (const __bf16*)HID;
        const long n8 = (long)B * h->C * HW / 8;
        if (!hmb_ready) hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, hm, (__bf16*)HID, n8);
        if (!frozen) hipLaunchKernelGGL(prep_weight_kernel, dim3((256 + 63) / 64, (D + 63) / 64), dim3(256), 0, s, p.patch_w, h->wscratch, (__bf16*)nullptr, D, 256, (long)D);
        EGO_HIP(zero_fill(SPK, 256, s));
        const XPatch xl{hmb0, (const __bf16*)SPK, h->patches()};
        const SEpiPatchF32 ep{p.patch_b, p.mask_tok, p.pos_emb, X, D, h->cells()};
        EGO_HIP(gemm_bf16s_launch(xl, frozen ? FW(fz.patch) : h->wscratch, 256L, ep, M, D, 256, device_cu_count(), s));
    } else {
        ALoadPatch al{hm, h->patches()};
        // [r3] fp32 at a batch that fills the chip: a zero page for the dummy cells (the head of the PU chain's ZERO slice, which is cleared as a
        // whole further down and not read before) makes the loader pure address math -> the LDS-DMA kernel instead of the register-staged one
        if (h->precision == EGOTAP_PREC_F32 && (long)((M + 255) / 256) * (D / 256) >= 160 && (size_t)B * H * 4 >= 1024) {
            EGO_HIP(zero_fill(ZERO, 1024, s));
            al.zeros = ZERO;
        }
        EpiPatch ep{p.patch_b, p.mask_tok, p.pos_emb, D, h->cells()};
        EGO_HIP((gemm_small(h, "patch_embed", al, segmat1(p.patch_w, D, 256), ep, X, D, M, D, 256, SPK, s)));
    }
    if (h->debug_stop == 1) return EGOTAP_OK;
    if (bf16s) {
        __bf16 *Yb = (__bf16*)Y, *QKVb = (__bf16*)QKV, *CTXb = (__bf16*)CTX, *HIDb = (__bf16*)HID, *Wb = h->wscratch;
        float* bias3 = SPK;
        const int cu = device_cu_count();
        auto prep = [&](const float* wsrc, __bf16* dst, int n, int k) {
            hipLaunchKernelGGL(prep_weight_kernel, dim3((k + 63) / 64, (n + 63) / 64), dim3(256), 0, s, wsrc, dst, (__bf16*)nullptr, n, k, (long)n);
        };
        auto ln = [&](const float* gg, const float* bb) {
            hipLaunchKernelGGL(ln_fwd_bf16_kernel<1024>, dim3((M + 3) / 4), dim3(256), 0, s, (const float*)X, Yb, gg, bb, (float*)nullptr, (float*)nullptr, M, 1e-12f);
        };
        for (int i = 0; i < h->cfg.vit_layers; ++i) {
            const auto& L = p.layer[i];
            ln(L.ln1_g, L.ln1_b);
            if (!frozen) {
                prep(L.q_w, Wb, D, D); prep(L.k_w, Wb + (size_t)D * D, D, D); prep(L.v_w, Wb + (size_t)2 * D * D, D, D);
                hipLaunchKernelGGL(concat3_kernel, dim3((D + 255) / 256), dim3(256), 0, s, L.q_b, L.k_b, L.v_b, bias3, D);
            }
            EGO_HIP(hipGetLastError());
            EGO_HIP(gemm_bf16s_plain_launch(XPlain{Yb, (long)D}, frozen ? FW(fz.qkv[i]) : Wb, (long)D,
                                            SEpiBf16{frozen ? (const float*)(h->lift_arena + fz.bias3[i]) : bias3, QKVb, 3L * D}, M, 3 * D, D, cu, s));
            EGO_HIP(attention_bf16s_fwd_launch(QKVb, CTXb, nullptr, B, h->seq, h->cfg.vit_heads, s));
            if (!frozen) prep(L.o_w, Wb, D, D);
            EGO_HIP(gemm_bf16s_plain_launch(XPlain{CTXb, (long)D}, frozen ? FW(fz.o[i]) : Wb, (long)D, SEpiResF32{L.o_b, X, X, (long)D}, M, D, D, cu, s));
            ln(L.ln2_g, L.ln2_b);
            if (!frozen) prep(L.up_w, Wb, 4 * D, D);
            EGO_HIP(gemm_bf16s_plain_launch(XPlain{Yb, (long)D}, frozen ? FW(fz.up[i]) : Wb, (long)D, SEpiGelu{L.up_b, HIDb, 4L * D}, M, 4 * D, D, cu, s));
            if (!frozen) prep(L.dn_w, Wb, D, 4 * D);
            EGO_HIP(gemm_bf16s_plain_launch(XPlain{HIDb, 4L * D}, frozen ? FW(fz.dn[i]) : Wb, 4L * D, SEpiResF32{L.dn_b, X, X, (long)D}, M, D, 4 * D, cu, s));
            if (h->debug_stop == 2 + i) return EGOTAP_OK;
        }
        ln(p.lnf_g, p.lnf_b);                               // tokens (bf16) -> fc1's gathering loader
        auto bnf = [](const LiftParams::Fc& f, float* out) { return SEpiBnLreluF32{f.b, f.g, f.beta, f.mean, f.var, 1e-5f, 0.2f, out, 2048L}; };
        auto bn = [](const LiftParams::Fc& f) { return EpiBnLrelu{f.b, f.g, f.beta, f.mean, f.var, 1e-5f, 0.2f}; };
        {
            const int K1 = h->ppd * h->ppd * D;
            if (!frozen) prep(p.pos_fc[0].w, Wb, 2048, K1);
            const __bf16* W1 = frozen ? FW(fz.fc1p) : Wb;
            // [r3] few encoder rows (EgoCap at 128 x 128 heatmaps, B = 32: 1088 rows = 40 tiles for 256 CUs, K = 65536): split K over the chip
            const XTokens xt{Yb, h->tokens()};
            const int sp = gemm_bf16s_ksplit(BT, 2048, K1, cu, SPLITK_FLOATS);
            if (sp > 1) EGO_HIP(gemm_bf16s_splitk_launch(xt, W1, (long)K1, bnf(p.pos_fc[0], Z1), SPK, sp, BT, 2048, K1, cu, s));
            else EGO_HIP(fc1_nt(h, 0, Yb, W1, (long)K1, bnf(p.pos_fc[0], Z1), BT, cu, s));
            EGO_HIP((fc_gemm(h, "pos_fc2", ALoadPlain{Z1, 2048}, segmat1(p.pos_fc[1].w, 512, 2048), bn(p.pos_fc[1]), Z2, 512, BT, 512, 2048, SPK, s)));
            EGO_HIP((fc_gemm(h, "pos_fc3", ALoadPlain{Z2, 512}, segmat1(p.pos_fc[2].w, hid, 512), bn(p.pos_fc[2]), POSZ, hid, BT, hid, 512, SPK, s)));
        }
        {
            const __bf16* hmb = hmb_ready ? hmb_ready : HIDb;      // the MLP's hidden buffer is free now: bf16 copy of the input heatmaps
            const long n8 = (long)B * h->C * HW / 8;
            if (!hmb_ready) hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, hm, HIDb, n8);
            if (!frozen) prep(p.rot_fc[0].w, Wb, 2048, 2 * HW);
            const __bf16* W1 = frozen ? FW(fz.fc1r) : Wb;
            EGO_HIP(hipGetLastError());
            const XRot xr{hmb, h->rots()};
            const int sp = gemm_bf16s_ksplit(BT, 2048, 2 * HW, cu, SPLITK_FLOATS);
            if (sp > 1) EGO_HIP(gemm_bf16s_splitk_launch(xr, W1, 2L * HW, bnf(p.rot_fc[0], Z1), SPK, sp, BT, 2048, 2 * HW, cu, s));
            else EGO_HIP(fc1_nt(h, 1, hmb, W1, 2L * HW, bnf(p.rot_fc[0], Z1), BT, cu, s));
            EGO_HIP((fc_gemm(h, "rot_fc2", ALoadPlain{Z1, 2048}, segmat1(p.rot_fc[1].w, 512, 2048), bn(p.rot_fc[1]), Z2, 512, BT, 512, 2048, SPK, s)));
            EGO_HIP((fc_gemm(h, "rot_fc3", ALoadPlain{Z2, 512}, segmat1(p.rot_fc[2].w, hid, 512), bn(p.rot_fc[2]), ROTZ, hid, BT, hid, 512, SPK, s)));
        }
    } else {
    // H3-H8: pre-LN transformer layers.  [r4] Every LayerNorm but the first follows a residual projection: gemm_res_ln runs the two as one launch
    // where the projection is split over K (serving batches); ln1 of layer i + 1 (or the final LayerNorm) therefore rides with layer i's MLP.
    const int NL = h->cfg.vit_layers;
    const bool prune = pose_only && lift_prune_last(h, B);
    const int share0 = lift_share_layer0(h, B, pose_only);       // > 0: layer 0's tokens from here on are projected for image 0 only
    EGO_HIP(launch_ln(X, Y, NL > 0 ? p.layer[0].ln1_g : p.lnf_g, NL > 0 ? p.layer[0].ln1_b : p.lnf_b, M, 1e-12f, s));
    for (int i = 0; i < NL; ++i) {
        const auto& L = p.layer[i];
        if (prune && i + 1 == NL) {
            // [r6] the last layer on the live rows, compact order (b, cell < T, patch row, patch col) = fc1's (LiveRows, gemm_f32.h).  Slices:
            // K | V of all M rows into QKV's K / V columns, compact Q into its Q columns (rows 0 .. Mc); compact attention output in CTX; the
            // compact residual stream Xc in QKV (dead after the attention), its LayerNorms in Y (dead after the projections), the MLP in HID.
            const LiveRows lr{h->seq, h->side, h->ppd, h->grid, h->T};
            const int Nq = h->T * h->ppd * h->ppd, Mc = B * Nq;
            float* Xc = QKV;
            SegMat Wkv; Wkv.p[0] = L.k_w; Wkv.p[1] = L.v_w; Wkv.p[2] = L.v_w; Wkv.seg = D; Wkv.ld = D;
            SegVec bkv; bkv.p[0] = L.k_b; bkv.p[1] = L.v_b; bkv.p[2] = L.v_b; bkv.seg = D;
            EGO_HIP((gemm_big(h, "kv", ALoadPlain{Y, D}, Wkv, EpiBias{bkv}, QKV + D, 3L * D, M, 2 * D, D, s)));
            EGO_HIP((gemm_rounds(h, "q_live", ALoadLive{Y, D, lr}, segmat1(L.q_w, D, D), EpiBias{segvec1(L.q_b, D)}, QKV, 3L * D, Mc, D, D, s)));
            EGO_HIP(attention_f32_live_launch(QKV, 3L * D, Nq, QKV, CTX, B, h->seq, h->cfg.vit_heads, s));
            EGO_HIP((gemm_rounds(h, "attn_out_live", ALoadPlain{CTX, D}, segmat1(L.o_w, D, D), EpiBiasResLive{segvec1(L.o_b, D), X, D, lr}, Xc, D, Mc, D, D, s)));
            EGO_HIP(launch_ln(Xc, Y, L.ln2_g, L.ln2_b, Mc, 1e-12f, s));
            EGO_HIP((gemm_rounds(h, "mlp_up_live", ALoadPlain{Y, D}, segmat1(L.up_w, 4 * D, D), EpiBiasGelu{segvec1(L.up_b, 4 * D)}, HID, 4L * D, Mc, 4 * D, D, s)));
            EGO_HIP((gemm_rounds(h, "mlp_down_live", ALoadPlain{HID, 4L * D}, segmat1(L.dn_w, D, 4 * D), EpiBiasRes{segvec1(L.dn_b, D), Xc, D}, Xc, D, Mc, D, 4 * D, s)));
            EGO_HIP(launch_ln(Xc, Y, p.lnf_g, p.lnf_b, Mc, 1e-12f, s));       // compact tokens: fc1 reads them as plain rows below
            break;
        }
        {
            SegMat Wqkv; Wqkv.p[0] = L.q_w; Wqkv.p[1] = L.k_w; Wqkv.p[2] = L.v_w; Wqkv.seg = D; Wqkv.ld = D;
            SegVec bqkv; bqkv.p[0] = L.q_b; bqkv.p[1] = L.k_b; bqkv.p[2] = L.v_b; bqkv.seg = D;
            if (i == 0 && share0 > 0) {
                // the live rows of every image: one launch of the 256 x 256 kernel over B * n0 compact rows, read from and stored to their physical
                // rows; then the shared tail of image 0, unsplit 128 x 128 tiles.  Rows (b > 0, n >= n0) of QKV are neither written nor read.
                const HeadRows hr = HeadRows::make(share0, h->seq);
                const int Ml = B * share0;
                {
                    static const std::string kdma = std::string("gemm_f32_dma_kernel<256x256x16,") + AlName<ALoadHead>::v + "," + EpiName<EpiBiasHead>::v + ">";
                    GemmTimer t(h, s, "qkv", kdma.c_str(), 2.0 * Ml * 3 * D * D);
                    EGO_HIP(gemm_f32_dma_launch(ALoadHead{Y, D, hr}, Wqkv, EpiBiasHead{{bqkv}, QKV, 3L * D, hr}, QKV, 3L * D, Ml, 3 * D, D, device_cu_count(), s));
                }
                EGO_HIP((gemm<TileA>(h, "qkv_shared", ALoadPlain{Y + (long)share0 * D, D}, Wqkv, EpiBias{bqkv}, QKV + (long)share0 * 3 * D, 3L * D, h->seq - share0, 3 * D, D, s)));
            } else
            EGO_HIP((gemm_small(h, "qkv", ALoadPlain{Y, D}, Wqkv, EpiBias{bqkv}, QKV, 3L * D, M, 3 * D, D, SPK, s)));
        }
        if (h->precision == EGOTAP_PREC_BF16X3 && h->seq % 32 == 0) EGO_HIP(attention_bf16_launch<3>(QKV, CTX, B, h->seq, h->cfg.vit_heads, s));
        else if (h->precision == EGOTAP_PREC_BF16 && h->seq % 32 == 0) EGO_HIP(attention_bf16_launch<1>(QKV, CTX, B, h->seq, h->cfg.vit_heads, s));
        else if (i == 0 && share0 > 0) EGO_HIP(attention_f32_shared_launch(QKV, CTX, B, h->seq, h->cfg.vit_heads, share0, s));
        else EGO_HIP(attention_f32_launch(QKV, CTX, B, h->seq, h->cfg.vit_heads, s, nullptr, SPK, SPLITK_FLOATS, device_cu_count()));   // (SPK: free between the GEMMs; key-split partials at B <= 2)
        EGO_HIP(gemm_res_ln(h, "attn_out", CTX, D, L.o_w, L.o_b, X, M, D, D, L.ln2_g, L.ln2_b, Y, SPK, s));
        EGO_HIP((gemm_small(h, "mlp_up", ALoadPlain{Y, D}, segmat1(L.up_w, 4 * D, D), EpiBiasGelu{segvec1(L.up_b, 4 * D)}, HID, 4L * D, M, 4 * D, D, SPK, s)));
        const bool last = i + 1 == NL;
        EGO_HIP(gemm_res_ln(h, "mlp_down", HID, 4L * D, L.dn_w, L.dn_b, X, M, D, 4 * D, last ? p.lnf_g : p.layer[i + 1].ln1_g, last ? p.lnf_b : p.layer[i + 1].ln1_b, Y,
                            SPK, s));
        if (h->debug_stop == 2 + i) return EGOTAP_OK;
    }
    // H9-H10: per-heatmap regroup folded into fc1's A loader; fc blocks with folded BatchNorm + LeakyReLU
    auto bn = [](const LiftParams::Fc& f) { return EpiBnLrelu{f.b, f.g, f.beta, f.mean, f.var, 1e-5f, 0.2f}; };
    // fc1 of the two encoders has few rows (30 / 34 per frame) and a huge K (16384 ... 65536): below 100 tiles of 256 x 256 (UnrealEgo:
    // B < 107; EgoCap with 128 x 128 heatmaps: B < 95) most CUs would idle, so K is split over them (exact fp32 in every mode)
    // (the bf16 modes keep their own kernels down to 1024 rows: at 16x the MFMA rate a quarter-filled chip still beats fp32 split-K)
    const bool skinny_fc1 = BT < SKINNY_ROWS || (h->precision == EGOTAP_PREC_F32 && (long)((BT + 255) / 256) * (2048 / 256) < 100);
    {
        const int K1 = h->ppd * h->ppd * D;
        auto fc1 = [&](const auto& al) -> hipError_t {
            if (skinny_fc1 && BT <= 64)     // [r4] at most 64 rows: the 64-row tile (TileS)
                return gemm_f32_splitk_launch<TileS>(al, segmat1(p.pos_fc[0].w, 2048, K1), bn(p.pos_fc[0]), Z1, 2048, SPK, SPLITK_FLOATS, BT, 2048, K1, s, device_cu_count());
            if (skinny_fc1)                 // few row tiles: split K over the CUs
                return gemm_f32_splitk_launch<TileA>(al, segmat1(p.pos_fc[0].w, 2048, K1), bn(p.pos_fc[0]), Z1, 2048, SPK, SPLITK_FLOATS, BT, 2048, K1, s);
            return gemm_big(h, "pos_fc1", al, segmat1(p.pos_fc[0].w, 2048, K1), bn(p.pos_fc[0]), Z1, 2048, BT, 2048, K1, s);
        };
        // [r6] after the pruned last layer Y holds the compact tokens, row (b, i) = ppd^2 * D contiguous floats: the same values in the same k order
        if (prune) EGO_HIP(fc1(ALoadPlain{Y, (long)K1}));
        else EGO_HIP(fc1(ALoadTokens{Y, h->tokens()}));
        EGO_HIP((fc_gemm(h, "pos_fc2", ALoadPlain{Z1, 2048}, segmat1(p.pos_fc[1].w, 512, 2048), bn(p.pos_fc[1]), Z2, 512, BT, 512, 2048, SPK, s)));
        EGO_HIP((fc_gemm(h, "pos_fc3", ALoadPlain{Z2, 512}, segmat1(p.pos_fc[2].w, hid, 512), bn(p.pos_fc[2]), POSZ, hid, BT, hid, 512, SPK, s)));
    }
    // H11-H12: rotation (cos/sin) heatmaps straight from the input tensor
    {
        ALoadRot al{hm, h->rots()};
        if (skinny_fc1 && BT <= 64)
            EGO_HIP((gemm_f32_splitk_launch<TileS>(al, segmat1(p.rot_fc[0].w, 2048, 2L * HW), bn(p.rot_fc[0]), Z1, 2048, SPK, SPLITK_FLOATS, BT, 2048, 2 * HW, s, device_cu_count())));
        else if (skinny_fc1)
            EGO_HIP((gemm_f32_splitk_launch<TileA>(al, segmat1(p.rot_fc[0].w, 2048, 2L * HW), bn(p.rot_fc[0]), Z1, 2048, SPK, SPLITK_FLOATS, BT, 2048, 2 * HW, s)));
        else
            EGO_HIP((gemm_big(h, "rot_fc1", al, segmat1(p.rot_fc[0].w, 2048, 2L * HW), bn(p.rot_fc[0]), Z1, 2048, BT, 2048, 2 * HW, s)));
        EGO_HIP((fc_gemm(h, "rot_fc2", ALoadPlain{Z1, 2048}, segmat1(p.rot_fc[1].w, 512, 2048), bn(p.rot_fc[1]), Z2, 512, BT, 512, 2048, SPK, s)));
        EGO_HIP((fc_gemm(h, "rot_fc3", ALoadPlain{Z2, 512}, segmat1(p.rot_fc[2].w, hid, 512), bn(p.rot_fc[2]), ROTZ, hid, BT, hid, 512, SPK, s)));
    }
    }       // fp32 tensors in HBM
    // H13-H14: propagation units.  State-independent projections of all J steps as GEMMs (rows time-major t*B+b) ...
    // ([r4] through fc_gemm: below 1024 rows -- serving batches: J rows per frame -- a 128-row tiling has one row tile and 4-16 column tiles,
    // 24-41 us per launch at B = 1 for work the chip does in 2; K is split like the encoders' fc layers)
    const int x = 2 * hid, NF0 = H + x;
    ALoadStereo xs{POSZ, B, J, hid};
    EGO_HIP((fc_gemm(h, "pu0_x2f", xs, segmat1(p.x2f0_w, NF0, x), EpiBias{segvec1(p.x2f0_b, NF0)}, F0, NF0, JB, NF0, x, SPK, s)));
    EGO_HIP((fc_gemm(h, "pu0_x2h", xs, segmat1(p.x2h0_w, 4 * H, x), EpiBias{segvec1(p.x2h0_b, 4 * H)}, G0, 4L * H, JB, 4 * H, x, SPK, s)));
    {
        ALoadStereoGated bs{ALoadStereo{ROTZ, B, J, hid}, F0, NF0, H};
        EGO_HIP((fc_gemm(h, "pu0_b2h", bs, segmat1(p.b2h0_w, 4 * H, x), EpiBiasRes{segvec1(p.b2h0_b, 4 * H), G0, 4L * H}, G0, 4L * H, JB, 4 * H, x, SPK, s)));
    }
    // ... then the two J-step recurrences (layer 0 never reads layer-1 state, so the layers run one after the other)
    EGO_HIP(zero_fill(C0, (size_t)(w.ZERO - w.C0) + al256((size_t)B * H * 4), s));   // C0, C1, ZERO are contiguous (256-byte aligned slices)
    pu_chain_probe(h);
    unsigned* FAULT = (unsigned*)(base + w.FAULT);
    const PuChain ch0{F0, (long)B * NF0, NF0, G0, (long)B * 4 * H, nullptr, p.h2h0_w, p.h2h0_b, nullptr, 0, HS0, (long)B * H, HPA, (long)B * H, B, H, J,
                      FAULT, h->pu_fault_dev};
    if (!pu_chain_launch(s, h->pu_resident[0], h->pu_resident[1], ch0, B, h->pu_debug_drop))
    for (int t = 0; t < J; ++t) {       // the gated state of step t + 1 comes out of step t (ping-pong buffers; zeros at t = 0)
        const float* hp_in = t == 0 ? ZERO : ((t & 1) ? HPA : HPB);
        pu_step_launch(s, B, H, hp_in, G0 + (size_t)t * B * 4 * H, p.h2h0_w, p.h2h0_b, C0, C0, HS0 + (size_t)t * B * H,
                       t + 1 < J ? F0 + (size_t)(t + 1) * B * NF0 : nullptr, NF0, (t & 1) ? HPB : HPA, nullptr);
    }
    EGO_HIP(hipGetLastError());
    EGO_HIP((fc_gemm(h, "pu1_x2f", ALoadPlain{HS0, H}, segmat1(p.x2f1_w, H, H), EpiBias{segvec1(p.x2f1_b, H)}, F1, H, JB, H, H, SPK, s)));
    EGO_HIP((fc_gemm(h, "pu1_x2h", ALoadPlain{HS0, H}, segmat1(p.x2h1_w, 4 * H, H), EpiBias{segvec1(p.x2h1_b, 4 * H)}, G1, 4L * H, JB, 4 * H, H, SPK, s)));
    const PuChain ch1{F1, (long)B * H, H, G1, (long)B * 4 * H, nullptr, p.h2h1_w, p.h2h1_b, nullptr, 0, HS1, (long)B * H, HPA, (long)B * H, B, H, J,
                      FAULT, h->pu_fault_dev};
    if (!pu_chain_launch(s, h->pu_resident[0], h->pu_resident[1], ch1, B, h->pu_debug_drop))
    for (int t = 0; t < J; ++t) {
        const float* hp_in = t == 0 ? ZERO : ((t & 1) ? HPA : HPB);
        pu_step_launch(s, B, H, hp_in, G1 + (size_t)t * B * 4 * H, p.h2h1_w, p.h2h1_b, C1, C1, HS1 + (size_t)t * B * H,
                       t + 1 < J ? F1 + (size_t)(t + 1) * B * H : nullptr, H, (t & 1) ? HPB : HPA, nullptr);
    }
    EGO_HIP(hipGetLastError());
    // H15: per-joint pose head (+ global offset and head joint for UnrealEgo)
    hipLaunchKernelGGL(pose_head_kernel, dim3(B, h->J + 1), dim3(256), 0, s, POSZ, HS1, p.pose_w, p.pose_b, p.glob_w, p.glob_b, pose, B,
                       J, hid, H, h->cfg.estimate_head);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_lift_forward(egotap_handle h, const float* hm, int B, float* pose, void* ws, size_t ws_bytes, void* stream) {
    return lift_forward_impl(h, hm, B, pose, ws, ws_bytes, stream, false, "egotap_lift_forward");
}
extern "C" int egotap_lift_predict_pose(egotap_handle h, const float* hm, int B, float* pose, void* ws, size_t ws_bytes, void* stream) {
    return lift_forward_impl(h, hm, B, pose, ws, ws_bytes, stream, true, "egotap_lift_predict_pose");
}

extern "C" int egotap_lift_frozen_bytes(egotap_handle h, size_t* bytes) {
    EGO_CHECK(h && bytes, "egotap_lift_frozen_bytes: null argument");
    *bytes = lift_frozen_route(h) ? lift_frozen_plan(h, nullptr, nullptr).total : 0;
    return EGOTAP_OK;
}
extern "C" int egotap_lift_freeze(egotap_handle h, void* arena, size_t bytes, void* stream) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(h->precision == EGOTAP_PREC_BF16, "egotap_lift_freeze: nothing to freeze in this precision mode (only EGOTAP_PREC_BF16 prepares weights; "
              "the fp32 and bf16x3 modes read the live fp32 parameters)");
    EGO_CHECK(lift_frozen_route(h), "egotap_lift_freeze: nothing to freeze: the bf16-storage forward needs vit_dim 1024 and a sequence that is a multiple of 32 "
              "(this handle: vit_dim %d, %d tokens)", h->D, h->seq);
    EGO_CHECK(arena && ((uintptr_t)arena & 255) == 0, "egotap_lift_freeze: the arena must be a 256-byte aligned device pointer");
    int rc = lift_resolve(h);
    if (rc != EGOTAP_OK) return rc;
    PrepTable T;
    const LiftFrozen f = lift_frozen_plan(h, &h->lp, &T);
    EGO_CHECK(T.nseg <= PrepTable::MAXS, "egotap_lift_freeze: more segments than the table holds");
    if (bytes < f.total) {
        egotap_set_error("egotap_lift_freeze: arena too small: %zu bytes given, %zu needed", bytes, f.total);
        return EGOTAP_ERR_WORKSPACE;
    }
    h->lift_arena = nullptr;
    const int grid = T.chunks < 2048 ? T.chunks : 2048;      // 8 workgroups per CU; the rest of the chunks by stride
    hipLaunchKernelGGL(prep_weights_all_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, T, (char*)arena);
    EGO_HIP(hipGetLastError());
    h->lift_arena = (char*)arena;
    return EGOTAP_OK;
}
extern "C" int egotap_lift_unfreeze(egotap_handle h) {
    EGO_CHECK(h, "null handle");
    h->lift_arena = nullptr;
    return EGOTAP_OK;
}

// ------------------------------------------------------------------------------------------------ heatmap estimator
static int hm_resolve(Handle* h, int net) {
    if (h->hm_resolved[net]) return EGOTAP_OK;
    bool ok = true;
    HmParams& p = h->hp[net];
    const std::string bb = "backbone.backbone.backbone.";
    auto bn = [&](const std::string& k) {
        auto n = h->bound[net].find(k + ".num_batches_tracked");
        long long* nbt = (n != h->bound[net].end() && n->second.dtype == EGOTAP_I64 && n->second.numel == 1) ? (long long*)n->second.ptr : nullptr;
        return HmParams::Bn{P(h, net, k + ".weight", ok), P(h, net, k + ".bias", ok), P(h, net, k + ".running_mean", ok),
                            P(h, net, k + ".running_var", ok), nbt};
    };
    p.stem_w = P(h, net, bb + "conv1.weight", ok);
    p.stem_bn = bn(bb + "bn1");
    for (int i = 0; i < 4; ++i) p.nblk[i] = hm_nblk(h, i);
    for (int i = 0; i < 4; ++i)
        for (int b = 0; b < p.nblk[i]; ++b) {
            const std::string k = bb + "layer" + std::to_string(i + 1) + "." + std::to_string(b);
            auto& B = p.blk[i][b];
            B.w1 = P(h, net, k + ".conv1.weight", ok); B.bn1 = bn(k + ".bn1");
            B.w2 = P(h, net, k + ".conv2.weight", ok); B.bn2 = bn(k + ".bn2");
            B.wd = nullptr;
            if (b == 0 && i > 0) { B.wd = P(h, net, k + ".downsample.0.weight", ok); B.bnd = bn(k + ".downsample.1"); }
        }
    const std::string a = "after_backbone.";
    for (int k = 0; k < 4; ++k) {
        const std::string n = a + "layer" + std::to_string(k + 1) + "_1x1.0";
        p.l1x1[k] = {P(h, net, n + ".weight", ok), P(h, net, n + ".bias", ok)};
    }
    for (int k = 0; k < 3; ++k) {
        const std::string n = a + "conv_up" + std::to_string(k + 1) + ".0";
        p.up[k] = {P(h, net, n + ".weight", ok), P(h, net, n + ".bias", ok)};
    }
    p.head = {P(h, net, a + "conv_heatmap.weight", ok), P(h, net, a + "conv_heatmap.bias", ok)};
    if (!ok) return EGOTAP_ERR_UNBOUND;
    h->hm_resolved[net] = true;
    return EGOTAP_OK;
}

// [r7] Where an estimator's frames come from: the normalised planar fp32 frames (left / right), or the camera's bytes (left8 / right8: uint8
// [B, S0, S0, 3], with the fp32 [3][256] value table).  Sides 64 / 128: both stems stage the bytes themselves.  Every other side: the frames are
// converted into `scratch` (2 x B x 3 x S0^2 floats, the caller's workspace slice) first and the forward proceeds on them as ever.
// [r8] the sensor's own frames behind a byte source (the sensor and lens entries only): frames of the layout `src` (packed RGB8, NV12 or YUYV,
// src.frame_stride bytes each), a source rectangle and a mirror flag per eye; each piece is converted and resized into `slice` (chunk x 2 x 3 S0^2
// bytes of the caller's workspace) and read there as camera bytes
// with maps (egotap_predict_pose_lens only): the frames are another lens's; the piece is gathered into the same slice through the two lens maps, an
// eye's fill where a map has no source -- rect and mirror say where the keypoints come out and are not read by the gather
// with map_streams > 0 (egotap_predict_pose_lens_streams only): each map pointer is a table of that many maps and frame b of the batch reads map b % map_streams
struct HmSensor {
    const unsigned char *left8, *right8;
    FrameSource src;
    int rect[2][4], mirror[2];
    const int *map_left, *map_right;
    unsigned fill[2];
    unsigned char* slice;
    int map_streams;
};
struct HmSrc {
    const float *left, *right;
    const unsigned char *left8, *right8;
    const float* table;
    float* scratch;
    const HmSensor* sensor = nullptr;      // [r8] set by the sensor entry alone
    bool bytes() const { return left8 != nullptr; }
    HmSrc at(long frame, long rgb) const {      // the source of the frames from `frame` on (rgb = 3 S0^2 elements per frame)
        HmSrc r = *this;
        if (left) { r.left = left + frame * rgb; r.right = right + frame * rgb; }
        if (left8) { r.left8 = left8 + frame * rgb; r.right8 = right8 + frame * rgb; }
        return r;
    }
};
static inline HmSrc hm_src_f32(const float* left, const float* right) { return HmSrc{left, right, nullptr, nullptr, nullptr, nullptr}; }
// the converter slice of a byte-source forward of B frames: nothing where the stems read the bytes themselves
static inline bool hm_stem_reads_bytes(int hm_size) { return hm_size == 64 || hm_size == 128; }
static inline size_t hm_u8_slice_bytes(const Handle* h, int B) {
    const size_t S0 = (size_t)h->cfg.hm_size * 4;
    return hm_stem_reads_bytes(h->cfg.hm_size) ? 0 : (size_t)B * 2 * 3 * S0 * S0 * 4;
}

struct HmWs {
    size_t L0, P0, S[4][4] /* per stage: Ta, Tb, Td, L */, U4, CAT3, X3, CAT2, X2, CAT1, X1, WPACK, WALL, total;
};
// [r3] every convolution's packed bf16 weights (+ padded bias) and every BatchNorm's folded scale / shift of one estimator, in the order
// the bf16 forward uses them; p == nullptr: sizes only.  Returns the bytes of the region; fills T (segment table of pack_all_bf16s_kernel).
// conv_heatmap's GEMM N: 30 / 34 / 60 / 68 heatmap channels padded to the 64- or 128-column tile (256 before: 4-8 x the MFMAs)
static inline int hm_head_np(int n_out) { return n_out <= 64 ? 64 : n_out <= 128 ? 128 : 256; }
// split count of a decoder convolution at serving batches: gemm_bf16s_ksplit's, capped at 8 so that every small batch lands on the SAME count
// (a frame's heatmaps then do not depend on the batch it arrives in, bit for bit -- the cap, not the batch, decides below ~8 frames)
static inline int hm_dec_ksplit(int M, int N, int K, int cus, size_t floats) {
    int sp = gemm_bf16s_ksplit(M, N, K, cus, floats);
    if (sp > 8) { sp = 8; while (sp > 1 && K % (sp * 32) != 0) --sp; }
    return sp;
}
static constexpr int HM_CAT3P = 1600;      // channels per pixel of the first decoder concat in the bf16 mode: 1024 + 516 = 1540, padded to a multiple of 64
// n2 / sides / cus / split_floats (forward only; the size query leaves them 0): image count, map side per stage and the split-K budget, from
// which the plan decides per BasicBlock 3x3 convolution whether it runs on the 64-deep GEMM (64-channel weight slabs) -- Cin a multiple of 64, Cout = 128
// (layer2, on the 256 x 128 tile) or a multiple of 256 (layer3 / layer4), and enough pixels that the 32-deep kernel's split-K path is not taken.  Same bytes either way.
static size_t hm_pack_plan(const HmParams* p, const int* nblk, PackTable* T, long n2 = 0, const int* sides = nullptr, int cus = 0, size_t split_floats = 0,
                           size_t dec_split_floats = 0, long n2_dec = -1) {
    if (n2_dec < 0) n2_dec = n2;            // [r5] the batch-statistics forward runs the backbone over the whole batch and the decoder in chunks
    size_t o = 0;
    int nw = 0, nb = 0, blk = 0;
    auto al = [&](size_t n) { size_t r = o; o = (o + n + 255) & ~(size_t)255; return r; };
    bool in_range = true;            // the table narrows offsets to 32 bits and channel counts to 16: checked here, once
    auto wseg = [&](const float* w, const float* b, int Cout, int Cin, int Cp, int Np, int taps, int slab = 32) {
        PackSeg sg{};
        sg.w = w; sg.b = b; sg.Cout = Cout; sg.Cin = Cin; sg.Cp = Cp; sg.Np = Np; sg.taps = (short)taps; sg.slab = (short)slab;
        const size_t ow = al((size_t)Np * taps * Cp * 2), ob = al((size_t)Np * 4);
        in_range = in_range && o < ((size_t)1 << 32) && Cout < 65536 && Cin < 65536 && Cp < 65536 && Np < 65536 && Cp % slab == 0;
        sg.dst_w = (unsigned)ow;
        sg.dst_b = (unsigned)ob;
        sg.first_block = blk;
        const long items = taps == 9 ? (long)Np * (Cp / 8) : (long)Np * (Cin / 8);       // 3x3: one thread per (co, 8 input channels), all taps
        blk += (int)((items + 255) / 256);
        if (T && nw < PackTable::MAXW) T->w[nw] = sg;
        ++nw;
    };
    struct Pending { HmParams::Bn bn; int C, Np; } pend[PackTable::MAXB];
    auto bseg = [&](const HmParams::Bn& bn, int C, int Np) { if (nb < PackTable::MAXB) pend[nb] = Pending{bn, C, Np}; ++nb; };
    static const HmParams::Bn nobn{nullptr, nullptr, nullptr, nullptr, nullptr};
    auto npad = [](int c) { return c <= 64 ? 64 : c <= 128 ? 128 : (c + 255) / 256 * 256; };
    int cin = 64;
    for (int i = 0; i < 4; ++i) {
        const int c = HM_CH[i];
        for (int bk = 0; bk < nblk[i]; ++bk) {
            const int bc = bk == 0 ? cin : c;
            const bool down = p ? p->blk[i][bk].wd != nullptr : (bk == 0 && i > 0);
            auto deep = [&](int K) { return sides && n2 > 0 && g_gemm_bf16s_bk != 32 && (c % 256 == 0 || c == 128) && gemm_bf16s_ksplit((int)(n2 * sides[i] * sides[i]), c, K, cus, split_floats) == 1; };
            // (conv1 of a stage's first block is the stride-2 one with Cin = Cout / 2: a multiple of 64 from layer2 on, 9 Cin >= 128)
            wseg(p ? p->blk[i][bk].w1 : nullptr, nullptr, c, bc, bc, npad(c), 9, bc % 64 == 0 && deep(9 * bc) ? 64 : 32); bseg(p ? p->blk[i][bk].bn1 : nobn, c, npad(c));
            if (down) { wseg(p ? p->blk[i][bk].wd : nullptr, nullptr, c, bc, bc, npad(c), 1); bseg(p ? p->blk[i][bk].bnd : nobn, c, npad(c)); }
            wseg(p ? p->blk[i][bk].w2 : nullptr, nullptr, c, c, c, npad(c), 9, deep(9 * c) ? 64 : 32); bseg(p ? p->blk[i][bk].bn2 : nobn, c, npad(c));
        }
        cin = c;
    }
    auto cv = [&](int which, int k) -> HmParams::Cv { return p ? (which == 0 ? p->l1x1[k] : which == 1 ? p->up[k] : p->head) : HmParams::Cv{nullptr, nullptr}; };
    wseg(cv(0, 3).w, cv(0, 3).b, 1024, 1024, 1024, 1024, 1);
    wseg(cv(0, 2).w, cv(0, 2).b, 516, 512, 512, 768, 1);
    // the three 3x3 decoder convolutions run on the 64-deep GEMM (gemm_bf16s64.h, X64Conv3): concat widths padded to a multiple of 64
    // (1540 -> HM_CAT3P = 1600), weights packed in 64-channel slabs
    // [r4] ... unless the map has so few pixels (serving batches: conv_up3 at B = 1 is one row tile x four column tiles walking K = 14400) that the
    // product is split over K: that path is the 32-deep kernel's (XConv3, 32-channel slabs), partial sums in the free head of the WPACK region
    auto dec_slab = [&](int k, int Cout, int Cp) {      // k: 2 = conv_up3 (side s16), 1 = conv_up2 (s32), 0 = conv_up1 (s64); sides[] = {s64, s32, s16, s8}
        if (!sides || n2_dec <= 0) return 64;
        if (g_gemm_bf16s_bk == 32) return 32;
        return hm_dec_ksplit((int)(n2_dec / 2 * sides[k] * sides[k]), Cout, 9 * Cp, cus, dec_split_floats) > 1 ? 32 : 64;
    };
    wseg(cv(1, 2).w, nullptr, 1024, 1540, HM_CAT3P, 1024, 9, dec_slab(2, 1024, HM_CAT3P));
    wseg(cv(0, 1).w, cv(0, 1).b, 256, 256, 256, 256, 1);
    wseg(cv(1, 1).w, nullptr, 512, 1280, 1280, 512, 9, dec_slab(1, 512, 1280));
    wseg(cv(0, 0).w, cv(0, 0).b, 128, 128, 128, 256, 1);
    wseg(cv(1, 0).w, nullptr, 512, 640, 640, 512, 9, dec_slab(0, 512, 640));
    wseg(cv(2, 0).w, cv(2, 0).b, p ? p->n_out : 30, 512, 512, p ? hm_head_np(p->n_out) : 256, 1);      // (sizes-only: the largest padding)
    const int blocks_w = blk;
    for (int k = 0; k < nb && k < PackTable::MAXB; ++k) {
        BnSeg bs{};
        bs.g = pend[k].bn.g; bs.b = pend[k].bn.b; bs.m = pend[k].bn.m; bs.v = pend[k].bn.v;
        bs.C = pend[k].C; bs.Np = pend[k].Np;
        bs.dst_sc = al((size_t)bs.Np * 4);
        bs.dst_sh = al((size_t)bs.Np * 4);
        bs.first_block = blk;
        blk += (bs.Np + 255) / 256;
        if (T) T->bn[k] = bs;
    }
    if (T) { T->nw = nw; T->nb = nb; T->blocks_w = blocks_w; T->blocks = blk; }
    return (nw <= PackTable::MAXW && nb <= PackTable::MAXB && in_range && o < ((size_t)1 << 32)) ? o : 0;
}
static HmWs hm_ws(const Handle* h, int B) {
    HmWs w;
    const size_t N2 = 2 * (size_t)B, S0 = (size_t)h->cfg.hm_size * 4;   // RGB side
    size_t o = 0;
    auto take = [&](size_t floats) { size_t r = o; o = al256(o + floats * 4); return r; };
    w.L0 = take(N2 * 64 * (S0 / 2) * (S0 / 2));
    w.P0 = take(N2 * 64 * (S0 / 4) * (S0 / 4));
    for (int i = 0; i < 4; ++i) {
        const size_t side = S0 / (4u << i), fl = N2 * HM_CH[i] * side * side;
        for (int k = 0; k < 4; ++k) w.S[i][k] = take(fl);
    }
    const size_t s8 = S0 / 32, s16 = S0 / 16, s32 = S0 / 8, s64 = S0 / 4;
    w.U4 = take((size_t)B * 1024 * s8 * s8);
    w.CAT3 = take((size_t)B * 1540 * s16 * s16); w.X3 = take((size_t)B * 1024 * s16 * s16);
    w.CAT2 = take((size_t)B * 1280 * s32 * s32); w.X2 = take((size_t)B * 512 * s32 * s32);
    w.CAT1 = take((size_t)B * 640 * s64 * s64);  w.X1 = take((size_t)B * 512 * s64 * s64);
    w.WPACK = take(conv_bf16_pack_bytes(1024, 1540) / 4);      // largest conv (conv_up3) repacked for the bf16 kernels
    const int nblk_[4] = {hm_nblk(h, 0), hm_nblk(h, 1), hm_nblk(h, 2), hm_nblk(h, 3)};
    w.WALL = take(hm_pack_plan(nullptr, nblk_, nullptr) / 4 + 64);    // [r3] bf16 mode: every layer's packed weights at once (one pack launch per forward)
    w.total = o;
    return w;
}

// ---- [r5] the bf16 channels-last forward as two pieces -- backbone (stem + four stages) and decoder -- so that the batch-statistics forward of the FROZEN
// estimators (egotap_hm_forward_bnbatch: train.py:91) can run the backbone over the whole batch (its BatchNorm couples the frames of a batch) and the
// decoder, which has no BatchNorm, in chunks.  The eval-mode egotap_hm_forward calls both with one set of buffers: same launches, same bits as before.
struct HmBf16Bufs {
    __bf16 *P0, *A[4], *Ta[4], *Tb[4], *Td[4];      // backbone: pooled stem, per stage the level (= pyramid level = decoder operand) and three temporaries
    __bf16 *T4, *C3, *Y3, *C2, *Y2, *C1, *Y1;        // decoder
    __bf16* ZP;                                     // 256 bytes of zeros
    char* reg;                                      // packed weights / folded BatchNorms (pack_all_bf16s_kernel)
    float* split_slab; size_t split_floats;         // split-K partials of the backbone's few-pixel layers
    float* dec_slab; size_t dec_split_floats;       // ... of the decoder's 3x3 convolutions at serving batches
    const float *ones, *zeros;                      // batch-statistics mode: unit scale / zero shift (1024 floats each) for the raw-output epilogue
};
struct HmBnBatch {                                  // batch-statistics mode: the scratch every BatchNorm of the forward reuses (stream-ordered)
    BnBatchScratch scr;
};
static inline int hm_ilog2(long v) { int l = 0; while ((1L << l) < v) ++l; return l; }
// [r5] the zero page of a convolution operand addressed from a scalar origin (gemm_bf16s64.h, X64ConvES / X64Conv3S) has to lie within 4 GB of the map:
// 256 bytes of zeros right behind every map a 3x3 convolution reads (in the eval-mode workspace the unused upper half of the map's fp32 slot; in the
// batch-statistics workspace 256 bytes taken with the map), written by one launch at the head of the backbone / of each decoder pass.
static inline __bf16* hm_zero_tail(const __bf16* map, size_t bytes) { return (__bf16*)((char*)map + ((bytes + 255) & ~(size_t)255)); }
struct ZeroPages { void* p[24]; };
static __global__ __launch_bounds__(64) void zero_pages_kernel(ZeroPages z) { ((float*)z.p[blockIdx.x])[threadIdx.x] = 0.f; }
static hipError_t hm_bf16_backbone(Handle* h, const HmParams& p, const PackTable& PT, int& li, int& bi, const HmBf16Bufs& q, const float* left, const float* right, int B,
                                   int S0, const HmBnBatch* bnb, hipStream_t s, const HmSrc* bytes = nullptr) {
    const int N2 = 2 * B, cus = device_cu_count();
    const int s64 = S0 / 4, s32 = S0 / 8, s16 = S0 / 16, s8 = S0 / 32;
    char* reg = q.reg;
    __bf16* ZP = q.ZP;
    {
        ZeroPages z{};
        int n = 0;
        z.p[n++] = hm_zero_tail(q.P0, (size_t)B * s64 * s64 * 128 * 2);
        for (int i = 0; i < 4; ++i) {
            const size_t side = (size_t)S0 / (4u << i), bytes = (size_t)B * side * side * 2 * HM_CH[i] * 2;
            for (__bf16* m : {q.A[i], q.Ta[i], q.Tb[i], q.Td[i]}) z.p[n++] = hm_zero_tail(m, bytes);
        }
        hipLaunchKernelGGL(zero_pages_kernel, dim3(n), dim3(64), 0, s, z);
    }
    // E1 + E2: stem conv7x7/2 + BN + ReLU + max-pool in one kernel (stem_bf16s.h): bf16 [B * s64^2, 2 x 64], image n = 2b + eye in the eye's column half
    if (!bnb && bytes) {          // [r7] the camera's bytes: the same kernel body behind a byte-source staging (stem_bf16s.h, stem_bf16s_body.inc)
        GemmTimer t(h, s, "hm.stem_u8", "stem_pool_bf16s_u8_kernel", 2.0 * N2 * 64 * 147 * (double)(S0 / 2) * (S0 / 2));
        hipError_t e = stem_pool_bf16s_u8_launch(bytes->left8, bytes->right8, bytes->table, p.stem_w, p.stem_bn.g, p.stem_bn.b, p.stem_bn.m, p.stem_bn.v, q.P0, S0, N2, cus, s);
        if (e != hipSuccess) return e;
    } else if (!bnb) {
        hipError_t e = stem_pool_bf16s_launch(left, right, p.stem_w, p.stem_bn.g, p.stem_bn.b, p.stem_bn.m, p.stem_bn.v, q.P0, S0, N2, cus, s);
        if (e != hipSuccess) return e;
    } else {
        // batch statistics: the convolution twice -- a statistics-only pass (the 128 x 128 x 64 map still never reaches HBM), then the fused pass with per-eye tables
        int grid = 0;
        hipError_t e = stem_pool_bf16s_launch_mode<1>(left, right, p.stem_w, nullptr, nullptr, nullptr, nullptr, (__bf16*)bnb->scr.part, S0, N2, cus, s, &grid);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(bn_finish_bf16s_kernel, dim3(64), dim3(128), 0, s, (const float*)bnb->scr.part, grid, 64, (double)B * (S0 / 2) * (S0 / 2), p.stem_bn.g, p.stem_bn.b,
                           (float*)p.stem_bn.m, (float*)p.stem_bn.v, p.stem_bn.nbt, bnb->scr.sc, bnb->scr.sh);
        e = stem_pool_bf16s_launch_mode<2>(left, right, p.stem_w, bnb->scr.sc, bnb->scr.sh, nullptr, nullptr, q.P0, S0, N2, cus, s);
        if (e != hipSuccess) return e;
    }
    // E3: the four stages on the same GEMM kernel (eye-interleaved rows, see conv_bf16s.h)
    auto bconv = [&](const char* role, const __bf16* in, int cin, int c, int taps, int stride, int side, const float* wgt,
                     const HmParams::Bn& bn, const __bf16* res_, int relu_, __bf16* o) -> hipError_t {
        // [r3] Cout = 64 / 128 run on the 64- / 128-column tile (256 x 64 NI, gemm_bf16s.h) instead of N = 256 with a column guard
        const int Np = c <= 64 ? 64 : c <= 128 ? 128 : (c + 255) / 256 * 256;
        const PackSeg& sg = PT.w[li++];
        const BnSeg& bs = PT.bn[bi++];
        if (sg.w != wgt || sg.Np != Np || sg.taps != taps || bs.g != bn.g) return hipErrorInvalidValue;
        const __bf16* WPl = (const __bf16*)(reg + sg.dst_w);
        // batch statistics: the convolution stores its raw bf16 output (unit scale, zero shift, no residual, no ReLU); bn_batch below does the rest in place
        const float *SC = bnb ? q.ones : (const float*)(reg + bs.dst_sc), *SH = bnb ? q.zeros : (const float*)(reg + bs.dst_sh);
        const __bf16* res = bnb ? nullptr : res_;
        const int relu = bnb ? 0 : relu_;
        const long M = (long)N2 * side * side;
        auto run = [&]() -> hipError_t {
            const bool direct = taps == 9 && stride == 1 && cin == 64 && c == 64;      // [r3] layer1: the direct kernel (conv64_bf16s.h)
            GemmTimer t(h, s, role, direct ? "conv64_direct_bf16s_kernel" : taps == 9 ? "gemm_bf16s_kernel<XConvE,3x3>" : "gemm_bf16s_kernel<XConvE,1x1>",
                        2.0 * M * c * taps * (double)cin);
            if (direct)
                return conv64_direct_bf16s_launch(in, ZP, WPl, SC, SH, res, o, hm_ilog2(side), N2, relu, cus, s);
            const SEpiBnBf16<false> ep{SC, SH, res, o, c, hm_ilog2(side), relu};
            if (sg.slab == 64) {      // [r4] layer3 / layer4's stride-1 convolutions on the 64-deep GEMM (the plan checked the shape rules)
                if (taps != 9 || cin % 64 != 0 || Np != c) return hipErrorInvalidValue;
                const long si = (long)side * stride;
                const __bf16* org;
                unsigned in_off, zero_off;
                const size_t in_bytes = (size_t)(N2 / 2) * si * si * 2 * cin * 2;
                if (s64_conv_origin(in, in_bytes, (size_t)(si + 1) * 2 * cin * 2, hm_zero_tail(in, in_bytes), org, in_off, zero_off)) {   // [r5] scalar origin + lane offsets
                    const X64ConvES xs{org, in_off, zero_off, cin, hm_ilog2(side), stride};
                    if (c == 128) return gemm_bf16s64_launch_x<X64ConvES, SEpiBnBf16<false>, 1>(xs, WPl, 9L * cin, ep, (int)M, Np, 9 * cin, cus, s);
                    return gemm_bf16s64_launch_x(xs, WPl, 9L * cin, ep, (int)M, Np, 9 * cin, cus, s);
                }
                const X64ConvE xl{in, ZP, cin, hm_ilog2(side), stride};
                if (c == 128) return gemm_bf16s64_launch_x<X64ConvE, SEpiBnBf16<false>, 1>(xl, WPl, 9L * cin, ep, (int)M, Np, 9 * cin, cus, s);   // layer2: 256 x 128 tile
                return gemm_bf16s64_launch_x(xl, WPl, 9L * cin, ep, (int)M, Np, 9 * cin, cus, s);
            }
            const XConvE xl{in, ZP, cin, hm_ilog2(side), stride, taps};
            if (Np == 64 && c == 64) return gemm_bf16s_launch<XConvE, SEpiBnBf16<false>, 1>(xl, WPl, (long)taps * cin, ep, (int)M, Np, taps * cin, cus, s);
            if (Np == 128 && c == 128) return gemm_bf16s_launch<XConvE, SEpiBnBf16<false>, 2>(xl, WPl, (long)taps * cin, ep, (int)M, Np, taps * cin, cus, s);
            if (Np == c) {
                // [r3] few pixels (layer3 / layer4 at small batches: 512 x 512 RGB at B = 32 leaves layer4 128 tiles for 256 CUs): split K,
                // partial sums in the (by now free) slot of the stem's map, BatchNorm / residual / ReLU in the fixed-order reduce
                const int sp = gemm_bf16s_ksplit((int)M, Np, taps * cin, cus, q.split_floats);
                if (sp > 1) return gemm_bf16s_splitk_launch(xl, WPl, (long)taps * cin, ep, q.split_slab, sp, (int)M, Np, taps * cin, cus, s);
                return gemm_bf16s_launch(xl, WPl, (long)taps * cin, ep, (int)M, Np, taps * cin, cus, s);
            }
            return gemm_bf16s_launch(xl, WPl, (long)taps * cin, SEpiBnBf16<true>{SC, SH, res, o, c, hm_ilog2(side), relu}, (int)M, Np, taps * cin, cus, s);
        };
        hipError_t e = run();
        if (e != hipSuccess || !bnb) return e;
        return bn_batch_bf16s_launch(o, res_, (long)B * side * side, c, bn.g, bn.b, (float*)bn.m, (float*)bn.v, bn.nbt, relu_, bnb->scr, s);
    };
    const int sides[4] = {s64, s32, s16, s8};
    const __bf16* x = q.P0;
    int cin = 64;
    for (int i = 0; i < 4; ++i) {
        const int c = HM_CH[i], side = sides[i], nb = p.nblk[i];
        __bf16 *Ta = q.Ta[i], *Tb = q.Tb[i], *Td = q.Td[i];                       // q.A[i] is the level itself
        const __bf16* xin = x;
        for (int bk = 0; bk < nb; ++bk) {
            const auto& K = p.blk[i][bk];
            const int stride = (bk == 0 && i > 0) ? 2 : 1, bc = bk == 0 ? cin : c;
            // block outputs alternate between Tb and the level so that the last block writes the level (a block never writes
            // the buffer it reads its identity from)
            __bf16* y = ((nb - 1 - bk) & 1) ? Tb : q.A[i];
            hipError_t e = bconv(HM_R1[i][bk], xin, bc, c, 9, stride, side, K.w1, K.bn1, nullptr, 1, Ta);
            if (e != hipSuccess) return e;
            const __bf16* idt = xin;
            if (K.wd) {
                e = bconv(HM_RD[i], xin, bc, c, 1, 2, side, K.wd, K.bnd, nullptr, 0, Td);
                if (e != hipSuccess) return e;
                idt = Td;
            }
            e = bconv(HM_R2[i][bk], Ta, c, c, 9, 1, side, K.w2, K.bn2, idt, 1, y);
            if (e != hipSuccess) return e;
            xin = y;
        }
        x = q.A[i];
        cin = c;
    }
    return hipSuccess;
}

// E4-E9 on Bc frames whose pyramid levels start at lv[0..3] (layer1 .. layer4 outputs, bf16 [Bc * s^2, 2 C]); li = first decoder entry of the pack table
// out_b != nullptr: conv_heatmap writes bf16 there instead (SEpiHeatBf16: the lifting head's bf16 operand, same image stride in elements) and `out` is not touched
static hipError_t hm_bf16_decoder(Handle* h, const HmParams& p, const PackTable& PT, int li, const HmBf16Bufs& q, const __bf16* const* lv, int B, int S0, float* out,
                                  int64_t out_image_stride, hipStream_t s, __bf16* out_b = nullptr) {
    const int cus = device_cu_count();
    const int s64 = S0 / 4, s32 = S0 / 8, s16 = S0 / 16, s8 = S0 / 32;
    const long p8 = (long)s8 * s8, p16 = (long)s16 * s16, p32 = (long)s32 * s32, p64 = (long)s64 * s64;
    char* reg = q.reg;
    __bf16* ZP = q.ZP;
    __bf16 *T4 = q.T4, *C3 = q.C3, *Y3 = q.Y3, *C2 = q.C2, *Y2 = q.Y2, *C1 = q.C1, *Y1 = q.Y1;
    auto up2 = [&](const __bf16* in, __bf16* o, int C, int hin, long ld) {
        const long total = (long)B * 4 * hin * hin * (C / 8);
        hipLaunchKernelGGL(upsample2x_nhwc_bf16s_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, in, o, C, hin, ld, total);
        return hipGetLastError();
    };
    // 1x1 convrelu: rows = pixels; the output goes to columns [0, Cout) of o (row stride ld)
    auto conv1 = [&](const char* role, const __bf16* in, long M, const HmParams::Cv& cv, int Cin, int Cout, __bf16* o, long ld) {
        const int Np = (Cout + 255) / 256 * 256;
        const PackSeg& sg = PT.w[li++];
        if (sg.w != cv.w || sg.Np != Np || sg.Cin != Cin) return hipErrorInvalidValue;      // the plan and the forward walk the layers in one order
        const __bf16* WPl = (const __bf16*)(reg + sg.dst_w);
        const float* BPl = (const float*)(reg + sg.dst_b);
        GemmTimer t(h, s, role, "gemm_bf16s_kernel<XPlain,conv1x1>", 2.0 * M * Cout * Cin);
        if (Np == Cout) return gemm_bf16s_launch(XPlain{in, Cin}, WPl, (long)Cin, SEpiConvBf16<false>{BPl, o, ld, Np, 1}, (int)M, Np, Cin, cus, s);
        return gemm_bf16s_launch(XPlain{in, Cin}, WPl, (long)Cin, SEpiConvBf16<true>{BPl, o, ld, (Cout + 7) / 8 * 8, 1}, (int)M, Np, Cin, cus, s);
    };
    // 3x3 convrelu on a concat buffer of Cp channels per pixel (Cp a multiple of 32; channels past Cin are zero)
    auto conv3 = [&](const char* role, const __bf16* in, long M, int side, const HmParams::Cv& cv, int Cin, int Cp, int Cout, __bf16* o) {
        const PackSeg& sg = PT.w[li++];
        if (sg.w != cv.w || sg.Cp != Cp || sg.Np != Cout) return hipErrorInvalidValue;
        if (sg.slab == 32) {      // [r4] few pixels: the 32-deep kernel, split over K when the plan's rule says so (serving batches)
            if (Cp % 32 != 0 || Cout % 256 != 0) return hipErrorInvalidValue;
            GemmTimer t(h, s, role, "gemm_bf16s_kernel<XConv3>", 2.0 * M * Cout * 9.0 * Cin);
            const XConv3 xl{in, ZP, Cp, hm_ilog2(side)};
            const SEpiConvBf16<false> ep{cv.b, o, (long)Cout, Cout, 1};
            const int sp = hm_dec_ksplit((int)M, Cout, 9 * Cp, cus, q.dec_split_floats);
            if (sp > 1) return gemm_bf16s_splitk_launch(xl, (const __bf16*)(reg + sg.dst_w), 9L * Cp, ep, q.dec_slab, sp, (int)M, Cout, 9 * Cp, cus, s);
            return gemm_bf16s_launch(xl, (const __bf16*)(reg + sg.dst_w), 9L * Cp, ep, (int)M, Cout, 9 * Cp, cus, s);
        }
        if (sg.slab != 64 || Cp % 64 != 0 || Cout % 256 != 0) return hipErrorInvalidValue;
        GemmTimer t(h, s, role, "gemm_bf16s64_kernel<X64Conv3>", 2.0 * M * Cout * 9.0 * Cin);
        const SEpiConvBf16<false> ep{cv.b, o, (long)Cout, Cout, 1};
        const __bf16* org;
        unsigned in_off, zero_off;
        if (s64_conv_origin(in, (size_t)M * Cp * 2, (size_t)(side + 1) * Cp * 2, hm_zero_tail(in, (size_t)M * Cp * 2), org, in_off, zero_off))      // [r5] scalar origin + lane offsets
            return gemm_bf16s64_launch_x(X64Conv3S{org, in_off, zero_off, Cp, hm_ilog2(side)}, (const __bf16*)(reg + sg.dst_w), 9L * Cp, ep, (int)M, Cout, 9 * Cp, cus, s);
        const X64Conv3 xl{in, ZP, Cp, hm_ilog2(side)};
        return gemm_bf16s64_launch_x(xl, (const __bf16*)(reg + sg.dst_w), 9L * Cp, ep, (int)M, Cout, 9 * Cp, cus, s);
    };
    const __bf16 *A1 = lv[0], *A2 = lv[1], *A3 = lv[2], *A4 = lv[3];
#define HMD(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return e_; } while (0)
    {
        ZeroPages z{};
        z.p[0] = hm_zero_tail(C3, (size_t)B * p16 * HM_CAT3P * 2);
        z.p[1] = hm_zero_tail(C2, (size_t)B * p32 * 1280 * 2);
        z.p[2] = hm_zero_tail(C1, (size_t)B * p64 * 640 * 2);
        hipLaunchKernelGGL(zero_pages_kernel, dim3(3), dim3(64), 0, s, z);
    }
    HMD(zero_fill(C3, (size_t)B * p16 * HM_CAT3P * 2, s));                    // channels 1544..1599 of the first concat are padding
    HMD(conv1("hm.layer4_1x1", A4, B * p8, p.l1x1[3], 1024, 1024, T4, 1024));
    HMD(up2(T4, C3, 1024, s8, HM_CAT3P));
    HMD(conv1("hm.layer3_1x1", A3, B * p16, p.l1x1[2], 512, 516, C3 + 1024, HM_CAT3P));
    HMD(conv3("hm.conv_up3", C3, B * p16, s16, p.up[2], 1540, HM_CAT3P, 1024, Y3));
    HMD(up2(Y3, C2, 1024, s16, 1280));
    HMD(conv1("hm.layer2_1x1", A2, B * p32, p.l1x1[1], 256, 256, C2 + 1024, 1280));
    HMD(conv3("hm.conv_up2", C2, B * p32, s32, p.up[1], 1280, 1280, 512, Y2));
    HMD(up2(Y2, C1, 512, s32, 640));
    HMD(conv1("hm.layer1_1x1", A1, B * p64, p.l1x1[0], 128, 128, C1 + 512, 640));
    HMD(conv3("hm.conv_up1", C1, B * p64, s64, p.up[0], 640, 640, 512, Y1));
    {   // conv_heatmap: fp32 NCHW into the caller's channel slice
        const PackSeg& sg = PT.w[li++];
        if (sg.w != p.head.w || li != PT.nw) return hipErrorInvalidValue;      // the pack plan is out of step with the forward
        GemmTimer t(h, s, "hm.conv_heatmap", "gemm_bf16s_kernel<XPlain,heatmap>", 2.0 * B * p64 * p.n_out * 512);
        const float* hb = (const float*)(reg + sg.dst_b);
        const __bf16* hw = (const __bf16*)(reg + sg.dst_w);
        const int hn = hm_head_np(p.n_out);
        auto head = [&](const auto& he) -> hipError_t {      // the same product, tile and k order under either epilogue
            using E = std::decay_t<decltype(he)>;
            if (hn == 64) return gemm_bf16s_launch<XPlain, E, 1>(XPlain{Y1, 512}, hw, 512L, he, (int)(B * p64), 64, 512, cus, s);
            if (hn == 128) return gemm_bf16s_launch<XPlain, E, 2>(XPlain{Y1, 512}, hw, 512L, he, (int)(B * p64), 128, 512, cus, s);
            return gemm_bf16s_launch(XPlain{Y1, 512}, hw, 512L, he, (int)(B * p64), 256, 512, cus, s);
        };
        if (out_b) HMD(head(SEpiHeatBf16{hb, out_b, (long)out_image_stride, p.n_out, hm_ilog2(p64)}));
        else
        HMD(head(SEpiHeatNCHW{hb, out, (long)out_image_stride, p.n_out, hm_ilog2(p64)}));
    }
#undef HMD
    return hipSuccess;
}

extern "C" int egotap_hm_workspace_bytes(egotap_handle h, int B, size_t* bytes) {
    EGO_CHECK(h && bytes, "null argument");
    EGO_CHECK(B >= 0, "negative batch");
    *bytes = hm_ws(h, B > 0 ? B : 1).total;
    return EGOTAP_OK;
}

extern "C" int egotap_hm_intermediate(egotap_handle h, int B, const char* name, size_t* offset, int64_t* numel) {
    EGO_CHECK(h && name && offset && numel, "null argument");
    const HmWs w = hm_ws(h, B > 0 ? B : 1);
    const int64_t N2 = 2LL * B, S0 = h->cfg.hm_size * 4;
    auto sq = [](int64_t v) { return v * v; };
    if (!strcmp(name, "layer0")) { *offset = w.L0; *numel = N2 * 64 * sq(S0 / 2); }
    else if (!strcmp(name, "pool0")) { *offset = w.P0; *numel = N2 * 64 * sq(S0 / 4); }      // stem + max-pool: fp32 NCHW, or (bf16 mode) bf16 [B * (S0/4)^2, 2 x 64]
    else if (!strcmp(name, "layer1_bf16")) { *offset = w.S[0][0]; *numel = N2 * 64 * sq(S0 / 4); }      // bf16 mode: bf16 [B * (S0/4)^2, 2 x 64]
    else if (!strcmp(name, "layer2_bf16")) { *offset = w.S[1][0]; *numel = N2 * 128 * sq(S0 / 8); }     // ... [B * (S0/8)^2, 2 x 128]: the decoder's operands
    else if (!strcmp(name, "layer3_bf16")) { *offset = w.S[2][0]; *numel = N2 * 256 * sq(S0 / 16); }
    else if (!strcmp(name, "layer4_bf16")) { *offset = w.S[3][0]; *numel = N2 * 512 * sq(S0 / 32); }
    else if (!strcmp(name, "layer1")) { *offset = w.S[0][3]; *numel = N2 * 64 * sq(S0 / 4); }
    else if (!strcmp(name, "layer2")) { *offset = w.S[1][3]; *numel = N2 * 128 * sq(S0 / 8); }
    else if (!strcmp(name, "layer3")) { *offset = w.S[2][3]; *numel = N2 * 256 * sq(S0 / 16); }
    else if (!strcmp(name, "layer4")) { *offset = w.S[3][3]; *numel = N2 * 512 * sq(S0 / 32); }
    else if (!strcmp(name, "u4")) { *offset = w.U4; *numel = (int64_t)B * 1024 * sq(S0 / 32); }
    else if (!strcmp(name, "cat3")) { *offset = w.CAT3; *numel = (int64_t)B * 1540 * sq(S0 / 16); }
    else if (!strcmp(name, "cat2")) { *offset = w.CAT2; *numel = (int64_t)B * 1280 * sq(S0 / 8); }
    else if (!strcmp(name, "cat1")) { *offset = w.CAT1; *numel = (int64_t)B * 640 * sq(S0 / 4); }
    else if (!strcmp(name, "conv_up3")) { *offset = w.X3; *numel = (int64_t)B * 1024 * sq(S0 / 16); }
    else if (!strcmp(name, "conv_up2")) { *offset = w.X2; *numel = (int64_t)B * 512 * sq(S0 / 8); }
    else if (!strcmp(name, "conv_up1")) { *offset = w.X1; *numel = (int64_t)B * 512 * sq(S0 / 4); }
    else { egotap_set_error("unknown intermediate '%s'", name); return EGOTAP_ERR_INVALID; }
    return EGOTAP_OK;
}

// the pack plan of the eval-mode bf16 forward at batch B (egotap_hm_forward and egotap_hm_freeze share it): the split-K budgets are the
// workspace slices egotap_hm_forward hands the backbone (the fp32 stem map's slot) and the decoder (40 MB of the WPACK region)
static size_t hm_forward_plan(const Handle* h, const HmParams& p, int B, PackTable* PT) {
    const int S0 = h->cfg.hm_size * 4;
    const int stage_sides[4] = {S0 / 4, S0 / 8, S0 / 16, S0 / 32};
    const size_t split_floats = (size_t)2 * B * 64 * (S0 / 2) * (S0 / 2), dec_split_floats = ((size_t)40 << 20) / 4;
    return hm_pack_plan(&p, p.nblk, PT, 2L * B, stage_sides, device_cu_count(), split_floats, dec_split_floats);
}
// frozen estimator: the arena holds the packed layout of the batch it was built for; a batch whose plan picks another K-slab depth for some
// weight (hm_pack_plan: 32- or 64-channel slabs by pixel count) does not fit and packs per call
static bool hm_arena_fits(const Handle* h, int net, const PackTable& PT) {
    if (!h->hm_arena[net] || h->hm_arena_nw[net] != PT.nw) return false;
    for (int i = 0; i < PT.nw; ++i)
        if (h->hm_arena_slab[net][i] != PT.w[i].slab) return false;
    return true;
}
// the precision / geometry for which an estimator has a packed region at all: the bf16 channels-last path (sides 64 / 128)
static bool hm_frozen_route(const Handle* h) { return h->precision == EGOTAP_PREC_BF16 && (h->cfg.hm_size == 64 || h->cfg.hm_size == 128); }

extern "C" int egotap_hm_frozen_bytes(egotap_handle h, int net, int B, size_t* bytes) {
    EGO_CHECK(h && bytes, "egotap_hm_frozen_bytes: null argument");
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "egotap_hm_frozen_bytes: net must be EGOTAP_NET_HM_POS or _ROT");
    EGO_CHECK(B > 0, "egotap_hm_frozen_bytes: batch must be positive");
    const int nblk_[4] = {hm_nblk(h, 0), hm_nblk(h, 1), hm_nblk(h, 2), hm_nblk(h, 3)};
    *bytes = hm_frozen_route(h) ? hm_pack_plan(nullptr, nblk_, nullptr) : 0;      // (the slices' sizes do not depend on the batch; their slab order does)
    return EGOTAP_OK;
}
extern "C" int egotap_hm_freeze(egotap_handle h, int net, int B, void* arena, size_t bytes, void* stream) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "egotap_hm_freeze: net must be EGOTAP_NET_HM_POS or _ROT");
    EGO_CHECK(B > 0, "egotap_hm_freeze: batch must be positive");
    EGO_CHECK(h->precision == EGOTAP_PREC_BF16, "egotap_hm_freeze: nothing to freeze in this precision mode (only EGOTAP_PREC_BF16 packs weights)");
    EGO_CHECK(hm_frozen_route(h), "egotap_hm_freeze: nothing to freeze at heatmap side %d: the bf16 channels-last path exists at sides 64 and 128", h->cfg.hm_size);
    EGO_CHECK(arena && ((uintptr_t)arena & 255) == 0, "egotap_hm_freeze: the arena must be a 256-byte aligned device pointer");
    int rc = hm_resolve(h, net);
    if (rc != EGOTAP_OK) return rc;
    const int nblk_[4] = {hm_nblk(h, 0), hm_nblk(h, 1), hm_nblk(h, 2), hm_nblk(h, 3)};
    const size_t need = hm_pack_plan(nullptr, nblk_, nullptr);
    if (bytes < need) {
        egotap_set_error("egotap_hm_freeze: arena too small: %zu bytes given, %zu needed", bytes, need);
        return EGOTAP_ERR_WORKSPACE;
    }
    PackTable PT;
    const size_t used = hm_forward_plan(h, h->hp[net], B, &PT);
    EGO_CHECK(used != 0 && used <= need, "egotap_hm_freeze: the estimator has more layers than the pack table holds");
    h->hm_arena[net] = nullptr;
    hipLaunchKernelGGL(pack_all_bf16s_kernel, dim3(PT.blocks), dim3(256), 0, (hipStream_t)stream, PT, (char*)arena);
    EGO_HIP(hipGetLastError());
    h->hm_arena_nw[net] = PT.nw;
    for (int i = 0; i < PT.nw; ++i) h->hm_arena_slab[net][i] = PT.w[i].slab;
    h->hm_arena[net] = (char*)arena;
    return EGOTAP_OK;
}
extern "C" int egotap_hm_unfreeze(egotap_handle h, int net) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "egotap_hm_unfreeze: net must be EGOTAP_NET_HM_POS or _ROT");
    h->hm_arena[net] = nullptr;
    return EGOTAP_OK;
}

// HeatMap_UnrealEgo_Shared.forward(left, right) (model/net_architecture.py:32-36, 45-51, 75-85, 139-173), eval mode.
// out_b != nullptr (egotap_predict_pose_rgb's hand-off, bf16 channels-last route only): the result as bf16 at out_b, `out` unused
static int hm_forward_impl(Handle* h, int net, const HmSrc& src, int B, float* out, int64_t out_image_stride, void* ws, size_t ws_bytes,
                           void* stream, __bf16* out_b) {
    // the bf16 channels-last route (fused stem, every convolution on the bf16-storage GEMM): hm_frozen_route is its one predicate, shared with the freeze entries
    // and with egotap_predict_pose_rgb's hand-off, which exists on this route only -- refused here, before anything is launched
    const bool fused_stem = hm_frozen_route(h);
    EGO_CHECK(out_b == nullptr || fused_stem, "egotap_hm_forward: the bf16 hand-off exists on the bf16 channels-last route only");
    const int S0 = h->cfg.hm_size * 4, s64 = S0 / 4, s32 = S0 / 8, s16 = S0 / 16, s8 = S0 / 32;
    // the bf16 channels-last path and the bf16 matrix-core convolutions exist at 64 / 128 only: every other side (any multiple of 16)
    // runs the exact-fp32 path in every precision mode -- the power-of-two conv instantiations where they exist, conv_f32_any_kernel elsewhere
    const bool built = s64 == 64 || s64 == 128;
    const bool exact = h->precision == EGOTAP_PREC_F32 || !built;
    int rc = hm_resolve(h, net);
    if (rc != EGOTAP_OK) return rc;
    const HmWs w = hm_ws(h, B);
    if (ws_bytes < w.total) {
        egotap_set_error("workspace too small: %zu bytes given, %zu needed for B=%d", ws_bytes, w.total, B);
        return EGOTAP_ERR_WORKSPACE;
    }
    const HmParams& p = h->hp[net];
    EGO_CHECK(out_image_stride >= (int64_t)p.n_out * s64 * s64, "out_image_stride smaller than the output image");
    h->conv_pack = built ? (__bf16*)((char*)ws + w.WPACK) : nullptr;      // (no conv_pack: conv_any takes no bf16 kernel)
    // [r4] exact-fp32 mode: the two weight-pack regions at the end of the workspace are unused -> scratch of the serving-batch channel split (conv_f32.h)
    struct PartGuard { Handle* h; ~PartGuard() { h->conv_part = nullptr; h->conv_part_floats = 0; } } part_guard{h};
    if (exact) {
        h->conv_part = (float*)((char*)ws + w.WPACK);
        h->conv_part_floats = (w.total - w.WPACK) / 4;
    }
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    auto F = [&](size_t off) { return (float*)(base + off); };
    const int N2 = 2 * B;
    // [r7] the source: fp32 frames, or bytes the stems stage themselves (sides 64 / 128), or bytes converted into the caller's slice first
    const float *left = src.left, *right = src.right;
    const bool stem_u8 = src.bytes() && built;
    static_assert(StemCfg::XT == 128 && StemPoolCfg::XS == 64, "sides 64 / 128 (RGB 256 / 512) are the geometries both stems take");
    if (src.bytes() && !built) {
        EGO_CHECK(src.scratch, "egotap_hm_forward: byte source without a converter slice");
        float* cl = src.scratch;
        float* cr = cl + (size_t)B * 3 * S0 * S0;
        GemmTimer t(h, s, "rgb_u8_to_f32", "rgb_u8_to_f32_kernel", 0.0);
        EGO_HIP(rgb_u8_to_f32_launch(src.left8, src.right8, src.table, cl, cr, B, S0, device_cu_count(), s));
        left = cl;
        right = cr;
    }

    // E1: stem conv7x7/2 + BN + ReLU on image n = 2b + eye (the L/R channel concat of every pyramid level is then a view); in the
    // bf16 mode it writes bf16 channels-last itself (half the bytes, and the layout the max-pool and the stages read)
    // [r3] ... bf16 mode: stem, BatchNorm, ReLU AND the max-pool in one kernel on the bf16 matrix cores (stem_bf16s.h): the 128 x 128 x 64
    // map never reaches HBM (round 2's two-kernel form -- fp32-MFMA stem writing bf16 channels-last, then a channels-last max-pool: 2.35 ms
    // against 0.66 per 512 images -- was retired in round 4).
    if (!fused_stem && stem_u8) {
        GemmTimer t(h, s, "hm.stem_u8", "stem_conv7_mfma_u8_kernel", 2.0 * N2 * 64 * 147 * (double)(S0 / 2) * (S0 / 2));
        EGO_HIP(stem_conv7_u8_launch(src.left8, src.right8, src.table, p.stem_w, p.stem_bn.g, p.stem_bn.b, p.stem_bn.m, p.stem_bn.v, F(w.L0), S0, N2, device_cu_count(), s));
    } else if (!fused_stem)
        EGO_HIP(stem_conv7_launch(left, right, p.stem_w, p.stem_bn.g, p.stem_bn.b, p.stem_bn.m, p.stem_bn.v, F(w.L0), S0, N2, device_cu_count(), s));
    if (fused_stem) {
        // bf16 mode: everything after the stem on bf16 channels-last activations, every convolution on the bf16-storage GEMM
        // (conv_bf16s.h).  Buffers live in the fp32 path's slots (each at most half as large).
        auto Hb = [&](size_t off) { return (__bf16*)(base + off); };
        HmBf16Bufs q{};
        q.P0 = Hb(w.P0);
        for (int i = 0; i < 4; ++i) { q.A[i] = Hb(w.S[i][0]); q.Ta[i] = Hb(w.S[i][1]); q.Tb[i] = Hb(w.S[i][2]); q.Td[i] = Hb(w.S[i][3]); }
        q.T4 = Hb(w.U4); q.C3 = Hb(w.CAT3); q.Y3 = Hb(w.X3); q.C2 = Hb(w.CAT2); q.Y2 = Hb(w.X2); q.C1 = Hb(w.CAT1); q.Y1 = Hb(w.X1);
        q.ZP = (__bf16*)(base + w.WPACK + ((size_t)40 << 20) + 32768);              // 256 bytes of zeros (taps outside the image)
        q.reg = base + w.WALL;
        q.split_slab = F(w.L0);                                                    // the fp32 stem map's slot: unused (fused stem)
        q.split_floats = (size_t)N2 * 64 * (S0 / 2) * (S0 / 2);
        q.dec_slab = (float*)(base + w.WPACK);                                     // [r4] the first 40 MB of the WPACK region (the zero page sits behind them): split-K partials of the decoder
        q.dec_split_floats = ((size_t)40 << 20) / 4;
        EGO_HIP(zero_fill(q.ZP, 256, s));
        // [r3] all 27 weight repacks and 19 BatchNorm folds of this forward in ONE launch (conv_bf16s.h, pack_all_bf16s_kernel): the
        // parameters stay the caller's live fp32 tensors, nothing is kept between calls ...
        PackTable PT;
        EGO_CHECK(hm_forward_plan(h, p, B, &PT) != 0, "egotap_hm_forward: the estimator has more layers than the pack table holds");
        // ... unless the caller froze this estimator (egotap_hm_freeze) and the batch's packed layout is the one in the arena: then the region is
        // the arena and nothing is packed
        if (hm_arena_fits(h, net, PT)) q.reg = h->hm_arena[net];
        else hipLaunchKernelGGL(pack_all_bf16s_kernel, dim3(PT.blocks), dim3(256), 0, s, PT, q.reg);
        EGO_HIP(hipGetLastError());
        int li = 0, bi = 0;
        EGO_HIP(hm_bf16_backbone(h, p, PT, li, bi, q, left, right, B, S0, nullptr, s, stem_u8 ? &src : nullptr));
        const __bf16* lv[4] = {q.A[0], q.A[1], q.A[2], q.A[3]};
        EGO_HIP(hm_bf16_decoder(h, p, PT, li, q, lv, B, S0, out, out_image_stride, s, out_b));
        EGO_CHECK(bi == PT.nb, "egotap_hm_forward: pack plan out of step with the forward");
        return EGOTAP_OK;
    }
    // E2: maxpool 3x3/2
    maxpool3s2_launch(F(w.L0), F(w.P0), (long)N2 * 64, S0 / 2, s);
    EGO_HIP(hipGetLastError());
    // E3: four stages of two BasicBlocks
    const float* x = F(w.P0);
    int cin = 64;
    const int sides[4] = {s64, s32, s16, s8};
    for (int i = 0; i < 4; ++i) {
        const int c = HM_CH[i], side = sides[i], nb = p.nblk[i];
        const long ist_in = (long)cin * (i == 0 ? side : 2 * side) * (i == 0 ? side : 2 * side);
        const long ist = (long)c * side * side;
        float *Ta = F(w.S[i][0]), *Tb = F(w.S[i][1]), *Td = F(w.S[i][2]), *L = F(w.S[i][3]);
        const float* xin = x;
        long xin_ist = ist_in;
        for (int b = 0; b < nb; ++b) {
            const auto& K = p.blk[i][b];
            const int stride = (b == 0 && i > 0) ? 2 : 1;
            const int bc = b == 0 ? cin : c;
            ConvArgs a1{xin, K.w1, Ta, nullptr, K.bn1.g, K.bn1.b, K.bn1.m, K.bn1.v, nullptr, xin_ist, ist, 0, N2, bc, c, 1, 0, 0};
            EGO_HIP(conv_any(h, HM_R1[i][b], 9, stride, side, a1, s));
            const float* idt = xin;
            long idt_ist = xin_ist;
            if (K.wd) {
                ConvArgs ad{xin, K.wd, Td, nullptr, K.bnd.g, K.bnd.b, K.bnd.m, K.bnd.v, nullptr, xin_ist, ist, 0, N2, bc, c, 0, 0, 0};
                EGO_HIP(conv_any(h, HM_RD[i], 1, 2, side, ad, s));
                idt = Td;
                idt_ist = ist;
            }
            float* y = ((nb - 1 - b) & 1) ? Tb : L;       // outputs alternate so that the last block writes the level
            ConvArgs a2{Ta, K.w2, y, idt, K.bn2.g, K.bn2.b, K.bn2.m, K.bn2.v, nullptr, ist, ist, idt_ist, N2, c, c, 1, 0, 0};
            EGO_HIP(conv_any(h, HM_R2[i][b], 9, 1, side, a2, s));
            xin = y;
            xin_ist = ist;
        }
        x = L;
        cin = c;
    }
    // E4-E9: decoder on the channel-concatenated pyramids ([2B, C, s, s] viewed as [B, 2C, s, s])
    const float *L1 = F(w.S[0][3]), *L2 = F(w.S[1][3]), *L3 = F(w.S[2][3]), *L4 = F(w.S[3][3]);
    float *U4 = F(w.U4), *CAT3 = F(w.CAT3), *X3 = F(w.X3), *CAT2 = F(w.CAT2), *X2 = F(w.X2), *CAT1 = F(w.CAT1), *X1 = F(w.X1);
    auto up = [&](const float* in, float* o, int C, int hin, long ist_in, long ist_out) {
        const long threads = (long)B * C * (2 * hin) * (2 * hin / 4);
        hipLaunchKernelGGL(upsample2x_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, in, o, B, C, hin, ist_in, ist_out);
        return hipGetLastError();
    };
    auto biasconv = [&](const char* role, int taps, int side, const float* in, long in_ist, const HmParams::Cv& cv, int Cin, int Cout,
                        float* o, long o_ist, int relu) {
        ConvArgs a{in, cv.w, o, nullptr, nullptr, nullptr, nullptr, nullptr, cv.b, in_ist, o_ist, 0, B, Cin, Cout, relu, 0, 0};
        return conv_any(h, role, taps, 1, side, a, s);
    };
    const long p8 = (long)s8 * s8, p16 = (long)s16 * s16, p32 = (long)s32 * s32, p64 = (long)s64 * s64;
    EGO_HIP(biasconv("hm.layer4_1x1", 1, s8, L4, 1024 * p8, p.l1x1[3], 1024, 1024, U4, 1024 * p8, 1));
    EGO_HIP(up(U4, CAT3, 1024, s8, 1024 * p8, 1540 * p16));
    EGO_HIP(biasconv("hm.layer3_1x1", 1, s16, L3, 512 * p16, p.l1x1[2], 512, 516, CAT3 + 1024 * p16, 1540 * p16, 1));
    EGO_HIP(biasconv("hm.conv_up3", 9, s16, CAT3, 1540 * p16, p.up[2], 1540, 1024, X3, 1024 * p16, 1));
    EGO_HIP(up(X3, CAT2, 1024, s16, 1024 * p16, 1280 * p32));
    EGO_HIP(biasconv("hm.layer2_1x1", 1, s32, L2, 256 * p32, p.l1x1[1], 256, 256, CAT2 + 1024 * p32, 1280 * p32, 1));
    EGO_HIP(biasconv("hm.conv_up2", 9, s32, CAT2, 1280 * p32, p.up[1], 1280, 512, X2, 512 * p32, 1));
    EGO_HIP(up(X2, CAT1, 512, s32, 512 * p32, 640 * p64));
    EGO_HIP(biasconv("hm.layer1_1x1", 1, s64, L1, 128 * p64, p.l1x1[0], 128, 128, CAT1 + 512 * p64, 640 * p64, 1));
    EGO_HIP(biasconv("hm.conv_up1", 9, s64, CAT1, 640 * p64, p.up[0], 640, 512, X1, 512 * p64, 1));
    EGO_HIP(biasconv("hm.conv_heatmap", 1, s64, X1, 512 * p64, p.head, 512, p.n_out, out, out_image_stride, 0));
    return EGOTAP_OK;
}

extern "C" int egotap_hm_forward(egotap_handle h, int net, const float* left, const float* right, int B, float* out,
                                 int64_t out_image_stride, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "egotap_hm_forward: net must be EGOTAP_NET_HM_POS or _ROT");
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(B > 0 && left && right && out && ws, "egotap_hm_forward: null argument or negative batch");
    EGO_CHECK((((uintptr_t)left | (uintptr_t)right | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ws & 255) == 0, "pointers must be 16-byte (ws: 256-byte) aligned");
    return hm_forward_impl(h, net, hm_src_f32(left, right), B, out, out_image_stride, ws, ws_bytes, stream, nullptr);
}

// ---- [r7] camera bytes: the converter, and one estimator from bytes
// (camera_bytes = false: frames of a sensor source that go through a resize or gather first, at whatever alignment their own fetch asks for)
static const char* rgb_u8_refusal(const void* left8, const void* right8, const void* table, bool camera_bytes = true) {
    if (!left8 || !right8) return "null frames (left8 and right8 are required)";
    if (!table) return "null table (the fp32 [3][256] value table is required)";
    if (camera_bytes && (((uintptr_t)left8 | (uintptr_t)right8) & 3) != 0) return "left8 and right8 must be 4-byte aligned (rows are read as aligned dwords)";
    if (((uintptr_t)table & 15) != 0) return "the table must be 16-byte aligned";
    return nullptr;
}
extern "C" int egotap_rgb_u8_to_f32(const uint8_t* left8, const uint8_t* right8, int B, int S0, const float* table, float* left_f32, float* right_f32,
                                    void* stream) {
    static const char* const who = "egotap_rgb_u8_to_f32";
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(B > 0, "%s: negative batch (B = %d)", who, B);
    EGO_CHECK(S0 > 0 && S0 % 4 == 0, "%s: the frame side must be a positive multiple of 4 (S0 = %d)", who, S0);
    const char* why = rgb_u8_refusal(left8, right8, table);
    EGO_CHECK(!why, "%s: %s", who, why);
    EGO_CHECK(left_f32 && right_f32, "%s: null output", who);
    EGO_CHECK((((uintptr_t)left_f32 | (uintptr_t)right_f32) & 15) == 0, "%s: left_f32 and right_f32 must be 16-byte aligned", who);
    EGO_HIP(rgb_u8_to_f32_launch(left8, right8, table, left_f32, right_f32, B, S0, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_hm_forward_u8_workspace_bytes(egotap_handle h, int B, size_t* bytes) {
    EGO_CHECK(h && bytes, "egotap_hm_forward_u8_workspace_bytes: null argument");
    EGO_CHECK(B >= 0, "egotap_hm_forward_u8_workspace_bytes: negative batch");
    const int b = B > 0 ? B : 1;
    *bytes = hm_ws(h, b).total + hm_u8_slice_bytes(h, b);
    return EGOTAP_OK;
}
extern "C" int egotap_hm_forward_u8(egotap_handle h, int net, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* out,
                                    int64_t out_image_stride, void* ws, size_t ws_bytes, void* stream) {
    static const char* const who = "egotap_hm_forward_u8";
    EGO_CHECK(h, "%s: null handle", who);
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "%s: net must be EGOTAP_NET_HM_POS or _ROT", who);
    EGO_CHECK(B > 0, "%s: the batch must be positive (B = %d)", who, B);
    const char* why = rgb_u8_refusal(left8, right8, table);
    EGO_CHECK(!why, "%s: %s", who, why);
    EGO_CHECK(out && ws, "%s: null argument (out and ws are required)", who);
    EGO_CHECK(((uintptr_t)out & 15) == 0 && ((uintptr_t)ws & 255) == 0, "%s: out must be 16-byte aligned, ws 256-byte aligned", who);
    if (hm_resolve(h, net) != EGOTAP_OK) {
        const std::string key = g_err;
        egotap_set_error("%s: unbound parameter of %s: %s", who, net == EGOTAP_NET_HM_POS ? "the position estimator" : "the limb estimator", key.c_str());
        return EGOTAP_ERR_INVALID;
    }
    const size_t hm_bytes = hm_ws(h, B).total, need = hm_bytes + hm_u8_slice_bytes(h, B);
    EGO_CHECK(ws_bytes >= need, "%s: workspace too small: %zu bytes given, %zu needed for B=%d", who, ws_bytes, need, B);
    const HmSrc src{nullptr, nullptr, left8, right8, table, (float*)((char*)ws + hm_bytes)};
    return hm_forward_impl(h, net, src, B, out, out_image_stride, ws, hm_bytes, stream, nullptr);
}

// ------------------------------------------------------------------------------------------------ stereo RGB -> pose in one call
// egotap_predict_pose_rgb: both estimators (eval mode, in pieces of `chunk` frames, one U-Net scratch) and then the pose-only head, composed from
// hm_forward_impl and lift_forward_impl -- every kernel choice is theirs.  Workspace: [ scratch = max(estimator scratch of a chunk, head scratch of the
// batch): the two never run at once | the heatmaps: fp32 [B, 6J, S, S] when the caller passes none, or their bf16 hand-off form | a byte source's
// converter slice of one chunk, where the stems do not read bytes themselves | [r8] a sensor source's resized bytes of one chunk: n frames x 2 eyes x
// 3 S0^2 bytes (OUTPUT frames: H and W do not enter) ].  The one statement of it: the size queries, the walk and the debug query read nothing else.
enum RgbSource { RGB_SRC_F32, RGB_SRC_U8, RGB_SRC_SENSOR };
struct RgbWs { size_t HM /* = the scratch's bytes */, conv, resized, total; };
static inline int rgb_chunk(int B, int chunk) { return chunk <= 0 || chunk > B ? B : chunk; }
static RgbWs rgb_ws(const Handle* h, int B, int chunk, RgbSource kind) {
    const int c = rgb_chunk(B, chunk);
    const size_t a = hm_ws(h, c).total, b = lift_ws(h, B).total, S0 = (size_t)h->cfg.hm_size * 4;
    RgbWs w;
    w.HM = al256(a > b ? a : b);
    w.conv = w.HM + al256((size_t)B * h->C * h->cfg.hm_size * h->cfg.hm_size * 4);
    w.resized = w.conv + (kind == RGB_SRC_F32 ? 0 : hm_u8_slice_bytes(h, c));
    w.total = w.resized + (kind == RGB_SRC_SENSOR ? (size_t)c * 2 * 3 * S0 * S0 : 0);
    return w;
}
// The hand-off: nobody asked for the fp32 heatmaps, the estimators run the bf16 channels-last route (whose conv_heatmap is the bf16-storage GEMM) and
// the head runs its bf16-storage route (which reads a bf16 copy of the heatmaps and nothing else of them): conv_heatmap then writes that copy itself.
static bool rgb_handoff(const Handle* h, int B, const float* heatmaps) { return heatmaps == nullptr && hm_frozen_route(h) && lift_bf16s_route(h, B); }

extern "C" int egotap_predict_pose_rgb_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes) {
    EGO_CHECK(h && bytes, "egotap_predict_pose_rgb_workspace_bytes: null argument");
    EGO_CHECK(B >= 0 && chunk >= 0, "egotap_predict_pose_rgb_workspace_bytes: negative batch or chunk");
    *bytes = rgb_ws(h, B > 0 ? B : 1, chunk, RGB_SRC_F32).total;
    return EGOTAP_OK;
}

// the walk the one-call entries share: `src` holds the whole batch's frames (fp32, or bytes, or a sensor's frames behind `src.sensor`); the argument
// checks that depend on the source are the entries' own
// keypoints != nullptr (the _kp entries): the peaks of the 2J position maps, one launch over the batch between the estimators and the head, read
// from whichever form of the heatmaps this call holds; kp_affine: 2 x 4 floats (left eye, right eye)
// limbs != nullptr (the _kpl entries): the records of the 2J (cos, sin) pairs of the limb maps (limb_decode.h), one more launch right behind it on the
// same tensor with the same affine
static int predict_pose_rgb_impl(const char* who, egotap_handle h, const HmSrc& src, int B, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                 void* stream, float* keypoints = nullptr, const float* kp_affine = nullptr, float* limbs = nullptr) {
    static const char* const net_name[EGOTAP_NET_COUNT] = {"the lifting head", "the position estimator", "the limb estimator"};
    for (int net = 0; net < EGOTAP_NET_COUNT; ++net) {
        if ((net == EGOTAP_NET_LIFT ? lift_resolve(h) : hm_resolve(h, net)) != EGOTAP_OK) {
            const std::string key = g_err;
            egotap_set_error("%s: unbound parameter of %s: %s", who, net_name[net], key.c_str());
            return EGOTAP_ERR_INVALID;
        }
    }
    const RgbSource kind = src.sensor ? RGB_SRC_SENSOR : src.bytes() ? RGB_SRC_U8 : RGB_SRC_F32;      // [r8] a sensor source is a byte source behind a resize
    const RgbWs w = rgb_ws(h, B, chunk, kind);
    const int c = rgb_chunk(B, chunk), S = h->cfg.hm_size, HW = S * S, J = h->J;
    EGO_CHECK(ws_bytes >= w.total, "%s: workspace too small: %zu bytes given, %zu needed for B=%d, chunk=%d", who, ws_bytes, w.total, B, chunk);
    HmSrc whole = src;
    HmSensor sensor{};
    whole.scratch = kind != RGB_SRC_F32 ? (float*)((char*)ws + w.conv) : nullptr;
    if (src.sensor) {
        sensor = *src.sensor;
        sensor.slice = (unsigned char*)ws + w.resized;
    }
    const long img = (long)h->C * HW, rgb = 3L * (4 * S) * (4 * S);
    const bool handoff = rgb_handoff(h, B, heatmaps);
    float* hm = heatmaps ? heatmaps : (float*)((char*)ws + w.HM);
    __bf16* hmb = handoff ? (__bf16*)((char*)ws + w.HM) : nullptr;
    h->rgb_form = EGOTAP_RGB_FORM_NONE;
    // position net: channels [0, 2J) (left | right); limb net: [2J, 6J) (left cos, sin | right cos, sin)
    const int nets[2] = {EGOTAP_NET_HM_POS, EGOTAP_NET_HM_ROT}, c0[2] = {0, 2 * J};
    const bool resize = src.sensor && !src.bytes(), stems = hm_stem_reads_bytes(S);
    if (resize || (src.bytes() && !stems)) {
        // the prepared walk (pieces outer, estimators inner): a piece's frames are made ready ONCE and both estimators read them there, sharing the
        // U-Net scratch one after the other, as ever.  [r8] A sensor's frames are resized into the slice and are camera bytes from there on.  (A sensor
        // source with bytes() set is the identity request: the caller's frames ARE the camera bytes and are read in place.)  Bytes are read by the
        // byte-source stems at sides 64 / 128 and go through the converter into its slice elsewhere (never with the hand-off: that exists at sides
        // 64 / 128 only).
        unsigned char* s8l = sensor.slice;
        const long frame = sensor.src.frame_stride;
        const bool gather = sensor.map_left != nullptr;
        const bool per_stream = gather && sensor.map_streams > 0;
        const char* const role = per_stream ? "lens_remap_streams" : gather ? "lens_remap" : sensor.src.fetch == FETCH_RGB8 ? "rgb_u8_resize" : "yuv_u8_resize";      // the timing hook's names
        const char* const kernel = per_stream ? "lens_remap_streams_kernel" : gather ? "lens_remap_kernel" : sensor.src.fetch == FETCH_RGB8 ? "rgb_u8_resize_kernel" : "yuv_u8_resize_kernel";
        for (int lo = 0; lo < B; lo += c) {
            const int n = B - lo < c ? B - lo : c;
            HmSrc piece = whole.at(lo, rgb);
            if (resize) {
                unsigned char* s8r = s8l + (size_t)n * rgb;
                const unsigned char *fl = sensor.left8 + lo * frame, *fr = sensor.right8 + lo * frame;
                GemmTimer t(h, (hipStream_t)stream, role, kernel, 0.0);
                if (per_stream)      // the piece's first frame is frame `lo` of the batch: its frames read maps (lo + b) % S
                    EGO_HIP(lens_remap_streams_launch(fl, fr, n, sensor.src, sensor.map_left, sensor.map_right, sensor.map_streams, (long)lo, sensor.fill[0],
                                                      sensor.fill[1], 4 * S, s8l, s8r, device_cu_count(), (hipStream_t)stream));
                else if (gather)
                    EGO_HIP(lens_remap_launch(fl, fr, n, sensor.src, sensor.map_left, sensor.map_right, sensor.fill[0], sensor.fill[1], 4 * S, s8l, s8r,
                                              device_cu_count(), (hipStream_t)stream));
                else
                    EGO_HIP(frame_resize_launch(fl, fr, n, sensor.src, sensor.rect[0], sensor.rect[1], sensor.mirror[0], sensor.mirror[1], 4 * S, s8l, s8r,
                                                device_cu_count(), (hipStream_t)stream));
                piece = HmSrc{nullptr, nullptr, s8l, s8r, src.table, nullptr};
            }
            if (!stems) {
                float *cl = whole.scratch, *cr = cl + (size_t)n * rgb;
                GemmTimer t(h, (hipStream_t)stream, "rgb_u8_to_f32", "rgb_u8_to_f32_kernel", 0.0);
                EGO_HIP(rgb_u8_to_f32_launch(piece.left8, piece.right8, src.table, cl, cr, n, 4 * S, device_cu_count(), (hipStream_t)stream));
                piece = hm_src_f32(cl, cr);
            }
            const bool ho = stems && handoff;
            for (int k = 0; k < 2; ++k) {
                const long at = lo * img + (long)c0[k] * HW;
                const int rc = hm_forward_impl(h, nets[k], piece, n, ho ? nullptr : hm + at, img, ws, w.HM, stream, ho ? hmb + at : nullptr);
                if (rc != EGOTAP_OK) return rc;
            }
        }
    } else      // float frames, and bytes the stems read themselves: estimators outer, pieces inner
    for (int k = 0; k < 2; ++k)
        for (int lo = 0; lo < B; lo += c) {
            const int n = B - lo < c ? B - lo : c;
            const long at = lo * img + (long)c0[k] * HW;
            const int rc = hm_forward_impl(h, nets[k], whole.at(lo, rgb), n, handoff ? nullptr : hm + at, img, ws, w.HM, stream, handoff ? hmb + at : nullptr);
            if (rc != EGOTAP_OK) return rc;
        }
    if (keypoints) {
        GemmTimer t(h, (hipStream_t)stream, "heatmap_peaks", "heatmap_peaks_kernel", 0.0);
        EGO_HIP(handoff ? heatmap_peaks_launch(hmb, B, S, img, 0, 2 * J, 2, kp_affine, keypoints, (hipStream_t)stream)
                        : heatmap_peaks_launch(hm, B, S, img, 0, 2 * J, 2, kp_affine, keypoints, (hipStream_t)stream));
    }
    if (limbs) {
        GemmTimer t(h, (hipStream_t)stream, "limb_decode", "limb_decode_kernel", 0.0);
        EGO_HIP(handoff ? limb_decode_launch(hmb, B, S, img, 2 * J, J, 2, kp_affine, limbs, (hipStream_t)stream)
                        : limb_decode_launch(hm, B, S, img, 2 * J, J, 2, kp_affine, limbs, (hipStream_t)stream));
    }
    const int rc = lift_forward_impl(h, handoff ? nullptr : hm, B, pose, ws, w.HM, stream, true, who, hmb);
    if (rc != EGOTAP_OK) return rc;
    h->rgb_form = handoff ? EGOTAP_RGB_FORM_HANDOFF : heatmaps ? EGOTAP_RGB_FORM_HEATMAPS : EGOTAP_RGB_FORM_SCRATCH;
    return EGOTAP_OK;
}

// ---- the 2D keypoints and limb records of the one-call entries (heatmap_peaks.h, limb_decode.h): each entry below is ONE body serving the parent (no
// extra output), its _kp form (keypoints required) and its _kpl form (keypoints and limbs, either may be NULL)
// what the entries refuse about their extra outputs, or nullptr; pose / heatmaps extents from the handle
static const char* rgb_kp_refusal(const Handle* h, int B, const float* pose, const float* heatmaps, bool kp_required, const float* kp, const float* limbs) {
    if (kp_required && !kp) return "null keypoints (device f32 [B, 2, n_joints_hm, 4])";
    if ((uintptr_t)kp & 15) return "keypoints must be 16-byte aligned";
    if ((uintptr_t)limbs & 15) return "limbs must be 16-byte aligned";
    const int S = h->cfg.hm_size;
    const size_t kp_bytes = (size_t)B * 2 * h->J * 16, limb_bytes = (size_t)B * 2 * h->J * 32;
    auto overlaps = [](const void* p, size_t pn, const void* q, size_t qn) {
        return p && q && (uintptr_t)p < (uintptr_t)q + qn && (uintptr_t)q < (uintptr_t)p + pn;
    };
    const size_t pose_bytes = (size_t)B * h->out_joints * 3 * 4, hm_bytes = (size_t)B * h->C * S * S * 4;
    if (overlaps(kp, kp_bytes, pose, pose_bytes) || overlaps(kp, kp_bytes, heatmaps, hm_bytes)) return "keypoints overlaps pose or heatmaps";
    if (overlaps(limbs, limb_bytes, pose, pose_bytes) || overlaps(limbs, limb_bytes, heatmaps, hm_bytes) || overlaps(limbs, limb_bytes, kp, kp_bytes))
        return "limbs overlaps pose, heatmaps or keypoints";
    return nullptr;
}
static const float kRgbKpAffine[8] = {4.f, 0.f, 4.f, 0.f, 4.f, 0.f, 4.f, 0.f};      // heatmap pixels -> pixels of the S0 = 4 S input frame, both eyes

// What the three *_entry functions below check alike, in the order they always did: the handle and the batch; `source_why`, what the entry's own
// source refuses about its frame arguments (nullptr: nothing; tested by the entry, told here, in its place); pose, ws, the chunk and the alignments --
// with the float entry's frames (`f32`: left, right; nullptr for a byte entry, whose source_why spoke for its frames) in the same two statements; for
// frames that go through the resize (`resized`) its side limit; the extra outputs.
static int rgb_entry_checks(const char* who, egotap_handle h, int B, const char* source_why, const float* const* f32, const float* pose, const float* heatmaps,
                            int chunk, const void* ws, bool resized, bool kp, const float* keypoints, const float* limbs) {
    EGO_CHECK(h, "%s: null handle", who);
    EGO_CHECK(B > 0, "%s: the batch must be positive (B = %d)", who, B);
    EGO_CHECK(!source_why, "%s: %s", who, source_why);
    const char* frames = f32 ? "left, right, " : "";
    EGO_CHECK((!f32 || (f32[0] && f32[1])) && pose && ws, "%s: null argument (%spose and ws are required; only heatmaps may be NULL)", who, frames);
    EGO_CHECK(chunk >= 0, "%s: negative chunk (0 = the whole batch)", who);
    const uintptr_t bits = (f32 ? (uintptr_t)f32[0] | (uintptr_t)f32[1] : 0) | (uintptr_t)pose | (uintptr_t)heatmaps;
    EGO_CHECK((bits & 15) == 0 && ((uintptr_t)ws & 255) == 0, "%s: %spose and heatmaps must be 16-byte aligned, ws 256-byte aligned", who, frames);
    const int S0 = 4 * h->cfg.hm_size;
    EGO_CHECK(!resized || S0 <= kResizeMaxSide, "%s: the frame side 4 * hm_size = %d is beyond the resize kernel's %d", who, S0, kResizeMaxSide);
    const char* why = rgb_kp_refusal(h, B, pose, heatmaps, kp, keypoints, limbs);
    EGO_CHECK(!why, "%s: %s", who, why);
    return EGOTAP_OK;
}

static int predict_pose_rgb_entry(const char* who, egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                                  size_t ws_bytes, void* stream, bool kp, float* keypoints, float* limbs) {
    const float* const frames[2] = {left, right};
    const int rc = rgb_entry_checks(who, h, B, nullptr, frames, pose, heatmaps, chunk, ws, false, kp, keypoints, limbs);
    if (rc != EGOTAP_OK) return rc;
    return predict_pose_rgb_impl(who, h, hm_src_f32(left, right), B, pose, heatmaps, chunk, ws, ws_bytes, stream, keypoints, kRgbKpAffine, limbs);
}
extern "C" int egotap_predict_pose_rgb(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                                       size_t ws_bytes, void* stream) {
    return predict_pose_rgb_entry("egotap_predict_pose_rgb", h, left, right, B, pose, heatmaps, chunk, ws, ws_bytes, stream, false, nullptr, nullptr);
}
extern "C" int egotap_predict_pose_rgb_kp(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                                          size_t ws_bytes, void* stream, float* keypoints) {
    return predict_pose_rgb_entry("egotap_predict_pose_rgb_kp", h, left, right, B, pose, heatmaps, chunk, ws, ws_bytes, stream, true, keypoints, nullptr);
}
extern "C" int egotap_predict_pose_rgb_kpl(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                                           size_t ws_bytes, void* stream, float* keypoints, float* limbs) {
    return predict_pose_rgb_entry("egotap_predict_pose_rgb_kpl", h, left, right, B, pose, heatmaps, chunk, ws, ws_bytes, stream, false, keypoints, limbs);
}

// [r7] the same call from camera bytes: uint8 [B, S0, S0, 3] per eye and the fp32 [3][256] value table
extern "C" int egotap_predict_pose_rgb_u8_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes) {
    EGO_CHECK(h && bytes, "egotap_predict_pose_rgb_u8_workspace_bytes: null argument");
    EGO_CHECK(B >= 0 && chunk >= 0, "egotap_predict_pose_rgb_u8_workspace_bytes: negative batch or chunk");
    *bytes = rgb_ws(h, B > 0 ? B : 1, chunk, RGB_SRC_U8).total;
    return EGOTAP_OK;
}
static int predict_pose_rgb_u8_entry(const char* who, egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose,
                                     float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, bool kp, float* keypoints, float* limbs) {
    const int rc = rgb_entry_checks(who, h, B, rgb_u8_refusal(left8, right8, table), nullptr, pose, heatmaps, chunk, ws, false, kp, keypoints, limbs);
    if (rc != EGOTAP_OK) return rc;
    const HmSrc src{nullptr, nullptr, left8, right8, table, nullptr};
    return predict_pose_rgb_impl(who, h, src, B, pose, heatmaps, chunk, ws, ws_bytes, stream, keypoints, kRgbKpAffine, limbs);
}
extern "C" int egotap_predict_pose_rgb_u8(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                                          int chunk, void* ws, size_t ws_bytes, void* stream) {
    return predict_pose_rgb_u8_entry("egotap_predict_pose_rgb_u8", h, left8, right8, B, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false, nullptr, nullptr);
}
extern "C" int egotap_predict_pose_rgb_u8_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                                             int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints) {
    return predict_pose_rgb_u8_entry("egotap_predict_pose_rgb_u8_kp", h, left8, right8, B, table, pose, heatmaps, chunk, ws, ws_bytes, stream, true, keypoints,
                                     nullptr);
}
extern "C" int egotap_predict_pose_rgb_u8_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                                              int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints, float* limbs) {
    return predict_pose_rgb_u8_entry("egotap_predict_pose_rgb_u8_kpl", h, left8, right8, B, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false, keypoints,
                                     limbs);
}

// ---- [r8] the sensor's own frames (frame_source.h): cropped, mirrored and resized (frame_resize.h) or gathered through lens maps (lens_remap.h) on
// the device, standalone and in front of the one call.  Each entry turns its arguments into a FrameSource and says what it refuses about them; the
// rest is shared: sensor_op_checks by the three standalone operators, predict_pose_sensor_impl by the three one-call entries.
static const char* rgb8_source_refusal(const void* left8, const void* right8, int H, int W, const int* rect_left, const int* rect_right, FrameSource* q) {
    if (!left8 || !right8) return "null frames (left8 and right8 are required)";
    if (!rect_left || !rect_right) return "null rectangle (rect_left and rect_right are four ints each: x0, y0, w, h)";
    if (const char* why = frame_layout_refusal(FETCH_RGB8, H, W, 0, 0L, 0L)) return why;
    *q = frame_source_rgb8(H, W);
    return resize_rects_refusal(*q, rect_left, rect_right);
}
// what the standalone operators check alike, in their order: the batch, the output side, the operator's source (`source_why`), the outputs
static int sensor_op_checks(const char* who, int B, int S0, const char* source_why, const void* out_left8, const void* out_right8) {
    EGO_CHECK(B > 0, "%s: the batch must be positive (B = %d)", who, B);
    EGO_CHECK(S0 > 0 && S0 % 4 == 0 && S0 <= kResizeMaxSide, "%s: the output side must be a positive multiple of 4, at most %d (S0 = %d)", who, kResizeMaxSide, S0);
    EGO_CHECK(!source_why, "%s: %s", who, source_why);
    EGO_CHECK(out_left8 && out_right8, "%s: null output", who);
    EGO_CHECK((((uintptr_t)out_left8 | (uintptr_t)out_right8) & 3) == 0, "%s: out_left8 and out_right8 must be 4-byte aligned (rows are written as aligned dwords)", who);
    return EGOTAP_OK;
}
extern "C" int egotap_rgb_u8_resize(const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rect_left, const int* rect_right, int mirror_left,
                                    int mirror_right, int S0, uint8_t* out_left8, uint8_t* out_right8, void* stream) {
    FrameSource q{};
    const int rc = sensor_op_checks("egotap_rgb_u8_resize", B, S0, rgb8_source_refusal(left8, right8, H, W, rect_left, rect_right, &q), out_left8, out_right8);
    if (rc != EGOTAP_OK) return rc;
    EGO_HIP(frame_resize_launch(left8, right8, B, q, rect_left, rect_right, mirror_left, mirror_right, S0, out_left8, out_right8, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_predict_pose_sensor_u8_workspace_bytes(egotap_handle h, int B, int H, int W, int chunk, size_t* bytes) {
    static const char* const who = "egotap_predict_pose_sensor_u8_workspace_bytes";
    EGO_CHECK(h && bytes, "%s: null argument", who);
    EGO_CHECK(B >= 0 && chunk >= 0, "%s: negative batch or chunk", who);
    const char* why = frame_layout_refusal(FETCH_RGB8, H, W, 0, 0L, 0L);
    EGO_CHECK(!why, "%s: %s", who, why);
    *bytes = rgb_ws(h, B > 0 ? B : 1, chunk, RGB_SRC_SENSOR).total;
    return EGOTAP_OK;
}
// heatmap pixels -> pixels of the eye's sensor frame: the inverse of the map the resize kernels apply (pixel centres at i + 0.5, align_corners = False); a
// mirrored eye's output column X shows source column S0 - 1 - X, so its x runs backwards from the rectangle's right edge
static void sensor_keypoint_affine(const Handle* h, const HmSensor& q, float* affine) {
    for (int e = 0; e < 2; ++e) {
        const float S = (float)h->cfg.hm_size, sx = (float)q.rect[e][2] / S;
        affine[4 * e + 0] = q.mirror[e] ? -sx : sx;
        affine[4 * e + 1] = (float)(q.rect[e][0] + (q.mirror[e] ? q.rect[e][2] : 0));
        affine[4 * e + 2] = (float)q.rect[e][3] / S;
        affine[4 * e + 3] = (float)q.rect[e][1];
    }
}
static const char* const kNullRectsOrMirrors = "null rectangles or mirror flags (rects: 2 x 4 ints, left then right; mirrors: 2 ints)";
// What the three sensor entries do alike once their source is stated.  `why`: what the entry refuses about its own arguments (nullptr: nothing), told
// in its place among the shared checks, the table's two behind it.  rects (2 x 4 ints) and mirrors (2 ints) are read once nothing is refused; `lens`
// brings the maps and fills of a gather.  `in_place`: the u8 entry's identity request, the caller's frames ARE the camera bytes.
static int predict_pose_sensor_impl(const char* who, egotap_handle h, const char* why, const uint8_t* left8, const uint8_t* right8, int B, const FrameSource& fs,
                                    const int* rects, const int32_t* mirrors, const egotap_lens_source* lens, bool in_place, const float* table, float* pose,
                                    float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, bool kp, float* keypoints, float* limbs,
                                    int lens_streams = 0) {
    if (!why) why = rgb_u8_refusal(left8, right8, table, false);
    const int rc = rgb_entry_checks(who, h, B, why, nullptr, pose, heatmaps, chunk, ws, true, kp, keypoints, limbs);
    if (rc != EGOTAP_OK) return rc;
    // (q.slice is the walk's to place: the workspace layout is read there, once)
    HmSensor q{left8, right8, fs, {{rects[0], rects[1], rects[2], rects[3]}, {rects[4], rects[5], rects[6], rects[7]}}, {mirrors[0] ? 1 : 0, mirrors[1] ? 1 : 0},
               lens ? (const int*)lens->map_left : nullptr, lens ? (const int*)lens->map_right : nullptr,
               {lens ? lens_fill(lens->fill[0]) : 0u, lens ? lens_fill(lens->fill[1]) : 0u}, nullptr, lens ? lens_streams : 0};
    HmSrc src{nullptr, nullptr, in_place ? left8 : nullptr, in_place ? right8 : nullptr, table, nullptr};
    src.sensor = &q;
    float affine[8];
    sensor_keypoint_affine(h, q, affine);
    return predict_pose_rgb_impl(who, h, src, B, pose, heatmaps, chunk, ws, ws_bytes, stream, keypoints, affine, limbs);
}
static int predict_pose_sensor_u8_entry(const char* who, egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects,
                                        const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream,
                                        bool kp, float* keypoints, float* limbs) {
    FrameSource fs{};
    const char* why = !(rects && mirrors) ? kNullRectsOrMirrors : rgb8_source_refusal(left8, right8, H, W, rects, rects + 4, &fs);
    if (!why) why = rgb_u8_refusal(left8, right8, table);      // frames a stem may read in place: its alignment, behind the table's presence as ever
    // the identity request (frames already S0 x S0, the full frame, no mirror): the caller's frames are read in place, nothing is resized
    const int S0 = h ? 4 * h->cfg.hm_size : 0;
    bool identity = !why && H == S0 && W == S0 && !mirrors[0] && !mirrors[1];
    for (int e = 0; identity && e < 2; ++e) identity = rects[4 * e] == 0 && rects[4 * e + 1] == 0 && rects[4 * e + 2] == S0 && rects[4 * e + 3] == S0;
    return predict_pose_sensor_impl(who, h, why, left8, right8, B, fs, rects, mirrors, nullptr, identity, table, pose, heatmaps, chunk, ws, ws_bytes, stream, kp,
                                    keypoints, limbs);
}
extern "C" int egotap_predict_pose_sensor_u8(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects, const int* mirrors,
                                             const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream) {
    return predict_pose_sensor_u8_entry("egotap_predict_pose_sensor_u8", h, left8, right8, B, H, W, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes, stream,
                                        false, nullptr, nullptr);
}
extern "C" int egotap_predict_pose_sensor_u8_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects,
                                                const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                                void* stream, float* keypoints) {
    return predict_pose_sensor_u8_entry("egotap_predict_pose_sensor_u8_kp", h, left8, right8, B, H, W, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes,
                                        stream, true, keypoints, nullptr);
}
extern "C" int egotap_predict_pose_sensor_u8_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects,
                                                 const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                                 void* stream, float* keypoints, float* limbs) {
    return predict_pose_sensor_u8_entry("egotap_predict_pose_sensor_u8_kpl", h, left8, right8, B, H, W, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes,
                                        stream, false, keypoints, limbs);
}

// ---- NV12 / YUYV sensor frames: the colour conversion inside the resize, standalone and in front of the one call
// what is wrong with a descriptor or the frames behind it, or nullptr; fills `q` (layout, fetch and integer coefficients) when nothing is
static const char* yuv_source_refusal(const egotap_yuv_source* src, const void* left8, const void* right8, FrameSource* q) {
    if (!src) return "null source descriptor (egotap_yuv_source)";
    if (src->struct_size != (int32_t)sizeof(egotap_yuv_source)) return "wrong struct_size (sizeof(egotap_yuv_source) expected)";
    if (src->format != EGOTAP_YUV_NV12 && src->format != EGOTAP_YUV_YUYV) return "unknown format (EGOTAP_YUV_NV12 or EGOTAP_YUV_YUYV)";
    const int fetch = src->format == EGOTAP_YUV_NV12 ? FETCH_NV12 : FETCH_YUYV;
    if (const char* why = frame_layout_refusal(fetch, src->H, src->W, src->pitch, (long)src->uv_offset, (long)src->frame_stride)) return why;
    if (src->matrix != EGOTAP_YUV_BT601 && src->matrix != EGOTAP_YUV_BT709) return "unknown matrix (EGOTAP_YUV_BT601 or EGOTAP_YUV_BT709)";
    if (src->range != EGOTAP_YUV_LIMITED && src->range != EGOTAP_YUV_FULL) return "unknown range (EGOTAP_YUV_LIMITED or EGOTAP_YUV_FULL)";
    if (!left8 || !right8) return "null frames (left8 and right8 are required)";
    if ((((uintptr_t)left8 | (uintptr_t)right8) & (uintptr_t)(frame_base_alignment(fetch) - 1)) != 0)
        return fetch == FETCH_NV12 ? "left8 and right8 must be 2-byte aligned (NV12: the chroma pair is one aligned 16-bit load)"
                                   : "left8 and right8 must be 4-byte aligned (YUYV: the pixel pair is one aligned dword)";
    *q = FrameSource{fetch, src->H, src->W, src->pitch, fetch == FETCH_NV12 ? (long)src->uv_offset : 0L, (long)src->frame_stride,
                     yuv_coefficients(src->matrix, src->range)};
    return nullptr;
}
extern "C" int egotap_yuv_u8_resize(const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rect_left, const int* rect_right,
                                    int mirror_left, int mirror_right, int S0, uint8_t* out_left8, uint8_t* out_right8, void* stream) {
    FrameSource q{};
    const char* why = yuv_source_refusal(src, left8, right8, &q);
    if (!why) why = !(rect_left && rect_right) ? "null rectangle (rect_left and rect_right are four ints each: x0, y0, w, h)" : resize_rects_refusal(q, rect_left, rect_right);
    const int rc = sensor_op_checks("egotap_yuv_u8_resize", B, S0, why, out_left8, out_right8);
    if (rc != EGOTAP_OK) return rc;
    EGO_HIP(frame_resize_launch(left8, right8, B, q, rect_left, rect_right, mirror_left, mirror_right, S0, out_left8, out_right8, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
// the sensor entry with the descriptor in place of H, W; never the identity request: a YUV source always converts
static int predict_pose_sensor_yuv_entry(const char* who, egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* ysrc,
                                         const int* rects, const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws,
                                         size_t ws_bytes, void* stream, bool kp, float* keypoints, float* limbs) {
    FrameSource fs{};
    const char* why = !(rects && mirrors) ? kNullRectsOrMirrors : yuv_source_refusal(ysrc, left8, right8, &fs);
    if (!why) why = resize_rects_refusal(fs, rects, rects + 4);
    return predict_pose_sensor_impl(who, h, why, left8, right8, B, fs, rects, mirrors, nullptr, false, table, pose, heatmaps, chunk, ws, ws_bytes, stream, kp,
                                    keypoints, limbs);
}
extern "C" int egotap_predict_pose_sensor_yuv(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                              const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                              void* stream) {
    return predict_pose_sensor_yuv_entry("egotap_predict_pose_sensor_yuv", h, left8, right8, B, src, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes, stream,
                                         false, nullptr, nullptr);
}
extern "C" int egotap_predict_pose_sensor_yuv_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                                 const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                                 void* stream, float* keypoints) {
    return predict_pose_sensor_yuv_entry("egotap_predict_pose_sensor_yuv_kp", h, left8, right8, B, src, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes,
                                         stream, true, keypoints, nullptr);
}
extern "C" int egotap_predict_pose_sensor_yuv_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                                  const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes,
                                                  void* stream, float* keypoints, float* limbs) {
    return predict_pose_sensor_yuv_entry("egotap_predict_pose_sensor_yuv_kpl", h, left8, right8, B, src, rects, mirrors, table, pose, heatmaps, chunk, ws, ws_bytes,
                                         stream, false, keypoints, limbs);
}

// ---- frames from another lens: the lens maps applied as a bilinear gather (lens_remap.h), standalone and in front of the one call
// what is wrong with a descriptor or the frames behind it, or nullptr; fills `q` (layout, fetch and integer coefficients) when nothing is
static const char* lens_source_refusal(const egotap_lens_source* src, const void* left8, const void* right8, FrameSource* q) {
    if (!src) return "null source descriptor (egotap_lens_source)";
    if (src->struct_size != (int32_t)sizeof(egotap_lens_source)) return "wrong struct_size (sizeof(egotap_lens_source) expected)";
    if (src->format != EGOTAP_LENS_RGB8 && src->format != EGOTAP_LENS_NV12 && src->format != EGOTAP_LENS_YUYV)
        return "unknown format (EGOTAP_LENS_RGB8, EGOTAP_LENS_NV12 or EGOTAP_LENS_YUYV)";
    if (src->format == EGOTAP_LENS_RGB8) {
        if (const char* why = frame_layout_refusal(FETCH_RGB8, src->H, src->W, 0, 0L, 0L)) return why;
        if (!left8 || !right8) return "null frames (left8 and right8 are required)";
        *q = frame_source_rgb8(src->H, src->W);
    } else {
        if (src->yuv.format != (src->format == EGOTAP_LENS_NV12 ? EGOTAP_YUV_NV12 : EGOTAP_YUV_YUYV)) return "the embedded egotap_yuv_source has another format than the descriptor";
        if (src->yuv.H != src->H || src->yuv.W != src->W) return "the embedded egotap_yuv_source has another H or W than the descriptor";
        if (const char* why = yuv_source_refusal(&src->yuv, left8, right8, q)) return why;
    }
    if (!src->map_left || !src->map_right) return "null lens map (map_left and map_right are device int32 [S0 * S0][2])";
    if ((((uintptr_t)src->map_left | (uintptr_t)src->map_right) & 15) != 0) return "map_left and map_right must be 16-byte aligned (four entries are two 16-byte loads)";
    return nullptr;
}
extern "C" int egotap_lens_remap(const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S0, uint8_t* out_left8, uint8_t* out_right8,
                                 void* stream) {
    FrameSource q{};
    const int rc = sensor_op_checks("egotap_lens_remap", B, S0, lens_source_refusal(src, left8, right8, &q), out_left8, out_right8);
    if (rc != EGOTAP_OK) return rc;
    EGO_HIP(lens_remap_launch(left8, right8, B, q, (const int*)src->map_left, (const int*)src->map_right, lens_fill(src->fill[0]), lens_fill(src->fill[1]), S0,
                              out_left8, out_right8, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_predict_pose_lens_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes) {
    static const char* const who = "egotap_predict_pose_lens_workspace_bytes";
    EGO_CHECK(h && bytes, "%s: null argument", who);
    EGO_CHECK(B >= 0 && chunk >= 0, "%s: negative batch or chunk", who);
    *bytes = rgb_ws(h, B > 0 ? B : 1, chunk, RGB_SRC_SENSOR).total;      // the sensor entry's: the slice holds OUTPUT frames
    return EGOTAP_OK;
}
// what is wrong with the number of streams of a batch of B frames, or nullptr (B <= 0 is the entry's own refusal)
static const char* lens_streams_refusal(int B, int S) {
    if (S < 1 || S > EGOTAP_MAX_STREAM_RIGS) return "the number of streams S must be between 1 and 4096 (map_left and map_right hold S maps each)";
    if (B > 0 && B % S != 0) return "the batch B must be a multiple of the number of streams S (frame b is gathered through map b % S)";
    return nullptr;
}
// the sensor entry with the descriptor in place of H, W, rectangles and mirrors; never the identity request: a lens source always gathers.  The
// keypoints come out in the model camera's calibration pixels: the sensor entry's affine on a frame of that size, the full rectangle, the eye's
// mirror flag.  `streams`: the _streams entries, S maps per eye (otherwise one map per eye and S is not read)
static int predict_pose_lens_entry(const char* who, egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* lsrc,
                                   const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, bool kp, float* keypoints,
                                   float* limbs, bool streams = false, int S = 0) {
    FrameSource fs{};
    const char* why = lens_source_refusal(lsrc, left8, right8, &fs);
    if (!why && streams) why = lens_streams_refusal(B, S);
    if (!why && (lsrc->model_h < 1 || lsrc->model_w < 1 || lsrc->model_h > kResizeMaxSrc || lsrc->model_w > kResizeMaxSrc))
        why = "the model camera's calibration image (model_h, model_w) must be between 1 and 16384 on each side";
    const int mw = why ? 0 : lsrc->model_w, mh = why ? 0 : lsrc->model_h;      // (a refused descriptor may be NULL)
    const int full[8] = {0, 0, mw, mh, 0, 0, mw, mh};
    return predict_pose_sensor_impl(who, h, why, left8, right8, B, fs, full, why ? nullptr : lsrc->mirror, lsrc, false, table, pose, heatmaps, chunk, ws, ws_bytes,
                                    stream, kp, keypoints, limbs, streams ? S : 0);
}
extern "C" int egotap_predict_pose_lens(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                                        float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream) {
    return predict_pose_lens_entry("egotap_predict_pose_lens", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false, nullptr, nullptr);
}
extern "C" int egotap_predict_pose_lens_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                                           float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints) {
    return predict_pose_lens_entry("egotap_predict_pose_lens_kp", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, true, keypoints,
                                   nullptr);
}
extern "C" int egotap_predict_pose_lens_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                                            float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints, float* limbs) {
    return predict_pose_lens_entry("egotap_predict_pose_lens_kpl", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false, keypoints,
                                   limbs);
}

// the standalone operator: maps c0 .. c0 + n - 1 of each image of a [B, C, S, S] tensor -> [B, n, 4] records; no handle
extern "C" int egotap_heatmap_peaks(const void* hm, int dtype, int B, int S, int64_t image_stride, int c0, int n, int groups, const float* affine, float* peaks,
                                    void* stream) {
    static const char* const who = "egotap_heatmap_peaks";
    EGO_CHECK(hm && peaks, "%s: null argument (hm and peaks are required; only affine may be NULL)", who);
    EGO_CHECK(dtype == EGOTAP_F32 || dtype == EGOTAP_BF16, "%s: unknown dtype %d (EGOTAP_F32 or EGOTAP_BF16)", who, dtype);
    EGO_CHECK(B > 0 && n > 0, "%s: the batch and the number of maps must be positive (B = %d, n = %d)", who, B, n);
    EGO_CHECK(groups > 0 && groups <= kPeaksMaxGroups, "%s: groups must be between 1 and %d (groups = %d)", who, kPeaksMaxGroups, groups);
    EGO_CHECK(n % groups == 0, "%s: n must be a multiple of groups (n = %d, groups = %d)", who, n, groups);
    EGO_CHECK(c0 >= 0, "%s: negative first channel (c0 = %d)", who, c0);
    EGO_CHECK(S >= 16 && S <= 128 && S % 16 == 0, "%s: the side must be a multiple of 16 from 16 to 128 (S = %d)", who, S);
    const int esz = dtype == EGOTAP_F32 ? 4 : 2;
    EGO_CHECK(image_stride >= (int64_t)(c0 + (int64_t)n) * S * S, "%s: image_stride %lld is smaller than (c0 + n) * S*S = %lld", who, (long long)image_stride,
              (long long)((c0 + (int64_t)n) * S * S));
    EGO_CHECK(image_stride * esz % 16 == 0, "%s: image_stride must be a multiple of 16 bytes (%lld elements of %d bytes)", who, (long long)image_stride, esz);
    EGO_CHECK((((uintptr_t)hm | (uintptr_t)peaks) & 15) == 0, "%s: hm and peaks must be 16-byte aligned", who);
    EGO_HIP(dtype == EGOTAP_F32 ? heatmap_peaks_launch((const float*)hm, B, S, (long)image_stride, c0, n, groups, affine, peaks, (hipStream_t)stream)
                                : heatmap_peaks_launch((const __bf16*)hm, B, S, (long)image_stride, c0, n, groups, affine, peaks, (hipStream_t)stream));
    return EGOTAP_OK;
}

// the standalone operator: the n_limbs (cos, sin) pairs of each of `eyes` eyes of each image of a [B, C, S, S] tensor -> [B, eyes, n_limbs, 8] records; no handle
extern "C" int egotap_limb_decode(const void* hm, int dtype, int B, int S, int64_t image_stride, int c0, int n_limbs, int eyes, const float* affine, float* limbs,
                                  void* stream) {
    static const char* const who = "egotap_limb_decode";
    EGO_CHECK(hm && limbs, "%s: null argument (hm and limbs are required; only affine may be NULL)", who);
    EGO_CHECK(dtype == EGOTAP_F32 || dtype == EGOTAP_BF16, "%s: unknown dtype %d (EGOTAP_F32 or EGOTAP_BF16)", who, dtype);
    EGO_CHECK(B > 0 && n_limbs > 0, "%s: the batch and the number of limbs must be positive (B = %d, n_limbs = %d)", who, B, n_limbs);
    EGO_CHECK(eyes > 0 && eyes <= kPeaksMaxGroups, "%s: eyes must be between 1 and %d (eyes = %d)", who, kPeaksMaxGroups, eyes);
    EGO_CHECK(c0 >= 0, "%s: negative first channel (c0 = %d)", who, c0);
    EGO_CHECK(S >= 16 && S <= 128 && S % 16 == 0, "%s: the side must be a multiple of 16 from 16 to 128 (S = %d)", who, S);
    const int esz = dtype == EGOTAP_F32 ? 4 : 2;
    const int64_t last = (c0 + 2 * (int64_t)eyes * n_limbs) * S * S;
    EGO_CHECK(image_stride >= last, "%s: image_stride %lld is smaller than (c0 + 2 * eyes * n_limbs) * S*S = %lld", who, (long long)image_stride, (long long)last);
    EGO_CHECK(image_stride * esz % 16 == 0, "%s: image_stride must be a multiple of 16 bytes (%lld elements of %d bytes)", who, (long long)image_stride, esz);
    EGO_CHECK((((uintptr_t)hm | (uintptr_t)limbs) & 15) == 0, "%s: hm and limbs must be 16-byte aligned", who);
    EGO_HIP(dtype == EGOTAP_F32 ? limb_decode_launch((const float*)hm, B, S, (long)image_stride, c0, n_limbs, eyes, affine, limbs, (hipStream_t)stream)
                                : limb_decode_launch((const __bf16*)hm, B, S, (long)image_stride, c0, n_limbs, eyes, affine, limbs, (hipStream_t)stream));
    return EGOTAP_OK;
}

// ---- the fisheye camera model, the stereo triangulation of the keypoints (ocam.h) and their fusion with the lifted joints (stereo_fuse.h): four operators, no handle
static bool ego_finite(double v) { return std::isfinite(v); }
// what is wrong with a camera model, or nullptr
static const char* ocam_refusal(const egotap_ocam* m) {
    if (!m) return "null camera model";
    if (m->n_pol < 1 || m->n_pol > EGOTAP_OCAM_MAX_POL) return "polynomialC2W (n_pol) must have 1 .. 8 coefficients";
    if (m->n_invpol < 1 || m->n_invpol > EGOTAP_OCAM_MAX_INVPOL) return "polynomialW2C (n_invpol) must have 1 .. 24 coefficients";
    bool fin = ego_finite(m->xc) && ego_finite(m->yc) && ego_finite(m->c) && ego_finite(m->d) && ego_finite(m->e);
    for (int k = 0; k < m->n_pol; ++k) fin = fin && ego_finite(m->pol[k]);
    for (int k = 0; k < m->n_invpol; ++k) fin = fin && ego_finite(m->invpol[k]);
    if (!fin) return "a calibration value is not finite";
    if (m->ue_flip != 0.0 && m->ue_flip != 1.0) return "ue_flip must be 0 or 1";
    if (m->c - m->d * m->e == 0.0) return "the affine is singular (c - d * e == 0)";
    return nullptr;
}
// the model as the kernels take it: the coefficients behind the lengths are zero, whatever the caller left there
static egotap_ocam ocam_clean(const egotap_ocam& m) {
    egotap_ocam o = m;
    for (int k = m.n_pol; k < EGOTAP_OCAM_MAX_POL; ++k) o.pol[k] = 0.0;
    for (int k = m.n_invpol; k < EGOTAP_OCAM_MAX_INVPOL; ++k) o.invpol[k] = 0.0;
    return o;
}
static bool ego_overlap(const void* p, size_t pn, const void* q, size_t qn) {
    return p && q && (uintptr_t)p < (uintptr_t)q + qn && (uintptr_t)q < (uintptr_t)p + pn;
}

static int ocam_points_entry(const char* who, bool project, const float* in, int N, const egotap_ocam* model, float* out, void* stream) {
    const char* in_name = project ? "points3d" : "points2d";
    const char* out_name = project ? "points2d" : "rays";
    EGO_CHECK(in && out, "%s: null argument (%s and %s are required)", who, in_name, out_name);
    EGO_CHECK(N > 0, "%s: the number of points must be positive (N = %d)", who, N);
    EGO_CHECK((((uintptr_t)in | (uintptr_t)out) & 3) == 0, "%s: %s and %s must be 4-byte aligned", who, in_name, out_name);
    const char* why = ocam_refusal(model);
    EGO_CHECK(!why, "%s: model: %s", who, why);
    const size_t in_bytes = (size_t)N * (project ? 3 : 2) * 4, out_bytes = (size_t)N * (project ? 2 : 3) * 4;
    EGO_CHECK(!ego_overlap(in, in_bytes, out, out_bytes), "%s: %s overlaps %s", who, out_name, in_name);
    const egotap_ocam m = ocam_clean(*model);
    GemmTimer t(g_timing_handle, (hipStream_t)stream, project ? "ocam_project" : "ocam_unproject", project ? "ocam_project_kernel" : "ocam_unproject_kernel", 0.0);
    EGO_HIP(project ? ocam_project_launch(in, N, m, out, (hipStream_t)stream) : ocam_unproject_launch(in, N, m, out, (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_ocam_project(const float* points3d, int N, const egotap_ocam* model, float* points2d, void* stream) {
    return ocam_points_entry("egotap_ocam_project", true, points3d, N, model, points2d, stream);
}
extern "C" int egotap_ocam_unproject(const float* points2d, int N, const egotap_ocam* model, float* rays, void* stream) {
    return ocam_points_entry("egotap_ocam_unproject", false, points2d, N, model, rays, stream);
}

// the sizes and the pose rows, as the single-rig and the per-stream entries refuse them alike
static int stereo_batch_checks(const char* who, int B, int J) {
    EGO_CHECK(B > 0 && J > 0, "%s: the batch and the number of joints must be positive (B = %d, J = %d)", who, B, J);
    EGO_CHECK(J <= kStereoMaxJoints, "%s: at most %d joints, one lane each (J = %d)", who, kStereoMaxJoints, J);
    return EGOTAP_OK;
}
static int stereo_pose_rows_check(const char* who, bool has_pose, int J, int P, int pose_row0) {
    if (has_pose) EGO_CHECK(pose_row0 >= 0 && (int64_t)pose_row0 + J <= P, "%s: pose rows pose_row0 .. pose_row0 + J - 1 = %d .. %lld are not inside the P = %d rows", who,
                            pose_row0, (long long)pose_row0 + J - 1, P);
    return EGOTAP_OK;
}
// what egotap_stereo_triangulate and egotap_stereo_fuse check alike, after their own pointers: the sizes, the two models, the pose rows, and the rig as the
// kernels take it (R NULL: identity, affine NULL: identity) with everything in it finite
static int stereo_rig_checks(const char* who, int B, int J, const egotap_ocam* left, const egotap_ocam* right, const double* R, const double* t, const double* affine,
                             double min_score, bool has_pose, int P, int pose_row0, StereoRig& rig) {
    if (int rc = stereo_batch_checks(who, B, J)) return rc;
    const char* why = ocam_refusal(left);
    EGO_CHECK(!why, "%s: left: %s", who, why);
    why = ocam_refusal(right);
    EGO_CHECK(!why, "%s: right: %s", who, why);
    if (int rc = stereo_pose_rows_check(who, has_pose, J, P, pose_row0)) return rc;
    rig.cam[0] = ocam_clean(*left);
    rig.cam[1] = ocam_clean(*right);
    bool fin = ego_finite(min_score);
    for (int k = 0; k < 9; ++k) fin = fin && ego_finite(rig.R[k] = R ? R[k] : (k % 4 == 0 ? 1.0 : 0.0));
    for (int k = 0; k < 3; ++k) fin = fin && ego_finite(rig.t[k] = t[k]);
    for (int k = 0; k < 8; ++k) fin = fin && ego_finite(rig.aff[k / 4][k % 4] = affine ? affine[k] : (k & 1 ? 0.0 : 1.0));
    rig.min_score = min_score;
    EGO_CHECK(fin, "%s: R, t, affine and min_score must be finite", who);
    return EGOTAP_OK;
}

static int stereo_triangulate_overlap_check(const char* who, const float* keypoints, int B, int J, const float* pose, int P, const float* joints3d, const float* frame) {
    const size_t kp_bytes = (size_t)B * 2 * J * 16, pose_bytes = pose ? (size_t)B * P * 12 : 0, j3_bytes = (size_t)B * J * 32, fr_bytes = (size_t)B * 32;
    EGO_CHECK(!ego_overlap(joints3d, j3_bytes, keypoints, kp_bytes) && !ego_overlap(joints3d, j3_bytes, pose, pose_bytes) &&
                  !ego_overlap(frame, fr_bytes, keypoints, kp_bytes) && !ego_overlap(frame, fr_bytes, pose, pose_bytes) &&
                  !ego_overlap(joints3d, j3_bytes, frame, fr_bytes),
              "%s: joints3d and frame must not overlap keypoints, pose or each other", who);
    return EGOTAP_OK;
}

extern "C" int egotap_stereo_triangulate(const float* keypoints, int B, int J, const egotap_ocam* left, const egotap_ocam* right, const double* R, const double* t,
                                         const double* affine, double min_score, const float* pose, int P, int pose_row0, float* joints3d, float* frame,
                                         void* stream) {
    static const char* const who = "egotap_stereo_triangulate";
    EGO_CHECK(keypoints && t && joints3d && frame, "%s: null argument (keypoints, t, joints3d and frame are required; R, affine and pose may be NULL)", who);
    EGO_CHECK((((uintptr_t)keypoints | (uintptr_t)joints3d | (uintptr_t)frame) & 15) == 0 && ((uintptr_t)pose & 3) == 0,
              "%s: keypoints, joints3d and frame must be 16-byte aligned, pose 4-byte aligned", who);
    StereoRig rig;
    if (int rc = stereo_rig_checks(who, B, J, left, right, R, t, affine, min_score, pose != nullptr, P, pose_row0, rig)) return rc;
    if (int rc = stereo_triangulate_overlap_check(who, keypoints, B, J, pose, P, joints3d, frame)) return rc;
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "stereo_triangulate", "stereo_triangulate_kernel", 0.0);
    EGO_HIP(stereo_triangulate_launch(keypoints, B, J, rig, pose, P, pose_row0, joints3d, frame, (hipStream_t)stream));
    return EGOTAP_OK;
}

// what egotap_stereo_fuse and egotap_stereo_fuse_streams check alike after the rig: the parameters (copied into `prm` as the kernel takes them) and the overlaps
static int stereo_fuse_arg_checks(const char* who, const float* keypoints, int B, int J, const float* pose, int P, const float* frame, const egotap_fuse_params* params,
                                  const float* fused, const float* pose_fused, const float* stats, egotap_fuse_params& prm) {
    const egotap_fuse_params& q = *params;
    EGO_CHECK(ego_finite(q.sigma_ray) && q.sigma_ray > 0.0, "%s: params: sigma_ray must be finite and > 0 (%g)", who, q.sigma_ray);
    EGO_CHECK(ego_finite(q.sigma_prior) && q.sigma_prior > 0.0, "%s: params: sigma_prior must be finite and > 0 (%g)", who, q.sigma_prior);
    EGO_CHECK(q.max_sigma >= 0.0, "%s: params: max_sigma must be >= 0, +inf for no gate (%g)", who, q.max_sigma);      // (a NaN fails the comparison)
    EGO_CHECK(q.min_joints >= 0, "%s: params: min_joints must not be negative (%d)", who, q.min_joints);
    const struct {
        const char* name;
        const void* p;
        size_t n;
    } in[3] = {{"keypoints", keypoints, (size_t)B * 2 * J * 16}, {"pose", pose, (size_t)B * P * 12}, {"frame", frame, (size_t)B * 32}},
      out[3] = {{"fused", fused, (size_t)B * J * 32}, {"pose_fused", pose_fused, (size_t)B * P * 12}, {"stats", stats, (size_t)B * 32}};
    for (int o = 0; o < 3; ++o) {
        for (int i = 0; i < 3; ++i) {
            if (o == 1 && i == 1 && pose_fused == pose) continue;      // in place
            EGO_CHECK(!ego_overlap(out[o].p, out[o].n, in[i].p, in[i].n), "%s: %s overlaps %s", who, out[o].name, in[i].name);
        }
        for (int p = o + 1; p < 3; ++p) EGO_CHECK(!ego_overlap(out[o].p, out[o].n, out[p].p, out[p].n), "%s: %s overlaps %s", who, out[o].name, out[p].name);
    }
    prm = egotap_fuse_params{q.sigma_ray, q.sigma_prior, q.max_sigma, q.min_joints};
    return EGOTAP_OK;
}

// the lifted joints fused with the keypoint rays (stereo_fuse.h): one operator behind the triangulation, no handle
extern "C" int egotap_stereo_fuse(const float* keypoints, int B, int J, const egotap_ocam* left, const egotap_ocam* right, const double* R, const double* t,
                                  const double* affine, double min_score, const float* pose, int P, int pose_row0, const float* frame,
                                  const egotap_fuse_params* params, float* fused, float* pose_fused, float* stats, void* stream) {
    static const char* const who = "egotap_stereo_fuse";
    EGO_CHECK(keypoints && t && pose && frame && params && fused && pose_fused && stats,
              "%s: null argument (keypoints, t, pose, frame, params, fused, pose_fused and stats are required; R and affine may be NULL)", who);
    EGO_CHECK((((uintptr_t)keypoints | (uintptr_t)frame | (uintptr_t)fused | (uintptr_t)stats) & 15) == 0 && (((uintptr_t)pose | (uintptr_t)pose_fused) & 3) == 0,
              "%s: keypoints, frame, fused and stats must be 16-byte aligned, pose and pose_fused 4-byte aligned", who);
    StereoRig rig;
    if (int rc = stereo_rig_checks(who, B, J, left, right, R, t, affine, min_score, true, P, pose_row0, rig)) return rc;
    egotap_fuse_params prm;
    if (int rc = stereo_fuse_arg_checks(who, keypoints, B, J, pose, P, frame, params, fused, pose_fused, stats, prm)) return rc;
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "stereo_fuse", "stereo_fuse_kernel", 0.0);
    EGO_HIP(stereo_fuse_launch(keypoints, B, J, rig, pose, P, pose_row0, frame, prm, fused, pose_fused, stats, (hipStream_t)stream));
    return EGOTAP_OK;
}

// ---- the pose, the root and the stereo joints filtered over time (pose_track.h): one operator in the camera's frame or in a world frame, no handle
// both entries: `world` adds rig_pose, ortho_tol and placed_cam, and calls the fourth output placed_world
static int pose_track_entry(const char* who, bool world, const float* pose, const float* frame, const float* joints3d, const double* rig_pose, int T, int S, int P,
                            int J, const float* dts, double dt, const egotap_track_params* params, double ortho_tol, const double* state_in, double* state_out,
                            float* tracks, float* placed, float* placed_cam, void* stream) {
    const char* const placed_name = world ? "placed_world" : "placed";
    if (world)
        EGO_CHECK(pose && state_in && state_out && tracks && placed && params && rig_pose && placed_cam,
                  "%s: null argument (pose, rig_pose, params, state_in, state_out, tracks, placed_world and placed_cam are required; frame, joints3d and dts may be "
                  "NULL)", who);
    else
        EGO_CHECK(pose && state_in && state_out && tracks && placed && params,
                  "%s: null argument (pose, params, state_in, state_out, tracks and placed are required; frame, joints3d and dts may be NULL)", who);
    EGO_CHECK(T > 0 && S > 0 && P > 0, "%s: T, S and P must be positive (T = %d, S = %d, P = %d)", who, T, S, P);
    EGO_CHECK(P <= kTrackMaxRows, "%s: at most %d pose rows, one lane each (P = %d)", who, kTrackMaxRows, P);
    EGO_CHECK(J >= 0 && J <= kTrackMaxRows, "%s: J must be 0 .. %d joints, one lane each (J = %d)", who, kTrackMaxRows, J);
    EGO_CHECK((J > 0) == (joints3d != nullptr), "%s: joints3d goes with J > 0 and NULL with J = 0 (J = %d, joints3d %s)", who, J, joints3d ? "given" : "NULL");
    EGO_CHECK((int64_t)T * S <= INT32_MAX, "%s: T * S = %lld frames do not fit an int", who, (long long)T * S);
    EGO_CHECK((((uintptr_t)pose | (uintptr_t)frame | (uintptr_t)joints3d | (uintptr_t)dts | (uintptr_t)placed) & 3) == 0,
              "%s: pose, frame, joints3d, dts and %s must be 4-byte aligned", who, placed_name);
    EGO_CHECK(((uintptr_t)placed_cam & 3) == 0, "%s: placed_cam must be 4-byte aligned", who);
    EGO_CHECK(((uintptr_t)tracks & 15) == 0, "%s: tracks must be 16-byte aligned", who);
    EGO_CHECK((((uintptr_t)state_in | (uintptr_t)state_out) & 7) == 0, "%s: state_in and state_out must be 8-byte aligned", who);
    EGO_CHECK(((uintptr_t)rig_pose & 7) == 0, "%s: rig_pose must be 8-byte aligned", who);
    EGO_CHECK(dts || (ego_finite(dt) && dt > 0.0), "%s: dt must be finite and > 0 when dts is NULL (dt = %g)", who, dt);
    EGO_CHECK(!world || ortho_tol >= 0.0, "%s: ortho_tol must be >= 0 (%g)", who, ortho_tol);      // (a NaN fails the comparison)
    const egotap_track_params& q = *params;
    const double cls[3][3] = {{q.pose_min_cutoff, q.pose_beta, q.pose_d_cutoff}, {q.root_min_cutoff, q.root_beta, q.root_d_cutoff},
                              {q.joints_min_cutoff, q.joints_beta, q.joints_d_cutoff}};
    static const char* const cls_name[3] = {"pose", "root", "joints"};
    for (int c = 0; c < 3; ++c) {
        EGO_CHECK(ego_finite(cls[c][0]) && cls[c][0] > 0.0, "%s: params: %s_min_cutoff must be finite and > 0 (%g)", who, cls_name[c], cls[c][0]);
        EGO_CHECK(ego_finite(cls[c][1]) && cls[c][1] >= 0.0, "%s: params: %s_beta must be finite and >= 0 (%g)", who, cls_name[c], cls[c][1]);
        EGO_CHECK(ego_finite(cls[c][2]) && cls[c][2] > 0.0, "%s: params: %s_d_cutoff must be finite and > 0 (%g)", who, cls_name[c], cls[c][2]);
    }
    EGO_CHECK(q.max_disagree >= 0.0, "%s: params: max_disagree must be >= 0, +inf for off (%g)", who, q.max_disagree);      // (a NaN fails the comparison)
    EGO_CHECK(q.max_gap >= 0.0, "%s: params: max_gap must be >= 0, +inf for off (%g)", who, q.max_gap);
    EGO_CHECK(q.max_joint_gap >= 0.0, "%s: params: max_joint_gap must be >= 0, +inf for off (%g)", who, q.max_joint_gap);
    EGO_CHECK(q.min_joints >= 0, "%s: params: min_joints must not be negative (%d)", who, q.min_joints);
    EGO_CHECK(q.max_hold >= 0, "%s: params: max_hold must not be negative (%d)", who, q.max_hold);
    const size_t B = (size_t)T * S, K = (size_t)P + 1 + J;
    const struct {
        const char* name;
        const void* p;
        size_t n;
    } in[6] = {{"pose", pose, B * P * 12}, {"frame", frame, B * 32}, {"joints3d", joints3d, B * J * 32}, {"dts", dts, (size_t)T * 4}, {"state_in", state_in, (size_t)S * K * 96},
               {"rig_pose", rig_pose, B * 96}},
      out[4] = {{"state_out", state_out, (size_t)S * K * 96}, {"tracks", tracks, B * K * 32}, {placed_name, placed, B * P * 12}, {"placed_cam", placed_cam, B * P * 12}};
    for (int o = 0; o < 4; ++o) {      // (the camera-frame entry's rig_pose and placed_cam are NULL: they overlap nothing)
        for (int i = 0; i < 6; ++i) {
            if (o == 0 && i == 4 && state_out == state_in) continue;      // in place
            EGO_CHECK(!ego_overlap(out[o].p, out[o].n, in[i].p, in[i].n), "%s: %s overlaps %s", who, out[o].name, in[i].name);
        }
        for (int p = o + 1; p < 4; ++p) EGO_CHECK(!ego_overlap(out[o].p, out[o].n, out[p].p, out[p].n), "%s: %s overlaps %s", who, out[o].name, out[p].name);
    }
    for (int i = 0; i < 5; ++i) EGO_CHECK(!ego_overlap(rig_pose, B * 96, in[i].p, in[i].n), "%s: rig_pose overlaps %s", who, in[i].name);
    if (world) {
        GemmTimer tm(g_timing_handle, (hipStream_t)stream, "pose_track_world", "pose_track_world_kernel", 0.0);
        EGO_HIP(pose_track_world_launch(pose, frame, joints3d, rig_pose, T, S, P, J, dts, dt, q, ortho_tol, state_in, state_out, tracks, placed, placed_cam,
                                        (hipStream_t)stream));
    } else {
        GemmTimer tm(g_timing_handle, (hipStream_t)stream, "pose_track", "pose_track_kernel", 0.0);
        EGO_HIP(pose_track_launch(pose, frame, joints3d, T, S, P, J, dts, dt, q, state_in, state_out, tracks, placed, (hipStream_t)stream));
    }
    return EGOTAP_OK;
}
extern "C" int egotap_pose_track(const float* pose, const float* frame, const float* joints3d, int T, int S, int P, int J, const float* dts, double dt,
                                 const egotap_track_params* params, const double* state_in, double* state_out, float* tracks, float* placed, void* stream) {
    return pose_track_entry("egotap_pose_track", false, pose, frame, joints3d, nullptr, T, S, P, J, dts, dt, params, 0.0, state_in, state_out, tracks, placed, nullptr,
                            stream);
}
extern "C" int egotap_pose_track_world(const float* pose, const float* frame, const float* joints3d, const double* rig_pose, int T, int S, int P, int J, const float* dts,
                                       double dt, const egotap_track_params* params, double ortho_tol, const double* state_in, double* state_out, float* tracks,
                                       float* placed_world, float* placed_cam, void* stream) {
    return pose_track_entry("egotap_pose_track_world", true, pose, frame, joints3d, rig_pose, T, S, P, J, dts, dt, params, ortho_tol, state_in, state_out, tracks,
                            placed_world, placed_cam, stream);
}

// ---- a rigid skeleton and bone rotations from the tracked pose (skeleton_fit.h): one operator behind the trackers, no handle
// (both entries: with_twist says which, and twist is read only then)
static int skeleton_fit_entry(const char* who, bool with_twist, const float* points, const float* tracks, int T, int S, const egotap_skeleton_rig* rig,
                              const egotap_skeleton_twist* twist, const egotap_skeleton_params* params, const double* state_in, double* state_out, float* rigid,
                              float* rotations, float* lengths, void* stream) {
    EGO_CHECK(points && rig && params && rigid && rotations && lengths,
              "%s: null argument (points, rig, params, rigid, rotations and lengths are required; tracks may be NULL)", who);
    EGO_CHECK(!with_twist || twist, "%s: null argument (twist is required: egotap_skeleton_fit is the entry without one)", who);
    const bool fixed = rig->has_fixed_length != 0;
    EGO_CHECK(fixed || (state_in && state_out), "%s: null argument (state_in and state_out are required unless the rig has fixed_length)", who);
    if (fixed) state_in = nullptr, state_out = nullptr;      // neither read nor written
    const int P = rig->P;
    EGO_CHECK(T > 0 && S > 0 && P > 0, "%s: T, S and P must be positive (T = %d, S = %d, P = %d)", who, T, S, P);
    EGO_CHECK(P <= kSkelMaxRows, "%s: at most %d rows, one lane each (P = %d)", who, kSkelMaxRows, P);
    EGO_CHECK((int64_t)T * S <= INT32_MAX, "%s: T * S = %lld frames do not fit an int", who, (long long)T * S);
    EGO_CHECK((((uintptr_t)points | (uintptr_t)tracks) & 3) == 0, "%s: points and tracks must be 4-byte aligned", who);
    EGO_CHECK((((uintptr_t)rigid | (uintptr_t)rotations | (uintptr_t)lengths) & 15) == 0, "%s: rigid, rotations and lengths must be 16-byte aligned", who);
    EGO_CHECK((((uintptr_t)state_in | (uintptr_t)state_out) & 7) == 0, "%s: state_in and state_out must be 8-byte aligned", who);
    // the rig, and what the kernel takes of it
    SkelRigDev dev = {};
    dev.P = P;
    dev.has_fixed = fixed;
    int roots = 0;
    for (int j = 0; j < P; ++j) roots += rig->parent[j] == -1;
    EGO_CHECK(roots > 0, "%s: rig: no root row (parent -1)", who);
    for (int j = 0; j < P; ++j) {
        const int p = rig->parent[j];
        EGO_CHECK(p == -1 || (p >= 0 && p < j), "%s: rig: parent[%d] = %d: a parent is -1 (a root row) or an earlier row, 0 <= parent < row", who, j, p);
        dev.parent[j] = (int8_t)p;
        dev.mirror[j] = -1;
        dev.depth[j] = p < 0 ? 0 : (int8_t)(dev.depth[p] + 1);
        dev.max_depth = dev.depth[j] > dev.max_depth ? dev.depth[j] : dev.max_depth;
    }
    const int32_t* fr = rig->frame_rows;
    EGO_CHECK(fr[0] >= 0 && fr[0] < P && fr[1] >= 0 && fr[1] < P && fr[2] >= 0 && fr[2] < P && fr[0] != fr[1] && fr[0] != fr[2] && fr[1] != fr[2],
              "%s: rig: frame_rows are three distinct rows 0 .. %d (%d, %d, %d)", who, P - 1, fr[0], fr[1], fr[2]);
    dev.fa = fr[0], dev.fb = fr[1], dev.fc = fr[2];
    SkelVec rest[kSkelMaxRows];
    for (int j = 0; j < P; ++j)
        for (int c = 0; c < 3; ++c) {
            EGO_CHECK(ego_finite(rig->rest_pos[j][c]), "%s: rig: rest_pos[%d][%d] is not finite", who, j, c);
            rest[j].v[c] = rig->rest_pos[j][c];
        }
    for (int j = 0; j < P; ++j) {
        if (dev.parent[j] < 0) continue;
        const SkelVec &a = rest[j], &b = rest[dev.parent[j]], d = {{a.v[0] - b.v[0], a.v[1] - b.v[1], a.v[2] - b.v[2]}};
        const double n = skel_norm3(d);
        EGO_CHECK(skel_pos_finite(n), "%s: rig: the rest bone of row %d has length %g: a zero or non-finite rest bone has no direction", who, j, n);
        for (int c = 0; c < 3; ++c) dev.rest_dir[j][c] = d.v[c] / n;
    }
    SkelVec frame[3];
    EGO_CHECK(skel_frame(rest[fr[0]], rest[fr[1]], rest[fr[2]], frame), "%s: rig: the rest pose's triangle of rows (%d, %d, %d) is degenerate", who, fr[0], fr[1],
              fr[2]);
    for (int k = 0; k < 3; ++k)
        for (int c = 0; c < 3; ++c) dev.rest_frame[k][c] = frame[k].v[c];
    if (rig->has_mirror)
        for (int j = 0; j < P; ++j) {
            const int m = rig->mirror[j];
            if (m == -1) continue;
            EGO_CHECK(m >= 0 && m < P && rig->mirror[m] == j, "%s: rig: mirror[%d] = %d is not an involution (mirror[mirror[j]] == j, or -1)", who, j, m);
            EGO_CHECK(dev.parent[j] >= 0 && dev.parent[m] >= 0, "%s: rig: mirror[%d] = %d pairs a root row, which has no bone", who, j, m);
            dev.mirror[j] = (int8_t)m;
        }
    if (fixed)
        for (int j = 0; j < P; ++j) {
            if (dev.parent[j] < 0) continue;
            EGO_CHECK(skel_pos_finite(rig->fixed_length[j]), "%s: rig: fixed_length[%d] = %g must be finite and > 0", who, j, rig->fixed_length[j]);
            dev.fixed_length[j] = rig->fixed_length[j];
        }
    // the twist table, and what the kernel takes of it
    SkelTwistDev tw = {};
    if (with_twist) {
        EGO_CHECK(twist->bend_lo >= 0.0 && twist->bend_lo < twist->bend_hi && twist->bend_hi <= 1.0,
                  "%s: twist: 0 <= bend_lo < bend_hi <= 1, sines of the bend angle (bend_lo = %g, bend_hi = %g)", who, twist->bend_lo, twist->bend_hi);
        tw.bend_lo = twist->bend_lo, tw.bend_hi = twist->bend_hi;
        for (int j = 0; j < kSkelMaxRows; ++j) tw.pole[j] = -1;
        for (int j = 0; j < P; ++j) {
            const int c = twist->pole[j];
            if (c == -1) continue;
            EGO_CHECK(c >= 0 && c < P, "%s: twist: pole[%d] = %d is -1 or a row 0 .. %d", who, j, c, P - 1);
            EGO_CHECK(dev.parent[j] >= 0, "%s: twist: pole[%d] = %d is set on a root row, which has no bone to roll", who, j, c);
            EGO_CHECK(dev.parent[c] == j, "%s: twist: pole[%d] = %d: the pole of a row is one of its children (parent[%d] = %d)", who, j, c, c, dev.parent[c]);
            const double* h = twist->hinge[j];
            EGO_CHECK(ego_finite(h[0]) && ego_finite(h[1]) && ego_finite(h[2]), "%s: twist: hinge[%d] is not finite", who, j);
            const double* e = dev.rest_dir[j];
            const double dot = (h[0] * e[0] + h[1] * e[1]) + h[2] * e[2];
            const SkelVec g = {{h[0] - dot * e[0], h[1] - dot * e[1], h[2] - dot * e[2]}};
            const double n = skel_norm3(g);
            EGO_CHECK(n >= 1e-6 && skel_pos_finite(n), "%s: twist: hinge[%d] is (nearly) parallel to the rest bone of row %d: its part at right angles has norm %g < 1e-6",
                      who, j, j, n);
            tw.pole[j] = (int8_t)c;
            for (int k = 0; k < 3; ++k) tw.g[j][k] = g.v[k] / n;
        }
    }
    const egotap_skeleton_params& q = *params;
    EGO_CHECK(q.window >= 1, "%s: params: window must be at least 1 (%d)", who, q.window);
    EGO_CHECK(q.min_samples >= 0, "%s: params: min_samples must not be negative (%d)", who, q.min_samples);
    EGO_CHECK(q.max_dev >= 0.0, "%s: params: max_dev must be >= 0, +inf for off (%g)", who, q.max_dev);      // (a NaN fails the comparison)
    EGO_CHECK(!tracks || q.track_rows == 0 || q.track_rows >= P, "%s: params: track_rows = %d: tracks holds at least the P = %d rows (0: exactly P)", who,
              q.track_rows, P);
    const size_t B = (size_t)T * S, K = tracks && q.track_rows ? (size_t)q.track_rows : (size_t)P;
    const SkelParamsDev prm = {(double)q.window, (double)q.min_samples, q.max_dev, q.freeze != 0, (int32_t)K};
    const struct {
        const char* name;
        const void* p;
        size_t n;
    } in[3] = {{"points", points, B * P * 12}, {"tracks", tracks, B * K * 32}, {"state_in", state_in, (size_t)S * P * 16}},
      out[4] = {{"state_out", state_out, (size_t)S * P * 16}, {"rigid", rigid, B * P * 16}, {"rotations", rotations, B * P * 32}, {"lengths", lengths, B * P * 8}};
    for (int o = 0; o < 4; ++o) {      // (with fixed_length the states are NULL: they overlap nothing)
        for (int i = 0; i < 3; ++i) {
            if (o == 0 && i == 2 && state_out == state_in) continue;      // in place
            EGO_CHECK(!ego_overlap(out[o].p, out[o].n, in[i].p, in[i].n), "%s: %s overlaps %s", who, out[o].name, in[i].name);
        }
        for (int p = o + 1; p < 4; ++p) EGO_CHECK(!ego_overlap(out[o].p, out[o].n, out[p].p, out[p].n), "%s: %s overlaps %s", who, out[o].name, out[p].name);
    }
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, with_twist ? "skeleton_fit_twist" : "skeleton_fit", "skeleton_fit_kernel", 0.0);
    if (with_twist)
        EGO_HIP(skeleton_fit_launch(points, tracks, T, S, dev, tw, prm, state_in, state_out, rigid, rotations, lengths, (hipStream_t)stream));
    else
        EGO_HIP(skeleton_fit_launch(points, tracks, T, S, dev, SkelNoTwist{}, prm, state_in, state_out, rigid, rotations, lengths, (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_skeleton_fit(const float* points, const float* tracks, int T, int S, const egotap_skeleton_rig* rig, const egotap_skeleton_params* params,
                                   const double* state_in, double* state_out, float* rigid, float* rotations, float* lengths, void* stream) {
    return skeleton_fit_entry("egotap_skeleton_fit", false, points, tracks, T, S, rig, nullptr, params, state_in, state_out, rigid, rotations, lengths, stream);
}
extern "C" int egotap_skeleton_fit_twist(const float* points, const float* tracks, int T, int S, const egotap_skeleton_rig* rig, const egotap_skeleton_twist* twist,
                                         const egotap_skeleton_params* params, const double* state_in, double* state_out, float* rigid, float* rotations,
                                         float* lengths, void* stream) {
    return skeleton_fit_entry("egotap_skeleton_fit_twist", true, points, tracks, T, S, rig, twist, params, state_in, state_out, rigid, rotations, lengths, stream);
}

extern "C" int egotap_debug_predict_pose_rgb_form(egotap_handle h, int* form) {
    EGO_CHECK(h && form, "egotap_debug_predict_pose_rgb_form: null argument");
    *form = h->rgb_form;
    return EGOTAP_OK;
}
extern "C" int egotap_debug_predict_pose_rgb_intermediate(egotap_handle h, int B, int chunk, const char* name, size_t* offset, int64_t* numel) {
    EGO_CHECK(h && name && offset && numel, "egotap_debug_predict_pose_rgb_intermediate: null argument");
    EGO_CHECK(B > 0 && chunk >= 0, "egotap_debug_predict_pose_rgb_intermediate: the batch must be positive, the chunk not negative");
    EGO_CHECK(!strcmp(name, "heatmaps") || !strcmp(name, "handoff"), "egotap_debug_predict_pose_rgb_intermediate: unknown intermediate '%s' (heatmaps, handoff)", name);
    *offset = rgb_ws(h, B, chunk, RGB_SRC_F32).HM;
    *numel = (int64_t)B * h->C * h->cfg.hm_size * h->cfg.hm_size;
    return EGOTAP_OK;
}

// ---- [r5] batch-statistics forward of a frozen estimator on the bf16 channels-last kernels (train.py:91; egotap_autoencoder_model.py:127-129, 177-216)
struct HmBnWs {
    size_t P0, S[4][4], T4, C3, Y3, C2, Y2, C1, Y1, WALL, DEC, ZP, SPLIT, PART, SC, SH, ONES, ZEROS, total;
};
static constexpr size_t HM_BN_SPLIT_FLOATS = (size_t)1 << 24;      // split-K partials of the backbone: tiles x splits <= CUs x 65536 floats
static HmBnWs hm_bn_ws(const Handle* h, int B, int chunk) {
    HmBnWs w;
    const size_t S0 = (size_t)h->cfg.hm_size * 4, s64 = S0 / 4, s32 = S0 / 8, s16 = S0 / 16, s8 = S0 / 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = al256(o + bytes); return r; };
    constexpr size_t ZT = 256;                                  // the zero page behind every map a 3x3 convolution reads (hm_zero_tail)
    w.P0 = take((size_t)B * s64 * s64 * 128 * 2 + ZT);
    for (int i = 0; i < 4; ++i) {
        const size_t side = S0 / (4u << i), bytes = (size_t)B * side * side * 2 * HM_CH[i] * 2;
        for (int k = 0; k < 4; ++k) w.S[i][k] = take(bytes + ZT);
    }
    const size_t c = (size_t)chunk;
    w.T4 = take(c * s8 * s8 * 1024 * 2);
    w.C3 = take(c * s16 * s16 * HM_CAT3P * 2 + ZT); w.Y3 = take(c * s16 * s16 * 1024 * 2);
    w.C2 = take(c * s32 * s32 * 1280 * 2 + ZT);     w.Y2 = take(c * s32 * s32 * 512 * 2);
    w.C1 = take(c * s64 * s64 * 640 * 2 + ZT);      w.Y1 = take(c * s64 * s64 * 512 * 2);
    const int nblk_[4] = {hm_nblk(h, 0), hm_nblk(h, 1), hm_nblk(h, 2), hm_nblk(h, 3)};
    w.WALL = take(hm_pack_plan(nullptr, nblk_, nullptr) + 256);
    w.DEC = take((size_t)40 << 20);
    w.ZP = take(256);
    w.SPLIT = take(HM_BN_SPLIT_FLOATS * 4);
    w.PART = take(BnBatchScratch::part_floats() * 4);
    w.SC = take(4096); w.SH = take(4096); w.ONES = take(4096); w.ZEROS = take(4096);
    w.total = o;
    return w;
}
static __global__ __launch_bounds__(256) void fill_f32_kernel(float* __restrict__ p, float v, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

extern "C" int egotap_hm_forward_bnbatch_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes) {
    EGO_CHECK(h && bytes, "null argument");
    EGO_CHECK(B >= 0 && chunk >= 0, "negative batch or chunk");
    const int b = B > 0 ? B : 1;
    *bytes = hm_bn_ws(h, b, chunk > 0 && chunk < b ? chunk : b).total;
    return EGOTAP_OK;
}

extern "C" int egotap_hm_forward_bnbatch_intermediate(egotap_handle h, int B, int chunk, const char* name, size_t* offset, int64_t* numel) {
    EGO_CHECK(h && name && offset && numel, "null argument");
    EGO_CHECK(B >= 1, "batch");
    const HmBnWs w = hm_bn_ws(h, B, chunk > 0 && chunk < B ? chunk : B);
    const int64_t S0 = h->cfg.hm_size * 4;
    auto px = [&](int i) { const int64_t side = S0 / (4 << i); return (int64_t)B * side * side; };
    if (!strcmp(name, "pool0")) { *offset = w.P0; *numel = px(0) * 128; }
    else if (!strcmp(name, "layer1")) { *offset = w.S[0][0]; *numel = px(0) * 2 * HM_CH[0]; }
    else if (!strcmp(name, "layer2")) { *offset = w.S[1][0]; *numel = px(1) * 2 * HM_CH[1]; }
    else if (!strcmp(name, "layer3")) { *offset = w.S[2][0]; *numel = px(2) * 2 * HM_CH[2]; }
    else if (!strcmp(name, "layer4")) { *offset = w.S[3][0]; *numel = px(3) * 2 * HM_CH[3]; }
    else { egotap_set_error("unknown intermediate '%s'", name); return EGOTAP_ERR_INVALID; }
    return EGOTAP_OK;
}

extern "C" int egotap_hm_forward_bnbatch(egotap_handle h, int net, const float* left, const float* right, int B, float* out, int64_t out_image_stride, int chunk,
                                         void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(net == EGOTAP_NET_HM_POS || net == EGOTAP_NET_HM_ROT, "egotap_hm_forward_bnbatch: net must be EGOTAP_NET_HM_POS or _ROT");
    EGO_CHECK(h->precision == EGOTAP_PREC_BF16, "egotap_hm_forward_bnbatch runs on the bf16 channels-last kernels: egotap_set_precision(EGOTAP_PREC_BF16) first "
              "(fp32 / bf16x3: compose the train-mode forward from egotap_hmtrain_conv_fwd + egotap_hmtrain_bn2d_fwd)");
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(B >= 2, "batch-statistics BatchNorm needs more than one value per channel and every map has them only from two frames on at the deepest level "
              "(torch raises for one 1 x 1 map; keep B >= 2)");
    EGO_CHECK(left && right && out && ws, "egotap_hm_forward_bnbatch: null argument");
    EGO_CHECK((((uintptr_t)left | (uintptr_t)right | (uintptr_t)out) & 15) == 0 && ((uintptr_t)ws & 255) == 0, "pointers must be 16-byte (ws: 256-byte) aligned");
    const int S0 = h->cfg.hm_size * 4, s64 = S0 / 4, s32 = S0 / 8, s16 = S0 / 16, s8 = S0 / 32;
    EGO_CHECK(s64 == 64 || s64 == 128, "egotap_hm_forward_bnbatch runs at heatmap sides 64 and 128 only (256x256 / 512x512 RGB); this handle's side is %d "
              "(the eval-mode egotap_hm_forward runs at every multiple of 16)", s64);
    if (chunk <= 0 || chunk > B) chunk = B;
    int rc = hm_resolve(h, net);
    if (rc != EGOTAP_OK) return rc;
    const HmBnWs w = hm_bn_ws(h, B, chunk);
    if (ws_bytes < w.total) {
        egotap_set_error("workspace too small: %zu bytes given, %zu needed for B=%d, chunk=%d", ws_bytes, w.total, B, chunk);
        return EGOTAP_ERR_WORKSPACE;
    }
    const HmParams& p = h->hp[net];
    EGO_CHECK(out_image_stride >= (int64_t)p.n_out * s64 * s64, "out_image_stride smaller than the output image");
    hipStream_t s = (hipStream_t)stream;
    char* base = (char*)ws;
    auto Hb = [&](size_t off) { return (__bf16*)(base + off); };
    HmBf16Bufs q{};
    q.P0 = Hb(w.P0);
    for (int i = 0; i < 4; ++i) { q.A[i] = Hb(w.S[i][0]); q.Ta[i] = Hb(w.S[i][1]); q.Tb[i] = Hb(w.S[i][2]); q.Td[i] = Hb(w.S[i][3]); }
    q.T4 = Hb(w.T4); q.C3 = Hb(w.C3); q.Y3 = Hb(w.Y3); q.C2 = Hb(w.C2); q.Y2 = Hb(w.Y2); q.C1 = Hb(w.C1); q.Y1 = Hb(w.Y1);
    q.ZP = Hb(w.ZP);
    q.reg = base + w.WALL;
    q.split_slab = (float*)(base + w.SPLIT); q.split_floats = HM_BN_SPLIT_FLOATS;
    q.dec_slab = (float*)(base + w.DEC);     q.dec_split_floats = ((size_t)40 << 20) / 4;
    q.ones = (const float*)(base + w.ONES);  q.zeros = (const float*)(base + w.ZEROS);
    HmBnBatch bnb{BnBatchScratch{(float*)(base + w.PART), (float*)(base + w.SC), (float*)(base + w.SH)}};
    const int cus = device_cu_count();
    EGO_HIP(zero_fill(q.ZP, 256, s));
    EGO_HIP(zero_fill((void*)q.zeros, 4096, s));
    hipLaunchKernelGGL(fill_f32_kernel, dim3(4), dim3(256), 0, s, (float*)q.ones, 1.f, 1024);
    EGO_HIP(hipGetLastError());
    PackTable PT;
    const int stage_sides[4] = {s64, s32, s16, s8};
    EGO_CHECK(hm_pack_plan(&p, p.nblk, &PT, 2L * B, stage_sides, cus, q.split_floats, q.dec_split_floats, 2L * chunk) != 0,
              "egotap_hm_forward_bnbatch: the estimator has more layers than the pack table holds");
    hipLaunchKernelGGL(pack_all_bf16s_kernel, dim3(PT.blocks), dim3(256), 0, s, PT, q.reg);      // (its eval-mode BatchNorm folds are written and not read here)
    EGO_HIP(hipGetLastError());
    int li = 0, bi = 0;
    EGO_HIP(hm_bf16_backbone(h, p, PT, li, bi, q, left, right, B, S0, &bnb, s));      // whole batch: the statistics couple its frames
    EGO_CHECK(bi == PT.nb, "egotap_hm_forward_bnbatch: pack plan out of step with the forward");
    const long px[4] = {(long)s64 * s64, (long)s32 * s32, (long)s16 * s16, (long)s8 * s8};
    for (int lo = 0; lo < B; lo += chunk) {                                             // the decoder has no BatchNorm: chunks keep its scratch small
        const int bc = B - lo < chunk ? B - lo : chunk;
        const __bf16* lv[4];
        for (int i = 0; i < 4; ++i) lv[i] = q.A[i] + (size_t)lo * px[i] * 2 * HM_CH[i];
        EGO_HIP(hm_bf16_decoder(h, p, PT, li, q, lv, bc, S0, out + (size_t)lo * out_image_stride, out_image_stride, s));
    }
    return EGOTAP_OK;
}

// ------------------------------------------------------------------------------------------------ single operators
template <class Cfg>
static hipError_t linear_tile(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int epi,
                              const float* r, const float* g, const float* beta, const float* mean, const float* var,
                              hipStream_t s) {
    const ALoadPlain al{x, K};
    const SegMat W = segmat1(w, N, K);
    switch (epi) {
        case 0: return gemm_f32_launch<Cfg>(al, W, EpiBias{segvec1(b, N)}, y, N, M, N, K, s);
        case 1: return gemm_f32_launch<Cfg>(al, W, EpiBiasRes{segvec1(b, N), r, N}, y, N, M, N, K, s);
        case 2: return gemm_f32_launch<Cfg>(al, W, EpiBiasGelu{segvec1(b, N)}, y, N, M, N, K, s);
        case 3: return gemm_f32_launch<Cfg>(al, W, EpiBnLrelu{b, g, beta, mean, var, 1e-5f, 0.2f}, y, N, M, N, K, s);
        default: return hipErrorInvalidValue;
    }
}

extern "C" int egotap_linear_f32(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int epi,
                                 const float* r, const float* g, const float* beta, const float* mean, const float* var,
                                 int tile, void* stream) {
    EGO_CHECK(x && w && b && y, "egotap_linear_f32: null argument");
    EGO_CHECK(M >= 0 && N > 0 && K > 0, "egotap_linear_f32: bad shape");
    EGO_CHECK(epi >= 0 && epi <= 3, "egotap_linear_f32: epi must be 0..3");
    EGO_CHECK(epi != 1 || r, "egotap_linear_f32: residual pointer missing");
    EGO_CHECK(epi != 3 || (g && beta && mean && var), "egotap_linear_f32: BatchNorm pointers missing");
    hipStream_t s = (hipStream_t)stream;
    hipError_t e;
    if (tile != 0 && tile != 1 && epi != 0) { egotap_set_error("non-default tiles are built for epi 0 only"); return EGOTAP_ERR_INVALID; }
    switch (tile) {
        case 0: case 1: e = linear_tile<TileA>(x, w, b, y, M, N, K, epi, r, g, beta, mean, var, s); break;
        case 2: e = gemm_f32_launch<TileB>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 3: e = gemm_f32_launch<TileC>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 4: e = gemm_f32_launch<TileD>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 5: e = gemm_f32_launch<TileE>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 6: e = gemm_f32_launch<TileF>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 7: e = gemm_f32_launch<TileG>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 8: e = gemm_f32_pipe_launch<PipeA>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 9: e = gemm_f32_pipe_launch<PipeB>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 10: e = gemm_f32_pipe_launch<PipeC>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 11: e = gemm_f32_pipe_launch<PipeD>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, s); break;
        case 12: e = gemm_f32_persist_launch<PipeD>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        case 13: e = gemm_bf16_persist_launch<BfCfg<3>>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        case 14: e = gemm_bf16_persist_launch<BfCfg<1>>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        case 15: e = gemm_bf16_persist_launch<BfCfg<3, 1>>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        case 16: e = gemm_bf16_persist_launch<BfCfg<1, 1>>(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        case 19: e = gemm_f32_dma_launch(ALoadPlain{x, K}, segmat1(w, N, K), EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), s); break;
        default: egotap_set_error("unknown tile id %d", tile); return EGOTAP_ERR_INVALID;
    }
    if (e == hipErrorInvalidValue) {
        egotap_set_error("egotap_linear_f32: N=%d / K=%d not a multiple of the tile (%s)", N, K, egotap_gemm_tile_name(tile));
        return EGOTAP_ERR_INVALID;
    }
    EGO_HIP(e);
    return EGOTAP_OK;
}

// y = x w^T + b on gemm_bf16_dma_kernel with CALLER-OWNED bf16 copies of both operands (x [M,K], w [N,K], row-major) -- the
// kernel the plain-bf16 mode runs after rounding its operands; exported for the operator tests
extern "C" int egotap_linear_bf16_dma(const void* x_bf16, const void* w_bf16, const float* b, float* y, int M, int N, int K, void* stream) {
    EGO_CHECK(x_bf16 && w_bf16 && b && y, "egotap_linear_bf16_dma: null argument");
    EGO_CHECK(M >= 0 && N > 0 && K > 0 && K % 8 == 0, "egotap_linear_bf16_dma: bad shape (K must be a multiple of 8)");
    EGO_CHECK((((uintptr_t)x_bf16 | (uintptr_t)w_bf16) & 15) == 0, "egotap_linear_bf16_dma: operands must be 16-byte aligned");
    SegMatB Bm;
    for (int i = 0; i < 3; ++i) Bm.p[i] = (const __bf16*)w_bf16;
    Bm.seg = N; Bm.ld = K;
    hipError_t e = gemm_bf16_dma_launch((const __bf16*)x_bf16, (long)K, Bm, EpiBias{segvec1(b, N)}, y, N, M, N, K, device_cu_count(), (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_linear_bf16_dma: N=%d / K=%d not a multiple of the 256 x 256 x 32 tile", N, K); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_layernorm_f32(const float* x, float* y, const float* gamma, const float* beta, int rows, int dim,
                                    float eps, void* stream) {
    EGO_CHECK(x && y && gamma && beta, "egotap_layernorm_f32: null argument");
    EGO_CHECK(dim == 1024, "egotap_layernorm_f32: dim must be 1024 (ViT hidden size)");
    EGO_HIP(launch_ln(x, y, gamma, beta, rows, eps, (hipStream_t)stream));
    return EGOTAP_OK;
}

extern "C" int egotap_attention_f32(const float* qkv, float* ctx, int B, int N, int heads, void* stream) {
    EGO_CHECK(qkv && ctx, "egotap_attention_f32: null argument");
    EGO_CHECK(N >= 32 && N % 4 == 0, "egotap_attention_f32: sequence length must be at least 32 and a multiple of 4 (any heatmap side that is a multiple of 16)");
    EGO_CHECK(heads > 0, "egotap_attention_f32: heads must be positive");
    EGO_HIP(attention_f32_launch(qkv, ctx, B, N, heads, (hipStream_t)stream));
    return EGOTAP_OK;
}

// (test hook) the exact-fp32 attention with the tokens from shared_from on read from image 0's rows: layer 0 of the pose-only forward
extern "C" int egotap_debug_attention_f32_shared(const float* qkv, float* ctx, int B, int N, int heads, int shared_from, void* stream) {
    EGO_CHECK(qkv && ctx, "egotap_debug_attention_f32_shared: null argument");
    EGO_CHECK(B >= 0 && N >= 32 && N % 4 == 0 && heads > 0, "egotap_debug_attention_f32_shared: bad shape B=%d N=%d heads=%d", B, N, heads);
    EGO_CHECK(shared_from > 0 && shared_from <= N && (shared_from == N || (N % 32 == 0 && shared_from % 32 == 0)),
              "egotap_debug_attention_f32_shared: shared_from=%d must be N, or a multiple of 32 below N with N a multiple of 32", shared_from);
    EGO_HIP(attention_f32_shared_launch(qkv, ctx, B, N, heads, shared_from, (hipStream_t)stream));
    return EGOTAP_OK;
}

// (test hook) the exact-fp32 attention as lift_forward launches it: with the caller's scratch for the key-split partials, the split count being
// attention_f32_ksplit's own decision for scratch_floats and num_cu (egotap_debug_attention_f32_ksplit tells which)
extern "C" int egotap_debug_attention_f32_split(const float* qkv, float* ctx, int B, int N, int heads, float* scratch, size_t scratch_floats, int num_cu, void* stream) {
    EGO_CHECK(qkv && ctx && scratch, "egotap_debug_attention_f32_split: null argument");
    EGO_CHECK(B >= 0 && N >= 32 && N % 4 == 0 && heads > 0, "egotap_debug_attention_f32_split: bad shape B=%d N=%d heads=%d (N at least 32 and a multiple of 4)", B, N, heads);
    EGO_CHECK(num_cu > 0, "egotap_debug_attention_f32_split: num_cu=%d must be positive", num_cu);
    EGO_HIP(attention_f32_launch(qkv, ctx, B, N, heads, (hipStream_t)stream, nullptr, scratch, scratch_floats, num_cu));
    return EGOTAP_OK;
}

// (test hook) the live-query attention of the pose-only forward's last layer: Nq compact query rows per image (row b * Nq + q of q, stride ldq)
// against the K / V columns of all N tokens of qkv; ctx [B * Nq, heads * 128]
extern "C" int egotap_debug_attention_f32_live(const float* q, int64_t ldq, int Nq, const float* qkv, float* ctx, int B, int N, int heads, void* stream) {
    EGO_CHECK(q && qkv && ctx, "egotap_debug_attention_f32_live: null argument");
    EGO_CHECK(B >= 0 && N >= 32 && N % 4 == 0 && heads > 0, "egotap_debug_attention_f32_live: bad shape B=%d N=%d heads=%d (N at least 32 and a multiple of 4)", B, N, heads);
    EGO_CHECK(Nq >= 32 && Nq <= N, "egotap_debug_attention_f32_live: Nq=%d must lie in [32, N=%d]", Nq, N);
    EGO_CHECK(ldq >= (int64_t)heads * 128 && ldq % 4 == 0, "egotap_debug_attention_f32_live: ldq=%lld must be a multiple of 4 and at least heads * 128", (long long)ldq);
    EGO_HIP(attention_f32_live_launch(q, (long)ldq, Nq, qkv, ctx, B, N, heads, (hipStream_t)stream));
    return EGOTAP_OK;
}

// (test aid, host only: no device call) the key-split count attention_f32_launch picks for a forward with scratch_floats of scratch on num_cu
// compute units: 1 = unsplit.  0 (never a split count) with egotap_last_error set where the arguments are refused
extern "C" int egotap_debug_attention_f32_ksplit(int B, int N, int heads, size_t scratch_floats, int num_cu) {
    if (!(B > 0 && N >= 32 && N % 4 == 0 && heads > 0)) {
        egotap_set_error("egotap_debug_attention_f32_ksplit: bad shape B=%d N=%d heads=%d (N at least 32 and a multiple of 4)", B, N, heads);
        return 0;
    }
    if (num_cu <= 0) {
        egotap_set_error("egotap_debug_attention_f32_ksplit: num_cu=%d must be positive", num_cu);
        return 0;
    }
    return attention_f32_ksplit(B, N, heads, scratch_floats, num_cu);
}

// per-sample MPJPE / PA-MPJPE of a batch of poses (egotap_autoencoder_model.py:329-350, utils/util.py:328-379)
extern "C" int egotap_pose_metrics(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pa_mpjpe, float* aligned,
                                   void* stream) {
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(pred && gt && mpjpe && pa_mpjpe, "egotap_pose_metrics: null argument");
    EGO_CHECK(B > 0 && J >= 1 && J <= EGOTAP_MAX_JOINTS, "egotap_pose_metrics: bad shape B=%d J=%d", B, J);
    hipLaunchKernelGGL(pose_metrics_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, pred, gt, B, J, mpjpe, pa_mpjpe, aligned);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

// the same metrics as the reference computes them for a batch of 2 or 3 frames (utils/util.py:337 skips its transpose there)
extern "C" int egotap_pose_metrics_batch_axes(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pa_mpjpe, float* aligned,
                                              void* stream) {
    EGO_CHECK(pred && gt && mpjpe && pa_mpjpe, "egotap_pose_metrics_batch_axes: null argument");
    EGO_CHECK((B == 2 || B == 3) && J >= 1 && J <= EGOTAP_MAX_JOINTS,
              "egotap_pose_metrics_batch_axes: the reference takes this branch for batches of 2 or 3 frames only (B=%d J=%d)", B, J);
    hipLaunchKernelGGL(pose_metrics_batch_axes_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, pred, gt, B, J, mpjpe, pa_mpjpe, aligned);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

// joints -> ground-truth heatmaps in the lifting head's input layout (dataloader/data_loader.py:76-215 with --use_gt_heatmap)
extern "C" int egotap_synth_heatmaps(const float* pts2d_left, const float* pts2d_right, const float* pose3d, const int* parents, int B,
                                     int J, int res, float* hm, float* plength, float* theta, void* stream) {
    if (B == 0) return EGOTAP_OK;
    EGO_CHECK(pts2d_left && pts2d_right && pose3d && parents && hm, "egotap_synth_heatmaps: null argument");
    EGO_CHECK(B > 0 && J >= 1 && J <= 64 && res >= 16 && res <= 128, "egotap_synth_heatmaps: bad shape B=%d J=%d res=%d", B, J, res);
    GaussTaps g;                                   // scipy.ndimage._gaussian_kernel1d(sigma = 1, order 0, radius 4)
    double sum = 0.0;
    for (int k = -4; k <= 4; ++k) { g.w[k + 4] = exp(-0.5 * k * k); sum += g.w[k + 4]; }
    for (int k = 0; k < 9; ++k) g.w[k] /= sum;
    const size_t lds = (size_t)2 * res * res * 4;
    EGO_HIP(ego_allow_dynamic_lds((const void*)heatmap_synth_kernel, 2 * 128 * 128 * 4));
    hipLaunchKernelGGL(heatmap_synth_kernel, dim3(B * 2 * J), dim3(256), lds, (hipStream_t)stream, pts2d_left, pts2d_right, pose3d, parents,
                       B, J, res, g, hm, plength, theta);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

// same operator with the arithmetic of egotap_set_precision (EGOTAP_PREC_*): fp32 MFMA, bf16x3 split or plain bf16
extern "C" int egotap_attention(const float* qkv, float* ctx, int B, int N, int heads, int precision, void* stream) {
    EGO_CHECK(qkv && ctx, "egotap_attention: null argument");
    EGO_CHECK(N >= 32 && N % 4 == 0, "egotap_attention: sequence length must be at least 32 and a multiple of 4");
    EGO_CHECK(heads > 0, "egotap_attention: heads must be positive");
    // [r5] the bf16 / bf16x3 kernels tile the sequence in whole 32-key blocks; sequence lengths that are not (heatmap sides 32, 48, 96 ...: the
    // reference allows every multiple of 16) run on the exact-fp32 kernel, which masks the last key tile -- a FALLBACK BY NAME, documented in egotap.h
    if (precision == EGOTAP_PREC_F32 || N % 32 != 0) EGO_HIP(attention_f32_launch(qkv, ctx, B, N, heads, (hipStream_t)stream));
    else if (precision == EGOTAP_PREC_BF16X3) EGO_HIP(attention_bf16_launch<3>(qkv, ctx, B, N, heads, (hipStream_t)stream));
    else if (precision == EGOTAP_PREC_BF16) EGO_HIP(attention_bf16_launch<1>(qkv, ctx, B, N, heads, (hipStream_t)stream));
    else { egotap_set_error("egotap_attention: unknown precision %d", precision); return EGOTAP_ERR_INVALID; }
    return EGOTAP_OK;
}
#endif

#if EGOTAP_IN(1)
#include "abi_train_lift.inc"
#endif

#if EGOTAP_IN(2)
// ================================================================================================ heatmap-estimator training
// Building blocks of one optimisation step of the stage-1 model (model/heatmap_shared_model.py:98-172: HeatMap_UnrealEgo_Shared
// in train mode, MSE losses, Adam), called by the autograd glue in egotap_amd/hm_training.py.  All tensors are caller-owned
// NCHW fp32 device buffers with explicit image strides (so concat slices are read and written in place).

// scratch for the repacked weights of the bf16 convolution kernels when the training operators run under a bf16 precision mode
// (egotap_hm_forward takes it from its workspace); bytes >= egotap_hmtrain_pack_bytes()
extern "C" int egotap_hmtrain_set_pack_buffer(egotap_handle h, void* buf, size_t bytes) {
    EGO_CHECK(h, "null handle");
    EGO_CHECK(buf == nullptr || bytes >= conv_bf16_pack_bytes(1024, 1540), "egotap_hmtrain_set_pack_buffer: buffer too small");
    EGO_CHECK(((uintptr_t)buf & 15) == 0, "egotap_hmtrain_set_pack_buffer: 16-byte alignment");
    h->conv_pack = (__bf16*)buf;
    return EGOTAP_OK;
}
extern "C" size_t egotap_hmtrain_pack_bytes(void) { return conv_bf16_pack_bytes(1024, 1540); }

extern "C" int egotap_hmtrain_conv_fwd(egotap_handle h, const float* x, const float* w, const float* bias, const float* res, float* y,
                                       int Nimg, int Cin, int Cout, int wout, int taps, int stride, int relu, int64_t in_istride,
                                       int64_t out_istride, int64_t res_istride, void* stream) {
    EGO_CHECK(h && x && w && bias && y, "egotap_hmtrain_conv_fwd: null argument");
    ConvArgs a{x, w, y, res, nullptr, nullptr, nullptr, nullptr, bias, in_istride, out_istride, res_istride, Nimg, Cin, Cout, relu, 0, 0};
    hipError_t e = conv_any(h, "hmtrain.conv", taps, stride, wout, a, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_hmtrain_conv_fwd: unsupported conv taps=%d stride=%d wout=%d Cin=%d Cout=%d", taps, stride, wout, Cin, Cout); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

// [r3] Eval-mode building blocks for the backbones the one-call forward does not cover (the Bottleneck ResNets of --model_name resnet50 /
// resnet101, net_architecture.py:61-64): y = [relu](BatchNorm_eval(conv(x, w)) [+ res]) on the fp32 convolution kernels, BatchNorm folded
// in the epilogue exactly as egotap_hm_forward folds it (gamma / sqrt(var + 1e-5)), and the stem with its BatchNorm + ReLU.
extern "C" int egotap_hm_conv_bn_fwd(egotap_handle h, const float* x, const float* w, const float* gamma, const float* beta, const float* mean,
                                     const float* var, const float* res, float* y, int Nimg, int Cin, int Cout, int wout, int taps, int stride,
                                     int relu, int64_t in_istride, int64_t out_istride, int64_t res_istride, void* stream) {
    EGO_CHECK(h && x && w && gamma && beta && mean && var && y, "egotap_hm_conv_bn_fwd: null argument");
    ConvArgs a{x, w, y, res, gamma, beta, mean, var, nullptr, in_istride, out_istride, res_istride, Nimg, Cin, Cout, relu, 0, 0};
    hipError_t e = conv_any(h, "hm.conv_bn", taps, stride, wout, a, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_hm_conv_bn_fwd: unsupported conv taps=%d stride=%d wout=%d Cin=%d Cout=%d", taps, stride, wout, Cin, Cout); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    return EGOTAP_OK;
}
extern "C" int egotap_hm_stem_bn_fwd(const float* left, const float* right, const float* w, const float* gamma, const float* beta, const float* mean,
                                     const float* var, float* y, int B, int S0, void* stream) {
    EGO_CHECK(left && right && w && gamma && beta && mean && var && y && B > 0 && S0 % 32 == 0, "egotap_hm_stem_bn_fwd: bad argument");
    EGO_HIP(stem_conv7_launch(left, right, w, gamma, beta, mean, var, y, S0, 2 * B, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}

// conv 7x7 / 2 of the ResNet stem without BatchNorm: z [2B, 64, S0/2, S0/2], image n = 2b + eye
extern "C" int egotap_hmtrain_stem_fwd(const float* left, const float* right, const float* w, float* z, int B, int S0, void* stream) {
    EGO_CHECK(left && right && w && z && B > 0 && S0 % 32 == 0, "egotap_hmtrain_stem_fwd: bad argument");
    EGO_HIP(stem_conv7_launch(left, right, w, nullptr, nullptr, nullptr, nullptr, z, S0, 2 * B, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}

static int bn_splits(int N, int C) { int s = (1024 + C - 1) / C; if (s > N) s = N; if (s < 1) s = 1; return s; }

extern "C" int egotap_hmtrain_bn2d_fwd(const float* z, float* y, const float* res, const float* gamma, const float* beta, float* mean, float* rstd,
                                       float* run_mean, float* run_var, int N, int C, int HW, int64_t z_istride, int64_t y_istride,
                                       int64_t res_istride, int relu, float eps, float momentum, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(z && y && gamma && beta && mean && rstd && ws, "egotap_hmtrain_bn2d_fwd: null argument");
    EGO_CHECK(HW % 4 == 0 && N > 0 && C > 0, "egotap_hmtrain_bn2d_fwd: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int splits = bn_splits(N, C), per = (N + splits - 1) / splits;
    EGO_CHECK((size_t)splits * C * 2 * 8 <= ws_bytes, "egotap_hmtrain_bn2d_fwd: workspace too small");
    hipLaunchKernelGGL(chan_sums_kernel<0>, dim3(C, splits), dim3(256), 0, s, z, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (double*)ws, N, C, HW, (long)z_istride, (long)z_istride, 0, per);
    hipLaunchKernelGGL(bn2d_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const double*)ws, splits, C, (double)N * HW, eps, momentum, mean, rstd,
                       run_mean, run_var);
    const long total = (long)N * C * (HW / 4);
    hipLaunchKernelGGL(bn2d_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, y, res, gamma, beta, (const float*)mean, (const float*)rstd,
                       N, C, HW, (long)z_istride, (long)y_istride, (long)res_istride, relu);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_bn2d_bwd(const float* z, const float* y, const float* dy, const float* gamma, const float* mean, const float* rstd,
                                       float* dz, float* dres, float* dgamma, float* dbeta, int N, int C, int HW, int64_t z_istride,
                                       int64_t dy_istride, int relu, int accumulate, int dres_accumulate, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(z && dy && gamma && mean && rstd && dz && dgamma && dbeta && ws, "egotap_hmtrain_bn2d_bwd: null argument");
    EGO_CHECK(!relu || y, "egotap_hmtrain_bn2d_bwd: the ReLU mask needs y");
    EGO_CHECK(HW % 4 == 0 && N > 0 && C > 0, "egotap_hmtrain_bn2d_bwd: bad shape");
    hipStream_t s = (hipStream_t)stream;
    const int splits = bn_splits(N, C), per = (N + splits - 1) / splits;
    const size_t need = (size_t)splits * C * 2 * 8 + (size_t)C * 2 * 4;
    EGO_CHECK(need <= ws_bytes, "egotap_hmtrain_bn2d_bwd: workspace too small");
    double* part = (double*)ws;
    float* sums = (float*)((char*)ws + (size_t)splits * C * 2 * 8);
    hipLaunchKernelGGL(chan_sums_kernel<1>, dim3(C, splits), dim3(256), 0, s, dy, z, y, mean, rstd, part, N, C, HW, (long)dy_istride, (long)z_istride,
                       relu, per);
    hipLaunchKernelGGL(bn2d_bwd_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const double*)part, splits, C, sums, dgamma, dbeta, accumulate);
    const long total = (long)N * C * (HW / 4);
    hipLaunchKernelGGL(bn2d_bwd_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, z, y, dy, gamma, mean, rstd, (const float*)sums, dz, dres,
                       N, C, HW, (long)z_istride, (long)dy_istride, 1.0f / ((float)N * HW), relu, dres_accumulate);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

static __global__ void chansum_finish_kernel(const double* __restrict__ part, int splits, int C, float* __restrict__ out, int accumulate) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s0 = 0.0;
    for (int k = 0; k < splits; ++k) s0 += part[((long)k * C + c) * 2];
    out[c] = (accumulate ? out[c] : 0.f) + (float)s0;
}

// per-channel sums over N*H*W (bias gradients)
extern "C" int egotap_hmtrain_chansum(const float* dy, float* out, int N, int C, int HW, int64_t istride, int accumulate, void* ws, size_t ws_bytes,
                                      void* stream) {
    EGO_CHECK(dy && out && ws && HW % 4 == 0, "egotap_hmtrain_chansum: bad argument");
    hipStream_t s = (hipStream_t)stream;
    const int splits = bn_splits(N, C), per = (N + splits - 1) / splits;
    EGO_CHECK((size_t)splits * C * 2 * 8 <= ws_bytes, "egotap_hmtrain_chansum: workspace too small");
    hipLaunchKernelGGL(chan_sums_kernel<0>, dim3(C, splits), dim3(256), 0, s, dy, (const float*)nullptr, (const float*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (double*)ws, N, C, HW, (long)istride, (long)istride, 0, per);
    hipLaunchKernelGGL(chansum_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const double*)ws, splits, C, out, accumulate);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_conv_wt(const float* w, float* wt, int Cout, int Cin, int taps, void* stream) {
    EGO_CHECK(w && wt && Cout > 0 && Cin > 0 && taps > 0, "egotap_hmtrain_conv_wt: bad argument");
    const long total = (long)Cout * Cin * taps;
    hipLaunchKernelGGL(conv_wt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w, wt, Cout, Cin, taps);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_zero_upsample(const float* in, float* out, int N, int C, int H, int64_t in_istride, int64_t out_istride, void* stream) {
    EGO_CHECK(in && out && N > 0 && C > 0 && H > 0, "egotap_hmtrain_zero_upsample: bad argument");
    const long total = (long)N * C * 4 * H * H;
    hipLaunchKernelGGL(zero_upsample2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, in, out, (long)N * C, H,
                       (long)in_istride, (long)out_istride, C);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

template <int KS, int STRIDE, int CI_T>
static hipError_t wgrad_w(int wout, const WgArgs& a, float* dw, size_t sb, int acc, hipStream_t s) {
    const int cu = device_cu_count();
    switch (wout) {
        case 128: if constexpr (KS == 7) return conv_wgrad_launch<WgCfg<KS, STRIDE, 7, CI_T, 64>>(a, dw, sb, cu, acc, s); else return hipErrorInvalidValue;
        case 64: if constexpr (KS != 7 && STRIDE == 1) return conv_wgrad_launch<WgCfg<KS, STRIDE, 6, CI_T>>(a, dw, sb, cu, acc, s); else return hipErrorInvalidValue;
        case 32: if constexpr (KS != 7) return conv_wgrad_launch<WgCfg<KS, STRIDE, 5, CI_T>>(a, dw, sb, cu, acc, s); else return hipErrorInvalidValue;
        case 16: if constexpr (KS != 7) return conv_wgrad_launch<WgCfg<KS, STRIDE, 4, CI_T>>(a, dw, sb, cu, acc, s); else return hipErrorInvalidValue;
        case 8: if constexpr (KS != 7) return conv_wgrad_launch<WgCfg<KS, STRIDE, 3, CI_T>>(a, dw, sb, cu, acc, s); else return hipErrorInvalidValue;
        default: return hipErrorInvalidValue;
    }
}

// dW[Cout][Cin][ks][ks] (+)= sum over images and pixels of dY x shifted X   (ks in {1, 3, 7}, stride in {1, 2}, pad (ks-1)/2)
template <int NP>
static hipError_t wgrad_bf(int wout, const WgArgs& a, float* dw, size_t sb, int acc, hipStream_t s) {
    const int cu = device_cu_count();
    if (wout == 64) return conv_wgrad_bf16_launch<WgBfCfg<6, NP>>(a, dw, sb, cu, acc, s);
    if (wout == 32) return conv_wgrad_bf16_launch<WgBfCfg<5, NP>>(a, dw, sb, cu, acc, s);
    if (wout == 16) return conv_wgrad_bf16_launch<WgBfCfg<4, NP>>(a, dw, sb, cu, acc, s);
    return hipErrorInvalidValue;
}

extern "C" int egotap_hmtrain_conv_wgrad(const float* dy, const float* x, float* dw, int Nimg, int Cin, int Cout, int wout, int ks, int stride,
                                         int64_t dy_istride, int64_t x_istride, int accumulate, int precision, void* ws, size_t ws_bytes,
                                         void* stream) {
    EGO_CHECK(dy && x && dw && ws, "egotap_hmtrain_conv_wgrad: null argument");
    WgArgs a{dy, x, (float*)ws, dy_istride, x_istride, Nimg, Cin, Cout, 0, 0, 1, 0};
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipErrorInvalidValue;
    if (ks == 3 && stride == 1 && precision != EGOTAP_PREC_F32 && (wout == 64 || wout == 32 || wout == 16))
        e = precision == EGOTAP_PREC_BF16X3 ? wgrad_bf<3>(wout, a, dw, ws_bytes, accumulate, s) : wgrad_bf<1>(wout, a, dw, ws_bytes, accumulate, s);
    // [r3] at most 64 output channels on 64 x 64 maps (layer1, conv_heatmap): 2 x 2 waves over 64 co x 2 ci groups instead of four waves over 128 co
    else if (ks == 3 && stride == 1 && wout == 64 && Cout <= 64) e = conv_wgrad_launch<WgCfg<3, 1, 6, 64, 64, 32>>(a, dw, ws_bytes, device_cu_count(), accumulate, s);
    else if (ks == 1 && stride == 1 && wout == 64 && Cout <= 64) e = conv_wgrad_launch<WgCfg<1, 1, 6, 192, 64, 96>>(a, dw, ws_bytes, device_cu_count(), accumulate, s);
    else if (ks == 3 && stride == 1) e = wgrad_w<3, 1, 32>(wout, a, dw, ws_bytes, accumulate, s);
    else if (ks == 3 && stride == 2) e = wgrad_w<3, 2, 32>(wout, a, dw, ws_bytes, accumulate, s);
    else if (ks == 1 && stride == 1) e = wgrad_w<1, 1, 96>(wout, a, dw, ws_bytes, accumulate, s);
    else if (ks == 1 && stride == 2) e = wgrad_w<1, 2, 96>(wout, a, dw, ws_bytes, accumulate, s);
    else if (ks == 7 && stride == 2) e = wgrad_w<7, 2, 3>(wout, a, dw, ws_bytes, accumulate, s);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_hmtrain_conv_wgrad: unsupported ks=%d stride=%d wout=%d", ks, stride, wout); return EGOTAP_ERR_INVALID; }
    if (e == hipErrorOutOfMemory) { egotap_set_error("egotap_hmtrain_conv_wgrad: workspace too small (%zu bytes)", ws_bytes); return EGOTAP_ERR_WORKSPACE; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_relu_bwd(const float* y, const float* dy, float* dz, int N, int C, int HW, int64_t y_istride, int64_t dy_istride,
                                       int64_t dz_istride, void* stream) {
    EGO_CHECK(y && dy && dz && HW % 4 == 0, "egotap_hmtrain_relu_bwd: bad argument");
    const long total = (long)N * C * (HW / 4);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, dy, dz, N, C, HW, (long)y_istride,
                       (long)dy_istride, (long)dz_istride);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_maxpool_bwd(const float* x, const float* dy, float* dx, int64_t planes, int HIN, void* stream) {
    EGO_CHECK(x && dy && dx && planes > 0 && HIN % 2 == 0, "egotap_hmtrain_maxpool_bwd: bad argument");
    const long total = planes * HIN * HIN;
    constexpr int RI = 16;
    const size_t lds = ((size_t)(RI + 3) * HIN + 2 * (size_t)(RI / 2 + 1) * (HIN / 2)) * 4;
    const long strips = planes * ((HIN + RI - 1) / RI);
    if (HIN % 4 == 0 && lds <= 60 * 1024 && strips < (1L << 31))
        hipLaunchKernelGGL(maxpool3s2_bwd_strip_kernel<RI>, dim3((unsigned)strips), dim3(256), lds, (hipStream_t)stream, x, dy, dx, (long)planes, HIN);
    else
        hipLaunchKernelGGL(maxpool3s2_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, (long)planes, HIN);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_upsample_bwd(const float* dy, float* dx, int N, int C, int HIN, int64_t dy_istride, int64_t dx_istride, void* stream) {
    EGO_CHECK(dy && dx && N > 0 && C > 0 && HIN > 1, "egotap_hmtrain_upsample_bwd: bad argument");
    const long total = (long)N * C * HIN * HIN;
    hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, dx, N, C, HIN, (long)dy_istride,
                       (long)dx_istride);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

// loss[0] = lambda * (mean_left + mean_right) of (pred - gt)^2 / plen,  dpred = d loss / d pred   (pred, gt contiguous [B, Cn, HW])
extern "C" int egotap_hmtrain_mse(const float* pred, const float* gt, const float* plen, float* dpred, float* loss, int B, int Cn, int HW,
                                  float lambda, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(pred && gt && dpred && loss && ws && HW % 4 == 0 && Cn > 0, "egotap_hmtrain_mse: bad argument");
    const int blocks = 512;
    EGO_CHECK((size_t)blocks * 8 <= ws_bytes, "egotap_hmtrain_mse: workspace too small");
    const float coef = lambda / ((float)B * (0.5f * Cn) * HW);      // two halves (left, right), each a mean over B * Cn/2 * HW
    hipLaunchKernelGGL(mse_loss_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pred, gt, plen, dpred, (double*)ws, B, Cn, HW, coef);
    hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const double*)ws, blocks, coef, loss);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_maxpool_fwd(const float* x, float* y, int64_t planes, int HIN, void* stream) {
    EGO_CHECK(x && y && planes > 0 && HIN % 2 == 0, "egotap_hmtrain_maxpool_fwd: bad argument");
    maxpool3s2_launch(x, y, (long)planes, HIN, (hipStream_t)stream);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_hmtrain_upsample_fwd(const float* x, float* y, int N, int C, int HIN, int64_t in_istride, int64_t out_istride, void* stream) {
    EGO_CHECK(x && y && N > 0 && C > 0 && HIN > 1, "egotap_hmtrain_upsample_fwd: bad argument");
    const long threads = (long)N * C * (2 * HIN) * (2 * HIN / 4);
    hipLaunchKernelGGL(upsample2x_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, N, C, HIN, (long)in_istride,
                       (long)out_istride);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}
#endif

#if EGOTAP_IN(3)
// ================================================================================================ bf16-storage operators (part 3)
// EGOTAP_PREC_BF16 with bf16 tensors in HBM: activations are written as bf16 by their producers, weights are rounded once per
// step; every GEMM reads bf16 through the LDS DMA (gemm_bf16s.h).  Single operators first (tests, tools), the whole step below.
int g_conv_addressing = 0;           // the one definition (gemm_bf16s64.h)
extern "C" int egotap_debug_conv_addressing(int mode) {
    EGO_CHECK(mode == 0 || mode == 1, "egotap_debug_conv_addressing: mode must be 0 (scalar origin where it fits) or 1 (per-lane pointers)");
    g_conv_addressing = mode;
    return EGOTAP_OK;
}
int g_gemm_bf16s_bk = 0;             // the one definition (gemm_bf16s64.h declares it for every part)
extern "C" int egotap_debug_gemm_bk(int bk) {
    EGO_CHECK(bk == 0 || bk == 32 || bk == 64, "egotap_debug_gemm_bk: 0 (by shape), 32 or 64");
    g_gemm_bf16s_bk = bk;
    return EGOTAP_OK;
}
extern "C" int egotap_bf16_gemm_nt(const void* x, int64_t ldx, const void* w, const float* bias, int M, int N, int K, int epi, const void* aux,
                                   void* out0, void* out1, int64_t ldo, void* stream) {
    EGO_CHECK(x && w && out0, "egotap_bf16_gemm_nt: null argument");
    EGO_CHECK(M >= 0 && N > 0 && K > 0 && N % 256 == 0 && K % 32 == 0, "egotap_bf16_gemm_nt: N must be a multiple of 256 and K of 32 (N=%d K=%d)", N, K);
    EGO_CHECK(ldx % 8 == 0 && ldo % 8 == 0 && ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)out0 | (uintptr_t)out1 | (uintptr_t)aux)) & 15) == 0,
              "egotap_bf16_gemm_nt: operands must be 16-byte aligned, leading dimensions multiples of 8");
    hipStream_t s = (hipStream_t)stream;
    const XPlain xl{(const __bf16*)x, (long)ldx};
    const __bf16* wb = (const __bf16*)w;
    const int cu = device_cu_count();
    hipError_t e;
    switch (epi) {
        case 0: e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiBf16{bias, (__bf16*)out0, (long)ldo}, M, N, K, cu, s); break;
        case 1: EGO_CHECK(bias && aux, "egotap_bf16_gemm_nt: epi 1 needs bias and residual");
                e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiResF32{bias, (const float*)aux, (float*)out0, (long)ldo}, M, N, K, cu, s); break;
        case 2: EGO_CHECK(bias && out1, "egotap_bf16_gemm_nt: epi 2 needs bias and the second output");
                e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiGeluSave{bias, (__bf16*)out0, (__bf16*)out1, (long)ldo}, M, N, K, cu, s); break;
        case 3: EGO_CHECK(aux, "egotap_bf16_gemm_nt: epi 3 needs the saved pre-activation");
                // out1 (optional): fp32 [2 * ceil(M / 256)][N] partial column sums of the stored output, one row per 128-row wave block
                if (out1) e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiGeluGradCS{{(const __bf16*)aux, (__bf16*)out0, (long)ldo}, (float*)out1}, M, N, K, cu, s);
                else e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiGeluGrad{(const __bf16*)aux, (__bf16*)out0, (long)ldo}, M, N, K, cu, s);
                break;
        case 4: EGO_CHECK(bias, "egotap_bf16_gemm_nt: epi 4 needs bias");
                e = gemm_bf16s_plain_launch(xl, wb, (long)K, SEpiF32{bias, (float*)out0, (long)ldo}, M, N, K, cu, s); break;
        default: egotap_set_error("egotap_bf16_gemm_nt: unknown epilogue %d", epi); return EGOTAP_ERR_INVALID;
    }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_gemm_tn(const void* dy, int64_t ldy, const void* x, int64_t ldx, float* dw, int M, int N, int K, int accumulate,
                                   const void* zeros, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(dy && x && dw && zeros, "egotap_bf16_gemm_tn: null argument");
    EGO_CHECK(M > 0 && N % 256 == 0 && K % 256 == 0, "egotap_bf16_gemm_tn: N and K must be multiples of 256 (N=%d K=%d)", N, K);
    EGO_CHECK(ldy % 8 == 0 && ldx % 8 == 0 && ((((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)zeros | (uintptr_t)ws)) & 15) == 0,
              "egotap_bf16_gemm_tn: operands must be 16-byte aligned, leading dimensions multiples of 8");
    hipError_t e = gemm_tn_bf16s_launch((const __bf16*)dy, (long)ldy, TXPlain{(const __bf16*)x, (long)ldx}, (const __bf16*)zeros, dw, (float*)ws, ws_bytes, M, N, K,
                                        device_cu_count(), accumulate, (hipStream_t)stream);
    if (e == hipErrorOutOfMemory) { egotap_set_error("egotap_bf16_gemm_tn: workspace too small for one partial slab (%zu bytes given)", ws_bytes); return EGOTAP_ERR_WORKSPACE; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_layernorm_fwd(const float* x, void* y, const float* g, const float* b, float* mean, float* rstd, int rows, float eps, void* stream) {
    EGO_CHECK(x && y && g && b, "egotap_bf16_layernorm_fwd: null argument");
    if (rows <= 0) return EGOTAP_OK;
    hipLaunchKernelGGL(ln_fwd_bf16_kernel<1024>, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, (__bf16*)y, g, b, mean, rstd, rows, eps);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

// ws >= (3 * blocks + 3 + 3 * ceil(blocks / 64)) * 1024 floats, blocks = ceil(rows / 64)
extern "C" int egotap_bf16_layernorm_bwd(const float* x, const void* dy, const float* g, const float* mean, const float* rstd, const float* dres, float* dx,
                                         void* dxb, float* dgamma, float* dbeta, float* dcolsum, int rows, int accumulate, void* ws, size_t ws_bytes,
                                         void* stream) {
    EGO_CHECK(x && dy && g && mean && rstd && dx && dgamma && dbeta && ws, "egotap_bf16_layernorm_bwd: null argument");
    hipStream_t s = (hipStream_t)stream;
    const int rows_per_wave = 16, blocks = (rows + 4 * rows_per_wave - 1) / (4 * rows_per_wave);
    const int gy = (blocks + 63) / 64;
    EGO_CHECK(ws_bytes >= ((size_t)blocks * 3072 + 3072 + (size_t)gy * 3072) * 4, "egotap_bf16_layernorm_bwd: workspace too small");
    float* part = (float*)ws;
    hipLaunchKernelGGL(ln_bwd_bf16_kernel<1024>, dim3(blocks), dim3(256), 0, s, x, (const __bf16*)dy, g, mean, rstd, dres, dx, (__bf16*)dxb, part, rows, rows_per_wave);
    EGO_HIP(hipGetLastError());
    float* tmp = part + (size_t)blocks * 3072;
    float* part2 = tmp + 3072;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(3072 / 4 / 64, gy), dim3(256), 0, s, (const float*)part, 3072L, part2, blocks, 3072, 64);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(3), dim3(256), 0, s, (const float*)part2, tmp, 3072L, gy, 0);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(1), dim3(256), 0, s, tmp, dgamma, 1024L, 1, accumulate);
    hipLaunchKernelGGL(reduce_slabs_kernel, dim3(1), dim3(256), 0, s, tmp + 1024, dbeta, 1024L, 1, accumulate);
    if (dcolsum) hipLaunchKernelGGL(reduce_slabs_kernel, dim3(1), dim3(256), 0, s, tmp + 2048, dcolsum, 1024L, 1, accumulate);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_colsum(const void* y, int64_t ldy, float* out, int M, int N, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(y && out && ws && N % 8 == 0 && ldy % 8 == 0, "egotap_bf16_colsum: bad argument");
    hipError_t e = colsum_bf16_launch((const __bf16*)y, (long)ldy, out, M, N, accumulate, (float*)ws, ws_bytes, (hipStream_t)stream);
    if (e == hipErrorOutOfMemory) { egotap_set_error("egotap_bf16_colsum: workspace too small"); return EGOTAP_ERR_WORKSPACE; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_prep_weight(const float* w, void* wb, void* wt, int N, int K, int64_t ldt, void* stream) {
    EGO_CHECK(w && wb && N > 0 && K > 0 && N % 8 == 0 && K % 8 == 0, "egotap_bf16_prep_weight: bad argument (N, K multiples of 8)");
    EGO_CHECK(wt == nullptr || (ldt >= N && ldt % 8 == 0), "egotap_bf16_prep_weight: ldt must be >= N and a multiple of 8");
    hipLaunchKernelGGL(prep_weight_kernel, dim3((K + 63) / 64, (N + 63) / 64), dim3(256), 0, (hipStream_t)stream, w, (__bf16*)wb, (__bf16*)wt, N, K, (long)ldt);
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_from_f32(const float* src, void* dst, int64_t n, void* stream) {
    EGO_CHECK(src && dst && n % 8 == 0, "egotap_bf16_from_f32: n must be a multiple of 8");
    if (n == 0) return EGOTAP_OK;
    hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (__bf16*)dst, (long)(n / 8));
    EGO_HIP(hipGetLastError());
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_attention_fwd(const void* qkv, void* ctx, float* lse, int B, int N, int heads, void* stream) {
    EGO_CHECK(qkv && ctx, "egotap_bf16_attention_fwd: null argument");
    hipError_t e = attention_bf16s_fwd_launch((const __bf16*)qkv, (__bf16*)ctx, lse, B, N, heads, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_bf16_attention_fwd: sequence length %d is not a multiple of 32", N); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* delta, void* dqkv, int B, int N, int heads,
                                         void* stream) {
    EGO_CHECK(qkv && ctx && dctx && lse && delta && dqkv, "egotap_bf16_attention_bwd: null argument");
    hipError_t e = attention_bf16s_bwd_launch((const __bf16*)qkv, (const __bf16*)ctx, (const __bf16*)dctx, lse, delta, (__bf16*)dqkv, B, N, heads, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_bf16_attention_bwd: sequence length %d is not a multiple of 32", N); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

// the same, also producing the q | k | v BIAS gradients (column sums of dqkv) without a pass over dqkv: the kernels' epilogues leave
// per-block partial sums in ws (fp32 [B * N / 32][3 * heads * 128]); three small fp32 column sums finish them.  Shapes
// without that epilogue (N % 64 != 0) take the column-sum pass over dqkv instead.
extern "C" int egotap_bf16_attention_bwd_bias(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* delta, void* dqkv, float* dq_bias,
                                              float* dk_bias, float* dv_bias, int B, int N, int heads, void* ws, size_t ws_bytes, void* stream) {
    EGO_CHECK(qkv && ctx && dctx && lse && delta && dqkv && dq_bias && dk_bias && dv_bias && ws, "egotap_bf16_attention_bwd_bias: null argument");
    const int D = heads * 128, M = B * N;
    float* db[3] = {dq_bias, dk_bias, dv_bias};
    const size_t part_bytes = (size_t)B * (N / 32) * 3 * D * 4;
    const bool fused = N % 64 == 0 && ws_bytes >= part_bytes + (64u << 20);
    hipError_t e = attention_bf16s_bwd_launch((const __bf16*)qkv, (const __bf16*)ctx, (const __bf16*)dctx, lse, delta, (__bf16*)dqkv, B, N, heads, (hipStream_t)stream,
                                              fused ? (float*)ws : nullptr);
    if (e == hipErrorInvalidValue) { egotap_set_error("egotap_bf16_attention_bwd_bias: sequence length %d is not a multiple of 32", N); return EGOTAP_ERR_INVALID; }
    EGO_HIP(e);
    for (int q = 0; q < 3; ++q) {
        if (fused) {
            EGO_HIP(colsum_f32_launch((const float*)ws + (size_t)q * D, 3L * D, db[q], (float*)((char*)ws + part_bytes), ws_bytes - part_bytes, B * (N / 32), D, 0,
                                      (hipStream_t)stream));
        } else {
            hipError_t e2 = colsum_bf16_launch((const __bf16*)dqkv + (size_t)q * D, 3L * D, db[q], M, D, 0, (float*)ws, ws_bytes, (hipStream_t)stream);
            if (e2 == hipErrorOutOfMemory) { egotap_set_error("egotap_bf16_attention_bwd_bias: workspace too small"); return EGOTAP_ERR_WORKSPACE; }
            EGO_HIP(e2);
        }
    }
    return EGOTAP_OK;
}

// fc1 of the two heatmap encoders on bf16 operands, the gathers folded into the loaders (net_architecture.py:388-406, 690-694):
//   which 0: rows = per-heatmap patch tokens gathered from tokens bf16 [B*seq, D];  1: rows = [cos | sin] maps from hm bf16 [B, C, S, S]
// [r3] patch embedding of the bf16-storage step on the bf16-storage GEMM: hmb = bf16 copy of the heatmaps [B, C, S, S], w = bf16 copy of
// projection.weight [D, 256] (egotap_bf16_prep_weight), zeros >= 16 bytes of zeros; x fp32 [B * seq, D] = the embeddings
// (net_architecture.py:326-336, modeling_vit.py:137-153).  Replaces the fp32-operand kernel of the opt-in modes (VALU conversion per element).
extern "C" int egotap_bf16_patch_fwd(egotap_handle h, const void* hmb, const void* w, const float* bias, const float* mask_tok, const float* pos,
                                     const void* zeros, float* x, int B, void* stream) {
    EGO_CHECK(h && hmb && w && bias && mask_tok && pos && zeros && x && B > 0, "egotap_bf16_patch_fwd: bad argument");
    const int S = h->cfg.hm_size, D = h->D, M = B * h->seq;
    const XPatch xl{(const __bf16*)hmb, (const __bf16*)zeros, h->patches()};
    const SEpiPatchF32 ep{bias, mask_tok, pos, x, D, h->cells()};
    EGO_HIP(gemm_bf16s_launch(xl, (const __bf16*)w, 256L, ep, M, D, 256, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_bf16_fc1_fwd(egotap_handle h, int which, const void* src, const void* w, const float* bias, float* z, int B, void* stream) {
    EGO_CHECK(h && src && w && bias && z && (which == 0 || which == 1), "egotap_bf16_fc1_fwd: bad argument");
    const int BT = B * h->T, S = h->cfg.hm_size, K = which == 0 ? h->ppd * h->ppd * h->D : 2 * S * S;
    EGO_HIP(fc1_nt(h, which, (const __bf16*)src, (const __bf16*)w, (long)K, SEpiF32{bias, z, 2048L}, BT, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}

extern "C" int egotap_bf16_fc1_wgrad(egotap_handle h, int which, const void* dz, const void* src, float* dw, int B, const void* zeros, void* ws,
                                     size_t ws_bytes, void* stream) {
    EGO_CHECK(h && dz && src && dw && zeros && ws && (which == 0 || which == 1), "egotap_bf16_fc1_wgrad: bad argument");
    const int BT = B * h->T, S = h->cfg.hm_size, K = which == 0 ? h->ppd * h->ppd * h->D : 2 * S * S;
    hipError_t e;
    if (which == 0) e = gemm_tn_bf16s_launch((const __bf16*)dz, 2048L, TXTokens{(const __bf16*)src, h->tokens()}, (const __bf16*)zeros, dw, (float*)ws, ws_bytes, BT, 2048, K, device_cu_count(), 0, (hipStream_t)stream);
    else e = gemm_tn_bf16s_launch((const __bf16*)dz, 2048L, TXRot{(const __bf16*)src, h->rots()}, (const __bf16*)zeros, dw, (float*)ws, ws_bytes, BT, 2048, K, device_cu_count(), 0, (hipStream_t)stream);
    if (e == hipErrorOutOfMemory) { egotap_set_error("egotap_bf16_fc1_wgrad: workspace too small"); return EGOTAP_ERR_WORKSPACE; }
    EGO_HIP(e);
    return EGOTAP_OK;
}

// input gradient of fc1 of the position encoder, scattered back to token order: dtok bf16 [B*seq, D] (cleared here: dummy cells get zero)
extern "C" int egotap_bf16_fc1_dgrad_tokens(egotap_handle h, const void* dz, const void* wt, void* dtok, int B, void* stream) {
    EGO_CHECK(h && dz && wt && dtok, "egotap_bf16_fc1_dgrad_tokens: null argument");
    const int BT = B * h->T, K1 = h->ppd * h->ppd * h->D;
    hipStream_t s = (hipStream_t)stream;
    EGO_HIP(zero_fill(dtok, (size_t)B * h->seq * h->D * 2, s));
    EGO_HIP(gemm_bf16s_plain_launch(XPlain{(const __bf16*)dz, 2048L}, (const __bf16*)wt, 2048L, SEpiScatterTokens{(__bf16*)dtok, h->tokens()}, BT, K1,
                                    2048, device_cu_count(), s));      // [r5] the 64-deep kernel where its shape rules hold (plain operand)
    return EGOTAP_OK;
}

// input gradient of fc1 of the rotation encoder, scattered back to the heatmaps (the inverse of the XRot gather): dz bf16 [B*T, 2048], wt bf16
// [2 S^2, 2048] = fc1.weight^T (egotap_bf16_prep_weight), dhm fp32 [B, C, S, S] (16-byte aligned): channels [2J, 6J) written, each element once
extern "C" int egotap_bf16_fc1_dgrad_rot(egotap_handle h, const void* dz, const void* wt, float* dhm, int B, void* stream) {
    EGO_CHECK(h && dz && wt && dhm && B > 0 && ((uintptr_t)dhm & 15) == 0, "egotap_bf16_fc1_dgrad_rot: bad argument");
    const int BT = B * h->T, S = h->cfg.hm_size;
    EGO_HIP(gemm_bf16s_plain_launch(XPlain{(const __bf16*)dz, 2048L}, (const __bf16*)wt, 2048L, SEpiScatterRot{dhm, h->rots()}, BT, 2 * S * S, 2048,
                                    device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}

// input gradient of the patch embedding, scattered back to the heatmaps (the inverse of the XPatch gather): dx bf16 [B*seq, D], wt bf16 [256, D]
// = projection.weight^T, dhm fp32 [B, C, S, S] (16-byte aligned): channels [0, 2J) written, each element once; dummy cells store nothing
extern "C" int egotap_bf16_patch_dgrad(egotap_handle h, const void* dx, const void* wt, float* dhm, int B, void* stream) {
    EGO_CHECK(h && dx && wt && dhm && B > 0 && ((uintptr_t)dhm & 15) == 0, "egotap_bf16_patch_dgrad: bad argument");
    const int M = B * h->seq, D = h->D, S = h->cfg.hm_size;
    EGO_HIP(gemm_bf16s_plain_launch(XPlain{(const __bf16*)dx, (long)D}, (const __bf16*)wt, (long)D,
                                    SEpiScatterPatch{dhm, h->patches()}, M, 256, D, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
#endif

#if EGOTAP_IN(0)
// ------------------------------------------------------------------------------------------------ one-call training step
// egotap_lift_forward_train + egotap_lift_backward: the lifting head's training-mode forward (activations kept in `saved`) and its
// whole backward as ONE call each (egotap_lift_forward(…, saved, …) / egotap_lift_backward; reference:
// egotap_autoencoder_model.py:284-311 loss.backward()).  They compose the granular training operators above in the order of
// egotap_amd/training.py's operator-by-operator Functions (LiftTrainFn, LiftTrainBf16Fn; the tests hold both bit-identical to this),
// read the parameters bound with egotap_bind_param and write the gradients into the buffers bound with egotap_bind_grad.  Two storage forms:
//  - fp32 tensors; the large GEMMs' arithmetic follows egotap_set_precision (f32 / bf16x3, and bf16 operand copies when vit_dim != 1024);
//  - bf16 storage (EGOTAP_PREC_BF16 with vit_dim 1024: BASELINE config 3, the wrapper's --use_amp): bf16 ViT activations and per-step bf16
//    weight copies in `saved`; the residual stream, the statistics, the small layers and every gradient stay fp32.
// They differ in the patch-embedding forward, the ViT layers and the encoders' fc1 (lift_forward_train16 / lift_backward16 against the fp32
// bodies in the entries); the plan, the buffer checks, fc2 / fc3 and the BatchNorms, the propagation units, the pose head, the bucket events
// and the patch-embedding gradients are shared.  Everything is enqueued on the caller's stream; no allocation, no synchronisation.
#define EGO_RC(call) do { const int rc_ = (call); if (rc_ != EGOTAP_OK) return rc_; } while (0)

struct LiftTrainPlan {      // byte offsets into `saved`; hmb, the w_* weight copies and b_qkv only in bf16 storage (0 otherwise)
    size_t hmb, X[9];       // X[i]: input of ViT layer i (X[0] = embeddings), X[L]: input of the final LayerNorm
    struct Layer { size_t m1, r1, y1, qkv, ctx, lse, xm, m2, r2, y2, z, hid, w_qkv, w_qkv_t, w_o, w_o_t, w_up, w_up_t, w_dn, w_dn_t, b_qkv; } layer[8];
    size_t mf, rf, tokens, w_fc1p, w_fc1p_t, w_fc1r;
    struct Fc { size_t z, y, mean, rstd; } pos[3], rot[3];
    size_t pu, pu_hs1, pu_bytes, total;
};
struct LiftBwdPlan {        // byte offsets into the backward workspace; R, A4, A3 in fp32 storage, F, Rb, A4b (= A3b), dzb, zero in bf16 storage
    size_t R[3], A4, A3, F[2], Rb[2], A4b, A3b, dzb, zero, WT, E[2], dposz, drotz, dhs1, delta, pu, pu_bytes, scr, scr_bytes, total;
};
static const int FC_OUT[2] = {2048, 512};
static bool lift_train_bf16s(const Handle* h) { return h->precision == EGOTAP_PREC_BF16 && h->D == 1024; }

static int lift_train_plan(Handle* h, int B, LiftTrainPlan& t, LiftBwdPlan& w) {
    const bool bf = lift_train_bf16s(h);
    const size_t M = (size_t)B * h->seq, D = h->D, BT = (size_t)B * h->T, heads = h->cfg.vit_heads, L = h->cfg.vit_layers;
    const size_t K1 = (size_t)h->ppd * h->ppd * D, K1r = 2 * (size_t)h->cfg.hm_size * h->cfg.hm_size;
    t = LiftTrainPlan();
    w = LiftBwdPlan();
    size_t o = 0;
    auto bytes = [&](size_t n) { size_t r = o; o = al256(o + n); return r; };
    auto f32 = [&](size_t n) { return bytes(n * 4); };
    auto b16 = [&](size_t n) { return bytes(n * 2); };
    auto act = [&](size_t n) { return bytes(n * (bf ? 2 : 4)); };       // what the ViT's GEMMs read: bf16 in bf16 storage
    if (bf) t.hmb = b16((size_t)B * h->C * h->cfg.hm_size * h->cfg.hm_size);
    for (size_t i = 0; i <= L; ++i) t.X[i] = f32(M * D);
    for (size_t i = 0; i < L; ++i) {
        auto& l = t.layer[i];
        l.m1 = f32(M); l.r1 = f32(M); l.y1 = act(M * D); l.qkv = act(M * 3 * D); l.ctx = act(M * D); l.lse = f32((size_t)B * heads * h->seq);
        l.xm = f32(M * D); l.m2 = f32(M); l.r2 = f32(M); l.y2 = act(M * D); l.z = act(M * 4 * D); l.hid = act(M * 4 * D);
        if (bf) {
            l.w_qkv = b16(3 * D * D); l.w_qkv_t = b16(3 * D * D); l.w_o = b16(D * D); l.w_o_t = b16(D * D);
            l.w_up = b16(4 * D * D); l.w_up_t = b16(4 * D * D); l.w_dn = b16(4 * D * D); l.w_dn_t = b16(4 * D * D); l.b_qkv = f32(3 * D);
        }
    }
    t.mf = f32(M); t.rf = f32(M); t.tokens = act(M * D);
    if (bf) { t.w_fc1p = b16(2048 * K1); t.w_fc1p_t = b16(2048 * K1); t.w_fc1r = b16(2048 * K1r); }
    for (int e = 0; e < 2; ++e)
        for (int j = 0; j < 3; ++j) {
            const size_t n = j < 2 ? (size_t)FC_OUT[j] : (size_t)h->hid;
            LiftTrainPlan::Fc& f = e == 0 ? t.pos[j] : t.rot[j];
            f.z = f32(BT * n); f.y = f32(BT * n); f.mean = f32(n); f.rstd = f32(n);
        }
    size_t pub = 0, hs1 = 0;
    EGO_RC(egotap_train_pu_saved_bytes(h, B, &pub, &hs1));
    t.pu = bytes(pub + 4); t.pu_hs1 = hs1; t.pu_bytes = pub;
    t.total = o;

    o = 0;
    if (bf) {
        w.F[0] = f32(M * D); w.F[1] = f32(M * D); w.Rb[0] = b16(M * D); w.Rb[1] = b16(M * D);
        w.A4b = b16(M * 4 * D); w.A3b = w.A4b;       // dz (MLP) is dead before dqkv (attention) is produced: one slot
        w.E[0] = f32(BT * 2048); w.E[1] = f32(BT * 2048); w.dzb = b16(BT * 2048);
        w.WT = f32((size_t)2048 * 512);
    } else {
        for (int i = 0; i < 3; ++i) w.R[i] = f32(M * D);
        w.A4 = f32(M * 4 * D); w.A3 = f32(M * 3 * D);
        w.WT = f32(std::max((size_t)4 * D * D, K1 * 2048));
        w.E[0] = f32(BT * 2048); w.E[1] = f32(BT * 2048);
    }
    w.dposz = f32(BT * h->hid); w.drotz = f32(BT * h->hid); w.dhs1 = f32((size_t)h->J * B * h->H);
    w.delta = f32((size_t)B * heads * h->seq);
    if (bf) w.zero = bytes(4096);
    size_t pwb = 0;
    EGO_RC(egotap_train_pu_bwd_ws_bytes(h, B, &pwb));
    w.pu = bytes(pwb + 4); w.pu_bytes = pwb;
    // split-M slabs of the weight-gradient GEMMs (8 slabs of the largest [N, K]) / column-sum partials / LayerNorm partials
    if (bf) {
        const size_t nb = (M + 63) / 64;
        w.scr_bytes = std::max(std::max((size_t)4 * 4 * D * D * 8, (size_t)4 * 2048 * K1 * 2), (3 * nb + 3 + 3 * ((nb + 63) / 64)) * 4096 + 4096);
        w.scr_bytes = std::max(w.scr_bytes, (size_t)64 << 20);
        w.scr_bytes = std::max(w.scr_bytes, (size_t)B * (h->seq / 32) * 3 * D * 4 + ((size_t)64 << 20));      // per-block bias-gradient sums of the attention backward
    } else {
        w.scr_bytes = std::max((size_t)64 << 20, (size_t)4 * 2048 * std::max(K1, K1r) * 8);
    }
    w.scr = bytes(w.scr_bytes);
    w.total = o;
    return EGOTAP_OK;
}

extern "C" int egotap_lift_train_bytes(egotap_handle h, int B, size_t* saved_bytes, size_t* ws_bytes) {
    EGO_CHECK(h && saved_bytes && ws_bytes && B > 0, "egotap_lift_train_bytes: bad argument");
    LiftTrainPlan t; LiftBwdPlan w;
    EGO_RC(lift_train_plan(h, B, t, w));
    *saved_bytes = t.total;
    *ws_bytes = w.total;
    return EGOTAP_OK;
}

extern "C" int egotap_bind_grad(egotap_handle h, const char* key, void* dev_ptr, int64_t numel) {
    EGO_CHECK(h && key && dev_ptr, "egotap_bind_grad: null argument");
    auto it = h->bound[EGOTAP_NET_LIFT].find(key);
    EGO_CHECK(it != h->bound[EGOTAP_NET_LIFT].end(), "egotap_bind_grad(%s): bind the parameter first", key);
    EGO_CHECK(it->second.numel == numel, "egotap_bind_grad(%s): %lld elements, the parameter has %lld", key, (long long)numel, (long long)it->second.numel);
    EGO_CHECK(((uintptr_t)dev_ptr & 15) == 0, "egotap_bind_grad(%s): pointer must be 16-byte aligned", key);
    Param p;
    p.ptr = dev_ptr; p.numel = numel; p.dtype = EGOTAP_F32;
    h->bound_grad[key] = p;
    h->grad_resolved = false;
    return EGOTAP_OK;
}

// one call's plans and buffers: S / Hb address the fp32 / bf16 slots of `saved`, W / Wh those of the workspace
struct LiftStep {
    LiftTrainPlan t;
    LiftBwdPlan w;
    char *sb, *wb;
    float* S(size_t off) const { return (float*)(sb + off); }
    void* Hb(size_t off) const { return sb + off; }
    float* W(size_t off) const { return (float*)(wb + off); }
    void* Wh(size_t off) const { return wb + off; }
    void* scr() const { return wb + w.scr; }
};
static float* G(const float* q) { return (float*)q; }      // a bound gradient (h->lg holds them as const pointers)

// plans the step for B and checks the caller's buffers against the plan (fn: the entry's name, for its messages)
static int lift_step(const char* fn, Handle* h, int B, const void* saved, size_t saved_bytes, void* ws, size_t ws_bytes, LiftStep& c) {
    EGO_RC(lift_train_plan(h, B, c.t, c.w));
    EGO_CHECK(saved_bytes >= c.t.total, "%s: saved buffer too small (%zu < %zu)", fn, saved_bytes, c.t.total);
    EGO_CHECK(ws_bytes >= c.w.total, "%s: workspace too small (%zu < %zu)", fn, ws_bytes, c.w.total);
    c.sb = (char*)saved;
    c.wb = (char*)ws;
    return EGOTAP_OK;
}

// the forward after the final LayerNorm, both storage forms: the two FC encoders, the propagation units and the pose head.  Only fc1 differs:
// the bf16-storage kernel on the bf16 tokens / heatmaps and the step's bf16 weight copy, or the fp32 GEMM gathering its rows itself
static int lift_heads_fwd(Handle* h, const LiftStep& c, const float* hm, int B, float* pose, void* stream) {
    const LiftParams& p = h->lp;
    const LiftTrainPlan& t = c.t;
    const int BT = B * h->T;
    for (int e = 0; e < 2; ++e) {
        const LiftTrainPlan::Fc* f = e == 0 ? t.pos : t.rot;
        for (int j = 0; j < 3; ++j) {
            const int n = j < 2 ? FC_OUT[j] : h->hid;
            const LiftParams::Fc& fc = e == 0 ? p.pos_fc[j] : p.rot_fc[j];
            if (j > 0)
                EGO_RC(egotap_train_gemm_nt(h, 0, c.S(f[j - 1].y), 0, nullptr, fc.w, fc.b, c.S(f[j].z), BT, n, FC_OUT[j - 1], 1, nullptr, nullptr, 0, stream));
            else if (lift_train_bf16s(h))
                EGO_RC(egotap_bf16_fc1_fwd(h, e, c.Hb(e == 0 ? t.tokens : t.hmb), c.Hb(e == 0 ? t.w_fc1p : t.w_fc1r), fc.b, c.S(f[0].z), B, stream));
            else            // loader 2: the tokens' fc1 rows, 3: the heatmaps' rotation channels
                EGO_RC(egotap_train_gemm_nt(h, e == 0 ? 2 : 3, e == 0 ? c.S(t.tokens) : hm, 0, nullptr, fc.w, fc.b, c.S(f[0].z), BT, n,
                                            e == 0 ? h->ppd * h->ppd * h->D : 2 * h->cfg.hm_size * h->cfg.hm_size, 1, nullptr, nullptr, 0, stream));
            // train-mode BatchNorm1d: batch statistics, running statistics updated in the bound buffers (momentum 0.1, unbiased variance)
            EGO_RC(egotap_train_bn_lrelu_fwd(c.S(f[j].z), c.S(f[j].y), fc.g, fc.beta, c.S(f[j].mean), c.S(f[j].rstd), (float*)fc.mean, (float*)fc.var,
                                             BT, n, 1e-5f, 0.1f, c.scr(), c.w.scr_bytes, stream));
        }
    }
    EGO_RC(egotap_train_pu_fwd(h, c.S(t.pos[2].y), c.S(t.rot[2].y), B, c.sb + t.pu, t.pu_bytes, stream));
    return egotap_train_pose_head_fwd(h, c.S(t.pos[2].y), c.S(t.pu + t.pu_hs1), B, pose, stream);
}

static int lift_forward_train16(Handle* h, const LiftStep& c, const float* hm, int B, float* pose, void* stream) {
    const LiftParams& p = h->lp;
    const LiftTrainPlan& t = c.t;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * h->seq, D = h->D, heads = h->cfg.vit_heads, L = h->cfg.vit_layers;
    const int K1 = h->ppd * h->ppd * D, K1r = 2 * h->cfg.hm_size * h->cfg.hm_size;
    // per-step bf16 copies of the GEMM weights (and transposed copies for the input-gradient GEMMs), kept with the activations
    for (int i = 0; i < L; ++i) {
        const auto& P_ = p.layer[i];
        const auto& l = t.layer[i];
        const float* qkvw[3] = {P_.q_w, P_.k_w, P_.v_w};
        for (int q = 0; q < 3; ++q)
            EGO_RC(egotap_bf16_prep_weight(qkvw[q], (__bf16*)c.Hb(l.w_qkv) + (size_t)q * D * D, (__bf16*)c.Hb(l.w_qkv_t) + (size_t)q * D, D, D, 3 * D, stream));
        EGO_RC(egotap_bf16_prep_weight(P_.o_w, c.Hb(l.w_o), c.Hb(l.w_o_t), D, D, D, stream));
        EGO_RC(egotap_bf16_prep_weight(P_.up_w, c.Hb(l.w_up), c.Hb(l.w_up_t), 4 * D, D, 4 * D, stream));
        EGO_RC(egotap_bf16_prep_weight(P_.dn_w, c.Hb(l.w_dn), c.Hb(l.w_dn_t), D, 4 * D, D, stream));
        hipLaunchKernelGGL(concat3_kernel, dim3((D + 255) / 256), dim3(256), 0, s, P_.q_b, P_.k_b, P_.v_b, c.S(l.b_qkv), D);
        EGO_HIP(hipGetLastError());
    }
    EGO_RC(egotap_bf16_prep_weight(p.pos_fc[0].w, c.Hb(t.w_fc1p), c.Hb(t.w_fc1p_t), 2048, K1, 2048, stream));
    EGO_RC(egotap_bf16_prep_weight(p.rot_fc[0].w, c.Hb(t.w_fc1r), nullptr, 2048, K1r, 2048, stream));
    EGO_RC(egotap_bf16_from_f32(hm, c.Hb(t.hmb), (int64_t)B * h->C * h->cfg.hm_size * h->cfg.hm_size, stream));
    {   // [r3] patch embedding on the bf16-storage GEMM (bf16 heatmaps by LDS DMA); its bf16 weight copy (512 KB) and a page of zeros live in
        // the step's scratch for the duration of the launch (the weight gradient still reads the fp32 heatmaps: egotap_lift_backward)
        char* pscr = (char*)c.scr();
        EGO_HIP(zero_fill(pscr, 256, s));
        EGO_RC(egotap_bf16_prep_weight(p.patch_w, pscr + 256, nullptr, D, 256, D, stream));
        EGO_RC(egotap_bf16_patch_fwd(h, c.Hb(t.hmb), pscr + 256, p.patch_b, p.mask_tok, p.pos_emb, pscr, c.S(t.X[0]), B, stream));
    }
    for (int i = 0; i < L; ++i) {
        const auto& P_ = p.layer[i];
        const auto& l = t.layer[i];
        float* x = c.S(t.X[i]);
        EGO_RC(egotap_bf16_layernorm_fwd(x, c.Hb(l.y1), P_.ln1_g, P_.ln1_b, c.S(l.m1), c.S(l.r1), M, 1e-12f, stream));
        EGO_RC(egotap_bf16_gemm_nt(c.Hb(l.y1), D, c.Hb(l.w_qkv), c.S(l.b_qkv), M, 3 * D, D, 0, nullptr, c.Hb(l.qkv), nullptr, 3 * D, stream));
        EGO_RC(egotap_bf16_attention_fwd(c.Hb(l.qkv), c.Hb(l.ctx), c.S(l.lse), B, h->seq, heads, stream));
        EGO_RC(egotap_bf16_gemm_nt(c.Hb(l.ctx), D, c.Hb(l.w_o), P_.o_b, M, D, D, 1, x, c.S(l.xm), nullptr, D, stream));
        EGO_RC(egotap_bf16_layernorm_fwd(c.S(l.xm), c.Hb(l.y2), P_.ln2_g, P_.ln2_b, c.S(l.m2), c.S(l.r2), M, 1e-12f, stream));
        EGO_RC(egotap_bf16_gemm_nt(c.Hb(l.y2), D, c.Hb(l.w_up), P_.up_b, M, 4 * D, D, 2, nullptr, c.Hb(l.z), c.Hb(l.hid), 4 * D, stream));
        EGO_RC(egotap_bf16_gemm_nt(c.Hb(l.hid), 4 * D, c.Hb(l.w_dn), P_.dn_b, M, D, 4 * D, 1, c.S(l.xm), c.S(t.X[i + 1]), nullptr, D, stream));
    }
    EGO_RC(egotap_bf16_layernorm_fwd(c.S(t.X[L]), c.Hb(t.tokens), p.lnf_g, p.lnf_b, c.S(t.mf), c.S(t.rf), M, 1e-12f, stream));
    return lift_heads_fwd(h, c, hm, B, pose, stream);
}

extern "C" int egotap_lift_forward_train(egotap_handle h, const float* hm, int B, float* pose, void* saved, size_t saved_bytes, void* ws,
                                         size_t ws_bytes, void* stream) {
    EGO_CHECK(h && hm && pose && saved && ws && B > 0, "egotap_lift_forward_train: bad argument");
    EGO_CHECK(h->seq % 32 == 0, "egotap_lift_forward_train: training needs a ViT sequence that is a multiple of 32 (heatmap sides 64, 128, ...: every shipped configuration); "
              "this head has %d tokens (heatmap side %d) -- evaluation runs at any side that is a multiple of 16", h->seq, h->cfg.hm_size);
    EGO_RC(lift_resolve(h));
    LiftStep c;
    EGO_RC(lift_step("egotap_lift_forward_train", h, B, saved, saved_bytes, ws, ws_bytes, c));
    if (lift_train_bf16s(h)) return lift_forward_train16(h, c, hm, B, pose, stream);
    const LiftParams& p = h->lp;
    const LiftTrainPlan& t = c.t;
    const int M = B * h->seq, D = h->D, heads = h->cfg.vit_heads, L = h->cfg.vit_layers;
    const int prec = h->precision == EGOTAP_PREC_BF16 ? EGOTAP_PREC_BF16 : EGOTAP_PREC_F32;   // attention: exact unless the whole step is bf16
    EGO_RC(egotap_train_patch_fwd(h, hm, B, p.patch_w, p.patch_b, p.mask_tok, p.pos_emb, c.S(t.X[0]), stream));
    for (int i = 0; i < L; ++i) {
        const auto& P_ = p.layer[i];
        const auto& l = t.layer[i];
        float* x = c.S(t.X[i]);
        EGO_RC(egotap_train_layernorm_fwd(x, c.S(l.y1), P_.ln1_g, P_.ln1_b, c.S(l.m1), c.S(l.r1), M, 1e-12f, stream));
        EGO_RC(egotap_train_qkv_fwd(h, c.S(l.y1), P_.q_w, P_.q_b, P_.k_w, P_.k_b, P_.v_w, P_.v_b, c.S(l.qkv), M, D, stream));
        EGO_RC(egotap_train_attention_fwd(c.S(l.qkv), c.S(l.ctx), c.S(l.lse), B, h->seq, heads, prec, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, c.S(l.ctx), 0, nullptr, P_.o_w, P_.o_b, c.S(l.xm), M, D, D, 2, x, nullptr, 0, stream));
        EGO_RC(egotap_train_layernorm_fwd(c.S(l.xm), c.S(l.y2), P_.ln2_g, P_.ln2_b, c.S(l.m2), c.S(l.r2), M, 1e-12f, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, c.S(l.y2), 0, nullptr, P_.up_w, P_.up_b, c.S(l.hid), M, 4 * D, D, 3, nullptr, c.S(l.z), 0, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, c.S(l.hid), 0, nullptr, P_.dn_w, P_.dn_b, c.S(t.X[i + 1]), M, D, 4 * D, 2, c.S(l.xm), nullptr, 0, stream));
    }
    EGO_RC(egotap_train_layernorm_fwd(c.S(t.X[L]), c.S(t.tokens), p.lnf_g, p.lnf_b, c.S(t.mf), c.S(t.rf), M, 1e-12f, stream));
    return lift_heads_fwd(h, c, hm, B, pose, stream);
}

// one event per gradient-arena bucket (arena order, egotap_amd/training.py _arena_layout), recorded once every gradient in it is final
struct LiftBuckets {
    void* const* events;
    int n_events, next;
    hipStream_t s;
    int done() {
        if (n_events) EGO_HIP(hipEventRecord((hipEvent_t)events[next], s));
        ++next;
        return EGOTAP_OK;
    }
};

// pose head + propagation units (fp32 in both storage forms): dposz, drotz and dhs1 into the workspace
static int lift_head_bwd(Handle* h, const LiftStep& c, const float* dpose, int B, void* stream) {
    const LiftParams& g = h->lg;
    const LiftTrainPlan& t = c.t;
    const LiftBwdPlan& w = c.w;
    const float *posz = c.S(t.pos[2].y), *rotz = c.S(t.rot[2].y), *hs1 = c.S(t.pu + t.pu_hs1);
    EGO_RC(egotap_train_pose_head_bwd(h, posz, hs1, dpose, B, c.W(w.dposz), c.W(w.dhs1), G(g.pose_w), G(g.pose_b), G(g.glob_w), G(g.glob_b), 0, stream));
    float* pug[14] = {G(g.x2f0_w), G(g.x2f0_b), G(g.x2h0_w), G(g.x2h0_b), G(g.b2h0_w), G(g.b2h0_b), G(g.h2h0_w), G(g.h2h0_b),
                      G(g.x2f1_w), G(g.x2f1_b), G(g.x2h1_w), G(g.x2h1_b), G(g.h2h1_w), G(g.h2h1_b)};
    return egotap_train_pu_bwd(h, posz, rotz, B, c.sb + t.pu, c.W(w.dhs1), c.W(w.dposz), c.W(w.drotz), pug, 0, c.wb + w.pu, w.pu_bytes, stream);
}

// patch embedding (fp32 operands: the input heatmaps): weight, position embeddings (sum over the batch: dx viewed as [B, seq * D]),
// bias / mask token; that completes the last two buckets
static int lift_patch_bwd(Handle* h, const LiftStep& c, const float* hm, const float* dx, int B, LiftBuckets& bk, void* stream) {
    const LiftParams& g = h->lg;
    EGO_RC(egotap_train_gemm_tn(h, 1, dx, 0, hm, nullptr, G(g.patch_w), B * h->seq, h->D, 256, 0, 0, c.scr(), c.w.scr_bytes, stream));
    EGO_RC(egotap_train_colsum(dx, 0, G(g.pos_emb), B, h->seq * h->D, 0, c.scr(), c.w.scr_bytes, stream));
    EGO_RC(egotap_train_patch_split(h, g.pos_emb, G(g.patch_b), G(g.mask_tok), 0, stream));
    EGO_RC(bk.done());
    return bk.done();
}

static int lift_backward16(const char* fn, Handle* h, const LiftStep& c, const float* hm, const float* dpose, int B, LiftBuckets& bk, void* stream,
                           float* dhm) {
    const LiftTrainPlan& t = c.t;
    const LiftBwdPlan& w = c.w;
    const size_t K1r = 2 * (size_t)h->cfg.hm_size * h->cfg.hm_size;
    // dhm: the bf16 copies of rotation fc1.weight (+ its transpose) and of projection.weight (+ transpose) live in the scratch while it is free
    EGO_CHECK(!dhm || w.scr_bytes >= 2 * 2048 * K1r * 2, "%s: scratch too small for the transposed rotation fc1 weight", fn);
    const int L = h->cfg.vit_layers;
    const LiftParams& p = h->lp;
    const LiftParams& g = h->lg;
    void* scr = c.scr();
    const size_t scrb = w.scr_bytes;
    hipStream_t s = (hipStream_t)stream;
    const int M = B * h->seq, D = h->D, BT = B * h->T, heads = h->cfg.vit_heads;
    const void* ZERO = c.wb + w.zero;
    EGO_HIP(zero_fill(c.wb + w.zero, 4096, s));
    EGO_RC(lift_head_bwd(h, c, dpose, B, stream));
    // FC encoders: fc3, fc2 in fp32 (small), fc1 on the bf16 kernels; the position encoder returns the token gradient (bf16, token order)
    auto encoder_bwd = [&](int e, const float* dy, void* dtok) -> int {
        for (int j = 2; j >= 0; --j) {
            const int n = j < 2 ? FC_OUT[j] : h->hid;
            const LiftParams::Fc& fc = e == 0 ? p.pos_fc[j] : p.rot_fc[j];
            const LiftParams::Fc& gc = e == 0 ? g.pos_fc[j] : g.rot_fc[j];
            const LiftTrainPlan::Fc& f = e == 0 ? t.pos[j] : t.rot[j];
            float* dz = c.W(w.E[0]);
            EGO_RC(egotap_train_bn_lrelu_bwd(c.S(f.z), c.S(f.y), dy, fc.g, c.S(f.mean), c.S(f.rstd), dz, G(gc.g), G(gc.beta), BT, n, 0, scr, scrb, stream));
            EGO_RC(egotap_train_colsum(dz, 0, G(gc.b), BT, n, 0, scr, scrb, stream));
            if (j > 0) {
                const int K = FC_OUT[j - 1];
                const float* a_in = c.S((e == 0 ? t.pos[j - 1] : t.rot[j - 1]).y);
                EGO_RC(egotap_train_gemm_tn(h, 0, dz, 0, a_in, nullptr, G(gc.w), BT, n, K, 0, 0, scr, scrb, stream));
                EGO_RC(egotap_train_transpose(fc.w, c.W(w.WT), n, K, 0, stream));
                EGO_RC(egotap_train_gemm_nt(h, 0, dz, 0, nullptr, c.W(w.WT), nullptr, c.W(w.E[1]), BT, K, n, 0, nullptr, nullptr, 0, stream));
                dy = c.W(w.E[1]);
            } else {
                EGO_RC(egotap_bf16_from_f32(dz, c.Wh(w.dzb), (int64_t)BT * 2048, stream));
                EGO_RC(egotap_bf16_fc1_wgrad(h, e, c.Wh(w.dzb), e == 0 ? c.Hb(t.tokens) : c.Hb(t.hmb), G(gc.w), B, ZERO, scr, scrb, stream));
                if (e == 0) {
                    EGO_RC(egotap_bf16_fc1_dgrad_tokens(h, c.Wh(w.dzb), c.Hb(t.w_fc1p_t), dtok, B, stream));
                } else if (dhm) {           // the heatmaps' rotation channels: the scratch is free between this weight gradient and the next
                    __bf16* wr = (__bf16*)scr;
                    EGO_RC(egotap_bf16_prep_weight(fc.w, wr, wr + 2048 * K1r, 2048, (int)K1r, 2048, stream));
                    EGO_RC(egotap_bf16_fc1_dgrad_rot(h, c.Wh(w.dzb), wr + 2048 * K1r, dhm, B, stream));
                }
            }
        }
        return EGOTAP_OK;
    };
    EGO_RC(encoder_bwd(1, c.W(w.drotz), nullptr));
    EGO_RC(encoder_bwd(0, c.W(w.dposz), c.Wh(w.Rb[0])));
    float *F0 = c.W(w.F[0]), *F1 = c.W(w.F[1]);
    void *R0 = c.Wh(w.Rb[0]), *R1 = c.Wh(w.Rb[1]), *A4 = c.Wh(w.A4b), *A3 = c.Wh(w.A3b);
    // final LayerNorm: dtok (R0) -> dx (F0, bf16 copy R1); column sums of dx = the last layer's output.dense.bias gradient
    EGO_RC(egotap_bf16_layernorm_bwd(c.S(t.X[L]), R0, p.lnf_g, c.S(t.mf), c.S(t.rf), nullptr, F0, R1, G(g.lnf_g), G(g.lnf_b), G(g.layer[L - 1].dn_b), M, 0,
                                     scr, scrb, stream));
    for (int i = L - 1; i >= 0; --i) {
        EGO_RC(bk.done());                                                       // everything above layer i is final
        const auto& P_ = p.layer[i];
        const auto& G_ = g.layer[i];
        const auto& l = t.layer[i];
        // MLP (dx = F0 fp32, R1 bf16)
        EGO_RC(egotap_bf16_gemm_tn(R1, D, c.Hb(l.hid), 4 * D, G(G_.dn_w), M, D, 4 * D, 0, ZERO, scr, scrb, stream));
        // dz; its column sums (= the intermediate.dense bias gradient) leave the epilogue as per-wave partial sums in R0 (free until dy2)
        EGO_RC(egotap_bf16_gemm_nt(R1, D, c.Hb(l.w_dn_t), nullptr, M, 4 * D, D, 3, c.Hb(l.z), A4, R0, 4 * D, stream));
        EGO_RC(egotap_train_colsum((const float*)R0, 0, G(G_.up_b), 2 * ((M + 255) / 256), 4 * D, 0, scr, scrb, stream));
        EGO_RC(egotap_bf16_gemm_tn(A4, 4 * D, c.Hb(l.y2), D, G(G_.up_w), M, 4 * D, D, 0, ZERO, scr, scrb, stream));
        EGO_RC(egotap_bf16_gemm_nt(A4, 4 * D, c.Hb(l.w_up_t), nullptr, M, D, 4 * D, 0, nullptr, R0, nullptr, D, stream));             // dy2
        EGO_RC(egotap_bf16_layernorm_bwd(c.S(l.xm), R0, P_.ln2_g, c.S(l.m2), c.S(l.r2), F0, F1, R1, G(G_.ln2_g), G(G_.ln2_b), G(G_.o_b), M, 0, scr, scrb,
                                         stream));                                                                                   // dxm = F1, R1
        // attention
        EGO_RC(egotap_bf16_gemm_tn(R1, D, c.Hb(l.ctx), D, G(G_.o_w), M, D, D, 0, ZERO, scr, scrb, stream));
        EGO_RC(egotap_bf16_gemm_nt(R1, D, c.Hb(l.w_o_t), nullptr, M, D, D, 0, nullptr, R0, nullptr, D, stream));                       // dctx
        // dqkv, and the q | k | v bias gradients from the kernels' epilogues (no pass over dqkv)
        EGO_RC(egotap_bf16_attention_bwd_bias(c.Hb(l.qkv), c.Hb(l.ctx), R0, c.S(l.lse), c.W(w.delta), A3, G(G_.q_b), G(G_.k_b), G(G_.v_b), B, h->seq, heads,
                                              scr, scrb, stream));
        float* gw[3] = {G(G_.q_w), G(G_.k_w), G(G_.v_w)};
        for (int q = 0; q < 3; ++q)
            EGO_RC(egotap_bf16_gemm_tn((const __bf16*)A3 + (size_t)q * D, 3 * D, c.Hb(l.y1), D, gw[q], M, D, D, 0, ZERO, scr, scrb, stream));
        EGO_RC(egotap_bf16_gemm_nt(A3, 3 * D, c.Hb(l.w_qkv_t), nullptr, M, D, 3 * D, 0, nullptr, R0, nullptr, D, stream));             // dy1
        EGO_RC(egotap_bf16_layernorm_bwd(c.S(t.X[i]), R0, P_.ln1_g, c.S(l.m1), c.S(l.r1), F1, F0, i > 0 || dhm ? R1 : nullptr, G(G_.ln1_g), G(G_.ln1_b),
                                         i > 0 ? G(g.layer[i - 1].dn_b) : nullptr, M, 0, scr, scrb, stream));                        // dx = F0, R1
    }
    EGO_RC(lift_patch_bwd(h, c, hm, F0, B, bk, stream));
    if (dhm) {                      // the heatmaps' position channels, behind the last bucket event (its all-reduce overlaps this product)
        __bf16* pw = (__bf16*)scr;
        EGO_RC(egotap_bf16_prep_weight(p.patch_w, pw, pw + (size_t)D * 256, D, 256, D, stream));
        EGO_RC(egotap_bf16_patch_dgrad(h, R1, pw + (size_t)D * 256, dhm, B, stream));
    }
    return EGOTAP_OK;
}

// the backward of egotap_lift_backward (dhm == nullptr) and of egotap_lift_backward_dhm (fn: the entry's name, for its messages)
static int lift_backward_impl(const char* fn, Handle* h, const float* hm, const float* dpose, int B, const void* saved, size_t saved_bytes,
                              void* ws, size_t ws_bytes, void* const* bucket_events, int n_events, void* stream, float* dhm) {
    EGO_RC(lift_resolve(h));
    if (!h->grad_resolved) {
        EGO_RC(lift_resolve_into(h, h->bound_grad, h->lg, false));
        h->grad_resolved = true;
    }
    const int L = h->cfg.vit_layers;
    EGO_CHECK(n_events == 0 || (bucket_events && n_events == L + 2), "%s: %d bucket events, the arena has %d buckets", fn, n_events, L + 2);
    LiftStep c;
    EGO_RC(lift_step(fn, h, B, saved, saved_bytes, ws, ws_bytes, c));
    LiftBuckets bk{bucket_events, n_events, 0, (hipStream_t)stream};
    if (lift_train_bf16s(h)) return lift_backward16(fn, h, c, hm, dpose, B, bk, stream, dhm);
    const LiftTrainPlan& t = c.t;
    const LiftBwdPlan& w = c.w;
    const LiftParams& p = h->lp;
    const LiftParams& g = h->lg;
    void* scr = c.scr();
    const size_t scrb = w.scr_bytes;
    const int M = B * h->seq, D = h->D, BT = B * h->T, heads = h->cfg.vit_heads;
    const int prec = h->precision == EGOTAP_PREC_BF16 ? EGOTAP_PREC_BF16 : EGOTAP_PREC_F32;
    EGO_RC(lift_head_bwd(h, c, dpose, B, stream));
    // the two FC encoders, last block first; returns in *dA the gradient w.r.t. the gathered fc1 rows (position encoder only)
    auto encoder_bwd = [&](int e, const float* dy, float** dA) -> int {
        for (int j = 2; j >= 0; --j) {
            const int n = j < 2 ? FC_OUT[j] : h->hid;
            const int K = j > 0 ? FC_OUT[j - 1] : (e == 0 ? h->ppd * h->ppd * D : 2 * h->cfg.hm_size * h->cfg.hm_size);
            const int loader = j > 0 ? 0 : (e == 0 ? 2 : 3);
            const LiftParams::Fc& fc = e == 0 ? p.pos_fc[j] : p.rot_fc[j];
            const LiftParams::Fc& gc = e == 0 ? g.pos_fc[j] : g.rot_fc[j];
            const LiftTrainPlan::Fc& f = e == 0 ? t.pos[j] : t.rot[j];
            const float* a_in = j > 0 ? c.S((e == 0 ? t.pos[j - 1] : t.rot[j - 1]).y) : (e == 0 ? c.S(t.tokens) : hm);
            float* dz = c.W(w.E[0]);
            EGO_RC(egotap_train_bn_lrelu_bwd(c.S(f.z), c.S(f.y), dy, fc.g, c.S(f.mean), c.S(f.rstd), dz, G(gc.g), G(gc.beta), BT, n, 0, scr, scrb, stream));
            EGO_RC(egotap_train_gemm_tn(h, loader, dz, 0, a_in, nullptr, G(gc.w), BT, n, K, 0, 0, scr, scrb, stream));
            EGO_RC(egotap_train_colsum(dz, 0, G(gc.b), BT, n, 0, scr, scrb, stream));
            if (j == 0 && e == 1) {                                          // the rotation encoder's input: the heatmaps
                if (dhm) {                                                   // their rotation channels, while dz (E[0]) is live
                    EGO_RC(egotap_train_transpose(fc.w, c.W(w.WT), n, K, 0, stream));                                            // [2 S^2, 2048]
                    EGO_RC(egotap_train_gemm_nt(h, 0, dz, 0, nullptr, c.W(w.WT), nullptr, dhm, BT, K, n, TE_SCATTER_ROT, nullptr, nullptr, 0, stream));
                }
                return EGOTAP_OK;
            }
            EGO_RC(egotap_train_transpose(fc.w, c.W(w.WT), n, K, 0, stream));  // [K, n]
            float* dnext = j == 0 ? c.W(w.R[1]) : c.W(w.E[1]);
            EGO_RC(egotap_train_gemm_nt(h, 0, dz, 0, nullptr, c.W(w.WT), nullptr, dnext, BT, K, n, 0, nullptr, nullptr, 0, stream));
            dy = dnext;
            if (j == 0) *dA = dnext;
        }
        return EGOTAP_OK;
    };
    float* dA = nullptr;
    EGO_RC(encoder_bwd(1, c.W(w.drotz), nullptr));
    EGO_RC(encoder_bwd(0, c.W(w.dposz), &dA));
    float *R0 = c.W(w.R[0]), *R1 = c.W(w.R[1]), *R2 = c.W(w.R[2]), *A4 = c.W(w.A4), *A3 = c.W(w.A3), *WT = c.W(w.WT);
    EGO_RC(egotap_train_tokens_scatter(h, dA, R0, B, stream));                                                   // dtok
    EGO_RC(egotap_train_layernorm_bwd(c.S(t.X[L]), R0, p.lnf_g, c.S(t.mf), c.S(t.rf), nullptr, R1, G(g.lnf_g), G(g.lnf_b), M, 0, scr, scrb, stream));
    float* dx = R1;
    for (int i = L - 1; i >= 0; --i) {
        const auto& P_ = p.layer[i];
        const auto& G_ = g.layer[i];
        const auto& l = t.layer[i];
        // output.dense.bias of layer i closes the bucket of layer i + 1 (or of the head, for the last layer)
        // [r3] every bias gradient of the layer comes out of the weight-gradient GEMM that stages the same dY (egotap_train_gemm_tn_bias)
        EGO_RC(egotap_train_gemm_tn_bias(h, dx, 0, c.S(l.hid), G(G_.dn_w), G(G_.dn_b), M, D, 4 * D, 0, scr, scrb, stream));
        EGO_RC(bk.done());
        // MLP
        EGO_RC(egotap_train_transpose(P_.dn_w, WT, D, 4 * D, 0, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, dx, 0, nullptr, WT, nullptr, A4, M, 4 * D, D, 5, c.S(l.z), nullptr, 0, stream));          // dz
        EGO_RC(egotap_train_gemm_tn_bias(h, A4, 0, c.S(l.y2), G(G_.up_w), G(G_.up_b), M, 4 * D, D, 0, scr, scrb, stream));
        EGO_RC(egotap_train_transpose(P_.up_w, WT, 4 * D, D, 0, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, A4, 0, nullptr, WT, nullptr, R0, M, D, 4 * D, 0, nullptr, nullptr, 0, stream));          // dy2
        EGO_RC(egotap_train_layernorm_bwd(c.S(l.xm), R0, P_.ln2_g, c.S(l.m2), c.S(l.r2), dx, R2, G(G_.ln2_g), G(G_.ln2_b), M, 0, scr, scrb, stream));
        float* dxm = R2;
        // attention
        EGO_RC(egotap_train_gemm_tn_bias(h, dxm, 0, c.S(l.ctx), G(G_.o_w), G(G_.o_b), M, D, D, 0, scr, scrb, stream));
        EGO_RC(egotap_train_transpose(P_.o_w, WT, D, D, 0, stream));
        EGO_RC(egotap_train_gemm_nt(h, 0, dxm, 0, nullptr, WT, nullptr, R0, M, D, D, 0, nullptr, nullptr, 0, stream));             // dctx
        EGO_RC(egotap_train_attention_bwd(c.S(l.qkv), c.S(l.ctx), R0, c.S(l.lse), c.W(w.delta), A3, B, h->seq, heads, prec, stream));   // dqkv
        const float* pw[3] = {P_.q_w, P_.k_w, P_.v_w};
        float* gw[3] = {G(G_.q_w), G(G_.k_w), G(G_.v_w)};
        float* gb[3] = {G(G_.q_b), G(G_.k_b), G(G_.v_b)};
        for (int q = 0; q < 3; ++q) {
            EGO_RC(egotap_train_gemm_tn_bias(h, A3 + (size_t)q * D, 3 * D, c.S(l.y1), gw[q], gb[q], M, D, D, 0, scr, scrb, stream));
            EGO_RC(egotap_train_transpose(pw[q], WT + (size_t)q * D, D, D, 3 * D, stream));                                         // [Wq^T | Wk^T | Wv^T]
        }
        EGO_RC(egotap_train_gemm_nt(h, 0, A3, 0, nullptr, WT, nullptr, R0, M, D, 3 * D, 0, nullptr, nullptr, 0, stream));          // dy1
        EGO_RC(egotap_train_layernorm_bwd(c.S(t.X[i]), R0, P_.ln1_g, c.S(l.m1), c.S(l.r1), dxm, R1, G(G_.ln1_g), G(G_.ln1_b), M, 0, scr, scrb, stream));
        dx = R1;
    }
    EGO_RC(lift_patch_bwd(h, c, hm, dx, B, bk, stream));
    if (dhm) {                      // the heatmaps' position channels, behind the last bucket event (its all-reduce overlaps this product)
        EGO_RC(egotap_train_transpose(p.patch_w, WT, D, 256, 0, stream));                                                       // [256, D]
        EGO_RC(egotap_train_gemm_nt(h, 0, dx, 0, nullptr, WT, nullptr, dhm, M, 256, D, TE_SCATTER_PATCH, nullptr, nullptr, 0, stream));
    }
    return EGOTAP_OK;
}

extern "C" int egotap_lift_backward(egotap_handle h, const float* hm, const float* dpose, int B, const void* saved, size_t saved_bytes,
                                    void* ws, size_t ws_bytes, void* const* bucket_events, int n_events, void* stream) {
    EGO_CHECK(h && hm && dpose && saved && ws && B > 0, "egotap_lift_backward: bad argument");
    return lift_backward_impl("egotap_lift_backward", h, hm, dpose, B, saved, saved_bytes, ws, ws_bytes, bucket_events, n_events, stream, nullptr);
}

// egotap_lift_backward that also returns the gradient w.r.t. the input heatmaps: dhm fp32 [B, C, S, S] (contiguous, 16-byte aligned, not
// overlapping hm), every element written exactly once -- position channels from the patch embedding, rotation channels from the rotation
// encoder's fc1.  dhm == nullptr: exactly egotap_lift_backward (same launches, same bits).  Same workspace (egotap_lift_train_bytes).
extern "C" int egotap_lift_backward_dhm(egotap_handle h, const float* hm, const float* dpose, int B, const void* saved, size_t saved_bytes,
                                        void* ws, size_t ws_bytes, void* const* bucket_events, int n_events, void* stream, float* dhm) {
    EGO_CHECK(h && hm && dpose && saved && ws && B > 0, "egotap_lift_backward_dhm: bad argument");
    if (dhm) {
        const size_t bytes = (size_t)B * h->C * h->cfg.hm_size * h->cfg.hm_size * sizeof(float);
        const uintptr_t a = (uintptr_t)dhm, b = (uintptr_t)hm;
        EGO_CHECK((a & 15) == 0, "egotap_lift_backward_dhm: dhm must be 16-byte aligned");
        EGO_CHECK(a + bytes <= b || b + bytes <= a, "egotap_lift_backward_dhm: dhm must not overlap hm");
    }
    return lift_backward_impl("egotap_lift_backward_dhm", h, hm, dpose, B, saved, saved_bytes, ws, ws_bytes, bucket_events, n_events, stream, dhm);
}

// ---- heatmaps, keypoints and bones drawn onto the frames (overlay.h): two operators, no handle
extern "C" int egotap_heat_u8(const void* hm, int dtype, int B, int C, int S, int64_t image_stride, int c0, int n, int groups, uint8_t* heat8, void* stream) {
    static const char* const who = "egotap_heat_u8";
    EGO_CHECK(hm && heat8, "%s: null argument (hm and heat8 are required)", who);
    EGO_CHECK(dtype == EGOTAP_F32 || dtype == EGOTAP_BF16, "%s: unknown dtype %d (EGOTAP_F32 or EGOTAP_BF16)", who, dtype);
    EGO_CHECK(B > 0, "%s: the batch must be positive (B = %d)", who, B);
    EGO_CHECK(n >= 1, "%s: the number of channels must be at least 1 (n = %d)", who, n);
    EGO_CHECK(groups >= 1 && n % groups == 0, "%s: n must be a multiple of groups >= 1 (n = %d, groups = %d)", who, n, groups);
    EGO_CHECK(c0 >= 0 && (int64_t)c0 + n <= C, "%s: channels c0 .. c0 + n - 1 = %d .. %lld are not inside the C = %d channels", who, c0, (long long)c0 + n - 1, C);
    EGO_CHECK(S > 0 && S % 16 == 0 && S <= kOverlayMaxHeatSide, "%s: the side must be a positive multiple of 16, at most %d (S = %d)", who, kOverlayMaxHeatSide, S);
    const int esz = dtype == EGOTAP_F32 ? 4 : 2;
    EGO_CHECK(image_stride >= (int64_t)C * S * S, "%s: image_stride %lld is smaller than C * S*S = %lld", who, (long long)image_stride, (long long)C * S * S);
    EGO_CHECK(image_stride * esz % 16 == 0, "%s: image_stride must be a multiple of 16 bytes (%lld elements of %d bytes)", who, (long long)image_stride, esz);
    EGO_CHECK(((uintptr_t)hm & 15) == 0 && ((uintptr_t)heat8 & 7) == 0, "%s: hm must be 16-byte aligned, heat8 8-byte aligned", who);
    const size_t in_bytes = ((size_t)(B - 1) * image_stride + (size_t)C * S * S) * esz, out_bytes = (size_t)B * groups * S * S;
    EGO_CHECK(!ego_overlap(heat8, out_bytes, hm, in_bytes), "%s: heat8 overlaps hm", who);
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "heat_u8", "heat_u8_kernel", 0.0);
    EGO_HIP(dtype == EGOTAP_F32 ? heat_u8_launch((const float*)hm, B, S, (long)image_stride, c0, n, groups, heat8, (hipStream_t)stream)
                                : heat_u8_launch((const __bf16*)hm, B, S, (long)image_stride, c0, n, groups, heat8, (hipStream_t)stream));
    return EGOTAP_OK;
}

extern "C" int egotap_overlay_u8(const uint8_t* left8, const uint8_t* right8, int B, int Hc, int Wc, const uint8_t* heat8, int S, const int32_t* tx_left,
                                 const int32_t* ty_left, const int32_t* tx_right, const int32_t* ty_right, const float* marks, const egotap_overlay_style* style,
                                 uint8_t* out_left8, uint8_t* out_right8, void* stream) {
    static const char* const who = "egotap_overlay_u8";
    EGO_CHECK(left8 && out_left8 && style, "%s: null argument (left8, out_left8 and style are required)", who);
    EGO_CHECK((right8 == nullptr) == (out_right8 == nullptr), "%s: right8 and out_right8 are both given or both NULL (one eye)", who);
    const int E = right8 ? 2 : 1;
    EGO_CHECK(B > 0 && B <= 65535, "%s: the batch must be between 1 and 65535 (B = %d)", who, B);
    EGO_CHECK(Hc >= 1 && Wc >= 4 && Wc % 4 == 0 && Hc <= kOverlayMaxSide && Wc <= kOverlayMaxSide,
              "%s: the canvas must be 1 .. %d rows of 4 .. %d pixels, the width a multiple of 4 (Hc = %d, Wc = %d)", who, kOverlayMaxSide, kOverlayMaxSide, Hc, Wc);
    EGO_CHECK((((uintptr_t)left8 | (uintptr_t)right8 | (uintptr_t)out_left8 | (uintptr_t)out_right8) & 3) == 0, "%s: every canvas must be 4-byte aligned", who);
    if (heat8) {
        EGO_CHECK(S >= 1 && S <= kOverlayMaxHeatSide, "%s: the heat side must be between 1 and %d (S = %d)", who, kOverlayMaxHeatSide, S);
        EGO_CHECK(tx_left && ty_left && (E == 1 || (tx_right && ty_right)), "%s: with heat8 every drawn eye needs its two tap tables (tx, ty)", who);
        EGO_CHECK((((uintptr_t)tx_left | (uintptr_t)(E == 2 ? tx_right : nullptr)) & 15) == 0 && (((uintptr_t)ty_left | (uintptr_t)(E == 2 ? ty_right : nullptr)) & 3) == 0,
                  "%s: the x tap tables must be 16-byte aligned, the y tap tables 4-byte aligned", who);
    }
    const egotap_overlay_style& q = *style;
    EGO_CHECK(q.r16 >= 0 && q.r16 <= kOverlayMaxR16 && q.w16 >= 0 && q.w16 <= kOverlayMaxR16, "%s: style: r16 and w16 must be between 0 and %d (%d, %d)", who,
              kOverlayMaxR16, q.r16, q.w16);
    EGO_CHECK(q.min_score == q.min_score, "%s: style: min_score must not be NaN", who);
    egotap_overlay_style st = q;
    if (marks) {
        EGO_CHECK(((uintptr_t)marks & 15) == 0, "%s: marks must be 16-byte aligned", who);
        EGO_CHECK(q.n_marks >= 1 && q.n_marks <= EGOTAP_OVERLAY_MAX, "%s: style: n_marks must be between 1 and %d (%d)", who, EGOTAP_OVERLAY_MAX, q.n_marks);
        EGO_CHECK(q.n_bones >= 0 && q.n_bones <= EGOTAP_OVERLAY_MAX, "%s: style: n_bones must be between 0 and %d (%d)", who, EGOTAP_OVERLAY_MAX, q.n_bones);
        for (int l = 0; l < q.n_bones; ++l)
            EGO_CHECK(q.bones[l][0] < q.n_marks && q.bones[l][1] < q.n_marks, "%s: style: bone %d joins marks %d and %d, outside 0 .. %d", who, l, q.bones[l][0],
                      q.bones[l][1], q.n_marks - 1);
    } else {
        st.n_marks = st.n_bones = 0;
    }
    const size_t canvas = (size_t)B * Hc * Wc * 3;
    const struct {
        const char* name;
        const void* p;
        size_t n;
    } arg[10] = {{"left8", left8, canvas},
                 {"right8", right8, canvas},
                 {"out_left8", out_left8, canvas},
                 {"out_right8", out_right8, canvas},
                 {"heat8", heat8, heat8 ? (size_t)B * E * S * S : 0},
                 {"tx_left", heat8 ? tx_left : nullptr, (size_t)Wc * 4},
                 {"ty_left", heat8 ? ty_left : nullptr, (size_t)Hc * 4},
                 {"tx_right", heat8 && E == 2 ? tx_right : nullptr, (size_t)Wc * 4},
                 {"ty_right", heat8 && E == 2 ? ty_right : nullptr, (size_t)Hc * 4},
                 {"marks", marks, marks ? (size_t)B * E * st.n_marks * 16 : 0}};
    for (int i = 0; i < 10; ++i)
        for (int j = i + 1; j < 10; ++j) {
            if ((i == 0 && j == 2 && out_left8 == left8) || (i == 1 && j == 3 && out_right8 == right8)) continue;      // in place
            EGO_CHECK(!ego_overlap(arg[i].p, arg[i].n, arg[j].p, arg[j].n), "%s: %s overlaps %s", who, arg[j].name, arg[i].name);
        }
    const OverlayEye el{left8, out_left8, heat8 ? tx_left : nullptr, heat8 ? ty_left : nullptr};
    const OverlayEye er{right8, out_right8, heat8 && E == 2 ? tx_right : nullptr, heat8 && E == 2 ? ty_right : nullptr};
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "overlay_u8", "overlay_u8_kernel", 0.0);
    EGO_HIP(overlay_u8_launch(el, er, E, B, Hc, Wc, heat8, S, marks, st, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}

// ---- a camera rig per stream (ocam.h, stereo_fuse.h, lens_remap.h): a table of S rigs, or S lens maps per eye, in device memory; frame b of a
// time-major batch is served by rig or map b % S.  The entries stand last in part 0's text, behind every kernel the other entries reference.
extern "C" int egotap_stereo_rigs_check(const egotap_stereo_rig* rigs_host, int S) {
    static const char* const who = "egotap_stereo_rigs_check";
    EGO_CHECK(rigs_host, "%s: null rig table (rigs_host is S egotap_stereo_rig in host memory)", who);
    EGO_CHECK(S >= 1 && S <= EGOTAP_MAX_STREAM_RIGS, "%s: the number of streams must be between 1 and %d (S = %d)", who, EGOTAP_MAX_STREAM_RIGS, S);
    for (int s = 0; s < S; ++s) {
        const egotap_stereo_rig& r = rigs_host[s];
        const char* why = ocam_refusal(&r.left);
        EGO_CHECK(!why, "%s: rig %d: left: %s", who, s, why);
        why = ocam_refusal(&r.right);
        EGO_CHECK(!why, "%s: rig %d: right: %s", who, s, why);
        bool fin = true;
        for (int k = 0; k < 9; ++k) fin = fin && ego_finite(r.R[k]);
        EGO_CHECK(fin, "%s: rig %d: R must be finite", who, s);
        for (int k = 0; k < 3; ++k) fin = fin && ego_finite(r.t[k]);
        EGO_CHECK(fin, "%s: rig %d: t must be finite", who, s);
        for (int k = 0; k < 8; ++k) fin = fin && ego_finite(r.affine[k / 4][k % 4]);
        EGO_CHECK(fin, "%s: rig %d: affine must be finite", who, s);
        EGO_CHECK(ego_finite(r.min_score), "%s: rig %d: min_score must be finite", who, s);
    }
    return EGOTAP_OK;
}
// what the two per-stream stereo entries refuse about the table and the batch, after the sizes
static int stereo_rig_table_checks(const char* who, int B, const egotap_stereo_rig* rigs_dev, int S) {
    EGO_CHECK(rigs_dev, "%s: null rig table (rigs_dev is S egotap_stereo_rig in device memory)", who);
    EGO_CHECK(((uintptr_t)rigs_dev & 7) == 0, "%s: the rig table (rigs_dev) must be 8-byte aligned", who);
    EGO_CHECK(S >= 1 && S <= EGOTAP_MAX_STREAM_RIGS, "%s: the number of streams must be between 1 and %d (S = %d)", who, EGOTAP_MAX_STREAM_RIGS, S);
    EGO_CHECK(B % S == 0, "%s: the batch must be a multiple of the number of streams: frame b uses rig b %% S (B = %d, S = %d)", who, B, S);
    return EGOTAP_OK;
}
extern "C" int egotap_stereo_triangulate_streams(const float* keypoints, int B, int J, const egotap_stereo_rig* rigs_dev, int S, const float* pose, int P,
                                                 int pose_row0, float* joints3d, float* frame, void* stream) {
    static const char* const who = "egotap_stereo_triangulate_streams";
    EGO_CHECK(keypoints && joints3d && frame, "%s: null argument (keypoints, joints3d and frame are required; pose may be NULL)", who);
    EGO_CHECK((((uintptr_t)keypoints | (uintptr_t)joints3d | (uintptr_t)frame) & 15) == 0 && ((uintptr_t)pose & 3) == 0,
              "%s: keypoints, joints3d and frame must be 16-byte aligned, pose 4-byte aligned", who);
    if (int rc = stereo_batch_checks(who, B, J)) return rc;
    if (int rc = stereo_rig_table_checks(who, B, rigs_dev, S)) return rc;
    if (int rc = stereo_pose_rows_check(who, pose != nullptr, J, P, pose_row0)) return rc;
    if (int rc = stereo_triangulate_overlap_check(who, keypoints, B, J, pose, P, joints3d, frame)) return rc;
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "stereo_triangulate_streams", "stereo_triangulate_streams_kernel", 0.0);
    EGO_HIP(stereo_triangulate_streams_launch(keypoints, B, J, (const StereoRig*)rigs_dev, S, pose, P, pose_row0, joints3d, frame, (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_stereo_fuse_streams(const float* keypoints, int B, int J, const egotap_stereo_rig* rigs_dev, int S, const float* pose, int P, int pose_row0,
                                          const float* frame, const egotap_fuse_params* params, float* fused, float* pose_fused, float* stats, void* stream) {
    static const char* const who = "egotap_stereo_fuse_streams";
    EGO_CHECK(keypoints && pose && frame && params && fused && pose_fused && stats,
              "%s: null argument (keypoints, pose, frame, params, fused, pose_fused and stats are required)", who);
    EGO_CHECK((((uintptr_t)keypoints | (uintptr_t)frame | (uintptr_t)fused | (uintptr_t)stats) & 15) == 0 && (((uintptr_t)pose | (uintptr_t)pose_fused) & 3) == 0,
              "%s: keypoints, frame, fused and stats must be 16-byte aligned, pose and pose_fused 4-byte aligned", who);
    if (int rc = stereo_batch_checks(who, B, J)) return rc;
    if (int rc = stereo_rig_table_checks(who, B, rigs_dev, S)) return rc;
    if (int rc = stereo_pose_rows_check(who, true, J, P, pose_row0)) return rc;
    egotap_fuse_params prm;
    if (int rc = stereo_fuse_arg_checks(who, keypoints, B, J, pose, P, frame, params, fused, pose_fused, stats, prm)) return rc;
    GemmTimer tm(g_timing_handle, (hipStream_t)stream, "stereo_fuse_streams", "stereo_fuse_streams_kernel", 0.0);
    EGO_HIP(stereo_fuse_streams_launch(keypoints, B, J, (const StereoRig*)rigs_dev, S, pose, P, pose_row0, frame, prm, fused, pose_fused, stats, (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_lens_remap_streams(const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S, int S0, uint8_t* out_left8,
                                         uint8_t* out_right8, void* stream) {
    FrameSource q{};
    const char* why = lens_source_refusal(src, left8, right8, &q);
    if (!why) why = lens_streams_refusal(B, S);
    const int rc = sensor_op_checks("egotap_lens_remap_streams", B, S0, why, out_left8, out_right8);
    if (rc != EGOTAP_OK) return rc;
    EGO_HIP(lens_remap_streams_launch(left8, right8, B, q, (const int*)src->map_left, (const int*)src->map_right, S, 0L, lens_fill(src->fill[0]),
                                      lens_fill(src->fill[1]), S0, out_left8, out_right8, device_cu_count(), (hipStream_t)stream));
    return EGOTAP_OK;
}
extern "C" int egotap_predict_pose_lens_streams(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S,
                                                const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream) {
    return predict_pose_lens_entry("egotap_predict_pose_lens_streams", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false, nullptr,
                                   nullptr, true, S);
}
extern "C" int egotap_predict_pose_lens_streams_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S,
                                                   const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream,
                                                   float* keypoints) {
    return predict_pose_lens_entry("egotap_predict_pose_lens_streams_kp", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, true,
                                   keypoints, nullptr, true, S);
}
extern "C" int egotap_predict_pose_lens_streams_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S,
                                                    const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream,
                                                    float* keypoints, float* limbs) {
    return predict_pose_lens_entry("egotap_predict_pose_lens_streams_kpl", h, left8, right8, B, src, table, pose, heatmaps, chunk, ws, ws_bytes, stream, false,
                                   keypoints, limbs, true, S);
}
#endif
