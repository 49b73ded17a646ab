/* egotap_debug.h -- test and measurement hooks of libegotap_hip.so.
 *
 * Not part of the drop-in boundary (include/egotap.h): nothing here is needed to run, train or evaluate the hot path.  The entry
 * points exist for this repo's parity tests (tests/), its bench (bench.py) and its profiling scripts; they are exported by the same
 * library and follow the same conventions (return codes, egotap_last_error, caller's stream).
 */
#ifndef EGOTAP_DEBUG_H
#define EGOTAP_DEBUG_H
#include "egotap.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- fault injection ---- */
/* Test hook: launch the one-launch recurrence with its last `n` workgroups missing (0 = off), which starves a row block exactly as a
 * shared device does. */
int egotap_debug_pu_drop_workgroups(egotap_handle h, int n);

/* ---- partial forward (parity tests against the reference's per-layer hidden states, tests/golden/lift_fwd_*.npz) ---- */
/* debugging aid for parity tests: 0 = full forward (default); 1 = return after the embeddings;
 * 2+i = return after ViT layer i.  The state is then readable as intermediate "x". */
int egotap_lift_debug_stop(egotap_handle h, int stage);

/* ---- layer 0 of the pose-only forward (egotap_lift_predict_pose at batches that fill the chip): the exact-fp32 attention of egotap_attention_f32
 * where tokens [shared_from, N) are the same in every image and only image 0 holds their rows of qkv [B * N, 3 * heads * 128]: key tiles and query
 * blocks from shared_from on read image 0's rows; rows (b > 0, n >= shared_from) of qkv are not read; ctx [B * N, heads * 128] is written for every
 * image.  shared_from = N shares nothing (any N egotap_attention_f32 takes); below N both must be multiples of 32. */
int egotap_debug_attention_f32_shared(const float* qkv, float* ctx, int B, int N, int heads, int shared_from, void* stream);

/* ---- the exact-fp32 attention's other modes, one operator call each (tests/test_gpu_attention_f32_modes.py) ---- */
/* as egotap_lift_forward launches it: scratch (scratch_floats floats, caller-owned) takes the key-split partials [k][B * N][heads * 128] followed by
 * their log-sum-exps [k][B * heads * N]; the split count k is the library's own decision for (B, N, heads, scratch_floats, num_cu) -- 1 = unsplit,
 * scratch untouched -- and is what egotap_debug_attention_f32_ksplit returns for the same arguments. */
int egotap_debug_attention_f32_split(const float* qkv, float* ctx, int B, int N, int heads, float* scratch, size_t scratch_floats, int num_cu, void* stream);
/* the last ViT layer of egotap_lift_predict_pose: Nq live queries per image (32 <= Nq <= N), row b * Nq + i of q with a row stride of ldq floats (a
 * multiple of 4; q == qkv, ldq = 3 * heads * 128 is the product's layout), against the K / V columns of all N tokens of qkv; ctx [B * Nq, heads * 128]. */
int egotap_debug_attention_f32_live(const float* q, int64_t ldq, int Nq, const float* qkv, float* ctx, int B, int N, int heads, void* stream);
/* (host only: no device call) the key-split count of a forward: a divisor of the number of 32-key tiles, at most 8, that keeps B * heads * query
 * groups * k within 4.5 workgroups per compute unit and the partials within scratch_floats; 1 = unsplit.  Returns 0 -- never a split count -- with
 * egotap_last_error set when the arguments are refused (the return value is the count, so the usual error codes cannot be told from it). */
int egotap_debug_attention_f32_ksplit(int B, int N, int heads, size_t scratch_floats, int num_cu);

/* ---- measurement / test switch (process wide, one definition in the library): which K-tile depth the bf16-storage NT GEMM with plain
 * operands uses: 0 (default) = 64-deep kernel (csrc/gemm_bf16s64.h) where the shape allows, else the 32-deep one (csrc/gemm_bf16s.h);
 * 32 / 64 = always that one (64 fails on shapes it does not take).  Both run the same MFMAs in the same k order: bit-identical results. */
int egotap_debug_gemm_bk(int bk);

/* ---- measurement / test switch (process wide): how the 64-deep GEMM addresses a convolution operand (csrc/gemm_bf16s64.h): 0 (default) = one
 * wave-uniform origin + 32-bit lane offsets where map and zero page lie within 4 GB of each other, 1 = a 64-bit pointer per lane always.  The same
 * bytes are fetched either way: bit-identical results. */
int egotap_debug_conv_addressing(int mode);

/* ---- egotap_predict_pose_rgb: which form the last call on the handle took, and where its heatmaps live inside ws ---- */
/* *form: NONE before the first successful call; HEATMAPS = fp32 heatmaps written to the caller's tensor; SCRATCH = heatmaps == NULL, fp32 heatmaps in
 * ws; HANDOFF = heatmaps == NULL and conv_heatmap wrote the head's bf16 operand directly (no fp32 heatmaps anywhere) */
enum { EGOTAP_RGB_FORM_NONE = 0, EGOTAP_RGB_FORM_HEATMAPS = 1, EGOTAP_RGB_FORM_SCRATCH = 2, EGOTAP_RGB_FORM_HANDOFF = 3 };
int egotap_debug_predict_pose_rgb_form(egotap_handle h, int* form);
/* name "heatmaps" (after a SCRATCH call: f32 [B, 6J, S, S]) or "handoff" (after a HANDOFF call: bf16 [B, 6J, S, S], element (b, c, y, x) =
 * bf16(heatmaps[b, c, y, x]) -- the layout the head's patch-embedding and rotation-fc1 loaders gather from); the same slot of ws either way.
 * offset in bytes, numel in elements */
int egotap_debug_predict_pose_rgb_intermediate(egotap_handle h, int B, int chunk, const char* name, size_t* offset, int64_t* numel);

/* ---- host-side planning, exposed for unit tests ---- */
/* (test aid, host only: no device call) the number of partial slabs a weight-gradient launch splits its contraction into, and the slabs per split:
 * workgroups in a row on the busiest CU x slabs each + a fixed part per workgroup + the traffic of the slab reduction, within slab_bytes of
 * workspace.  0 when not even one slab of n_floats fits. */
int egotap_debug_wgrad_splits(int tiles, int64_t slabs, int64_t n_floats, size_t slab_bytes, int num_cu, int lds_bytes, double slab_us, double fixed_us,
                              int* per);

/* (test aid) which kernels the PU stage of training (egotap_train_pu_fwd, egotap_train_pu_bwd) launches at batch B on this handle: the batch alone
 * picks them, and the answers come from the predicates the launches themselves call.  out[n >= EGOTAP_PU_ROUTE_WORDS]:
 *   CHAIN        0 = per-step kernels, 1 = pu_chain_kernel<1>, 2 = pu_chain_kernel<2>;  CHUNKS = chain launches per layer (0 per step)
 *   ROW_BLOCKS   ceil(B / 16);  LAST_ROWS = rows of the last row block
 *   WGRAD_*[7]   weight gradients in the order of the grads argument (x2f0, x2h0, b2h0, h2h0, x2f1, x2h1, h2h1): SPLITS of the J * B rows,
 *                FAMILY (EGOTAP_TN_*), CAPPED = 1 when the workspace, not the shape, set the split count
 *   DGRAD_SPLITK[6]  input gradients (one step of the recurrence, x2h1, x2f1, b2h0, x2h0, x2f0): 1 = K split over the CUs
 *   COLSUM_GY    partial rows of the bias gradients' column sums over J * B rows
 * The first form asks the device (resident workgroups of the chain kernels, CU count; follows egotap_set_pu_chain and the handle's precision);
 * _for is host only: the caller states them. */
enum { EGOTAP_PU_ROUTE_CHAIN = 0, EGOTAP_PU_ROUTE_CHUNKS = 1, EGOTAP_PU_ROUTE_ROW_BLOCKS = 2, EGOTAP_PU_ROUTE_LAST_ROWS = 3, EGOTAP_PU_ROUTE_WGRAD_SPLITS = 4,
       EGOTAP_PU_ROUTE_WGRAD_FAMILY = 11, EGOTAP_PU_ROUTE_WGRAD_CAPPED = 18, EGOTAP_PU_ROUTE_DGRAD_SPLITK = 25, EGOTAP_PU_ROUTE_COLSUM_GY = 31,
       EGOTAP_PU_ROUTE_WORDS = 32 };
enum { EGOTAP_TN_NONE = 0, EGOTAP_TN_F32_BIG = 1, EGOTAP_TN_F32_SMALL = 2, EGOTAP_TN_F32_DMA = 3, EGOTAP_TN_BF16X3 = 4, EGOTAP_TN_BF16 = 5 };
int egotap_debug_pu_train_routes(egotap_handle h, int B, int* out, int n);
int egotap_debug_pu_train_routes_for(egotap_handle h, int B, int resident1, int resident2, int num_cu, int* out, int n);

/* ---- measurement hooks (bench.py roofline) ---- */
/* when enabled, every GEMM launch of the handle is bracketed by HIP events on the caller's stream */
int egotap_timing_enable(egotap_handle h, int enable);
/* synchronises the recorded events; returns launches, summed milliseconds and summed algorithmic FLOPs
 * of the fp32 GEMM kernel since the last reset, then resets */
int egotap_timing_read(egotap_handle h, int* launches, double* total_ms, double* total_flops);
/* JSON array written by the last egotap_timing_read: one object per GEMM role
 * {"role","kernel","launches","ms","flops"}; the pointer stays valid until the next read */
const char* egotap_timing_detail(egotap_handle h);

#ifdef __cplusplus
}
#endif
#endif /* EGOTAP_DEBUG_H */
