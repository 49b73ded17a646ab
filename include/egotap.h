/* egotap.h -- C ABI of libegotap_hip.so: EgoTAP's heatmap -> 3D lifting hot path on MI355X (gfx950).
 *
 * The reference (tho-kn/EgoTAP) is pure Python/PyTorch and has no FFI of its own; the boundary it
 * offers is the nn.Module call.  Each entry point below names the reference interface it replaces
 * (paths under the reference repo).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Contract
 *   - plain pointers and sizes only; every pointer marked "device" is a HIP device pointer owned
 *     by the caller (PyTorch allocates params, activations, workspace); the library borrows them.
 *   - no device allocation, no synchronisation, no internal streams: all work is enqueued on the
 *     caller's stream (pass torch.cuda.current_stream().cuda_stream as a void*).  Graph-capture safe
 *     after one eager call per handle (the first forward asks the device for its occupancy figures).
 *   - every function returns 0 on success, an EGOTAP_ERR_* code otherwise; the message is in
 *     egotap_last_error() (thread local).  No C++ exception crosses the ABI.
 *   - a handle is not thread-safe; data parallelism = one process + one handle per GPU.
 *   - the library reads no environment variable.  Test and measurement hooks (fault injection, partial forward, GEMM event timing)
 *     are exported too but declared separately, in egotap_debug.h: nothing a deployment calls.
 */
#ifndef EGOTAP_H
#define EGOTAP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): egotap_config grew (hm_blocks, round 3); test / measurement hooks moved to egotap_debug.h; egotap_pose_metrics_batch_axes added */
#define EGOTAP_ABI_VERSION 2

enum { EGOTAP_OK = 0, EGOTAP_ERR_INVALID = 1, EGOTAP_ERR_HIP = 2, EGOTAP_ERR_UNBOUND = 3, EGOTAP_ERR_WORKSPACE = 4 };

/* which of the wrapper's three networks a parameter belongs to
 * (model/egotap_autoencoder_model.py:109-111: net_AutoEncoder, net_HeatMap, net_RotHeatMap) */
enum { EGOTAP_NET_LIFT = 0, EGOTAP_NET_HM_POS = 1, EGOTAP_NET_HM_ROT = 2, EGOTAP_NET_COUNT = 3 };

enum { EGOTAP_F32 = 0, EGOTAP_I64 = 1, EGOTAP_BF16 = 2 };      /* (EGOTAP_BF16: egotap_heatmap_peaks' maps only; parameters are bound as F32 / I64) */

/* Options that shape the networks; mirrors the reference flags
 * --joint_preset/--num_heatmap/--ae_hidden_size/--load_size_heatmap (options/base_options.py:52-66,
 * options/dataset_options.py:29-41) and the fixed ViT/PU sizes of model/net_architecture.py:340-348, 650. */
typedef struct egotap_config {
    int32_t struct_bytes;   /* sizeof(egotap_config), for ABI checking */
    int32_t n_joints_hm;    /* heatmaps per eye: 15 UnrealEgo, 17 EgoCap */
    int32_t estimate_head;  /* 1: UnrealEgo (head joint + global offset from global_mlp), 0: EgoCap */
    int32_t hm_size;        /* heatmap side (64; 128 for 512x512 RGB) */
    int32_t hidden;         /* --ae_hidden_size (128) */
    int32_t vit_dim;        /* 1024 */
    int32_t vit_heads;      /* 8 */
    int32_t vit_layers;     /* 3 */
    int32_t patch;          /* 16 */
    int32_t pu_hidden;      /* 512 */
    int32_t hm_blocks[4];   /* BasicBlocks per ResNet stage of the heatmap estimators (--model_name, net_architecture.py:57-64):
                             * {2,2,2,2} resnet18 (all zeros mean this), {3,4,6,3} resnet34; at most 6 per stage */
} egotap_config;

typedef struct egotap_handle_s* egotap_handle;

/* library */
int egotap_abi_version(void);
const char* egotap_last_error(void);

/* replaces network.define_AutoEncoder / define_HeatMap (model/network.py:11-33): host-side state only */
int egotap_create(const egotap_config* cfg, egotap_handle* out);
void egotap_destroy(egotap_handle h);

/* replaces nn.Module parameter ownership: bind one state_dict entry (the reference's own key,
 * SURVEY.md Appendix B, e.g. "pos_heatmap_encoder.vit.encoder.layer.0.attention.attention.query.weight")
 * to a device pointer.  numel and dtype are checked against the expected shape. */
int egotap_bind_param(egotap_handle h, int net, const char* state_dict_key, void* dev_ptr, int64_t numel, int dtype);
/* number of state_dict entries the forward of `net` needs that are not bound yet (0 = ready) */
int egotap_unbound_count(egotap_handle h, int net, int* count);

/* EgoTAPAutoEncoder.forward / predict_pose (model/net_architecture.py:679-758), eval mode:
 *   hm    device f32 [B, 6*n_joints_hm, hm_size, hm_size]  (L pos, R pos, L cos, L sin, R cos, R sin)
 *   pose  device f32 [B, n_joints_hm + estimate_head, 3]   (head joint last)
 *   ws    device scratch of at least egotap_lift_workspace_bytes(B), 256-byte aligned
 * The reference's three all-zero outputs (rot, indep_pos, reconstructed heatmaps; :718-719, 756) are
 * not computed here: the host mirror returns cached zeros. */
int egotap_lift_workspace_bytes(egotap_handle h, int B, size_t* bytes);
int egotap_lift_forward(egotap_handle h, const float* hm, int B, float* pose, void* ws, size_t ws_bytes, void* stream);
/* [r6] predict_pose: the same arguments, checks and pose bits as egotap_lift_forward, but only `pose` is defined afterwards.  Where
 * every product of the last ViT layer would run unsplit (exact fp32, batches that fill the chip) that layer runs on the live tokens
 * alone -- the grid's dummy cells feed it only through their keys and values, and fc1 never reads their outputs.  Otherwise, and
 * whenever egotap_lift_debug_stop is set, it runs the full forward. */
int egotap_lift_predict_pose(egotap_handle h, const float* hm, int B, float* pose, void* ws, size_t ws_bytes, void* stream);

/* where an intermediate lives inside ws after egotap_lift_forward (for parity tests):
 * name in {"tokens","pos_embed","rot_embed","skel_embed"}; offset in bytes, numel in floats.
 * After egotap_lift_predict_pose "tokens" (and "x") are unspecified: the pruned last layer leaves compact rows there. */
int egotap_lift_intermediate(egotap_handle h, int B, const char* name, size_t* offset, int64_t* numel);

/* HeatMap_UnrealEgo_Shared.forward(left, right) (model/net_architecture.py:25-173; resnet18 backbone), eval mode:
 *   net    EGOTAP_NET_HM_POS (2*n_joints_hm output channels) or EGOTAP_NET_HM_ROT (4*n_joints_hm)
 *   left, right  device f32 [B, 3, 4*hm_size, 4*hm_size]
 *   out    device f32, channel 0 of this net's output; image b starts at out + b*out_image_stride (floats), so the
 *          result can be written straight into a channel slice of the lifting head's input
 *          (torch.cat of egotap_autoencoder_model.py:195-216 is never materialised)
 *   ws     device scratch of at least egotap_hm_workspace_bytes(B), 256-byte aligned (shared by both nets)
 * Heatmap sides: every hm_size the handle accepts (a multiple of 16; RGB 4*hm_size).  The bf16 channels-last path (EGOTAP_PREC_BF16)
 * and the bf16 matrix-core convolutions (EGOTAP_PREC_BF16X3 / _BF16) exist at sides 64 and 128 only; at every other side each precision
 * mode runs the exact-fp32 path BY NAME (the same launches and bits as EGOTAP_PREC_F32), as egotap_attention does for ragged sequences.
 * Convolutions whose map width has no power-of-two instantiation run on conv_f32_any_kernel (exact fp32, batch-independent bits). */
int egotap_hm_workspace_bytes(egotap_handle h, int B, size_t* bytes);
int egotap_hm_forward(egotap_handle h, int net, const float* left, const float* right, int B, float* out,
                      int64_t out_image_stride, void* ws, size_t ws_bytes, void* stream);
/* name in {"layer0".."layer4" (backbone pyramid, images interleaved n = 2b + eye), "conv_up3","conv_up2","conv_up1"} (fp32 NCHW).
 * EGOTAP_PREC_BF16 at sides 64 / 128: "pool0" and "layer1_bf16".."layer4_bf16" hold the pyramid as bf16 [B * s^2, left C | right C]; "u4",
 * "cat3", "conv_up3", "cat2", "conv_up2", "cat1", "conv_up1" hold the decoder's bf16 channels-last maps [B * s^2, C] with C = 1024, 1600
 * (1540 + zero padding), 1024, 1280, 512, 640, 512 (numel stays the fp32 layout's). */
int egotap_hm_intermediate(egotap_handle h, int B, const char* name, size_t* offset, int64_t* numel);
/* [r5] The same forward with BATCH-statistics BatchNorm2d and no graph: what the reference's FROZEN estimators compute while the lifting
 * head trains -- train.py:91 model.train() leaves their BatchNorm2d in training mode (model/egotap_autoencoder_model.py:127-129 freezes
 * parameters only, :177-216 calls them under autocast); the shared backbone runs once per eye (model/net_architecture.py:45-50), so each
 * BatchNorm normalises every eye's batch with that eye's statistics and updates its bound buffers twice per call, left then right:
 * running_mean / running_var (momentum 0.1, unbiased variance) and, where bound as EGOTAP_I64, num_batches_tracked += 2.
 * EGOTAP_PREC_BF16 only (bf16 channels-last kernels; the fp32 form is composed from egotap_hmtrain_conv_fwd / egotap_hmtrain_bn2d_fwd).
 * The backbone runs over the whole batch (its statistics couple the frames); the decoder, which has no BatchNorm, runs in pieces of
 * `chunk` frames (0 = the whole batch) so that its scratch stays at the chunk's size.  B >= 2.  Arguments as egotap_hm_forward;
 * ws at least egotap_hm_forward_bnbatch_workspace_bytes(B, chunk).  Heatmap sides 64 and 128 only: EGOTAP_ERR_INVALID, naming them, at any other. */
int egotap_hm_forward_bnbatch_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes);
int egotap_hm_forward_bnbatch(egotap_handle h, int net, const float* left, const float* right, int B, float* out, int64_t out_image_stride,
                              int chunk, void* ws, size_t ws_bytes, void* stream);
/* where a backbone map lives inside ws after egotap_hm_forward_bnbatch (parity tests): name in {"pool0" (stem + max-pool), "layer1" ..
 * "layer4"}; bf16 [B * s * s, 2 C], pixel (b, y, x) = [left C | right C]; offset in bytes, numel in bf16 elements */
int egotap_hm_forward_bnbatch_intermediate(egotap_handle h, int B, int chunk, const char* name, size_t* offset, int64_t* numel);

/* ---- stereo RGB -> pose in one call (serving; needs no ground truth) ----
 * What utils/evaluate.py:104-114 does per batch without the metrics -- model.set_input(data) + model.evaluate() -- i.e. the wrapper's
 * forward_heatmap() + net_AutoEncoder.predict_pose() (model/egotap_autoencoder_model.py:177-223) on a handle that has all three networks bound:
 * both estimators in eval mode (folded running statistics) in pieces of `chunk` frames (0 = the whole batch; a piece is what one
 * egotap_hm_forward call would get, so a frame's heatmaps are those of egotap_hm_forward at that piece's size), sharing one U-Net scratch, then
 * the head through the egotap_lift_predict_pose route.  Every kernel is the one the separate entries choose for the handle's precision and heatmap
 * side, and the arenas of egotap_lift_freeze / egotap_hm_freeze are honoured as those entries honour them.
 *   left, right  device f32 [B, 3, 4*hm_size, 4*hm_size]
 *   pose         device f32 [B, n_joints_hm + estimate_head, 3]          (egotap_lift_predict_pose's layout)
 *   heatmaps     NULL, or device f32 [B, 6*n_joints_hm, hm_size, hm_size]: the head's input (position net -> channels [0, 2J), limb net ->
 *                [2J, 6J)), the same bits as egotap_hm_forward writes
 *   ws           device scratch of at least egotap_predict_pose_rgb_workspace_bytes(B, chunk), 256-byte aligned
 * The workspace holds one fp32 [B, 6J, S, S] slot for the heatmaps whatever the call passes (one size per (B, chunk): a server sizes it once); a caller
 * that passes `heatmaps` does not use the slot, the hand-off uses half of it.
 * heatmaps == NULL: the heatmaps live in ws.  In EGOTAP_PREC_BF16 at heatmap sides 64 / 128, where the head takes its bf16-storage route (a
 * weight scratch attached), they are then never written in fp32 at all: the head's only use of them is a bf16 (round-to-nearest-even) copy, and
 * conv_heatmap's epilogue writes that copy itself -- the same rounding of the same sums, so the pose has the bits of the call with heatmaps given.
 * Unlike the older entries this one reports EVERY refusal as EGOTAP_ERR_INVALID, by name and before any launch: a NULL handle / left / right /
 * pose / ws, B <= 0, chunk < 0, a misaligned pointer (16 bytes; ws 256), a workspace that is too small, a network with unbound parameters. */
int egotap_predict_pose_rgb_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes);
int egotap_predict_pose_rgb(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                            size_t ws_bytes, void* stream);

/* ---- camera bytes: uint8 stereo frames straight into the stems (additive; EGOTAP_ABI_VERSION stays 2) ----
 * What a camera, decoder or capture card delivers is uint8 HWC; the reference turns it into the estimators' input offline (reprocess_*_data.py ->
 * utils/util.py:437-440, :188-197 normalize_ImageNet): astype(float32) / 255, subtract the mean, divide by the std, HWC -> CHW.  The normalised value
 * of a pixel is a function of one byte and one channel, so these entries take the bytes and a 768-entry table instead:
 *   left8, right8  device uint8 [B, S0, S0, 3], RGB order, S0 = 4*hm_size, contiguous; the base pointer 4-byte aligned (a row is 3*S0 bytes, a
 *                  multiple of 4: rows are read as aligned dwords, and no load touches a byte outside B*S0*S0*3)
 *   table          device f32 [3][256], 16-byte aligned, caller-owned: table[c][v] = float32((float64(float32(v) / float32(255)) - mean[c]) / std[c])
 *                  (egotap_amd/spec.py rgb_u8_table builds it; pinned against the reference by tests/golden/rgb_u8_norm.npz)
 * Every result equals, bit for bit, that of the fp32 entry on the host gather T(x8)[b][c][y][x] = table[c][x8[b][y][x][c]]: the byte paths read the
 * same values and keep every summation order.  Pixels outside the image are 0.0 as ever (not table[c][0]).  Every refusal is EGOTAP_ERR_INVALID,
 * by name and before any launch: null frames / table / outputs, a misaligned pointer, a workspace that is too small, unbound parameters.
 *
 * egotap_rgb_u8_to_f32: the standalone converter to the planar fp32 layout the other entries read (left_f32, right_f32: device f32
 *   [B, 3, S0, S0], 16-byte aligned; S0 any positive multiple of 4); one launch, 3 bytes in and 12 out per pixel.  B = 0 is a no-op.
 * egotap_hm_forward_u8: egotap_hm_forward from bytes.  Heatmap sides 64 / 128: the stem kernels stage the bytes themselves (the bf16 channels-last
 *   stem in EGOTAP_PREC_BF16, the fp32 matrix-core stem otherwise) and everything behind the stem is the launches of egotap_hm_forward; the workspace
 *   is egotap_hm_workspace_bytes(B).  Every other side: the converter runs into a slice at the end of the workspace, which is larger by exactly
 *   B*2*3*S0*S0*4 bytes, and the forward proceeds as egotap_hm_forward.
 * egotap_predict_pose_rgb_u8: egotap_predict_pose_rgb with the byte source -- the same composition, chunk walk, hand-off, frozen arenas and refusals.
 *   Workspace: egotap_predict_pose_rgb_workspace_bytes(B, chunk) at sides 64 / 128, larger by exactly chunk*2*3*S0*S0*4 bytes elsewhere (the
 *   converter runs chunk by chunk). */
int egotap_rgb_u8_to_f32(const uint8_t* left8, const uint8_t* right8, int B, int S0, const float* table, float* left_f32, float* right_f32,
                         void* stream);
int egotap_hm_forward_u8_workspace_bytes(egotap_handle h, int B, size_t* bytes);
int egotap_hm_forward_u8(egotap_handle h, int net, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* out,
                         int64_t out_image_stride, void* ws, size_t ws_bytes, void* stream);
int egotap_predict_pose_rgb_u8_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes);
int egotap_predict_pose_rgb_u8(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                               int chunk, void* ws, size_t ws_bytes, void* stream);

/* ---- the sensor's own frames: crop, mirror and bilinear resize on the device (additive; EGOTAP_ABI_VERSION stays 2) ----
 * No sensor delivers S0 x S0 frames; the reference brings them there offline (reprocess_egocap_data.py:72-88 crop_resize_images: centre crop,
 * F.interpolate(..., size=(256, 256), mode='bilinear', align_corners=False) on the uint8 tensor; :100-104, :221 a flip for the second camera; the loader's
 * resize to 4*hm_size, dataloader/data_loader.py:70-74).  These entries take the frames as they come:
 *   left8, right8  device uint8 [B, H, W, 3], RGB order, contiguous, 1 <= H, W <= 16384; every source byte is loaded as a byte at an offset inside
 *                  its rectangle, so no load touches a byte outside B*H*W*3
 *   rect           per eye four ints (x0, y0, w, h) in source pixels: inside the frame, w, h >= 1
 *   mirror         per eye 0 / 1: output column X takes what column S0 - 1 - X takes without it (the reference flips, then crops: its x0' in flipped
 *                  coordinates is x0 = W - x0' - w here)
 * The arithmetic is fixed in integers (egotap_amd/spec.py resize_taps / resize_u8 restate it on the host; the results are equal bit for bit).  Along an
 * axis of source length L the taps of output index X are n = max((2X + 1) L - S0, 0), i0 = n div 2S0, r = n mod 2S0, w1 = (r * 2048 + S0) div 2S0,
 * w0 = 2048 - w1, i1 = min(i0 + 1, L - 1); the output byte is (sum_{a, b} wy_a wx_b p[y0 + iy_a][x0 + ix_b][c] + 2^21) >> 22: one rounding, within
 * 0.5 + 510 / 4096 of exact bilinear interpolation.  w = h = S0 is an exact copy.
 * Every refusal is EGOTAP_ERR_INVALID, by name and before any launch: null pointers, B <= 0, a rectangle outside the frame or empty, a misaligned
 * base, a workspace that is too small, unbound parameters.
 *
 * egotap_rgb_u8_resize: the standalone operator, both eyes in one launch; out_left8 / out_right8 device uint8 [B, S0, S0, 3], 4-byte aligned, S0 a
 *   positive multiple of 4 (at most 4096); the source frames may sit at any address.
 * egotap_predict_pose_sensor_u8: egotap_predict_pose_rgb_u8 behind the resize -- rects 2 x 4 ints (left, right), mirrors 2 ints, host memory read
 *   during the call; left8 / right8 4-byte aligned.  The resize runs chunk by chunk into a workspace slice of chunk*2*3*S0*S0 bytes which the byte source
 *   then reads (the byte-source stems at sides 64 / 128, the converter elsewhere): same composition, hand-off, frozen arenas and refusals.  Workspace:
 *   egotap_predict_pose_rgb_u8_workspace_bytes(B, chunk) plus exactly that slice (H and W do not change it).  The identity request (H = W = S0, full
 *   rectangles, no mirror) reads the caller's frames in place and launches no resize. */
int egotap_rgb_u8_resize(const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rect_left, const int* rect_right, int mirror_left,
                         int mirror_right, int S0, uint8_t* out_left8, uint8_t* out_right8, void* stream);
int egotap_predict_pose_sensor_u8_workspace_bytes(egotap_handle h, int B, int H, int W, int chunk, size_t* bytes);
int egotap_predict_pose_sensor_u8(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects, const int* mirrors,
                                  const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream);

/* ---- 2D joints and confidences from the position heatmaps (additive; EGOTAP_ABI_VERSION stays 2) ----
 * What a tracker wants of the maps is where each joint is in each eye's image and how sure the estimator is: the ground-truth maps
 * (utils/projection.py:263-279 coord2d_to_heatmap) are unit-peak Gaussians for a joint in view and all zero for one out of view, so the peak value gates
 * "this joint was not seen".  Each map is reduced to one 16-byte record of four floats (x, y, score, index):
 *   index  iy * S + ix of the maximum.  Values are compared as fp32 (bf16 upcast exactly); a larger value wins, among equal values the smallest linear
 *          index; a NaN never beats a number; a map may be all negative (the maximum starts at -inf); a map of only NaNs gives index 0
 *   score  the element at index, as fp32
 *   x      ix + 0.5 + 0.25 * sgn(h[iy][ix + 1] - h[iy][ix - 1]): the reference's target puts its delta at int(x), so a joint in [ix, ix + 1) peaks at ix
 *          and ix + 0.5 is the unbiased read-out; the quarter-pixel step towards the higher neighbour is the usual one of heatmap estimators.  The step is
 *          0 where a neighbour lies outside the map or the difference is zero or NaN.  y the same from the rows above and below.  Exact in fp32.
 *   affine G groups of n / G consecutive channels, each (ax, bx, ay, by): x_out = fmaf(ax, x, bx), y_out = fmaf(ay, y, by).  NULL = identity:
 *          heatmap-pixel units, pixel centres at i + 0.5.  The values are read during the call and passed to the kernel by value.
 * Every record is defined bit for bit (egotap_amd/spec.py heatmap_peaks_ref restates it on the host).
 *
 * egotap_heatmap_peaks: the standalone operator; needs no handle, one launch on the caller's stream, allocates nothing.
 *   hm     device, EGOTAP_F32 or EGOTAP_BF16, the lifting head's input layout: element (b, c, y, x) at b * image_stride + c * S*S + y * S + x (elements),
 *          so a channel slice of a larger tensor is read in place; maps c0 .. c0 + n - 1 of each of the B images
 *   peaks  device f32 [B, n, 4]
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL hm / peaks; B, n or groups <= 0; more than 32 groups; n % groups != 0; c0 < 0;
 * image_stride < (c0 + n) * S*S or not a multiple of 16 bytes; S not a multiple of 16 or outside 16 .. 128; hm or peaks not 16-byte aligned; an unknown dtype.
 *
 * egotap_predict_pose_rgb_kp / _rgb_u8_kp / _sensor_u8_kp: the three one-call serving entries with one more output -- the same implementation, the parents
 * are it with keypoints = NULL.  keypoints: device f32 [B, 2, n_joints_hm, 4] (eye, joint, record), the peaks of the 2J position channels (c0 = 0, n = 2J,
 * groups = 2: one per eye) in ONE launch over the whole batch, after the last piece's estimators and before the head.  It reads the tensor the call
 * holds anyway: the fp32 `heatmaps` output, the workspace copy without one, or on the hand-off route the head's bf16 operand -- so the hand-off stays on
 * and the workspace sizes are the parents'.  Units: _rgb_kp and _rgb_u8_kp pixels of the S0 x S0 input frame (ax = ay = 4, bx = by = 0); _sensor_u8_kp
 * pixels of that eye's SENSOR frame, the inverse of the resize's map: for the eye's rectangle (x0, y0, w, h), ax = w / S, bx = x0 (mirrored: ax = -w / S,
 * bx = x0 + w), ay = h / S, by = y0, each rounded to fp32.  Further refusals (EGOTAP_ERR_INVALID, before any launch): a NULL keypoints, one that is not
 * 16-byte aligned, one that overlaps pose or heatmaps. */
int egotap_heatmap_peaks(const void* hm, int dtype, int B, int S, int64_t image_stride, int c0, int n, int groups, const float* affine, float* peaks,
                         void* stream);
int egotap_predict_pose_rgb_kp(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                               size_t ws_bytes, void* stream, float* keypoints);
int egotap_predict_pose_rgb_u8_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                                  int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints);
int egotap_predict_pose_sensor_u8_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects, const int* mirrors,
                                     const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints);

/* ---- limb elevation angles and 2D segments from the sin/cos limb heatmaps (additive; EGOTAP_ABI_VERSION stays 2) ----
 * The reference draws each target limb map as the anti-aliased segment parent -> joint, Gaussian-blurred and doubled, and multiplies it by cos(theta) and by
 * sin(theta), theta = arctan(dz / |dxy|) the limb's elevation out of the image plane (utils/data.py:197-252, dataloader/data_loader.py:193-199).  Each
 * (cos, sin) pair of maps c, s of side S is reduced to one 32-byte record of eight floats (theta, coherence, x, y, phi, length, peak, mass).  Values are
 * fp32 (bf16 upcast exactly); every sum runs over all S*S pixels in float64; pixel centres sit at ix + 0.5, iy + 0.5:
 *   m = sqrt(c^2 + s^2)   M = sum m   C = sum c   Sn = sum s   X = sum m x   Y = sum m y   XX = sum m x^2   YY = sum m y^2   XY = sum m x y
 *   theta      atan2(Sn, C), radians: exact for a target pair (both maps are the same non-negative map times sin / cos theta).  An angle of the pose's own
 *              frame: the affine and the mirror do not touch it
 *   coherence  hypot(C, Sn) / M, in [0, 1]: 1 when every pixel votes for the same angle
 *   x, y       ax * X/M + bx, ay * Y/M + by: the mass centre under the eye's affine (ax, bx, ay, by)
 *   phi        atan2(2 mu11', mu20' - mu02') / 2 in (-pi/2, pi/2]: the segment's orientation in the output frame, from the central moments
 *              mu20 = XX/M - (X/M)^2, mu02 = YY/M - (Y/M)^2, mu11 = XY/M - (X/M)(Y/M) scaled by ax^2, ay^2, ax ay
 *   length     sqrt(12 sqrt(D)), D = (mu20' - mu02')^2 + 4 mu11'^2: a uniform segment of length l blurred by an isotropic sigma has variance
 *              l^2/12 + sigma^2 along its axis and sigma^2 across it; the difference of the two eigenvalues is sqrt(D), so the blur drops out.  Exact when
 *              |ax| = |ay|: a non-uniform sensor crop makes the blur anisotropic in the output frame and bends phi and length
 *   peak       max m (a NaN never wins; starts at 0)
 *   mass       (float)M
 * The segment's ends are (x, y) +- length / 2 * (cos phi, sin phi).  Empty rule, when !(M > 0) or M is not finite (an all-zero pair, a NaN or inf
 * inside): theta = coherence = phi = length = 0, (x, y) the affine of the map centre (S/2, S/2), peak as computed, mass = (float)M.  A limb out of view has
 * all-zero target maps, so mass and peak gate "not seen" the way the keypoint score does.  Each value is rounded once from float64
 * (egotap_amd/spec.py limb_decode_ref restates the record on the host; the order of the sums differs, so the two agree to rounding, not in bits).
 *
 * egotap_limb_decode: the standalone operator; needs no handle, one launch on the caller's stream, allocates nothing.
 *   hm      device, EGOTAP_F32 or EGOTAP_BF16, the layout of egotap_heatmap_peaks.  For eye e and limb l the cos map is channel c0 + e * 2 n_limbs + l, the
 *           sin map channel c0 + e * 2 n_limbs + n_limbs + l: the reference's cat(cos, sin) per eye
 *   affine  host, [eyes, 4] = (ax, bx, ay, by) per eye; NULL = identity.  Read during the call and passed to the kernel by value
 *   limbs   device f32 [B, eyes, n_limbs, 8]
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL hm / limbs; B, n_limbs or eyes <= 0; more than 32 eyes; c0 < 0;
 * image_stride < (c0 + 2 eyes n_limbs) * S*S or not a multiple of 16 bytes; S not a multiple of 16 or outside 16 .. 128; hm or limbs not 16-byte aligned;
 * an unknown dtype.
 *
 * egotap_predict_pose_rgb_kpl / _rgb_u8_kpl / _sensor_u8_kpl: the three _kp entries with one more trailing output -- the same implementation.  Either of
 * keypoints / limbs may be NULL; with both NULL the call is the parent.  limbs: device f32 [B, 2, n_joints_hm, 8] (eye, limb, record), the records of the
 * 4J limb channels (c0 = 2J, n_limbs = J, eyes = 2) in ONE launch over the whole batch right after the keypoint launch, on the same tensor (the fp32
 * `heatmaps` output, the workspace copy, or on the hand-off route the head's bf16 operand: the hand-off stays on, the workspace sizes are the parents')
 * and with the keypoints' affine, so (x, y), phi and length are in the keypoints' units.  Further refusals (EGOTAP_ERR_INVALID, before any launch): a
 * keypoints or limbs that is not 16-byte aligned, keypoints overlapping pose or heatmaps, limbs overlapping pose, heatmaps or keypoints. */
int egotap_limb_decode(const void* hm, int dtype, int B, int S, int64_t image_stride, int c0, int n_limbs, int eyes, const float* affine, float* limbs,
                       void* stream);
int egotap_predict_pose_rgb_kpl(egotap_handle h, const float* left, const float* right, int B, float* pose, float* heatmaps, int chunk, void* ws,
                                size_t ws_bytes, void* stream, float* keypoints, float* limbs);
int egotap_predict_pose_rgb_u8_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const float* table, float* pose, float* heatmaps,
                                   int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints, float* limbs);
int egotap_predict_pose_sensor_u8_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, int H, int W, const int* rects, const int* mirrors,
                                      const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints,
                                      float* limbs);

/* ---- NV12 / YUYV sensor frames: colour conversion inside the resize (additive; EGOTAP_ABI_VERSION stays 2) ----
 * UVC, V4L2 and ISP pipelines hand out NV12 (4:2:0: a Y plane followed by an interleaved UV plane) or YUYV (packed 4:2:2), with a row pitch that is
 * usually wider than the image -- not uint8 RGB.  These entries read the camera's buffer itself: 1.5 or 2 bytes per pixel instead of 3, nothing is
 * unpacked or converted by the caller.  egotap_yuv_source describes one frame (egotap_amd/spec.py YuvLayout, YuvColour):
 *   struct_size   sizeof(egotap_yuv_source)
 *   format        EGOTAP_YUV_NV12: Y(y, x) at y * pitch + x; the chroma pair of pixel (y, x) at uv_offset + (y >> 1) * pitch + 2 * (x >> 1), U then V.
 *                   H and W even, pitch >= W, uv_offset >= pitch * (H - 1) + W, the last chroma byte inside frame_stride; pitch, uv_offset,
 *                   frame_stride and the address of frame 0 even (the chroma pair is one aligned 16-bit load)
 *                 EGOTAP_YUV_YUYV: the pixel pair x >> 1 of row y is the four bytes Y0 U Y1 V at y * pitch + 4 * (x >> 1).  W even, pitch >= 2 W, the last
 *                   row inside frame_stride; pitch, frame_stride and the address of frame 0 multiples of 4 (the pair is one aligned dword); uv_offset
 *                   is not read
 *   matrix, range EGOTAP_YUV_BT601 (Kr, Kb = 0.299, 0.114) or _BT709 (0.2126, 0.0722); EGOTAP_YUV_LIMITED (Y 16 .. 235) or _FULL (0 .. 255)
 *   H, W          1 .. 16384, the same for both eyes; frame b of an eye starts at b * frame_stride
 * Chroma is replicated: every pixel of a 2 x 2 block (NV12) or of a pair (YUYV) takes the block's U and V.  The arithmetic is fixed in integers
 * (spec.py yuv_to_rgb_u8 / yuv_resize_u8 restate it on the host; the results are equal bit for bit).  With Kg = 1 - Kr - Kb and (cy, cc, y_off) =
 * (255/219, 255/224, 16) limited or (1, 1, 0) full, the real coefficients are rv = 2 (1 - Kr) cc, bu = 2 (1 - Kb) cc, gu = 2 Kb (1 - Kb) / Kg cc,
 * gv = 2 Kr (1 - Kr) / Kg cc; each integer coefficient is round(real * 2^14), and
 *   R = clip((CY (Y - y_off) + RV (V - 128) + 2^13) >> 14, 0, 255)
 *   G = clip((CY (Y - y_off) - GU (U - 128) - GV (V - 128) + 2^13) >> 14, 0, 255)
 *   B = clip((CY (Y - y_off) + BU (U - 128) + 2^13) >> 14, 0, 255)
 * (arithmetic shift, one rounding: within 0.5 + (max |Y - y_off| + sum of max |C - 128| over the channel's chroma terms) * 2^-15 of the real formula).
 * Each of the four taps of an output pixel is converted to these bytes and the resize's bilinear formula (above) runs on them: the result is
 * egotap_rgb_u8_resize on the converted frame, bit for bit.  Nothing is interpolated in YUV.  No load touches a byte outside B * frame_stride or a
 * byte of a row past pitch.
 *
 * egotap_yuv_u8_resize: the standalone operator; needs no handle, one launch for both eyes on the caller's stream, allocates nothing.  Rectangles,
 *   mirrors, S0 and the outputs as egotap_rgb_u8_resize.
 * egotap_predict_pose_sensor_yuv / _kp / _kpl: egotap_predict_pose_sensor_u8 / _kp / _kpl with the descriptor in place of H, W -- the same walk: each
 *   piece is converted and resized ONCE into the workspace slice of chunk*2*3*S0*S0 bytes and both estimators read it as camera bytes; hand-off, frozen
 *   arenas, the keypoint affine (from the rectangles) and the limb records are the sensor entry's.  Workspace:
 *   egotap_predict_pose_sensor_u8_workspace_bytes(B, H, W, chunk) -- there is no query of its own.  There is no identity request: a YUV source always
 *   converts.  The descriptor, rects and mirrors are host memory read during the call.
 * Every refusal is EGOTAP_ERR_INVALID, by name and before any launch: a NULL descriptor or a wrong struct_size; an unknown format, matrix or range; an
 * odd H or W where the format needs it even; a pitch that is too small; planes that overlap; a last byte past frame_stride; a pitch, uv_offset,
 * frame_stride or frame address that is not a multiple of what the format's loads need (2 bytes for NV12, 4 for YUYV); and everything the RGB
 * operator or the sensor entry refuses. */
#define EGOTAP_YUV_NV12 0
#define EGOTAP_YUV_YUYV 1
#define EGOTAP_YUV_BT601 0
#define EGOTAP_YUV_BT709 1
#define EGOTAP_YUV_LIMITED 0
#define EGOTAP_YUV_FULL 1
typedef struct egotap_yuv_source {
    int32_t struct_size, format, matrix, range, H, W, pitch;
    int64_t uv_offset, frame_stride;
} egotap_yuv_source;
int egotap_yuv_u8_resize(const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rect_left, const int* rect_right,
                         int mirror_left, int mirror_right, int S0, uint8_t* out_left8, uint8_t* out_right8, void* stream);
int egotap_predict_pose_sensor_yuv(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                   const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream);
int egotap_predict_pose_sensor_yuv_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                      const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream,
                                      float* keypoints);
int egotap_predict_pose_sensor_yuv_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_yuv_source* src, const int* rects,
                                       const int* mirrors, const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream,
                                       float* keypoints, float* limbs);

/* ---- frames from another lens: a per-eye lens map in front of the one call (additive; EGOTAP_ABI_VERSION stays 2) ----
 * The estimators were trained on one fisheye lens.  A rig with another lens, another image centre or a camera mounted a few degrees off must show
 * them what THAT lens would have seen; the entries above only crop, mirror and resize.  These entries gather each frame through a LENS MAP: for every
 * pixel (X, Y) of the S0 x S0 frame the stems read, one entry (fx, fy) of int32 [S0 * S0][2] (row-major, entry Y * S0 + X): the pixel coordinates in
 * the sensor's H x W frame it is sampled at, in Q11 (pixels * 2048, rounded), or (-1, -1) where the sensor does not see it.  The map is built once
 * per rig on the host in float64 from the model camera's and the sensor's OCamCalib models and the rotation between them (egotap_amd/spec.py
 * lens_map: calibration pixel -> ray -> rotated ray -> sensor pixel, valid inside both image circles and the frame) and uploaded by the caller; the
 * library cannot inspect device memory, so that a map was built for this H x W is the caller's contract -- the kernel clamps every tap to the frame
 * on both sides, so whatever a map holds no load leaves B * frame bytes.  Per entry, with ix0 = fx >> 11, wx1 = fx & 2047, wx0 = 2048 - wx1,
 * ix1 = min(ix0 + 1, W - 1), and likewise iy0, wy1, wy0, iy1 from fy:
 *   byte = (wy0 (wx0 p[iy0][ix0] + wx1 p[iy0][ix1]) + wy1 (wx0 p[iy1][ix0] + wx1 p[iy1][ix1]) + 2^21) >> 22      (the resize's formula, above)
 * and the eye's fill bytes where the entry is invalid (spec.py lens_remap_u8 restates it on the host; equal bit for bit).  egotap_lens_source:
 *   struct_size   sizeof(egotap_lens_source)
 *   format        EGOTAP_LENS_RGB8: uint8 [B, H, W, 3] at any address.  EGOTAP_LENS_NV12 / _YUYV: the camera's buffer, described by the embedded `yuv`
 *                   (an egotap_yuv_source with the matching format and the same H, W; its rules and the frame alignment are those above); each tap is
 *                   converted to RGB bytes first -- the result is the RGB8 remap of the converted frame, nothing is interpolated in YUV
 *   H, W          the sensor frame, 1 .. 16384, the same for both eyes
 *   model_h, model_w, mirror[2]   the model camera's calibration image and the mirror flag each map was built with: read by the one-call entries only,
 *                   for the keypoint affine
 *   map_left, map_right   device pointers, 16-byte aligned, int32 [S0 * S0][2] each
 *   fill[2][3]    (R, G, B) of an invalid pixel, left eye then right
 * egotap_lens_remap: the standalone operator; needs no handle, ONE launch for both eyes on the caller's stream, allocates nothing.  S0 a positive
 *   multiple of 4, at most 4096; outputs uint8 [B, S0, S0, 3], 4-byte aligned.
 * egotap_predict_pose_lens / _kp / _kpl: egotap_predict_pose_sensor_u8 / _kp / _kpl with the descriptor in place of H, W, rectangles and mirrors -- the
 *   same walk: each piece is gathered ONCE into the workspace slice of chunk*2*3*S0*S0 bytes (S0 = 4 * hm_size) and both estimators read it as camera
 *   bytes; hand-off, frozen arenas and the limb records are the sensor entry's.  Keypoints and limb records come out in the MODEL camera's calibration
 *   pixels: per eye the sensor entry's affine for the rectangle (0, 0, model_w, model_h) and mirror[eye] (ax = model_w / S, bx = 0; mirrored:
 *   ax = -model_w / S, bx = model_w; ay = model_h / S, by = 0).  Workspace: egotap_predict_pose_lens_workspace_bytes(B, chunk), equal to
 *   egotap_predict_pose_sensor_u8_workspace_bytes for any frame size.  There is no identity request: a lens source always gathers.  The descriptor is
 *   host memory read during the call; the maps must stay valid until the stream has run it.
 * Every refusal is EGOTAP_ERR_INVALID, by name and before any launch: a NULL descriptor, frame, map or output; a wrong struct_size; an unknown
 * format; H or W outside 1 .. 16384; a map that is not 16-byte aligned; an embedded yuv source of another format, H or W, or one egotap_yuv_u8_resize
 * refuses (layout, matrix, range, frame alignment); S0 not a positive multiple of 4 up to 4096 or outputs not 4-byte aligned (the operator);
 * model_h or model_w outside 1 .. 16384 (the one-call entries); B <= 0; and everything the sensor entry refuses about its other arguments. */
#define EGOTAP_LENS_RGB8 0
#define EGOTAP_LENS_NV12 1
#define EGOTAP_LENS_YUYV 2
typedef struct egotap_lens_source {
    int32_t struct_size, format, H, W, model_h, model_w, mirror[2];
    const int32_t *map_left, *map_right;
    uint8_t fill[2][3];
    egotap_yuv_source yuv;
} egotap_lens_source;
int egotap_lens_remap(const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S0, uint8_t* out_left8, uint8_t* out_right8,
                      void* stream);
int egotap_predict_pose_lens_workspace_bytes(egotap_handle h, int B, int chunk, size_t* bytes);
int egotap_predict_pose_lens(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                             float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream);
int egotap_predict_pose_lens_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                                float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints);
int egotap_predict_pose_lens_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, const float* table,
                                 float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints, float* limbs);

/* ---- the fisheye camera model and stereo triangulation of the keypoints (additive; EGOTAP_ABI_VERSION stays 2) ----
 * The reference carries each camera as an OCamCalib model (utils/projection.py:13-144): cam2world takes a pixel to a unit ray through the polynomial
 * pol in the pixel radius, world2cam a 3D point to its pixel through the polynomial invpol in the elevation angle, both behind the affine (c, d, e) and the
 * centre (xc, yc).  egotap_ocam is that model by value: doubles and two lengths, filled on the host (egotap_amd/spec.py OcamModel / ocam_from_json read the
 * reference's fisheye.calibration_{side}.json: xc = image_center[1], yc = image_center[0], affine = [c, d, e]).  ue_flip is 1.0 exactly for the model
 * named "unreal_ego_pose" (projection.py:96, 141), else 0.0.  All arithmetic is float64 without contraction, each polynomial the reference's
 * running-power sum (r_i *= r; z += r_i * pol[i]), inputs and outputs fp32, every output rounded once:
 *   project    (world2cam) with ue_flip y and z are negated first; norm = sqrt(x^2 + y^2); norm <= 1e-8 gives (xc, yc); otherwise theta = atan(z / norm),
 *              rho = invpol(theta), x' = x * (1 / norm) * rho, y' = y * (1 / norm) * rho, u = x' c + y' d + xc, v = x' e + y' + yc; with ue_flip v <- 2 yc - v
 *   unproject  (cam2world, as the inverse convention of project) with ue_flip v <- 2 yc - v first; invdet = 1 / (c - d e), xp = invdet ((u - xc) - d (v - yc)),
 *              yp = invdet (-e (u - xc) + c (v - yc)), r = sqrt(xp^2 + yp^2), zp = pol(r), ray = (xp, yp, zp) / |(xp, yp, zp)|; with ue_flip (rx, -ry, -rz)
 * egotap_amd/spec.py ocam_world2cam_ref / ocam_cam2world_ref restate both in float64 numpy, operation for operation; only atan and the divisions may differ
 * from the host in the last float64 bit.
 *
 * egotap_stereo_triangulate: keypoints [B, 2, J, 4] (what the _kp serving entries write: eye, joint, (x, y, score, index)) -> joints3d [B, J, 8] and
 * frame [B, 8].  R (row-major 3 x 3, NULL = identity) and t (3) are the right camera's axes and origin in the left camera's frame, in the pose's units;
 * affine ([2, 4] = (ax, bx, ay, by) per eye, NULL = identity) takes keypoint units to the calibration's pixels.  left, right, R, t and affine are host
 * memory, read during the call and passed to the kernel by value.  Per (frame, joint), float64 without contraction:
 *   seen  = both scores >= min_score (a NaN fails) and the four coordinates finite
 *   pL = (ax x + bx, ay y + by), dL = unproject_left(pL), dR = R unproject_right(pR), w0 = -t
 *   b = dL.dR, d = dL.w0, e = dR.w0, den = 1 - b^2, s = (b e - d) / den, u = (e - b d) / den
 *   PL = s dL, PR = t + u dR, X = (PL + PR) / 2, gap = |PL - PR|
 *   valid = seen and den > 0 and s > 0 and u > 0 and everything finite (with a pose: the joint's pose row too)
 * Per frame, summed over the valid joints in ascending joint order: n = #valid; with pose (device f32 [B, P, 3], NULL = none) and n >= 1,
 * t_hat = sum X / n - sum pose[pose_row0 + j] / n -- the pelvis-relative pose placed in the left camera's frame without ground truth -- and
 * disagree_j = |X_j - pose[pose_row0 + j] - t_hat|.
 *   joints3d = (X, Y, Z, gap, den, s, disagree, valid in {0, 1}); an invalid joint is all zeros
 *   frame    = (t_hat x, y, z, n, rms disagree, max disagree, rms gap, max gap); without a pose t_hat and the disagreements are 0; n = 0 gives zeros
 * One wave per frame (lane = joint, J <= 64), four frames per workgroup.  egotap_amd/spec.py stereo_triangulate_ref restates the records.
 *
 * All three need no handle, do one launch on the caller's stream, allocate nothing, and use plain vector stores: no atomics, no workspace.  While a handle's
 * timing hook is on (egotap_timing_enable; the handle enabled last) their launches are recorded there as ocam_project, ocam_unproject, stereo_triangulate.
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL or misaligned pointer (points 4, keypoints / joints3d / frame 16 bytes); an output that
 * overlaps an input or another output; N, B or J <= 0; J > 64; pose_row0 < 0 or pose_row0 + J > P; n_pol outside 1 .. 8, n_invpol outside 1 .. 24;
 * c - d e == 0; a non-finite calibration value, R, t, affine or min_score; a ue_flip that is neither 0 nor 1. */
#define EGOTAP_OCAM_MAX_POL 8
#define EGOTAP_OCAM_MAX_INVPOL 24
typedef struct egotap_ocam {
    double pol[EGOTAP_OCAM_MAX_POL];       /* polynomialC2W, n_pol coefficients */
    double invpol[EGOTAP_OCAM_MAX_INVPOL]; /* polynomialW2C, n_invpol coefficients */
    double xc, yc, c, d, e;
    double ue_flip;
    int32_t n_pol, n_invpol;
} egotap_ocam;
int egotap_ocam_project(const float* points3d, int N, const egotap_ocam* model, float* points2d, void* stream);
int egotap_ocam_unproject(const float* points2d, int N, const egotap_ocam* model, float* rays, void* stream);
int egotap_stereo_triangulate(const float* keypoints, int B, int J, const egotap_ocam* left, const egotap_ocam* right, const double* R, const double* t,
                              const double* affine, double min_score, const float* pose, int P, int pose_row0, float* joints3d, float* frame, void* stream);

/* ---- the lifted joints fused with the keypoint rays, one eye enough (additive; EGOTAP_ABI_VERSION stays 2) ----
 * The lifted pose placed by t_hat and the keypoints are two opinions about where a joint is.  egotap_stereo_fuse merges them per joint: the placed
 * joint is a prior with an isotropic standard deviation, every eye that sees the joint adds the constraint "the joint lies on my ray" with an angular
 * standard deviation, and the fused joint is the weighted least-squares point -- a 3 x 3 symmetric positive-definite solve, no iteration.  One ray is
 * enough: a joint only one eye sees is pulled onto that ray and keeps the prior's depth along it.  Nothing here was tuned on data.
 * keypoints, left, right, R, t, affine, min_score, pose, P and pose_row0 are egotap_stereo_triangulate's; frame [B, 8] is its frame record, of which only
 * t_hat = frame[0:3] and n = frame[3] are read.  params is host memory, read during the call:
 *   sigma_ray    angular standard deviation of a keypoint's ray [rad]
 *   sigma_prior  standard deviation of a lifted joint, in the pose's units
 *   max_sigma    the gate, in standard deviations; +inf: no gate
 *   min_joints   fewest triangulated joints behind a t_hat that places a prior
 * Float64 without contraction, every comparison false on a NaN, dot(p, q) = p0 q0 + p1 q1 + p2 q2 and |p| = sqrt(dot(p, p)), in exactly this order:
 *   per frame   root_ok = n >= min_joints and t_hat finite;  wp = 1 / (sigma_prior sigma_prior)
 *   prior       q = pose[pose_row0 + j];  exists when root_ok and q is finite;  x0 = q + t_hat.  Without a prior the record is all zeros.
 *   eye e       (left, then right) seen = score >= min_score and both coordinates finite;  d = the triangulation's dL / dR;  o = 0 (left), t (right)
 *               y0 = x0 - o, a = dot(d, y0), rho = |y0|, r = y0 - a d, sr = sigma_ray rho, sr2 = sr sr,
 *               g = |r| / sqrt(sr2 + sigma_prior sigma_prior)
 *               a seen eye is   not in front  when not (a > 0) or g is not finite      mode bit 32 (left) / 64 (right)
 *                               gated         otherwise, when not (g <= max_sigma)     mode bit 8 / 16
 *                               used          otherwise, with w = score / sr2          mode bit 2 / 4
 *   system      A = wp I, b = wp x0;  then per used eye, left before right:  m_kk = 1 - d_k d_k, m_kl = -(d_k d_l),  A_kl = A_kl + w m_kl (six entries),
 *               and for the right eye c_k = (m_k0 t_0 + m_k1 t_1) + m_k2 t_2, b_k = b_k + w c_k  (the left origin is 0 and adds nothing to b)
 *   LDL^T       l10 = A01 / A00, l20 = A02 / A00, D1 = A11 - l10 A01, c21 = A12 - l20 A01, l21 = c21 / D1, D2 = (A22 - l20 A02) - l21 c21
 *               z1 = b1 - l10 b0, z2 = (b2 - l20 b0) - l21 z1;  y0 = b0 / A00, y1 = z1 / D1, y2 = z2 / D2
 *               x2 = y2, x1 = y1 - l21 x2, x0' = (y0 - l10 x1) - l20 x2;  x = (x0', x1, x2).  The pivots are >= wp > 0.  Without a used eye x = x0: no solve.
 *   post-fit    per used eye v = x - o, c = dot(v, d), p = v - c d, res = |p| / sr;  the eye passes when res <= max_sigma and c > 0.
 *               A used eye that does not pass, or an x that is not finite, is the FALLBACK: x = x0 and mode bit 128; the used bits stay set.
 *   mode        bit 1 (a prior exists) plus the bits above
 * Outputs, f32, each value rounded once from float64:
 *   fused [B, J, 8]      (x, y, z, move = |x - x0|, res left, res right, share, mode), in the left camera's frame.  res is 0 for an eye that is not used
 *                        or whose res is not finite;  share = sw / (wp + sw) with sw the used eyes' w added left before right;  move and share are 0
 *                        where x = x0 (no used eye, fallback)
 *   pose_fused [B, P, 3] row pose_row0 + j = x - t_hat, subtracted in float64, where a fit was kept (a used eye, no bit 128).  Every other row -- no
 *                        prior, no used eye, fallback, rows outside the joint rows, every row of a frame without root_ok -- is the input's bits
 *                        ((q + t_hat) - t_hat need not return q: where nothing moved nothing is rounded again).  It takes pose's place in
 *                        egotap_pose_track's arguments.
 *   stats [B, 8]         (joints with a prior, joints whose kept fit used both eyes, joints whose kept fit used one eye, eyes rejected = eyes not in
 *                        front or gated plus the used eyes of a fallback, rms move, max move, rms res, max res).  move runs over the joints with a
 *                        prior, res over the used eyes of kept fits; the sums are added in ascending joint order, left before right; zeros where
 *                        there is nothing to count.
 * One wave per frame (lane = joint, J <= 64), four frames per workgroup, one launch on the caller's stream, no handle, no synchronisation, no allocation, no
 * atomics, no workspace, plain vector stores; recorded as stereo_fuse while a handle's timing hook is on.  pose_fused may be pose itself (in place): every
 * element is then read and written by the same thread.  egotap_amd/spec.py stereo_fuse_ref restates the records; FuseParams there holds the defaults.
 * EGOTAP_ERR_INVALID, by name and before any launch: what egotap_stereo_triangulate refuses of the arguments the two share (pose is required here); a NULL
 * frame, params, fused, pose_fused or stats; fused, stats or frame not 16-byte aligned, pose_fused not 4-byte aligned; a sigma_ray or sigma_prior that is
 * not finite and > 0; a max_sigma that is NaN or < 0; min_joints < 0; an output that overlaps an input or another output, except pose_fused == pose. */
typedef struct egotap_fuse_params {
    double sigma_ray, sigma_prior, max_sigma;
    int32_t min_joints;
} egotap_fuse_params;
int egotap_stereo_fuse(const float* keypoints, int B, int J, const egotap_ocam* left, const egotap_ocam* right, const double* R, const double* t,
                       const double* affine, double min_score, const float* pose, int P, int pose_row0, const float* frame, const egotap_fuse_params* params,
                       float* fused, float* pose_fused, float* stats, void* stream);

/* ---- a camera rig per stream: a rig table and a lens map per stream in front of the tracker (additive; EGOTAP_ABI_VERSION stays 2) ----
 * egotap_pose_track and egotap_skeleton_fit take T frames of S streams, time-major (frame b = t * S + s), one camera rig per stream.  These entries feed
 * them: each is the entry of the same name with S rigs or S lens maps in DEVICE memory in place of one, ONE launch for the whole batch, frame b served by
 * rig (or map) b % S.  B must be a multiple of S.  Nothing about a rig is a kernel argument, so a captured graph holds the table's address and not its
 * contents: a rig rewritten in place (in stream order) is served by the next replay.
 *
 * egotap_stereo_rig is one rig by value: the two models, R (row-major 3 x 3), t, affine ([2][4] = (ax, bx, ay, by) per eye) and min_score, every value
 * spelled out -- the identity R and affine that the single-rig entries take as NULL are written as numbers here, and the coefficients behind n_pol and
 * n_invpol are ignored.  792 bytes.  A TABLE is S of them, contiguous, 8-byte aligned, in device memory the caller owns and uploads.
 * egotap_stereo_rigs_check: host only, launches nothing.  rigs_host is the table in HOST memory before the upload.  EGOTAP_ERR_INVALID, by name and with
 *   the stream's index in the message ("rig 2: left: ..."): everything egotap_stereo_triangulate refuses about one rig -- n_pol outside 1 .. 8, n_invpol
 *   outside 1 .. 24, c - d e == 0, a non-finite calibration value, R, t, affine or min_score, a ue_flip that is neither 0 nor 1 -- and S < 1, S > 4096 or
 *   a NULL table.  The library cannot inspect device memory: that the uploaded table equals the checked one is the caller's contract, as for a lens map.
 *   The kernels are memory-safe whatever a table holds: the stream index is b % S, and n_pol is clamped to the array's length before the polynomial is
 *   read (the kernels unproject only and never read invpol), so a corrupt table gives wrong numbers and never a load outside the table.
 * egotap_stereo_triangulate_streams / egotap_stereo_fuse_streams: egotap_stereo_triangulate / egotap_stereo_fuse with (rigs_dev, S) in place of (left,
 *   right, R, t, affine, min_score).  The same records, the same kernels' shape (one wave per frame, lane = joint, four frames per workgroup), the same
 *   device functions: rows s, s + S, s + 2 S .. equal the single-rig entry on those rows with rig s in every bit -- where a value of the rig was loaded from
 *   does not enter the float64 arithmetic.  The wave of frame b reads rig b % S with uniform loads, once per wave.  One egotap_fuse_params serves all
 *   streams; pose_fused may be pose.  No handle, no atomics, no workspace, no allocation; recorded as stereo_triangulate_streams / stereo_fuse_streams
 *   while a handle's timing hook is on.  Refused by name before any launch: what the single-rig entry refuses of the arguments the two share; a NULL
 *   table or one that is not 8-byte aligned; S < 1 or S > 4096; B not a multiple of S.
 * egotap_lens_remap_streams, egotap_predict_pose_lens_streams / _kp / _kpl: egotap_lens_remap and egotap_predict_pose_lens / _kp / _kpl with S after the
 *   descriptor.  map_left and map_right then point at int32 [S][S0 * S0][2]: stream s's map starts s * 2 * S0 * S0 ints in (16-byte aligned where the
 *   first is, S0 being a multiple of 4), and frame b of the batch is gathered through map b % S.  H, W, the YUV layout, fill, mirror, model_h and
 *   model_w are shared by the streams: the model camera is one camera, every stream's keypoints come out in the same calibration pixels, and a stream's
 *   own crop or resize is expressed in its map.  The one-call entries gather piece by piece and each piece indexes by the frame's place in the whole
 *   batch, whatever chunk is.  Workspace: egotap_predict_pose_lens_workspace_bytes.  S = 1 gives the bits of the entries without _streams.  Refused by
 *   name before any launch: what the entry without _streams refuses; S < 1 or S > 4096; B not a multiple of S. */
#define EGOTAP_MAX_STREAM_RIGS 4096
typedef struct egotap_stereo_rig {
    egotap_ocam left, right;
    double R[9], t[3], affine[2][4], min_score;
} egotap_stereo_rig;
int egotap_stereo_rigs_check(const egotap_stereo_rig* rigs_host, int S);
int egotap_stereo_triangulate_streams(const float* keypoints, int B, int J, const egotap_stereo_rig* rigs_dev, int S, const float* pose, int P, int pose_row0,
                                      float* joints3d, float* frame, void* stream);
int egotap_stereo_fuse_streams(const float* keypoints, int B, int J, const egotap_stereo_rig* rigs_dev, int S, const float* pose, int P, int pose_row0,
                               const float* frame, const egotap_fuse_params* params, float* fused, float* pose_fused, float* stats, void* stream);
int egotap_lens_remap_streams(const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S, int S0, uint8_t* out_left8,
                              uint8_t* out_right8, void* stream);
int egotap_predict_pose_lens_streams(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S, const float* table,
                                     float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream);
int egotap_predict_pose_lens_streams_kp(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S,
                                        const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints);
int egotap_predict_pose_lens_streams_kpl(egotap_handle h, const uint8_t* left8, const uint8_t* right8, int B, const egotap_lens_source* src, int S,
                                         const float* table, float* pose, float* heatmaps, int chunk, void* ws, size_t ws_bytes, void* stream, float* keypoints,
                                         float* limbs);

/* ---- the pose, the root and the stereo joints filtered over time (additive; EGOTAP_ABI_VERSION stays 2) ----
 * Every serving output is a single-frame estimate; egotap_pose_track follows them over time with a One-Euro filter (Casiez et al. 2012) on 3-vectors in
 * which a missing sample is irregular sampling.  A TRACK is one 3-vector followed over time, a STREAM one camera rig.  A call carries T consecutive frames of
 * S streams, time-major: frame b = t * S + s, B = T * S.  Stream s has K = P + 1 + J tracks:
 *   0 .. P-1      pose[b, row]            (device f32 [B, P, 3])                             accepted when the three values are finite
 *   P (the root)  frame[b, 0:3] = t_hat   (device f32 [B, 8], the triangulation's; or NULL)  accepted when frame is given, n >= min_joints, t_hat is
 *                                                                                             finite, rms disagree <= max_disagree, rms gap <= max_gap
 *   P+1 .. P+J    joints3d[b, j, 0:3] = X (device f32 [B, J, 8], the triangulation's; NULL   accepted when valid == 1, X is finite,
 *                                          exactly when J = 0)                                gap <= max_joint_gap
 * Every comparison is false on a NaN; a threshold of +inf lets every value but a NaN through.  state [S, K, 12] float64 on the device holds per track
 * (x^[3], v^[3], m_prev[3], gap_t, age, live); all zeros is "never seen", so a reset is a memset.  One step of one track with measurement m, accept flag a
 * and step time dt, in float64 without contraction and in exactly this order; ok = dt finite and dt > 0; alpha(fc, te) = r / (r + 1) with
 * r = (6.283185307179586 fc) te:
 *   not live, a      x^ = m_prev = m, v^ = 0, gap_t = 0, age = 0, live = 1                               status 1, cutoff = min_cutoff  (needs no dt)
 *   not live, not a                                                                                      status 0, the record all zeros
 *   live, a and ok   te = gap_t + dt, ad = alpha(d_cutoff, te); per c: dx = (m_c - m_prev_c) / te, v^_c = v^_c + ad (dx - v^_c);
 *                    speed = sqrt(v^x v^x + v^y v^y + v^z v^z) (added in that order); fc = min_cutoff + beta speed, ax = alpha(fc, te);
 *                    per c: x^_c = x^_c + ax (m_c - x^_c); m_prev = m, gap_t = 0, age = 0                status 1, cutoff = fc
 *   live, otherwise  age += 1; if ok: gap_t += dt;  age > max_hold: the track's state zeroed             status 0, the record all zeros
 *                                                   else: x^, v^ unchanged                               status 2, cutoff = 0
 * The derivative is taken between ACCEPTED RAW samples (the paper's own code), so v^ converges to the slope of a ramp; a held frame is a missing sample:
 * the next accepted one sees the elapsed time te, and a dropped frame gives the bits of "the frame removed, the next dt longer".  A rejected measurement is
 * never read into the state.  Outputs are f32, each value rounded once from float64:
 *   tracks [B, K, 8] = (x^, y^, z^, v^x, v^y, v^z, cutoff, status)
 *   placed [B, P, 3] = the filtered pose row plus the filtered root, added in float64, when the root's status is 1 or 2; the filtered pose row alone when
 *                      it is 0; zeros for a pose row whose own status is 0 -- the skeleton in the left camera's frame, smoothed and held over bad frames
 * Time: dts (device f32 [T], one value per time step, shared by the S streams) or, with dts NULL, the host double dt for every step.
 * One wave per stream, four streams per workgroup, the T steps a loop inside the ONE launch, the state in registers between its one read and its one write;
 * no handle, no allocation, no atomics, no workspace, plain vector stores; recorded as pose_track while a handle's timing hook is on.  state_out may be
 * state_in (in place).  egotap_amd/spec.py pose_track_ref restates the records and the state; TrackParams there holds the defaults.
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL pose, state_in, state_out, tracks, placed or params; a misaligned pointer (f32 arrays 4 bytes,
 * tracks 16, the states 8); T, S or P <= 0; P > 64; J < 0, J > 64, J > 0 without joints3d or joints3d with J = 0; dts NULL with a dt that is not finite
 * and > 0; a min_cutoff or d_cutoff that is not finite and > 0; a beta that is not finite and >= 0; a gate that is NaN or < 0; min_joints < 0;
 * max_hold < 0; an output that overlaps an input or another output (state_out partly overlapping state_in included). */
typedef struct egotap_track_params {
    double pose_min_cutoff, pose_beta, pose_d_cutoff;       /* Hz, 1 / (pose unit / s), Hz */
    double root_min_cutoff, root_beta, root_d_cutoff;
    double joints_min_cutoff, joints_beta, joints_d_cutoff;
    double max_disagree, max_gap, max_joint_gap;            /* the gates, in the pose's units; +inf: off */
    int32_t min_joints, max_hold;                           /* fewest triangulated joints behind an accepted t_hat; most consecutive held steps */
} egotap_track_params;
int egotap_pose_track(const float* pose, const float* frame, const float* joints3d, int T, int S, int P, int J, const float* dts, double dt,
                      const egotap_track_params* params, const double* state_in, double* state_out, float* tracks, float* placed, void* stream);
/* ---- the same filter in a world frame, from the headset's own pose (additive; EGOTAP_ABI_VERSION stays 2) ----
 * egotap_pose_track filters in the left camera's frame, and the camera sits on a head: every head turn moves a motionless body through that frame, so the
 * filter either lags the whole skeleton or opens its cutoff and passes the jitter it exists to remove.  egotap_pose_track_world takes, per frame, the pose of
 * the LEFT CAMERA IN THE WORLD and filters there.  Tracks (K = P + 1 + J), state [S, K, 12] float64, time-major frames b = t * S + s, egotap_track_params,
 * dts / dt and the step are those of egotap_pose_track, all float64 without contraction.  New:
 *   rig_pose   device f64 [B, 12], 8-byte aligned: the row-major 3 x 4 (R | t) with x_w = R x_c + t, t in the pose's units
 *   ortho_tol  host double, >= 0
 * A frame's rig pose is SEEN when all three hold (every comparison false on a NaN): its 12 values are finite; every |E_ij| <= ortho_tol with
 * E_ij = ((r_i0 r_j0 + r_i1 r_j1) + r_i2 r_j2) - delta_ij; det R > 0 by cofactors along row 0,
 * det = (r00 (r11 r22 - r12 r21) - r01 (r10 r22 - r12 r20)) + r02 (r10 r21 - r11 r20).  (ortho_tol = +inf leaves only "finite products" and the sign of det.)
 * The acceptance tests of egotap_pose_track (finite, valid, gates) apply to the camera-frame values; an accepted measurement m then enters the step as
 *   the root and the joints (points)          m_w[r] = (((R[r][0] m0 + R[r][1] m1) + R[r][2] m2) + t[r])
 *   the pose rows (pelvis-relative offsets)   m_w[r] =  ((R[r][0] m0 + R[r][1] m1) + R[r][2] m2)
 * A frame whose rig pose is not seen accepts NO track: by the step's own rule that is a missing sample (the tracks hold, gap_t grows, they expire after
 * max_hold), and a rig pose that is not seen is never read into the state.  Outputs, f32, each value rounded once from float64:
 *   tracks       [B, K, 8]  as egotap_pose_track's, in the world
 *   placed_world [B, P, 3]  egotap_pose_track's placed rule: pose row + root while the root's status is 1 or 2, the pose row alone otherwise, zeros for a
 *                           pose row of status 0
 *   placed_cam   [B, P, 3]  the same float64 value p brought back into THIS frame's camera (what an overlay draws): d = p - t where the root took part,
 *                           d = p where it did not; out[c] = ((R[0][c] d0 + R[1][c] d1) + R[2][c] d2); zeros where placed_world is zeros and for a frame
 *                           whose rig pose is not seen
 * A STATE BELONGS TO THE FRAME IT WAS MADE IN: one written by egotap_pose_track holds camera-frame values, one written here world values (of one world:
 * re-anchoring the world needs a reset), and neither entry can tell.  A zeroed state suits both.
 * One launch of the same shape (one wave per stream, four streams per workgroup, the state in registers over the T steps), no handle, no allocation, no
 * atomics, no workspace, plain vector stores; recorded as pose_track_world while a handle's timing hook is on.  egotap_amd/spec.py pose_track_world_ref
 * restates it; spec.rig_pose / spec.rig_compose build the 12 values ("device in world o left camera in device").
 * EGOTAP_ERR_INVALID, by name and before any launch: everything egotap_pose_track refuses (its placed is placed_world here); a NULL or misaligned rig_pose
 * (8 bytes) or placed_cam (4 bytes); an ortho_tol that is NaN or < 0; any overlap that involves rig_pose, placed_world or placed_cam. */
int egotap_pose_track_world(const float* pose, const float* frame, const float* joints3d, const double* rig_pose, int T, int S, int P, int J, const float* dts,
                            double dt, const egotap_track_params* params, double ortho_tol, const double* state_in, double* state_out, float* tracks,
                            float* placed_world, float* placed_cam, void* stream);
/* ---- a rigid skeleton and bone rotations from the tracked pose (additive; EGOTAP_ABI_VERSION stays 2) ----
 * The trackers return joint POSITIONS, each row filtered on its own: a limb's length changes from frame to frame, and a skinned avatar is driven by a
 * rotation per bone.  egotap_skeleton_fit runs behind them: it calibrates a length per bone over time, re-imposes it, and derives a rotation per bone
 * against the avatar's rest pose.  Frames are egotap_pose_track's: T steps of S streams, time-major, b = t * S + s; a stream has P <= 64 rows.  All
 * arithmetic is float64 without contraction, in exactly the order written here; every comparison is false on a NaN; each output is rounded to f32 once.
 * THE RIG, egotap_skeleton_rig, a HOST struct of 2584 bytes, checked before any launch; the kernel takes what the entry derives from it (rest directions,
 * the rest frame, depths: 2344 bytes) by value, under the 4 KB kernel-argument segment:
 *   P, parent[P]      parent[j] = -1 makes j a ROOT ROW (its position passes through, it has no bone); otherwise 0 <= parent[j] < j (the walk's order)
 *   rest_pos[P][3]    the avatar's rest pose, in any unit; rest_dir[j] = d / sqrt((d0 d0 + d1 d1) + d2 d2) with d = rest_pos[j] - rest_pos[parent[j]]
 *   frame_rows[3]     (a, b, c), three distinct rows whose triangle orients the root rows.  The frame of three points, rows (e0, e1, e2):
 *                     e0 = normalize(x_b - x_c); w = x_a - (x_b + x_c) / 2; e1 = normalize(w - (w . e0) e0); e2 = e0 x e1; a norm that is zero or not
 *                     finite anywhere makes it DEGENERATE (an exactly collinear triangle; a nearly collinear one gives an ill-conditioned frame).
 *                     M_rest is the frame of rest_pos.
 *   mirror[P]         with has_mirror: the row on the other side of the body or -1, an involution; fixed_length[P], with has_fixed_length: the avatar's
 *                     own bone lengths; then nothing is calibrated and the state is neither read nor written (retargeting to other proportions)
 * egotap_skeleton_params: window >= 1, min_samples >= 0, max_dev >= 0 (relative; +inf: off), freeze 0 / 1; track_rows = K of tracks (0: P).  Nobody has
 * tuned these on data (spec.SkeletonParams holds the defaults 120, 10, +inf, 0).
 * state [S, P, 2] float64 on the device = (L^, n) per row; all zeros is uncalibrated, so a reset is a memset; state_out may be state_in (in place).
 * One step of one stream:
 *   1 seen      row j's three inputs are finite; with tracks (device f32 [B, K, 8], egotap_pose_track's records, K >= P) its status is also 1 or 2
 *   2 sample    non-root: d = x_j - x_p, l = sqrt((d0 d0 + d1 d1) + d2 d2); VALID when both ends are seen and l is finite and > 0; u_j = d / l
 *   3 update    valid, not frozen, and (n < min_samples or |l - L^| <= max_dev L^): n = min(n + 1, window), then L^ = L^ + (l - L^) / n -- the exact
 *               mean of the first `window` samples, then an exponential average with alpha = 1 / window; the first sample gives L^ = l in bits; a
 *               rejected sample is never read into the state (min_samples = 0 on an empty state accepts nothing: |l - 0| <= max_dev 0 is false)
 *   4 length    L_j = fixed_length[j]; else, after all rows' updates of this step, L^_j where n_j >= 1 -- (L^_j + L^_m) / 2 with a mirror m that also
 *               has n_m >= 1, so both sides get the same bits; unavailable otherwise
 *   5 rigid     a seen root row passes through; a non-root row with a valid sample, an available L_j and a parent whose rigid position is ok gets
 *               r_j[c] = r_p[c] + L_j u_j[c]; anything else is not ok and stores zeros, and so do all its descendants
 *   6 rotation  unit quaternions (w, x, y, z) with w >= 0 (at w == 0 the first non-zero of x, y, z is positive).  Root rows, when a, b, c are seen and
 *               their frame is not degenerate: Q = quat(M_cur M_rest^T) by Shepperd's rule (spec.quat_from_frames spells it out).  A non-root row
 *               with a valid sample and a parent whose rotation is ok: v = rotate(Q_p, rest_dir_j); the swing s is the shortest arc v -> u_j (c = v . u;
 *               c > -1 + 1e-12: s = normalize(1 + c, v x u); otherwise s = (0, normalize(v x e_k)), k the lowest index of the smallest |v_k|);
 *               Q_j = normalize(s (x) Q_p); local_j = conj(Q_p) (x) Q_j.  Anything else is not ok, stores the identity, and so do its descendants.
 *               TWIST about a bone cannot be observed from positions: it follows the parent.  (egotap_skeleton_fit_twist, below, observes it for
 *               the bones that have a POLE: from the plane of a bent two-bone chain.)
 * Outputs, f32, 16-byte aligned:
 *   rigid     [B, P, 4]  (x, y, z, flags), flags = 1 (position ok) + 2 (rotation ok) as a float
 *   rotations [B, P, 8]  (global wxyz, local wxyz); for a root row local = global
 *   lengths   [B, P, 2]  (L_j or 0, n_j); zeros for root rows (and n = 0 with fixed_length)
 * Global rotations and rigid positions live in the frame of the input: placed_world for an avatar in the world, placed / placed_cam for an overlay.
 * One launch on the caller's stream: one wave per stream, four streams per workgroup, lane j owns row j, the state in registers over the T steps, the
 * tree walked level by level with cross-lane reads; no handle, no allocation, no atomics, no workspace, plain vector stores, never synchronises;
 * recorded as skeleton_fit while a handle's timing hook is on.  egotap_amd/spec.py skeleton_fit_ref restates it.
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL points, rig, params or output; NULL states without fixed_length; a misaligned pointer (f32
 * inputs 4 bytes, the three outputs 16, the states 8); T, S or P <= 0; P > 64; a parent out of order or out of range; no root row; frame_rows out of
 * range or not distinct; a zero or non-finite rest bone; a degenerate rest frame; a mirror that is no involution or pairs a root row; a fixed_length that
 * is not finite and > 0 on a non-root row; window < 1; min_samples < 0; a max_dev that is NaN or < 0; tracks with 0 < track_rows < P; an output that
 * overlaps an input or another output (state_out partly overlapping state_in included). */
#define EGOTAP_SKELETON_MAX_ROWS 64
typedef struct egotap_skeleton_rig {
    int32_t P, has_mirror, has_fixed_length;
    int32_t frame_rows[3];
    int32_t parent[EGOTAP_SKELETON_MAX_ROWS];
    int32_t mirror[EGOTAP_SKELETON_MAX_ROWS];
    double rest_pos[EGOTAP_SKELETON_MAX_ROWS][3];
    double fixed_length[EGOTAP_SKELETON_MAX_ROWS];
} egotap_skeleton_rig;
typedef struct egotap_skeleton_params {
    double max_dev;
    int32_t window, min_samples, freeze, track_rows;
} egotap_skeleton_params;
int egotap_skeleton_fit(const float* points, const float* tracks, int T, int S, const egotap_skeleton_rig* rig, const egotap_skeleton_params* params,
                        const double* state_in, double* state_out, float* rigid, float* rotations, float* lengths, void* stream);
/* ---- bone twist from the bend plane of the child bone (additive; EGOTAP_ABI_VERSION stays 2) ----
 * egotap_skeleton_fit leaves the roll of a bone about its own axis to the parent, so an upper arm, a thigh or a shank never rolls and the child's swing
 * absorbs whatever roll the pose has: the local quaternion of an elbow that simply flexes is then no rotation about the elbow's hinge.  A bent two-bone
 * chain defines a plane, and the plane's normal fixes the roll of the upper bone.  egotap_skeleton_fit_twist is egotap_skeleton_fit with that one step
 * added; steps 1 - 5 and step 6 for root rows are egotap_skeleton_fit's, and rigid[..., 0:3], lengths and the state equal its outputs in bits.
 * THE TWIST TABLE, egotap_skeleton_twist, a HOST struct of 1808 bytes, checked before any launch; the kernel takes what the entry derives from it (pole as
 * int8, g, the two thresholds: 1616 bytes) by value beside the rig's 2344, 4056 bytes of arguments in all under the 4 KB kernel-argument segment:
 *   pole[P]           for row j the row c whose bone bends against j's bone, or -1: parent[c] == j, and j is no root row
 *   hinge[P][3]       row j's hinge axis IN THE REST POSE: where rest_dir_j x rest_dir_c would point if the joint were bent the way it anatomically bends;
 *                     only roughly at right angles to rest_dir_j: the entry takes g_j = normalize(hinge_j - (hinge_j . rest_dir_j) rest_dir_j) in float64
 *                     (the dot product added left to right) and refuses a hinge that is not finite or whose g_j has a norm below 1e-6 before normalising;
 *                     read only where pole[j] >= 0
 *   bend_lo, bend_hi  0 <= bend_lo < bend_hi <= 1, SINES of the bend angle: below bend_lo the twist is not observed, from bend_hi on it is fully taken.
 *                     spec.skeleton_twist defaults to sin 10 deg and sin 25 deg; nobody has tuned these on data.
 * Step 6 for a non-root row j with a valid sample and a parent whose rotation is ok: s the swing as above, Q_s = normalize(s (x) Q_p) (egotap_skeleton_fit's
 * Q_j before its sign).  When pole[j] = c >= 0 and c's sample is valid, float64 without contraction in this order, every comparison false on a NaN:
 *   m = u_j x u_c, sigma = sqrt((m0 m0 + m1 m1) + m2 m2)
 *   w = 0 unless sigma > bend_lo; w = 1 if sigma >= bend_hi; otherwise t = (sigma - bend_lo) / (bend_hi - bend_lo), w = (t t)(3 - 2 t)
 *   if w > 0: n = m / sigma; h = rotate(Q_s, g_j), h' = normalize(h - (h . u_j) u_j); b = normalize((1 - w) h' + w n); a norm that is zero or not finite
 *             (sigma's included) makes the twist NOT OBSERVED
 *   the twist tw is the arc h' -> b: k = h' . b; k > -1 + 1e-12: tw = normalize(1 + k, h' x b); otherwise the half turn ABOUT THE BONE, (0, u_j)
 *   Q_j = sign(normalize(tw (x) Q_s)) and the row's flags gain 4 (twist observed, w > 0)
 * Not observed: Q_j = sign(Q_s), as egotap_skeleton_fit has it, and the flags gain nothing.  Then local_j = sign(conj(Q_p) (x) Q_j) as there.  Descendants
 * read the twisted Q_j as their parent and their swings absorb it: rotate(Q_j, rest_dir_j) = u_j holds for every row as before.  Only square roots,
 * divisions, products and sums: no atan2, sin or cos.  The twist is taken frame by frame: over a straight limb (sigma <= bend_lo) it falls back to the
 * parent's, nothing is held.
 * Outputs as egotap_skeleton_fit's, with flags = 1 (position ok) + 2 (rotation ok) + 4 (twist observed).  One launch of the same shape, the second
 * instantiation of the same kernel: lane j takes its pole child's input position from the child's lane next to the bone sample; no handle, no allocation,
 * no atomics, no workspace, plain vector stores, never synchronises; recorded as skeleton_fit_twist while a handle's timing hook is on.
 * egotap_amd/spec.py skeleton_fit_twist_ref restates it; spec.skeleton_twist builds the table, spec.skeleton_hinges_from_pose takes the hinges from one
 * frame with bent elbows and knees.
 * EGOTAP_ERR_INVALID, by name and before any launch: everything egotap_skeleton_fit refuses; a NULL twist; a pole[j] that is not -1 and out of range, whose
 * parent is not j, or that is set on a root row; a hinge of a pole row that is not finite or (nearly) parallel to its rest bone; thresholds outside
 * 0 <= bend_lo < bend_hi <= 1 (a NaN included). */
typedef struct egotap_skeleton_twist {
    int32_t pole[EGOTAP_SKELETON_MAX_ROWS];
    double hinge[EGOTAP_SKELETON_MAX_ROWS][3];
    double bend_lo, bend_hi;
} egotap_skeleton_twist;
int egotap_skeleton_fit_twist(const float* points, const float* tracks, int T, int S, const egotap_skeleton_rig* rig, const egotap_skeleton_twist* twist,
                              const egotap_skeleton_params* params, const double* state_in, double* state_out, float* rigid, float* rotations, float* lengths,
                              void* stream);

/* ---- heatmaps, keypoints and bones drawn onto the frames (additive; EGOTAP_ABI_VERSION stays 2) ----
 * Nothing in the serving chain let a person see what the estimators saw and found; a wrong crop rectangle, mirror flag, lens map or keypoint affine
 * shows at once in a picture.  Two operators, no handle, one launch each on the caller's stream, no synchronisation, no allocation, no atomics, no
 * workspace; recorded as heat_u8 and overlay_u8 while a handle's timing hook is on.  egotap_amd/spec.py restates both (heat_u8, overlay_taps,
 * overlay_u8); the device equals the restatement in every byte.
 *
 * egotap_heat_u8: the reference's picture of a heatmap stack (utils/util.py:160-175 tensor2im(is_heatmap=True)) per group of channels.  hm is
 * [B, C, S, S], EGOTAP_F32 or EGOTAP_BF16, element (b, c, y, x) at b * image_stride + c * S*S + y * S + x (image_stride in elements, >= C * S*S: a channel
 * slice of a wider tensor is read in place); heat8 is uint8 [B, groups, S, S], contiguous.  Group g is the n / groups consecutive channels from
 * c0 + g * n / groups.  Per pixel, in fp32 (bf16 upcast exactly), nothing contracted:
 *   v = the group's channels added in ascending order;  v = v > 0 ? (v < 1 ? v : 1) : 0, so a NaN gives 0;  byte = (uint8)(int)(v * 255.0f), truncated
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL hm or heat8; an unknown dtype; B < 1; n < 1; groups < 1 or not dividing n; c0 < 0 or
 * c0 + n > C; S not a positive multiple of 16, or above 4096; image_stride below C * S*S or no multiple of 16 bytes; hm not 16-byte or heat8 not 8-byte
 * aligned; heat8 overlapping hm.
 *
 * egotap_overlay_u8: three layers blended onto packed RGB8 canvases, uint8 [B, Hc, Wc, 3], left and right; right8 and out_right8 both NULL: one eye
 * (E = 1, otherwise E = 2).  Wc % 4 == 0, every canvas base 4-byte aligned, Hc, Wc <= 16384, B <= 65535.  out == in exactly (per eye) is the one
 * permitted overlap: any other overlap between any two array arguments is refused.  The layers go on in this order -- the heat, the bones in
 * ascending index, the marks in ascending index -- and every layer changes every channel as
 *   c = (c * (65536 - t) + colour * t + 32768) >> 16      t = coverage (0 .. 256) * alpha (0 .. 255);  t = 0 returns c
 * heat   (heat8 NULL: none)  heat8 uint8 [B, E, S, S], as egotap_heat_u8 writes it with groups = E, and per eye two tap tables on the device, int32
 *        [Wc] (tx) and [Hc] (ty), built once on the host in float64 (spec.overlay_taps(a, b, S, L) from the eye's keypoint affine component (a, b):
 *        canvas coordinate = a * u + b, heat pixel centres at i + 0.5, a < 0 a mirror).  An entry is i0 | w1 << 16 with w1 the second tap's weight in
 *        Q11, or -1 where the canvas pixel lies outside the map's extent; the second tap is min(i0 + 1, S - 1).  A pixel whose x or y entry is -1 is
 *        left alone.  Otherwise A = (wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) + 2^21) >> 22 (the sensor front ends' blend of one byte),
 *        t = A * heat alpha, the one colour heat_rgba.  The device reads the tables and never the affine; an index past S - 1 is clamped to it.
 * marks  (marks NULL: none, and no bones; the style's n_marks and n_bones are then not read)  fp32 [B, E, M, 4] = (x, y, score, _) in canvas pixels,
 *        pixel centres at X + 0.5 -- the keypoint record of the _kp entries passed straight in.  A mark is eligible when score >= min_score (false on
 *        a NaN), x and y are finite and |x|, |y| < 32768.  In sixteenths of a pixel: mx = rint(16 x), my = rint(16 y) (ties to even), a pixel centre
 *        is (16 X + 8, 16 Y + 8), d = isqrt(dx^2 + dy^2) (a floor), coverage = clamp(r16 + 8 - d, 0, 16) * 16; colour and alpha mark_rgba[j].
 * bones  bones[l] = two mark indices; drawn when both marks are eligible.  a, b their sixteenths, e = b - a, dd = e . e, s = (p - a) . e:
 *        dd == 0 or s <= 0: d = the distance to a, as above;  s >= dd: to b;  otherwise d = |cross(p - a, e)| div isqrt(dd), an integer floor division;
 *        coverage = clamp(w16 + 8 - d, 0, 16) * 16; colour and alpha bone_rgba[l].
 * Every intermediate is an integer below 2^42 (|mx| <= 2^19, a pixel centre < 2^18, so a difference is below 2^20 and a sum of two products below 2^41).
 * The style is host memory, read during the call.  One thread draws four pixels of a row; a frame's marks, bones and culling boxes are prepared once per
 * workgroup; culling changes no byte.
 * EGOTAP_ERR_INVALID, by name and before any launch: a NULL left8, out_left8 or style; right8 and out_right8 not both NULL or both given; B < 1 or
 * > 65535; Hc < 1, Wc < 4, Wc % 4 != 0, Hc or Wc > 16384; a canvas base not 4-byte aligned; heat8 given with S < 1 or S > 4096, a NULL tap table of a
 * drawn eye, tx not 16-byte or ty not 4-byte aligned; marks not 16-byte aligned; with marks: n_marks outside 1 .. 64, n_bones outside 0 .. 64, a bone index
 * outside 0 .. n_marks - 1; r16 or w16 outside 0 .. 16384; a NaN min_score; any overlap other than out == in. */
#define EGOTAP_OVERLAY_MAX 64
typedef struct egotap_overlay_style {
    int32_t n_marks, n_bones;                        /* M, L */
    int32_t r16, w16;                                /* the marks' radius and the bones' half-width, sixteenths of a pixel */
    float min_score;
    uint8_t heat_rgba[4];                            /* R, G, B, alpha */
    uint8_t bones[EGOTAP_OVERLAY_MAX][2];
    uint8_t mark_rgba[EGOTAP_OVERLAY_MAX][4];
    uint8_t bone_rgba[EGOTAP_OVERLAY_MAX][4];
} egotap_overlay_style;
int egotap_heat_u8(const void* hm, int dtype, int B, int C, int S, int64_t image_stride, int c0, int n, int groups, uint8_t* heat8, void* stream);
int egotap_overlay_u8(const uint8_t* left8, const uint8_t* right8, int B, int Hc, int Wc, const uint8_t* heat8, int S, const int32_t* tx_left,
                      const int32_t* ty_left, const int32_t* tx_right, const int32_t* ty_right, const float* marks, const egotap_overlay_style* style,
                      uint8_t* out_left8, uint8_t* out_right8, void* stream);

/* Arithmetic of the large GEMMs of the lifting head (nn.Linear layers of the ViT and fc1; everything else is always fp32).
 *   EGOTAP_PREC_F32     v_mfma_f32_32x32x2_f32: exact fp32 products (default; what the headline benchmark measures)
 *   EGOTAP_PREC_BF16X3  each fp32 operand split in registers into hi + lo bf16 (16 significant bits), a*b taken as
 *                       a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation; operands and
 *                       results stay fp32 in HBM.  Error ~2^-16 per product against 2^-24: opt-in fast mode, the reference
 *                       offers the analogous knob as --use_amp (egotap_autoencoder_model.py:177-183).
 *   EGOTAP_PREC_BF16    operands rounded to bf16 in registers (round to nearest even), one MFMA per product, fp32 accumulate,
 *                       fp32 master weights / activations / gradients in HBM: the reduced-precision training configurations
 *                       (the reference trains under fp16 autocast, egotap_autoencoder_model.py:299-323 + --use_amp).
 * The mode also selects the kernels of egotap_train_gemm_nt / egotap_train_gemm_tn (forward, input-gradient and
 * weight-gradient GEMMs of the training step) for shapes the bf16 kernels cover (N, K multiples of 256, M >= 1024). */
enum { EGOTAP_PREC_F32 = 0, EGOTAP_PREC_BF16X3 = 1, EGOTAP_PREC_BF16 = 2 };
int egotap_set_precision(egotap_handle h, int mode);
/* The propagation units' recurrence (custom_cells.py:149-197) runs as ONE launch per layer whose workgroups hand the state to each other
 * inside the launch: they must all be resident together, which holds when the calling process has the device to itself while a
 * forward runs (one process per GPU, the deployment this library is written for).  Where the device is shared -- another process, or
 * another stream of this one running long kernels -- pass enable = 0: the recurrence then runs as one kernel per step (same bits,
 * ~2x the latency of that part).  With the chain enabled on a shared device the waits inside it are bounded and run out: the
 * workgroups concerned store nothing and raise a fault word in the workspace, and a second kernel queued behind every chain launch
 * (idle otherwise) then redoes that launch without cross-workgroup waits -- the call's results are RIGHT (same bits), it only took
 * ~0.1-0.2 s longer.  The library notices at its next call on the handle (a host-mapped word, no synchronisation) and from then on
 * uses the per-step kernels for that handle by itself. */
int egotap_set_pu_chain(egotap_handle h, int enable);
/* *enabled: whether the handle still uses the one-launch recurrence; *faults: chain launches that had to be redone so far (see above).
 * Exact for calls whose stream the caller has synchronised. */
int egotap_pu_chain_status(egotap_handle h, int* enabled, int* faults);
/* EGOTAP_PREC_BF16 only: caller-owned device scratch (16-byte aligned) into which a GEMM's weight matrix is rounded to bf16 right
 * before the launch (stream ordered; nothing is cached, the live fp32 parameters stay the source of truth).  Halves the W operand's
 * vector-memory bytes, which bound that mode.  bytes >= 2 * the largest N*K (67 MB for fc1 of the position encoder); NULL = off. */
int egotap_set_weight_scratch(egotap_handle h, void* buf, size_t bytes);
/* EGOTAP_PREC_BF16 only: caller-owned device scratch (16-byte aligned) into which a GEMM's plain row-major activation operand [M, K]
 * is rounded to bf16 right before the launch; with both operands in bf16 the product runs on the LDS-DMA kernel (gemm_bf16_dma.h,
 * same rounding and summation order as without it -- bit-identical results, about twice the GEMM rate).  bytes >= 2 * the largest
 * M*K (tokens x 4096 for the ViT MLP: 1.2 GB at B = 256); a GEMM whose operand does not fit falls back to the register-staged
 * kernel.  NULL = off. */
int egotap_set_act_scratch(egotap_handle h, void* buf, size_t bytes);

/* ---- frozen-weight serving (opt-in): keep the prepared weights across forwards ----
 * By default the EGOTAP_PREC_BF16 forwards prepare their weights on every call (the lifting head rounds each GEMM's weight matrix into the
 * weight scratch and fuses the q | k | v bias; an estimator repacks its convolution weights and folds its BatchNorms), so that the live fp32
 * parameters stay the only source of truth.  A server whose weights do not change can FREEZE a network instead: the caller hands the library
 * an arena, ONE launch fills it with every prepared weight, and from then on the inference forwards read the arena and launch no weight
 * preparation.  The results are the same bits: the same kernels multiply by the same bf16 values.
 *   - The library still allocates nothing and never synchronises.  The arena is a caller-owned device buffer (256-byte aligned, at least
 *     *_frozen_bytes) that the handle BORROWS until the matching unfreeze or egotap_destroy; the caller must keep it alive and untouched that
 *     long.  A freeze enqueues its one launch on `stream` and is ordered there like any forward; freezing again (same or another arena)
 *     re-prepares from the live parameters.
 *   - Lifting head: while frozen, egotap_lift_forward / egotap_lift_predict_pose on the bf16-storage route (EGOTAP_PREC_BF16, vit_dim 1024, a
 *     sequence that is a multiple of 32, a weight scratch attached) read the bf16 weight copies and the fused q | k | v biases from the arena.
 *     Every other parameter (biases, LayerNorm / BatchNorm tensors, embeddings) is read live as always.  Every other route (fp32, bf16x3,
 *     ragged sequences) ignores the arena: egotap_lift_frozen_bytes reports 0 there and egotap_lift_freeze fails, naming the reason.
 *   - Estimators: while frozen, egotap_hm_forward in EGOTAP_PREC_BF16 at sides 64 / 128 reads the packed weights, padded biases and folded
 *     BatchNorms (running statistics) from the arena; the stem's weight and BatchNorm are read live.  The packed layout depends on the batch
 *     (below a pixel count a convolution's weights are packed in 32-channel slabs for the split-K kernel, above it in 64-channel slabs): the
 *     arena holds the layout of the batch B it was built for.  A call at a batch with another layout does not read it and packs per call, as
 *     if not frozen; the library decides per call.  Other precisions / sides: bytes = 0, freeze fails by name.
 *   - Staleness is the caller's business with one exception the library can see: egotap_bind_param with a DIFFERENT pointer for a tensor whose
 *     prepared copy is kept, and every egotap_set_precision, unfreeze (the lifting head and both estimators for set_precision; the net
 *     concerned for bind_param).  A stale arena is never read silently after those.  Writing new values into the same parameter memory is
 *     invisible to the library: freeze again afterwards.
 *   - Training never reads an arena: egotap_lift_forward_train / egotap_lift_backward* build their own copies in `saved`, and
 *     egotap_hm_forward_bnbatch (batch statistics) packs per call, so their results do not depend on whether the handle is frozen. */
int egotap_lift_frozen_bytes(egotap_handle h, size_t* bytes);
int egotap_lift_freeze(egotap_handle h, void* arena, size_t bytes, void* stream);
int egotap_lift_unfreeze(egotap_handle h);
int egotap_hm_frozen_bytes(egotap_handle h, int net, int B, size_t* bytes);
int egotap_hm_freeze(egotap_handle h, int net, int B, void* arena, size_t bytes, void* stream);
int egotap_hm_unfreeze(egotap_handle h, int net);


/* ---- single operators (same kernels the forward uses; exported for unit tests and reuse) ---- */
/* y = epi(x W^T + b): nn.Linear (+ residual / exact GELU / BatchNorm1d-eval + LeakyReLU 0.2).
 * epi: 0 bias, 1 bias + residual r[M,N], 2 bias + GELU(erf), 3 bias + BN(eval) + LeakyReLU (bn = gamma,beta,mean,var; eps 1e-5)
 * tile: 0 default, else a tile-shape id (see egotap_gemm_tile_name) */
int egotap_linear_f32(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int epi,
                      const float* r, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                      const float* bn_var, int tile, void* stream);
const char* egotap_gemm_tile_name(int tile);
/* y = x w^T + b with both operands already bf16 (caller-owned copies x [M,K], w [N,K], 16-byte aligned; N % 256 == 0, K % 32 == 0):
 * the LDS-DMA kernel of EGOTAP_PREC_BF16 (gemm_bf16_dma.h), fp32 accumulate, fp32 result */
int egotap_linear_bf16_dma(const void* x_bf16, const void* w_bf16, const float* b, float* y, int M, int N, int K, void* stream);
/* nn.LayerNorm over the last dim (1024), modeling_vit.py:357-358 */
int egotap_layernorm_f32(const float* x, float* y, const float* gamma, const float* beta, int rows, int dim, float eps,
                         void* stream);
/* ViTSelfAttention core (modeling_vit.py:233-252) on a fused [B*N, 3*heads*128] q|k|v buffer -> ctx [B*N, heads*128].
 * N >= 32, a multiple of 4: every heatmap side the reference allows (a multiple of 16, net_architecture.py:327: N = 36 (side / 16)^2 for
 * UnrealEgo) -- a ragged last 32-key tile is masked, the last 32-query block overlaps its predecessor. */
int egotap_attention_f32(const float* qkv, float* ctx, int B, int N, int heads, void* stream);
/* the same operator with the arithmetic of egotap_set_precision (EGOTAP_PREC_F32 / _BF16X3 / _BF16).  The bf16 / bf16x3 kernels need
 * N % 32 == 0 (heatmap sides 64, 128: every shipped configuration); for other N the call -- and egotap_lift_forward in those modes -- runs the
 * exact-fp32 kernel above instead (a fallback by name: the result is MORE exact than asked for).  The attention BACKWARD
 * (egotap_train_attention_bwd, egotap_lift_backward) needs N % 32 == 0 and says so. */
int egotap_attention(const float* qkv, float* ctx, int B, int N, int heads, int precision, void* stream);

/* Evaluation metrics of EgoTAPAutoEncoderModel.evaluate (model/egotap_autoencoder_model.py:329-350): per-sample MPJPE and
 * Procrustes-aligned MPJPE (utils/util.py:328-379 batch_compute_similarity_transform_torch: 3x3 SVD, reflection fix,
 * scale, translation), one launch for the batch instead of the reference's two Python loops.
 *   pred, gt  device f32 [B, J, 3];  mpjpe, pa_mpjpe  device f32 [B] (input units);  aligned  device f32 [B, J, 3] or NULL */
int egotap_pose_metrics(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pa_mpjpe, float* aligned, void* stream);
/* The same metrics AS THE REFERENCE COMPUTES THEM FOR A BATCH OF 2 OR 3 FRAMES.  utils/util.py:337 decides whether to transpose its
 * [B, J, 3] input by testing shape[0] against 3 and 2 (meant for unbatched 3 x N / 2 x N point sets), so for B = 2 or 3 the similarity
 * transform is solved over the wrong axes (J "coordinates", 3 "points"; a J x J SVD of rank <= 2) and PA-MPJPE of a frame depends on
 * the size of the batch it arrives in.  test.py / utils/evaluate.py:149-168 print exactly these numbers for a ragged last batch, so the
 * wrapper's evaluate() calls this entry for B in {2, 3} by default (opt.pa_mpjpe_reference_batch_axes).
 * B must be 2 or 3; same arguments as egotap_pose_metrics; `aligned` = the reference's S1_hat (not transposed back, as there). */
int egotap_pose_metrics_batch_axes(const float* pred, const float* gt, int B, int J, float* mpjpe, float* pa_mpjpe, float* aligned, void* stream);

/* Ground-truth heatmaps from joints, written in the lifting head's input layout (the data loader's per-frame CPU work when
 * training with --use_gt_heatmap: dataloader/data_loader.py:76-215, utils/projection.py:263-279 coord2d_to_heatmap,
 * utils/data.py:175-262 get_limb_data / overwrite_limb_data).
 *   pts2d_left/right  device f32 [B, J+1, 2]  joints in the 1024-pixel image frame (gt_camera_2d_*), joint 0 = root
 *   pose3d            device f32 [B, J+1, 3]  gt_local_pose (the pelvis offset cancels in the limb direction)
 *   parents           device i32 [J+1]        kinematic parents (utils/util.py:51-52)
 *   hm                device f32 [B, 6J, res, res]: L pos, R pos, L cos, L sin, R cos, R sin
 *   plength           device f32 [B, 2, J] or NULL (gt_pixel_length_left/right);  theta  device f32 [B, J] or NULL */
int egotap_synth_heatmaps(const float* pts2d_left, const float* pts2d_right, const float* pose3d, const int* parents, int B, int J,
                          int res, float* hm, float* plength, float* theta, void* stream);

/* ---- training-step operators (fp32), called by the autograd glue (egotap_amd/training.py) ------------------------------
 * They implement the backward of the modules above plus loss / optimizer (egotap_autoencoder_model.py:284-323,
 * utils/loss.py:54-85, network.py:72-78 AdamW).  All buffers are caller-owned device memory; reductions have a fixed order.
 * loader: 0 plain, 1 ViT patch gather, 2 per-heatmap token regroup, 3 stereo cos/sin gather, 4 stereo joint features,
 *         5 stereo joint features x sigmoid gate (aux).  epi: 0 none, 1 bias, 2 bias + residual r, 3 bias + GELU (stores
 *         the pre-activation to z), 4 accumulate onto r, 5 multiply by GELU'(r), 7 / 8 scatter into the heatmaps' gradient:
 *         y = dhm f32 [B, 6J, S, S] (16-byte aligned), loader 0, no bias.  7: position channels [0, 2J) from the patch embedding's
 *         output gradient (x [B*seq, D], w = projection.weight^T [256, D]; M = B*seq, N = 256, K = D; dummy grid cells are no pixel);
 *         8: rotation channels [2J, 6J) from the rotation encoder's fc1 pre-activation gradient (x [B*T, 2048], w = fc1.weight^T
 *         [2 S^2, 2048]; M = B*T, N = 2 S^2, K = 2048).  Each writes every element of its channels exactly once. */
int egotap_train_gemm_nt(egotap_handle h, int loader, const float* x, int64_t lda, const float* aux, const float* w, const float* b,
                         float* y, int M, int N, int K, int epi, const float* r, float* z, int Bsz, void* stream);
int egotap_train_gemm_tn(egotap_handle h, int loader, const float* dy, int64_t ldy, const float* x, const float* aux, float* dw, int M,
                         int N, int K, int accumulate, int Bsz, void* ws, size_t ws_bytes, void* stream);
int egotap_train_colsum(const float* y, int64_t ldy, float* out, int M, int N, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* [r3] weight and bias gradient of one nn.Linear with a plain input in one call: dw[N,K] (+)= dy^T x, db[N] (+)= column sums of dy (autograd of
 * the ViT layers' Linear modules, model/modeling_vit.py:226-230, 271, 319-344).  fp32 with M % 32 == 0: the workgroups that stage dy for the
 * product also sum its columns (one pass over dy); otherwise egotap_train_gemm_tn followed by egotap_train_colsum. */
int egotap_train_gemm_tn_bias(egotap_handle h, const float* dy, int64_t ldy, const float* x, float* dw, float* db, int M, int N, int K,
                              int accumulate, void* ws, size_t ws_bytes, void* stream);
int egotap_train_transpose(const float* in, float* out, int R, int C, int64_t ldo, void* stream);
int egotap_train_add_inplace(float* out, const float* in, int64_t n, void* stream);
int egotap_train_patch_fwd(egotap_handle h, const float* hm, int B, const float* w, const float* b, const float* mask_tok,
                           const float* pos, float* x, void* stream);
int egotap_train_patch_split(egotap_handle h, const float* dpos, float* dbias, float* dmask, int accumulate, void* stream);
int egotap_train_tokens_scatter(egotap_handle h, const float* dA, float* dtok, int B, void* stream);
int egotap_train_layernorm_fwd(const float* x, float* y, const float* g, const float* b, float* mean, float* rstd, int rows,
                               float eps, void* stream);
int egotap_train_layernorm_bwd(const float* x, const float* dy, const float* g, const float* mean, const float* rstd,
                               const float* dres, float* dx, float* dgamma, float* dbeta, int rows, int accumulate,
                               void* ws, size_t ws_bytes, void* stream);
int egotap_train_bn_lrelu_fwd(const float* z, float* y, const float* gamma, const float* beta, float* mean, float* rstd,
                              float* run_mean, float* run_var, int R, int C, float eps, float momentum, void* ws,
                              size_t ws_bytes, void* stream);
int egotap_train_bn_lrelu_bwd(const float* z, const float* y, const float* dy, const float* gamma, const float* mean,
                              const float* rstd, float* dz, float* dgamma, float* dbeta, int R, int C, int accumulate,
                              void* ws, size_t ws_bytes, void* stream);
int egotap_train_qkv_fwd(egotap_handle h, const float* y, const float* wq, const float* bq, const float* wk, const float* bk, const float* wv,
                         const float* bv, float* qkv, int M, int D, void* stream);
int egotap_train_attention_fwd(const float* qkv, float* ctx, float* lse, int B, int N, int heads, int precision, void* stream);
int egotap_train_attention_bwd(const float* qkv, const float* ctx, const float* dctx, const float* lse, float* delta,
                               float* dqkv, int B, int N, int heads, int precision, void* stream);
int egotap_train_pu_saved_bytes(egotap_handle h, int B, size_t* bytes, size_t* hs1_offset);
int egotap_train_pu_fwd(egotap_handle h, const float* posz, const float* rotz, int B, void* saved, size_t saved_bytes, void* stream);
int egotap_train_pu_bwd_ws_bytes(egotap_handle h, int B, size_t* bytes);
int egotap_train_pu_bwd(egotap_handle h, const float* posz, const float* rotz, int B, const void* saved, const float* dhs1,
                        float* dposz, float* drotz, float* const* grads, int accumulate, void* ws, size_t ws_bytes, void* stream);
int egotap_train_pose_head_fwd(egotap_handle h, const float* posz, const float* hs1, int B, float* pose, void* stream);
int egotap_train_pose_head_bwd(egotap_handle h, const float* posz, const float* hs1, const float* dpose, int B, float* dposz,
                               float* dhs1, float* dWp, float* dbp, float* dWg, float* dbg, int accumulate, void* stream);
/* out[2] = (loss_pose, loss_cos_sim) as backward_AutoEncoder weighs them; dpred [2, B, J, 3]: plane 0 = d loss_pose / d pred,
 * plane 1 = d loss_cos_sim / d pred; partial [B, 2] scratch */
int egotap_train_pose_loss(egotap_handle h, const float* pred, const float* gt, float* dpred, float* out, float* partial,
                           int B, float lambda_mpjpe, float lambda_cos_sim, void* stream);
/* torch.optim.AdamW update of one tensor; hyper-parameters are doubles (python floats): the bias corrections 1 - beta^step are
 * computed in double on the host, as torch does */
int egotap_train_adamw(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps,
                       double weight_decay, int step, void* stream);
/* the same update for every tensor of a network in ONE launch (the optimizer step of egotap_autoencoder_model.py:313-314): gradients
 * and the two moment buffers are flat arenas of `span` floats with one layout, table = device int64 [nseg][3] = {arena offset, numel,
 * parameter pointer} sorted by offset (segments may be separated by padding) */
int egotap_train_adamw_multi(const void* table, int nseg, const float* g, float* m, float* v, int64_t span, double lr, double beta1,
                             double beta2, double eps, double weight_decay, int step, void* stream);

/* ---- the lifting head's training step as one call per direction (reference: the autograd graph behind
 * egotap_autoencoder_model.py:284-311 forward() + loss.backward()) -----------------------------------------------------------
 * egotap_lift_forward_train = egotap_lift_forward in train mode (BatchNorm1d on batch statistics, running statistics updated in
 * the bound buffers; num_batches_tracked is the caller's bookkeeping) keeping every activation the backward needs in `saved`;
 * egotap_lift_backward walks the layers in reverse and OVERWRITES the gradient buffers bound with egotap_bind_grad (same keys as
 * egotap_bind_param; every trained tensor must have one).  Both compose the granular operators above, in a fixed order, on the
 * caller's stream.  fp32 tensors; the large GEMMs follow egotap_set_precision (f32 / bf16x3 / bf16 operand copies).
 *   hm        device f32 [B, 6J, S, S]          pose    device f32 [B, out_joints, 3]        dpose  device f32 [B, out_joints, 3]
 *   saved     device, egotap_lift_train_bytes   ws      device scratch, egotap_lift_train_bytes (shared by both calls)
 *   bucket_events  NULL / n_events = 0, or vit_layers + 2 hipEvent_t: event k is recorded on `stream` when every gradient of
 *             bucket k is final -- bucket 0: pose head, propagation units, both FC encoders, final LayerNorm and the last ViT layer's
 *             output.dense.bias; bucket 1 + j: ViT layer L-1-j plus the output.dense.bias of the layer below; last: embeddings --
 *             so that a data-parallel caller starts each bucket's all-reduce behind its event while the backward goes on. */
int egotap_bind_grad(egotap_handle h, const char* key, void* dev_ptr, int64_t numel);
int egotap_lift_train_bytes(egotap_handle h, int B, size_t* saved_bytes, size_t* ws_bytes);
int egotap_lift_forward_train(egotap_handle h, const float* hm, int B, float* pose, void* saved, size_t saved_bytes, void* ws,
                              size_t ws_bytes, void* stream);
int egotap_lift_backward(egotap_handle h, const float* hm, const float* dpose, int B, const void* saved, size_t saved_bytes, void* ws,
                         size_t ws_bytes, void* const* bucket_events, int n_events, void* stream);
/* egotap_lift_backward that also writes the gradient w.r.t. the input heatmaps (autograd reaching the head's input, as the reference's
 * plain-PyTorch head does: the estimators can then be trained through the pose loss).  dhm device f32 [B, 6J, S, S], contiguous,
 * 16-byte aligned, not overlapping hm; every element is written exactly once (no clearing needed), bit-reproducibly.  The rotation
 * channels are computed inside the backward, the position channels after the last bucket event.  Same saved buffer and workspace
 * (egotap_lift_train_bytes).  dhm == NULL: exactly egotap_lift_backward, launch for launch. */
int egotap_lift_backward_dhm(egotap_handle h, const float* hm, const float* dpose, int B, const void* saved, size_t saved_bytes, void* ws,
                             size_t ws_bytes, void* const* bucket_events, int n_events, void* stream, float* dhm);

/* ---- heatmap-estimator training operators (fp32), called by the autograd glue (egotap_amd/hm_training.py) ----------------
 * One optimisation step of the stage-1 model (model/heatmap_shared_model.py:98-172): HeatMap_UnrealEgo_Shared in train mode
 * (model/net_architecture.py:25-173: BatchNorm2d on batch statistics), MSE / limb-length-normalised MSE losses, Adam.
 * All tensors NCHW fp32 with explicit image strides (floats), so concat slices are read and written in place.
 *   conv_fwd     convolution + bias (+ residual) (+ ReLU) on the forward kernels; also the INPUT gradient: dX = conv(dY, conv_wt(W)),
 *                stride-2 layers after zero_upsample(dY)
 *   conv_wgrad   dW[Cout][Cin][ks][ks] (+)= sum_{n,y,x} dY * shifted X  (ks 1 / 3 / 7, stride 1 / 2; split over images,
 *                fixed-order reduction: bitwise reproducible)
 *   bn2d_fwd     batch statistics over N*H*W, running-stat update (momentum, unbiased variance), y = [relu](bn(z) [+ res])
 *   bn2d_bwd     dz, dgamma, dbeta (and the residual branch's gradient dres = dy * [y > 0]) */
int egotap_hmtrain_conv_fwd(egotap_handle h, const float* x, const float* w, const float* bias, const float* res, float* y, int Nimg, int Cin,
                            int Cout, int wout, int taps, int stride, int relu, int64_t in_istride, int64_t out_istride, int64_t res_istride,
                            void* stream);
/* [r3] Eval-mode building blocks for the backbones egotap_hm_forward does not cover -- the Bottleneck ResNets behind --model_name resnet50 /
 * resnet101 (reference: model/net_architecture.py:61-64 torchvision resnet50 / resnet101, :108-111 feature_scale 4).  The host side composes
 * the forward from them (egotap_amd/networks.py): y = [relu](BatchNorm_eval(conv(x, w)) [+ res]) with the BatchNorm folded in the epilogue as
 * gamma / sqrt(var + 1e-5) (what egotap_hm_forward does for the BasicBlock nets), and the 7x7 / 2 stem with its BatchNorm + ReLU
 * (y [2B, 64, S0/2, S0/2], image n = 2b + eye).  fp32 only. */
int egotap_hm_conv_bn_fwd(egotap_handle h, const float* x, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                          const float* res, float* y, int Nimg, int Cin, int Cout, int wout, int taps, int stride, int relu, int64_t in_istride,
                          int64_t out_istride, int64_t res_istride, void* stream);
int egotap_hm_stem_bn_fwd(const float* left, const float* right, const float* w, const float* gamma, const float* beta, const float* mean,
                          const float* var, float* y, int B, int S0, void* stream);
/* bf16 precision modes: the 3x3 stride-1 convolutions (forward and input gradient) of the training step run on conv_bf16 once a
 * scratch buffer for their repacked weights is set (egotap_hmtrain_pack_bytes() bytes, caller-owned, 16-byte aligned) */
int egotap_hmtrain_set_pack_buffer(egotap_handle h, void* buf, size_t bytes);
size_t egotap_hmtrain_pack_bytes(void);
int egotap_hmtrain_stem_fwd(const float* left, const float* right, const float* w, float* z, int B, int S0, void* stream);
int egotap_hmtrain_bn2d_fwd(const float* z, float* y, const float* res, const float* gamma, const float* beta, float* mean, float* rstd,
                            float* run_mean, float* run_var, int N, int C, int HW, int64_t z_istride, int64_t y_istride, int64_t res_istride,
                            int relu, float eps, float momentum, void* ws, size_t ws_bytes, void* stream);
int egotap_hmtrain_bn2d_bwd(const float* z, const float* y, const float* dy, const float* gamma, const float* mean, const float* rstd, float* dz,
                            float* dres, float* dgamma, float* dbeta, int N, int C, int HW, int64_t z_istride, int64_t dy_istride, int relu,
                            int accumulate, int dres_accumulate, void* ws, size_t ws_bytes, void* stream);
int egotap_hmtrain_chansum(const float* dy, float* out, int N, int C, int HW, int64_t istride, int accumulate, void* ws, size_t ws_bytes, void* stream);
int egotap_hmtrain_conv_wt(const float* w, float* wt, int Cout, int Cin, int taps, void* stream);
int egotap_hmtrain_zero_upsample(const float* in, float* out, int N, int C, int H, int64_t in_istride, int64_t out_istride, void* stream);
int egotap_hmtrain_conv_wgrad(const float* dy, const float* x, float* dw, int Nimg, int Cin, int Cout, int wout, int ks, int stride,
                              int64_t dy_istride, int64_t x_istride, int accumulate, int precision, void* ws, size_t ws_bytes, void* stream);
int egotap_hmtrain_relu_bwd(const float* y, const float* dy, float* dz, int N, int C, int HW, int64_t y_istride, int64_t dy_istride,
                            int64_t dz_istride, void* stream);
int egotap_hmtrain_maxpool_bwd(const float* x, const float* dy, float* dx, int64_t planes, int HIN, void* stream);
int egotap_hmtrain_upsample_bwd(const float* dy, float* dx, int N, int C, int HIN, int64_t dy_istride, int64_t dx_istride, void* stream);
int egotap_hmtrain_maxpool_fwd(const float* x, float* y, int64_t planes, int HIN, void* stream);
int egotap_hmtrain_upsample_fwd(const float* x, float* y, int N, int C, int HIN, int64_t in_istride, int64_t out_istride, void* stream);
int egotap_hmtrain_mse(const float* pred, const float* gt, const float* plen, float* dpred, float* loss, int B, int Cn, int HW, float lambda,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- bf16-storage operators (EGOTAP_PREC_BF16 with bf16 tensors in HBM; gemm_bf16s.h) -----------------------------------------
 * nn.Linear forward / input gradient on bf16 operands:  OUT = epi(x[M,K] w[N,K]^T), x row stride ldx, outputs row stride ldo
 * (elements).  N % 256 == 0, K % 32 == 0, 16-byte aligned pointers.  epi:
 *   0  out0 bf16 = acc (+ bias if not NULL)                    1  out0 f32 = acc + bias + aux (aux: f32 residual, may alias out0)
 *   2  out0 bf16 = z = acc + bias (may be NULL), out1 bf16 = GELU(z)      3  out0 bf16 = acc * GELU'(aux), aux: bf16 z;
 *   4  out0 f32 = acc + bias                                        with epi 3, out1 (optional) f32 [2 ceil(M / 256)][N]: per
 *      128-row block partial column sums of the stored out0 (finish with egotap_train_colsum over those rows: the bias gradient of
 *      the layer whose output gradient out0 is, without another pass over out0) */
int egotap_bf16_gemm_nt(const void* x, int64_t ldx, const void* w, const float* bias, int M, int N, int K, int epi, const void* aux,
                        void* out0, void* out1, int64_t ldo, void* stream);

/* nn.Linear weight gradient on bf16 operands: dw[N,K] (+)= dy[M,N]^T x[M,K] (fp32 result).  N, K % 256 == 0.  zeros: >= 512 bytes of
 * zeros (rows past M are fetched from it); ws: scratch for the split-M partial slabs (>= 4*N*K bytes per split, up to 256 splits are
 * used when it allows; fixed-order reduction: bitwise reproducible) */
int egotap_bf16_gemm_tn(const void* dy, int64_t ldy, const void* x, int64_t ldx, float* dw, int M, int N, int K, int accumulate,
                        const void* zeros, void* ws, size_t ws_bytes, void* stream);

/* LayerNorm(1024) with a bf16 output (the next GEMM's operand) and its backward: dy bf16, dx fp32 (+ dxb: a bf16 copy when not NULL),
 * dgamma / dbeta, and dcolsum (not NULL): column sums of dx = the bias gradient of the Linear layer whose output gradient dx is.
 * ws >= (3 * ceil(rows / 64) + 3 + 3 * ceil(ceil(rows / 64) / 64)) * 4096 bytes */
int egotap_bf16_layernorm_fwd(const float* x, void* y, const float* g, const float* b, float* mean, float* rstd, int rows, float eps, void* stream);
int egotap_bf16_layernorm_bwd(const float* x, const void* dy, const float* g, const float* mean, const float* rstd, const float* dres, float* dx,
                              void* dxb, float* dgamma, float* dbeta, float* dcolsum, int rows, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* out[N] (+)= column sums of a bf16 matrix y[M, N] (row stride ldy): bias gradients */
int egotap_bf16_colsum(const void* y, int64_t ldy, float* out, int M, int N, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* per-step weight preparation: w fp32 [N, K] (the live master weights) -> wb bf16 [N, K] and, when wt != NULL, wt bf16 [K, N] with row
 * stride ldt (so three projections can share one transposed [K, 3N] matrix) */
int egotap_bf16_prep_weight(const float* w, void* wb, void* wt, int N, int K, int64_t ldt, void* stream);
int egotap_bf16_from_f32(const float* src, void* dst, int64_t n, void* stream);
/* ViTSelfAttention core on bf16 tensors (modeling_vit.py:233-252): qkv bf16 [B*N, 3*heads*128] -> ctx bf16 [B*N, heads*128], lse fp32
 * [B*heads*N]; backward: dqkv bf16 (same layout as qkv), delta fp32 [B*heads*N] scratch.  Two backward kernels (dQ; dK + dV). */
int egotap_bf16_attention_fwd(const void* qkv, void* ctx, float* lse, int B, int N, int heads, void* stream);
int egotap_bf16_attention_bwd(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* delta, void* dqkv, int B, int N, int heads,
                              void* stream);
/* The same, and the q | k | v bias gradients (column sums of dqkv) as well: the kernels' epilogues leave per-block partial sums in ws
 * (needs (B N / 32)(3 heads 128) floats + 64 MB), three small fp32 column sums finish them -- no pass over dqkv.  Shapes without that
 * epilogue (N % 64 != 0) fall back to the column-sum pass. */
int egotap_bf16_attention_bwd_bias(const void* qkv, const void* ctx, const void* dctx, const float* lse, float* delta, void* dqkv, float* dq_bias,
                                   float* dk_bias, float* dv_bias, int B, int N, int heads, void* ws, size_t ws_bytes, void* stream);
/* fc1 of the two heatmap encoders on bf16 operands (which 0: position encoder, src = final-LayerNorm tokens bf16 [B*seq, D];
 * 1: rotation encoder, src = the head's input heatmaps as bf16 [B, 6J, S, S]); z fp32 [B*T, 2048] = x w^T + bias.
 * wgrad: dw fp32 [2048, K1] = dz^T x;  dgrad_tokens (position encoder): dtok bf16 [B*seq, D] = scatter(dz wt^T), wt bf16 [K1, 2048] */
int egotap_bf16_fc1_fwd(egotap_handle h, int which, const void* src, const void* w, const float* bias, float* z, int B, void* stream);
/* Patch embedding of the position heatmaps on bf16 operands (ViTPatchEmbeddings + mask token + position embeddings over the tiled heatmap
 * image: net_architecture.py:326-336, modeling_vit.py:137-153): hmb = the head's input heatmaps as bf16 [B, 6J, S, S], w = bf16 copy of
 * projection.weight [D, 256], zeros >= 16 bytes of zeros (dummy cells); x fp32 [B*seq, D]. */
int egotap_bf16_patch_fwd(egotap_handle h, const void* hmb, const void* w, const float* bias, const float* mask_tok, const float* pos,
                          const void* zeros, float* x, int B, void* stream);
int egotap_bf16_fc1_wgrad(egotap_handle h, int which, const void* dz, const void* src, float* dw, int B, const void* zeros, void* ws, size_t ws_bytes,
                          void* stream);
int egotap_bf16_fc1_dgrad_tokens(egotap_handle h, const void* dz, const void* wt, void* dtok, int B, void* stream);
/* the heatmaps' gradient in the bf16-storage step, fp32 into dhm [B, 6J, S, S] (16-byte aligned), each element written once:
 *   fc1_dgrad_rot  rotation channels [2J, 6J): dz bf16 [B*T, 2048] x wt bf16 [2 S^2, 2048] (rotation fc1.weight^T)
 *   patch_dgrad    position channels [0, 2J): dx bf16 [B*seq, D] (patch-embedding output gradient) x wt bf16 [256, D] (projection.weight^T) */
int egotap_bf16_fc1_dgrad_rot(egotap_handle h, const void* dz, const void* wt, float* dhm, int B, void* stream);
int egotap_bf16_patch_dgrad(egotap_handle h, const void* dx, const void* wt, float* dhm, int B, void* stream);


#ifdef __cplusplus
}
#endif
#endif /* EGOTAP_H */
