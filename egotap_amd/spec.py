"""Presets and state_dict contracts of the hot path.

The key names, shapes and order are the reference's, so released checkpoints
(`*_net_AutoEncoder.pth`, `*_net_HeatMap.pth`) load unchanged:
  lifting head      model/net_architecture.py:579-677 (+ modeling_vit.py, custom_cells.py)
  heatmap estimator model/net_architecture.py:25-173 over torchvision resnet18
"""
from __future__ import annotations

import math
from dataclasses import dataclass

BUFFER_LEAVES = ("running_mean", "running_var", "num_batches_tracked")


@dataclass(frozen=True)
class LiftPreset:
    name: str
    n_joints_hm: int          # J: heatmaps per eye == PU chain length
    estimate_head: bool       # UnrealEgo: head joint (+ global offset) from global_mlp, output LAST
    hm_size: int = 64
    hidden: int = 128         # --ae_hidden_size
    vit_dim: int = 1024
    vit_heads: int = 8
    vit_layers: int = 3
    patch: int = 16
    pu_hidden: int = 512

    @property
    def tokens(self):          # T: heatmap tokens per sample (stereo)
        return 2 * self.n_joints_hm

    @property
    def grid(self):            # net_architecture.py:328
        return int(math.sqrt(self.tokens - 1)) + 1

    @property
    def ppd(self):             # patches per heatmap side
        return self.hm_size // self.patch

    @property
    def side(self):
        return self.grid * self.ppd

    @property
    def seq(self):
        return self.side * self.side

    @property
    def out_joints(self):
        return self.n_joints_hm + (1 if self.estimate_head else 0)

    @property
    def in_channels(self):
        return 6 * self.n_joints_hm


def lift_preset(joint_preset: str = "UnrealEgo", hm_size: int = 64, hidden: int = 128) -> LiftPreset:
    if joint_preset == "UnrealEgo":
        return LiftPreset("UnrealEgo", 15, True, hm_size, hidden)
    if joint_preset == "EgoCap":
        return LiftPreset("EgoCap", 17, False, hm_size, hidden)
    raise ValueError("joint_preset is {} which is undefined".format(joint_preset))


def _linear(pre, n_out, n_in):
    return [(pre + ".weight", (n_out, n_in)), (pre + ".bias", (n_out,))]


def _fc_block(pre, n_in, n_out):
    return _linear(pre + ".fc", n_out, n_in) + [
        (pre + ".bn.weight", (n_out,)), (pre + ".bn.bias", (n_out,)),
        (pre + ".bn.running_mean", (n_out,)), (pre + ".bn.running_var", (n_out,)),
        (pre + ".bn.num_batches_tracked", ()),
    ]


def lift_state_spec(p: LiftPreset):
    """[(key, shape)] of EgoTAPAutoEncoder.state_dict(), in the reference's order."""
    D, H = p.vit_dim, p.pu_hidden
    v = "pos_heatmap_encoder.vit."
    s = [
        (v + "embeddings.cls_token", (1, 1, D)),
        (v + "embeddings.mask_token", (1, 1, D)),
        (v + "embeddings.position_embeddings", (1, p.seq, D)),
        (v + "embeddings.patch_embeddings.projection.weight", (D, 1, p.patch, p.patch)),
        (v + "embeddings.patch_embeddings.projection.bias", (D,)),
    ]
    for i in range(p.vit_layers):
        l = f"{v}encoder.layer.{i}."
        for n in ("query", "key", "value"):
            s += _linear(l + "attention.attention." + n, D, D)
        s += _linear(l + "attention.output.dense", D, D)
        s += _linear(l + "intermediate.dense", 4 * D, D)
        s += _linear(l + "output.dense", D, 4 * D)
        s += [(l + "layernorm_before.weight", (D,)), (l + "layernorm_before.bias", (D,)),
              (l + "layernorm_after.weight", (D,)), (l + "layernorm_after.bias", (D,))]
    s += [(v + "layernorm.weight", (D,)), (v + "layernorm.bias", (D,))]
    s += _linear(v + "pooler.dense", D, D)
    for enc, k1 in (("pos_heatmap_encoder", p.ppd * p.ppd * D), ("rot_heatmap_encoder", 2 * p.hm_size * p.hm_size)):
        s += _fc_block(enc + ".fc1", k1, 2048)
        s += _fc_block(enc + ".fc2", 2048, 512)
        s += _fc_block(enc + ".fc3", 512, p.hidden)
    x = 2 * p.hidden                       # per-joint stereo feature (left|right)
    c = "skel_sequential_layer.lstm_custom.layers."
    s += _linear(c + "0.x2f", H + x, x) + _linear(c + "0.x2h", 4 * H, x)
    s += _linear(c + "0.b2h", 4 * H, x) + _linear(c + "0.h2h", 4 * H, H)
    s += _linear(c + "1.x2f", H, H) + _linear(c + "1.x2h", 4 * H, H) + _linear(c + "1.h2h", 4 * H, H)
    s += _linear("pose_mlp.pose_fcs.0", 3, x + H)
    if p.estimate_head:
        s += _linear("global_mlp.pose_fcs.0", 6, p.n_joints_hm * H)
    return s


def is_buffer(key: str) -> bool:
    return key.rsplit(".", 1)[-1] in BUFFER_LEAVES


# keys that exist in the checkpoint but never receive a gradient / are never read on the path
# (modeling_vit.py:610 pooler output discarded; use_cls_token=False, net_architecture.py:358)
LIFT_DEAD_KEYS = (
    "pos_heatmap_encoder.vit.embeddings.cls_token",
    "pos_heatmap_encoder.vit.pooler.dense.weight",
    "pos_heatmap_encoder.vit.pooler.dense.bias",
)


# ----------------------------------------------------------------------------------------- heatmap estimator
HM_STAGES = ((64, 1), (128, 2), (256, 2), (512, 2))    # torchvision resnet18: (channels, stride of first block)


def _bn2d(pre, c):
    return [(pre + ".weight", (c,)), (pre + ".bias", (c,)), (pre + ".running_mean", (c,)),
            (pre + ".running_var", (c,)), (pre + ".num_batches_tracked", ())]


# heatmap sides at which the estimators' batch-statistics forwards (forward_bnbatch_into, hm_training) and stage-1 training are built; the
# eval-mode forward runs at every multiple of 16 (egotap.h egotap_hm_forward)
HM_BATCH_STATS_SIDES = (64, 128)


def hm_check_batch_stats_side(hm_size: int, what: str) -> None:
    """raise NotImplementedError, naming the built sides, when `what` (a batch-statistics path) is asked for at another side"""
    if hm_size not in HM_BATCH_STATS_SIDES:
        raise NotImplementedError(f"{what} is built at heatmap sides {' and '.join(map(str, HM_BATCH_STATS_SIDES))} only "
                                  f"(256x256 / 512x512 RGB), not {hm_size}; the eval-mode estimator forward runs at every multiple of 16")


# ... and the sides at which the estimator's BACKWARD is built: the 3x3 / 1x1 weight-gradient kernels (hm_train.h conv_wgrad_kernel) have no
# instantiation at map width 128 (their double-buffered row tiles exceed the LDS there), so a stage-1 step at 512x512 RGB cannot finish
HM_TRAIN_SIDES = (64,)


def hm_check_train_side(hm_size: int, what: str) -> None:
    """raise NotImplementedError by name when `what` (a path that needs the estimator's gradient) is asked for at a side without a backward"""
    hm_check_batch_stats_side(hm_size, what)
    if hm_size not in HM_TRAIN_SIDES:
        raise NotImplementedError(f"{what} is built at heatmap side {' and '.join(map(str, HM_TRAIN_SIDES))} only (256x256 RGB), not {hm_size}: "
                                  f"the weight-gradient kernels have no instantiation at map width {hm_size}; the batch-statistics forward "
                                  f"without a gradient (hm_train_forward_nograd) runs at sides {' and '.join(map(str, HM_BATCH_STATS_SIDES))}")


HM_BLOCKS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}      # BasicBlock ResNets of torchvision (net_architecture.py:57-60)
HM_BOTTLENECK = {"resnet50": (3, 4, 6, 3), "resnet101": (3, 4, 23, 3)}  # Bottleneck ResNets (net_architecture.py:61-64), expansion 4


def hm_blocks(model_name: str = "resnet18"):
    """BasicBlocks per stage of the nets the one-call C forward, the bf16 modes and stage-1 training cover; raises for resnet50 / resnet101
    (Bottleneck blocks: hm_bottleneck_blocks -- fp32 eval forward composed from the operator entry points, networks.py)"""
    if model_name not in HM_BLOCKS:
        raise NotImplementedError(f"backbone {model_name!r}: only the BasicBlock ResNets run on this path ({', '.join(HM_BLOCKS)}; the shipped scripts use resnet18)")
    return HM_BLOCKS[model_name]


def hm_is_bottleneck(model_name: str) -> bool:
    return model_name in HM_BOTTLENECK


def hm_all_blocks(model_name: str = "resnet18"):
    if model_name in HM_BOTTLENECK:
        return HM_BOTTLENECK[model_name]
    return hm_blocks(model_name)


def hm_feature_scale(model_name: str = "resnet18") -> int:
    """net_architecture.py:104-111: channels of the pyramid levels relative to resnet18 (Bottleneck expansion 4)"""
    return 4 if model_name in HM_BOTTLENECK else 1


def resnet18_spec(model_name: str = "resnet18"):
    """[(key, shape)] of torchvision.models.resnet18().state_dict() (public architecture; 122 entries) -- or resnet34's (218 entries),
    resnet50's (320) and resnet101's (626): Bottleneck = conv1 1x1 -> conv2 3x3 (carries the stride, torchvision's v1.5) -> conv3 1x1 to
    4 x width, downsample in the first block of every stage (layer1's too: 64 -> 256 channels)."""
    s = [("conv1.weight", (64, 3, 7, 7))] + _bn2d("bn1", 64)
    cin = 64
    blocks = hm_all_blocks(model_name)
    bott = hm_is_bottleneck(model_name)
    for i, (c, stride) in enumerate(HM_STAGES, start=1):
        cout = 4 * c if bott else c
        for b in range(blocks[i - 1]):
            pre = f"layer{i}.{b}"
            bc_in = cin if b == 0 else cout
            if bott:
                s += [(pre + ".conv1.weight", (c, bc_in, 1, 1))] + _bn2d(pre + ".bn1", c)
                s += [(pre + ".conv2.weight", (c, c, 3, 3))] + _bn2d(pre + ".bn2", c)
                s += [(pre + ".conv3.weight", (cout, c, 1, 1))] + _bn2d(pre + ".bn3", cout)
            else:
                s += [(pre + ".conv1.weight", (c, bc_in, 3, 3))] + _bn2d(pre + ".bn1", c)
                s += [(pre + ".conv2.weight", (c, c, 3, 3))] + _bn2d(pre + ".bn2", c)
            if b == 0 and (stride != 1 or cin != cout):
                s += [(pre + ".downsample.0.weight", (cout, bc_in, 1, 1))] + _bn2d(pre + ".downsample.1", cout)
        cin = cout
    s += [("fc.weight", (1000, cin)), ("fc.bias", (1000,))]
    return s


def hm_state_spec(n_hm_per_eye: int, model_name: str = "resnet18"):
    """[(key, shape, alias_of)] of HeatMap_UnrealEgo_Shared(resnet18, stereo).state_dict() in the reference's order.

    Encoder_Block registers the ResNet and, again, its slices layer0..layer4 (net_architecture.py:58, 68-73), so
    every backbone tensor appears under two keys; alias_of names the canonical key of the shared tensor.
    n_hm_per_eye = num_heatmap + 2 * num_rot_heatmap of that net (15 for the position net, 30 for the sin/cos net).
    """
    rs = resnet18_spec(model_name)
    root = "backbone.backbone."
    out = [(root + "backbone." + k, shp, None) for k, shp in rs]

    def dup(prefix_new, prefix_old):
        for k, shp in rs:
            if k.startswith(prefix_old):
                out.append((root + prefix_new + k[len(prefix_old):], shp, root + "backbone." + k))

    dup("layer0.0.", "conv1.")
    dup("layer0.1.", "bn1.")
    dup("layer1.1.", "layer1.")
    dup("layer2.", "layer2.")
    dup("layer3.", "layer3.")
    dup("layer4.", "layer4.")
    a = "after_backbone."

    def conv(name, cout, cin, k):
        return [(a + name + ".weight", (cout, cin, k, k), None), (a + name + ".bias", (cout,), None)]

    f = 2 * hm_feature_scale(model_name)            # feature_scale * input_channel_scale (net_architecture.py:113)
    out += conv("layer1_1x1.0", 64 * f, 64 * f, 1) + conv("layer2_1x1.0", 128 * f, 128 * f, 1)
    out += conv("layer3_1x1.0", 258 * f, 256 * f, 1) + conv("layer4_1x1.0", 512 * f, 512 * f, 1)
    out += conv("conv_up3.0", 512 * f, 258 * f + 512 * f, 3) + conv("conv_up2.0", 256 * f, 128 * f + 512 * f, 3)
    out += conv("conv_up1.0", 256 * f, 64 * f + 256 * f, 3)
    out += conv("conv_heatmap", 2 * n_hm_per_eye, 256 * f, 1)
    return out


# ---- camera bytes -> network input (egotap.h: egotap_rgb_u8_to_f32 / egotap_hm_forward_u8 / egotap_predict_pose_rgb_u8) -----------------
RGB_MEAN = (0.485, 0.456, 0.406)          # utils/util.py:188-197 normalize_ImageNet
RGB_STD = (0.229, 0.224, 0.225)


def rgb_u8_table(opt=None):
    """fp32 numpy [3, 256]: the network input value of byte v in channel c, with the reference's arithmetic evaluated once per (channel, byte)

        float32( (float64(float32(v) / float32(255)) - mean[c]) / std[c] )

    -- astype(float32) / 255 (utils/util.py:438), normalize_ImageNet's float64 numpy branch, the loader's .float() last.  ``opt.rgb_mean`` /
    ``opt.rgb_std`` (three floats each) override the ImageNet statistics.  Pinned bit for bit by tests/golden/rgb_u8_norm.npz."""
    import numpy as np
    mean = tuple(getattr(opt, "rgb_mean", None) or RGB_MEAN)
    std = tuple(getattr(opt, "rgb_std", None) or RGB_STD)
    if len(mean) != 3 or len(std) != 3 or any(float(s) == 0.0 for s in std):
        raise ValueError(f"rgb_mean / rgb_std: three values each and no zero std, got {mean} / {std}")
    x = (np.arange(256, dtype=np.uint8).astype(np.float32) / np.float32(255.0)).astype(np.float64).reshape(1, 256)
    t = (x - np.array(mean, dtype=np.float64).reshape(3, 1)) / np.array(std, dtype=np.float64).reshape(3, 1)
    return np.ascontiguousarray(t.astype(np.float32))


# ---- sensor frames -> camera bytes: crop, mirror, bilinear resize (egotap.h: egotap_rgb_u8_resize / egotap_predict_pose_sensor_u8) ------
RESIZE_WEIGHT_ONE = 2048          # one axis weight in fixed point (11 bits); two axes and a byte: 2048^2 * 255 + 2^21 < 2^31


def resize_taps(L: int, S0: int):
    """The two source taps and the weight of the second one, for each of the S0 output indices along an axis of source length L, in integers
    (align_corners=False, what F.interpolate bilinear and cv2 INTER_LINEAR sample): with n = max((2X + 1) L - S0, 0),

        i0 = n div 2S0,  r = n mod 2S0,  w1 = (r * 2048 + S0) div 2S0,  w0 = 2048 - w1,  i1 = min(i0 + 1, L - 1)

    Returns int64 numpy arrays (i0, i1, w1).  L = S0 gives i0 = X, w1 = 0: an exact copy.  Each weight is within 2^-12 of the real one."""
    import numpy as np
    if L < 1 or S0 < 1:
        raise ValueError(f"resize_taps: source length and output side must be positive, got {L}, {S0}")
    X = np.arange(S0, dtype=np.int64)
    n = np.maximum((2 * X + 1) * L - S0, 0)
    i0, r = n // (2 * S0), n % (2 * S0)
    w1 = (r * RESIZE_WEIGHT_ONE + S0) // (2 * S0)
    return i0, np.minimum(i0 + 1, L - 1), w1


def check_resize_rect(who: str, rect, H: int, W: int):
    """(x0, y0, w, h) in source pixels, inside the H x W frame, w, h >= 1; returns it as four ints"""
    if rect is None:
        return (0, 0, int(W), int(H))
    if len(rect) != 4:
        raise ValueError(f"{who}: a rectangle is (x0, y0, w, h), got {tuple(rect)}")
    x0, y0, w, h = (int(v) for v in rect)
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
        raise ValueError(f"{who}: rectangle (x0, y0, w, h) = {(x0, y0, w, h)} is empty or outside the {H} x {W} frame")
    return x0, y0, w, h


def resize_u8(frames, rect, mirror: bool, S0: int):
    """The whole resize, restated in integers on the host: frames uint8 [n, H, W, 3] (numpy array or torch tensor on any device) -> uint8
    [n, S0, S0, 3] of the same kind.  The source rectangle ``rect`` = (x0, y0, w, h) (None: the full frame) is sampled with ``resize_taps``
    along each axis and

        out = (sum_{a, b in {0, 1}} wy_a wx_b p[y0 + iy_a][x0 + ix_b][c] + 2^21) >> 22          (one rounding; the sum is exact in int32)

    With ``mirror``, output column X takes the value column S0 - 1 - X has without it.  The reference flips the frame and then crops
    (reprocess_egocap_data.py:100-104): its rectangle x0' in flipped coordinates is x0 = W - x0' - w here.  This is what rgb_u8_resize_kernel
    computes, bit for bit; against exact bilinear interpolation E every byte satisfies |out - E| <= 0.5 + 510 / 4096."""
    import numpy as np
    import torch
    is_np = isinstance(frames, np.ndarray)
    x = torch.from_numpy(frames) if is_np else frames
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"resize_u8: frames are uint8 [n, H, W, 3], got {x.dtype} {tuple(x.shape)}")
    H, W = int(x.shape[1]), int(x.shape[2])
    x0, y0, w, h = check_resize_rect("resize_u8", rect, H, W)
    dev = x.device
    ix0, ix1, wx1 = (torch.from_numpy(a).to(dev) for a in resize_taps(w, S0))
    iy0, iy1, wy1 = (torch.from_numpy(a).to(dev) for a in resize_taps(h, S0))
    if mirror:
        ix0, ix1, wx1 = ix0.flip(0), ix1.flip(0), wx1.flip(0)
    wx0, wy0 = RESIZE_WEIGHT_ONE - wx1, RESIZE_WEIGHT_ONE - wy1
    acc = torch.zeros((x.shape[0], S0, S0, 3), dtype=torch.int64, device=dev)
    for iy, wy in ((iy0, wy0), (iy1, wy1)):
        rows = x[:, y0 + iy]                                                     # [n, S0, W, 3]
        for ix, wx in ((ix0, wx0), (ix1, wx1)):
            acc += rows[:, :, x0 + ix].to(torch.int64) * (wy.view(1, S0, 1, 1) * wx.view(1, 1, S0, 1))
    out = ((acc + (1 << 21)) >> 22).to(torch.uint8)
    return out.numpy() if is_np else out


# ---- NV12 / YUYV sensor frames -> RGB bytes -> camera bytes (egotap.h: egotap_yuv_u8_resize / egotap_predict_pose_sensor_yuv) ------------
YUV_FORMATS = {"nv12": 0, "yuyv": 1}                 # egotap.h EGOTAP_YUV_NV12 / _YUYV
YUV_MATRICES = {"bt601": (0, 0.299, 0.114), "bt709": (1, 0.2126, 0.0722)}      # egotap.h EGOTAP_YUV_BT601 / _BT709: (code, Kr, Kb)
YUV_RANGES = {"limited": 0, "full": 1}               # egotap.h EGOTAP_YUV_LIMITED / _FULL
YUV_SHIFT = 14                                       # coefficients are round(real * 2^14); every intermediate stays below 2^24 in magnitude
YUV_MAX_SIDE = 16384                                 # H, W <= 16384, as for the resize


@dataclass(frozen=True)
class YuvLayout:
    """Where the bytes of one H x W frame sit inside its ``frame_stride`` bytes (egotap.h egotap_yuv_source).

    nv12: Y(y, x) at y * pitch + x; the chroma pair of pixel (y, x) at uv_offset + (y >> 1) * pitch + 2 * (x >> 1), U then V.  H and W even,
          pitch >= W, uv_offset >= pitch * (H - 1) + W (the planes do not overlap), the last chroma byte inside frame_stride; pitch, uv_offset and
          frame_stride even (the chroma pair is one aligned 16-bit load).
    yuyv: the pixel pair x >> 1 of row y is the four bytes Y0 U Y1 V at y * pitch + 4 * (x >> 1).  W even, pitch >= 2 W, the last row inside
          frame_stride; pitch and frame_stride multiples of 4 (the pair is one aligned dword); uv_offset is 0.
    Chroma is replicated: every pixel of a 2 x 2 block (nv12) or of a pair (yuyv) takes the block's U and V.  Use the constructors ``nv12`` /
    ``yuyv``: their defaults give the tight layout."""
    format: str
    H: int
    W: int
    pitch: int
    uv_offset: int
    frame_stride: int

    def __post_init__(self):
        f, H, W, pitch, uv, fs = self.format, self.H, self.W, self.pitch, self.uv_offset, self.frame_stride
        if f not in YUV_FORMATS:
            raise ValueError(f"YuvLayout: unknown format {f!r} (one of {sorted(YUV_FORMATS)})")
        who = f"YuvLayout.{f}"
        if not (1 <= H <= YUV_MAX_SIDE and 1 <= W <= YUV_MAX_SIDE):
            raise ValueError(f"{who}: the frame height and width must be between 1 and {YUV_MAX_SIDE}, got {H} x {W}")
        if f == "nv12":
            if H % 2 or W % 2:
                raise ValueError(f"{who}: H and W must be even (4:2:0 chroma covers 2 x 2 blocks), got {H} x {W}")
            if pitch < W:
                raise ValueError(f"{who}: pitch {pitch} is smaller than W = {W}")
            if uv < pitch * (H - 1) + W:
                raise ValueError(f"{who}: the planes overlap: uv_offset {uv} is smaller than pitch * (H - 1) + W = {pitch * (H - 1) + W}")
            if uv + (H // 2 - 1) * pitch + W > fs:
                raise ValueError(f"{who}: the last chroma byte {uv + (H // 2 - 1) * pitch + W - 1} is past frame_stride {fs}")
            if pitch % 2 or uv % 2 or fs % 2:
                raise ValueError(f"{who}: pitch, uv_offset and frame_stride must be even, got {pitch}, {uv}, {fs}")
        else:
            if W % 2:
                raise ValueError(f"{who}: W must be even (4:2:2 chroma covers pixel pairs), got {W}")
            if pitch < 2 * W:
                raise ValueError(f"{who}: pitch {pitch} is smaller than 2 W = {2 * W}")
            if uv != 0:
                raise ValueError(f"{who}: a packed format has no chroma plane (uv_offset must be 0, got {uv})")
            if (H - 1) * pitch + 2 * W > fs:
                raise ValueError(f"{who}: the last byte {(H - 1) * pitch + 2 * W - 1} is past frame_stride {fs}")
            if pitch % 4 or fs % 4:
                raise ValueError(f"{who}: pitch and frame_stride must be multiples of 4, got {pitch}, {fs}")

    @staticmethod
    def nv12(H, W, pitch=None, uv_offset=None, frame_stride=None):
        H, W = int(H), int(W)
        pitch = W if pitch is None else int(pitch)
        uv_offset = pitch * H if uv_offset is None else int(uv_offset)
        frame_stride = uv_offset + pitch * (H // 2) if frame_stride is None else int(frame_stride)
        return YuvLayout("nv12", H, W, pitch, uv_offset, frame_stride)

    @staticmethod
    def yuyv(H, W, pitch=None, frame_stride=None):
        H, W = int(H), int(W)
        pitch = 2 * W if pitch is None else int(pitch)
        return YuvLayout("yuyv", H, W, pitch, 0, pitch * H if frame_stride is None else int(frame_stride))

    @property
    def base_alignment(self):
        """what the address of frame 0 must be a multiple of: the widest load of the format"""
        return 2 if self.format == "nv12" else 4


@dataclass(frozen=True)
class YuvColour:
    """Which Y'CbCr a source carries: matrix bt601 (Kr, Kb = 0.299, 0.114) or bt709 (0.2126, 0.0722), range limited (Y 16 .. 235, chroma
    16 .. 240) or full (0 .. 255).  With Kg = 1 - Kr - Kb, (cy, cc, y_off) = (255/219, 255/224, 16) limited or (1, 1, 0) full:

        rv = 2 (1 - Kr) cc    bu = 2 (1 - Kb) cc    gu = 2 Kb (1 - Kb) / Kg cc    gv = 2 Kr (1 - Kr) / Kg cc

    ``coefficients()`` returns the integers (CY, RV, GU, GV, BU, y_off), each coefficient round(real * 2^14)."""
    matrix: str = "bt601"
    range: str = "limited"

    def __post_init__(self):
        if self.matrix not in YUV_MATRICES:
            raise ValueError(f"YuvColour: unknown matrix {self.matrix!r} (one of {sorted(YUV_MATRICES)})")
        if self.range not in YUV_RANGES:
            raise ValueError(f"YuvColour: unknown range {self.range!r} (one of {sorted(YUV_RANGES)})")

    def real_coefficients(self):
        """(cy, rv, gu, gv, bu, y_off) as float64"""
        _, kr, kb = YUV_MATRICES[self.matrix]
        kg = 1.0 - kr - kb
        limited = self.range == "limited"
        cy = 255.0 / 219.0 if limited else 1.0
        cc = 255.0 / 224.0 if limited else 1.0
        return (cy, 2.0 * (1.0 - kr) * cc, 2.0 * kb * (1.0 - kb) / kg * cc, 2.0 * kr * (1.0 - kr) / kg * cc, 2.0 * (1.0 - kb) * cc,
                16 if limited else 0)

    def coefficients(self):
        real = self.real_coefficients()
        return tuple(int(math.floor(v * float(1 << YUV_SHIFT) + 0.5)) for v in real[:5]) + (real[5],)


def yuv_rgb_bytes(Y, U, V, colour: YuvColour):
    """The colour arithmetic alone, elementwise on integer torch tensors of one shape holding bytes: returns (R, G, B) as int32 tensors in 0 .. 255.

        R = clip((CY (Y - y_off) + RV (V - 128) + 2^13) >> 14, 0, 255)
        G = clip((CY (Y - y_off) - GU (U - 128) - GV (V - 128) + 2^13) >> 14, 0, 255)
        B = clip((CY (Y - y_off) + BU (U - 128) + 2^13) >> 14, 0, 255)

    The shift is arithmetic, there is one rounding, every intermediate stays below 2^24 in magnitude.  Against the real formula every byte is within
    0.5 + (max |Y - y_off| + the sum of max |C - 128| over the channel's chroma terms) * 2^-15: each coefficient is off by at most 2^-15."""
    import torch
    cy, rv, gu, gv, bu, y_off = colour.coefficients()
    half = 1 << (YUV_SHIFT - 1)
    c = cy * (Y.to(torch.int32) - y_off) + half
    u, v = U.to(torch.int32) - 128, V.to(torch.int32) - 128
    return tuple(((t) >> YUV_SHIFT).clamp_(0, 255) for t in (c + rv * v, c - gu * u - gv * v, c + bu * u))


def yuv_to_rgb_u8(frames, layout: YuvLayout, colour: YuvColour):
    """NV12 / YUYV frames -> RGB bytes, restated in integers on the host: ``frames`` uint8 (numpy array or torch tensor on any device) of n frames
    of ``layout.frame_stride`` bytes each (any shape whose first axis is n) -> uint8 [n, H, W, 3] of the same kind.  Each pixel takes its own Y and
    the U, V of its block (``YuvLayout``: replicated chroma, no interpolation) through ``yuv_rgb_bytes``.  Bytes outside the planes (row padding
    past W or 2 W, the gap in front of the chroma plane, the tail of the frame) are never read."""
    import numpy as np
    import torch
    is_np = isinstance(frames, np.ndarray)
    x = torch.from_numpy(frames) if is_np else frames
    n = int(x.shape[0]) if x.dim() else 0
    fs, H, W, pitch = layout.frame_stride, layout.H, layout.W, layout.pitch
    if x.dtype != torch.uint8 or x.dim() < 1 or x.numel() != n * fs:
        raise ValueError(f"yuv_to_rgb_u8: frames are uint8, n frames of frame_stride = {fs} bytes each, got {x.dtype} {tuple(x.shape)}")
    x = x.reshape(n, fs).contiguous()
    at = x.storage_offset()
    if layout.format == "nv12":
        Y = torch.as_strided(x, (n, H, W), (fs, pitch, 1), at)
        U, V = (torch.as_strided(x, (n, H // 2, W // 2), (fs, pitch, 2), at + layout.uv_offset + k).repeat_interleave(2, 1).repeat_interleave(2, 2)
                for k in (0, 1))
    else:
        Y = torch.as_strided(x, (n, H, W), (fs, pitch, 2), at)
        U, V = (torch.as_strided(x, (n, H, W // 2), (fs, pitch, 4), at + k).repeat_interleave(2, 2) for k in (1, 3))
    out = torch.stack(yuv_rgb_bytes(Y, U, V, colour), dim=-1).to(torch.uint8)
    return out.numpy() if is_np else out


def yuv_resize_u8(frames, layout: YuvLayout, colour: YuvColour, rect, mirror: bool, S0: int):
    """The whole conversion-and-resize, by definition ``resize_u8(yuv_to_rgb_u8(frames, layout, colour), rect, mirror, S0)``: each of the four taps
    of an output pixel is converted to RGB bytes (clipped and rounded), then the bilinear formula runs on those bytes -- nothing is interpolated in
    YUV.  This is what yuv_u8_resize_kernel computes, bit for bit."""
    return resize_u8(yuv_to_rgb_u8(frames, layout, colour), rect, mirror, S0)


# ---- heatmaps -> 2D joints and confidences (egotap.h: egotap_heatmap_peaks / egotap_predict_pose_*_kp) ----------------------------------
def _fma_f32(a, x, b):
    """float32(a * x + b) with ONE rounding, for float32 arrays: the product is exact in float64, the sum is rounded to odd there (TwoSum gives its
    error), so the final rounding to float32 sees the exact sum's side of every tie -- what fmaf computes."""
    import numpy as np
    p = a.astype(np.float64) * x.astype(np.float64)
    b = b.astype(np.float64)
    s = p + b
    bb = s - p
    err = (p - (s - bb)) + (b - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even & np.isfinite(s), np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def sensor_keypoint_affine(rect, mirror: bool, S: int):
    """(ax, bx, ay, by) as float32: heatmap pixels (side S, pixel centres at i + 0.5) -> pixels of the sensor frame the eye's rectangle
    (x0, y0, w, h) was cut from -- the inverse of ``resize_u8``'s map (align_corners=False).  With ``mirror`` output column X shows what
    column 4S - 1 - X shows without it, so x runs backwards from the rectangle's right edge."""
    import numpy as np
    x0, y0, w, h = (int(v) for v in rect)
    sx = np.float32(w) / np.float32(S)
    return (np.float32(-sx if mirror else sx), np.float32(x0 + (w if mirror else 0)), np.float32(h) / np.float32(S), np.float32(y0))


def heatmap_peaks_ref(hm, groups: int = 1, affine=None):
    """The record egotap_heatmap_peaks writes, restated in numpy: hm [B, n, S, S] (float32, or anything exactly representable in it -- bf16
    values upcast) -> float32 [B, n, 4] = (x, y, score, index) per map.

        index = iy * S + ix   the maximum's position: values compared as float32, a larger value wins, among equal values the smallest linear
                              index; a NaN never beats a number (the maximum starts at -inf: a map may be all negative); only NaNs -> 0
        score = hm[iy][ix]
        x     = ix + 0.5 + 0.25 * sgn(hm[iy][ix + 1] - hm[iy][ix - 1])      0 step when a neighbour is outside the map or the difference is 0 / NaN
        y     = iy + 0.5 + 0.25 * sgn(hm[iy + 1][ix] - hm[iy - 1][ix])

    The reference's target (utils/projection.py:263-279) puts its delta at int(x): a joint in [ix, ix + 1) peaks at ix, so ix + 0.5 is the unbiased
    read-out; the quarter-pixel step towards the higher neighbour is the usual one of heatmap estimators.  ``affine``: [groups, 4] = (ax, bx, ay, by)
    for each group of n / groups consecutive channels, x_out = fma(ax, x, bx), y_out = fma(ay, y, by) in float32 (None: identity).  Every step is
    exact or a single float32 rounding, so the result is defined bit for bit."""
    import numpy as np
    h = np.asarray(hm, dtype=np.float32)
    if h.ndim != 4 or h.shape[2] != h.shape[3]:
        raise ValueError(f"heatmap_peaks_ref: maps are [B, n, S, S], got {h.shape}")
    B, n, S, _ = h.shape
    if groups < 1 or n % groups:
        raise ValueError(f"heatmap_peaks_ref: n = {n} is no multiple of groups = {groups}")
    flat = h.reshape(B * n, S * S)
    valid = ~np.isnan(flat)
    top = np.where(valid, flat, -np.inf).max(axis=1, keepdims=True)
    index = np.where(valid.any(axis=1), np.argmax(valid & (flat == top), axis=1), 0)        # (argmax of booleans: the first True)
    iy, ix = index // S, index % S
    rows = np.arange(B * n)
    maps = flat.reshape(B * n, S, S)

    def step(lo_ok, hi_ok, lo, hi):
        with np.errstate(invalid="ignore"):
            d = hi - lo                                                                     # (inf - inf = NaN: no step)
        return np.where(lo_ok & hi_ok, np.float32(0.25) * np.sign(np.nan_to_num(d, nan=0.0, posinf=1.0, neginf=-1.0)), 0).astype(np.float32)
    dx = step(ix > 0, ix < S - 1, maps[rows, iy, np.maximum(ix - 1, 0)], maps[rows, iy, np.minimum(ix + 1, S - 1)])
    dy = step(iy > 0, iy < S - 1, maps[rows, np.maximum(iy - 1, 0), ix], maps[rows, np.minimum(iy + 1, S - 1), ix])
    x = ix.astype(np.float32) + np.float32(0.5) + dx
    y = iy.astype(np.float32) + np.float32(0.5) + dy
    if affine is not None:
        a = np.asarray(affine, dtype=np.float32)
        if a.shape != (groups, 4):
            raise ValueError(f"heatmap_peaks_ref: affine is [groups, 4] = (ax, bx, ay, by) per group, got {a.shape}")
        a = np.tile(np.repeat(a, n // groups, axis=0), (B, 1))                              # one row per map
        x, y = _fma_f32(a[:, 0], x, a[:, 1]), _fma_f32(a[:, 2], y, a[:, 3])
    out = np.stack([x, y, flat[rows, index], index.astype(np.float32)], axis=1).astype(np.float32)
    return out.reshape(B, n, 4)


# ---- sin/cos limb heatmaps -> elevation angles and 2D segments (egotap.h: egotap_limb_decode / egotap_predict_pose_*_kpl) ------------------
def limb_decode_ref(hm, c0: int, n_limbs: int, eyes: int, affine=None):
    """The record egotap_limb_decode writes, restated in float64 numpy: hm [B, C, S, S] (float32, or anything exactly representable in it -- bf16
    values upcast) -> float32 [B, eyes, n_limbs, 8] = (theta, coherence, x, y, phi, length, peak, mass) per (cos, sin) pair.  For eye e and limb l
    the cos map c is channel c0 + e * 2 n_limbs + l and the sin map s channel c0 + e * 2 n_limbs + n_limbs + l (the reference's cat(cos, sin) per
    eye).  Every sum runs over all S*S pixels in float64, pixel centres at ix + 0.5, iy + 0.5:

        m = sqrt(c^2 + s^2)   M = sum m   C = sum c   Sn = sum s   X = sum m x   Y = sum m y   XX = sum m x^2   YY = sum m y^2   XY = sum m x y
        peak      = max m                      a NaN never wins; starts at 0
        theta     = atan2(Sn, C)               exact for a target pair: both maps are the same non-negative map times sin / cos theta
        coherence = hypot(C, Sn) / M           in [0, 1]; 1 when every pixel votes for the same angle
        x, y      = ax * X/M + bx, ay * Y/M + by                                     the eye's affine (ax, bx, ay, by); None: identity
        mu20 = XX/M - (X/M)^2, mu02 = YY/M - (Y/M)^2, mu11 = XY/M - (X/M)(Y/M), scaled by ax^2, ay^2, ax ay;   D = (mu20' - mu02')^2 + 4 mu11'^2
        phi       = atan2(2 mu11', mu20' - mu02') / 2                                the segment's orientation in the output frame, in (-pi/2, pi/2]
        length    = sqrt(12 sqrt(D))           a uniform segment of length l blurred by an isotropic sigma has variance l^2/12 + sigma^2 along its
                                               axis and sigma^2 across it: the eigenvalues differ by sqrt(D), the blur drops out (exact for |ax| = |ay|)
        mass      = M

    The segment's ends are (x, y) +- length / 2 * (cos phi, sin phi).  theta is an angle of the pose's own frame: the affine does not touch it.
    Empty rule, when not (M > 0) or M is not finite (an all-zero pair, a NaN or inf inside): theta = coherence = phi = length = 0, (x, y) the
    affine of the map centre (S/2, S/2), peak as computed, mass = float32(M).  Each value is rounded once from float64."""
    import numpy as np
    h = np.asarray(hm, dtype=np.float32)
    if h.ndim != 4 or h.shape[2] != h.shape[3]:
        raise ValueError(f"limb_decode_ref: maps are [B, C, S, S], got {h.shape}")
    B, Cn, S, _ = h.shape
    if c0 < 0 or n_limbs < 1 or eyes < 1 or c0 + 2 * eyes * n_limbs > Cn:
        raise ValueError(f"limb_decode_ref: channels {c0} .. {c0 + 2 * eyes * n_limbs - 1} are not inside the {Cn} channels")
    a = np.tile(np.array([1.0, 0.0, 1.0, 0.0]), (eyes, 1)) if affine is None else np.asarray(affine, dtype=np.float32).astype(np.float64)
    if a.shape != (eyes, 4):
        raise ValueError(f"limb_decode_ref: affine is [eyes, 4] = (ax, bx, ay, by) per eye, got {a.shape}")
    pairs = h[:, c0:c0 + 2 * eyes * n_limbs].astype(np.float64).reshape(B, eyes, 2, n_limbs, S, S)
    c, s = pairs[:, :, 0], pairs[:, :, 1]                                                   # [B, eyes, n_limbs, S, S]
    x = (np.arange(S) + 0.5).reshape(1, 1, 1, 1, S)
    y = (np.arange(S) + 0.5).reshape(1, 1, 1, S, 1)
    ax, bx, ay, by = (a[:, k].reshape(1, eyes, 1) for k in range(4))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.sqrt(c * c + s * s)
        mx, my = m * x, m * y
        M, C, Sn, X, Y, XX, YY, XY = (t.sum(axis=(3, 4)) for t in (m, c, s, mx, my, mx * x, my * y, mx * y))
        peak = np.where(np.isnan(m), 0.0, m).max(axis=(3, 4))
        full = (M > 0) & np.isfinite(M)
        Md = np.where(full, M, 1.0)
        xb = np.where(full, X / Md, 0.5 * S)
        yb = np.where(full, Y / Md, 0.5 * S)
        m20, m02, m11 = (XX / Md - xb * xb) * (ax * ax), (YY / Md - yb * yb) * (ay * ay), (XY / Md - xb * yb) * (ax * ay)
        d = m20 - m02
        D = d * d + 4.0 * (m11 * m11)
        rec = [np.arctan2(Sn, C), np.hypot(C, Sn) / Md, ax * xb + bx, ay * yb + by,
               0.5 * np.arctan2(2.0 * m11 + 0.0, d),                                        # (+ 0.0: a -0 numerator would turn pi/2 into -pi/2)
               np.sqrt(12.0 * np.sqrt(D)), peak, M]
        for k in (0, 1, 4, 5):
            rec[k] = np.where(full, rec[k], 0.0)
        return np.stack(np.broadcast_arrays(*rec), axis=-1).astype(np.float32)


# ---- the fisheye camera model and stereo triangulation (egotap.h: egotap_ocam_project / _ocam_unproject / egotap_stereo_triangulate) ------
OCAM_MAX_POL, OCAM_MAX_INVPOL = 8, 24          # egotap.h EGOTAP_OCAM_MAX_POL / _MAX_INVPOL
STEREO_MAX_JOINTS = 64                         # one lane per joint
STEREO_MIN_SCORE = 0.5                         # target maps peak at 1 for a joint in view and are all zero otherwise (utils/projection.py:263-279)


@dataclass(frozen=True)
class OcamModel:
    """One camera's OCamCalib model as the reference reads it (utils/projection.py:13-50): ``pol`` the cam2world polynomial in the pixel
    radius (polynomialC2W), ``invpol`` the world2cam polynomial in the elevation angle (polynomialW2C), the centre (xc, yc) -- xc multiplies
    the FIRST pixel coordinate, as in world2cam -- and the affine (c, d, e).  ``size`` (h, w) and ``radius`` (the image circle, 0: none) are carried; only ``lens_map`` reads them."""
    name: str
    pol: tuple
    invpol: tuple
    xc: float
    yc: float
    c: float = 1.0
    d: float = 0.0
    e: float = 0.0
    size: tuple = (1024, 1024)
    radius: float = 0.0

    def __post_init__(self):
        object.__setattr__(self, "pol", tuple(float(v) for v in self.pol))
        object.__setattr__(self, "invpol", tuple(float(v) for v in self.invpol))
        for k in ("xc", "yc", "c", "d", "e", "radius"):
            object.__setattr__(self, k, float(getattr(self, k)))
        object.__setattr__(self, "size", tuple(int(v) for v in self.size))
        if not 1 <= len(self.pol) <= OCAM_MAX_POL:
            raise ValueError(f"OcamModel {self.name!r}: polynomialC2W has {len(self.pol)} coefficients, 1 .. {OCAM_MAX_POL} are supported")
        if not 1 <= len(self.invpol) <= OCAM_MAX_INVPOL:
            raise ValueError(f"OcamModel {self.name!r}: polynomialW2C has {len(self.invpol)} coefficients, 1 .. {OCAM_MAX_INVPOL} are supported")
        if not all(math.isfinite(v) for v in self.pol + self.invpol + (self.xc, self.yc, self.c, self.d, self.e)):
            raise ValueError(f"OcamModel {self.name!r}: a calibration value is not finite")
        if self.c - self.d * self.e == 0.0:
            raise ValueError(f"OcamModel {self.name!r}: the affine is singular (c - d * e == 0)")

    @property
    def ue_flip(self):         # utils/projection.py:96, 141
        return self.name == "unreal_ego_pose"


def ocam_from_json(data) -> OcamModel:
    """An OcamModel from the reference's ``fisheye.calibration_{side}.json`` -- a path, or the parsed dict -- with the reference's field mapping
    (utils/projection.py:26-44): xc = image_center[1], yc = image_center[0], affine = [c, d, e]."""
    if not isinstance(data, dict):
        import json
        with open(data) as f:
            data = json.load(f)
    aff = data["affine"]
    if len(aff) != 3:
        raise ValueError(f"ocam_from_json: affine is [c, d, e], got {len(aff)} values")
    return OcamModel(name=data["name"], pol=data["polynomialC2W"], invpol=data["polynomialW2C"], xc=data["image_center"][1], yc=data["image_center"][0],
                     c=aff[0], d=aff[1], e=aff[2], size=tuple(data["size"]), radius=data["imageCircleRadius"])


def _ocam_poly(coef, r):
    """the reference's running-power sum (projection.py:73-79, 115-122): z = coef[0]; r_i *= r; z += r_i * coef[i] -- not Horner"""
    import numpy as np
    z = np.full(r.shape, coef[0], dtype=np.float64)
    r_i = np.ones_like(r)
    for k in range(1, len(coef)):
        r_i = r_i * r
        z = z + r_i * coef[k]
    return z


def ocam_world2cam_ref(points3d, model: OcamModel):
    """utils/projection.py:89-144 world2cam in float64 numpy, operation for operation: [..., 3] -> pixels [..., 2].  With ``ue_flip`` y and z are
    negated first (UEp2CVp) and v <- 2 yc - v last; norm = sqrt(x^2 + y^2); norm <= 1e-8 (isclose(norm, 0)) gives (xc, yc); otherwise
    theta = arctan(z / norm), rho = invpol(theta), x' = x * (1 / norm) * rho, y' likewise, u = x' c + y' d + xc, v = x' e + y' + yc."""
    import numpy as np
    p = np.array(points3d, dtype=np.float64)
    if p.shape[-1] != 3:
        raise ValueError(f"ocam_world2cam_ref: points are [..., 3], got {p.shape}")
    m = model
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    if m.ue_flip:
        y, z = y * -1.0, z * -1.0
    with np.errstate(all="ignore"):
        norm = np.sqrt(x * x + y * y)
        zero = norm <= 1e-8
        safe = np.where(zero, 1.0, norm)
        theta = np.arctan(z / safe)
        invnorm = 1.0 / safe
        rho = _ocam_poly(m.invpol, theta)
        xs, ys = x * invnorm * rho, y * invnorm * rho
        u = np.where(zero, m.xc, xs * m.c + ys * m.d + m.xc)
        v = np.where(zero, m.yc, xs * m.e + ys + m.yc)
        if m.ue_flip:
            v = m.yc * 2 - v
    return np.stack([u, v], axis=-1)


def ocam_cam2world_ref(points2d, model: OcamModel):
    """utils/projection.py:55-87 cam2world in float64 numpy, operation for operation, wrapped so that it inverts ``ocam_world2cam_ref``'s
    convention: pixels [..., 2] -> unit rays [..., 3] in the frame of the points world2cam takes.  With ``ue_flip``, v <- 2 yc - v before and
    (rx, -ry, -rz) after.  (The polynomials are fitted as each other's inverse: a ray's polynomial z has the sign of world2cam's z.)"""
    import numpy as np
    q = np.array(points2d, dtype=np.float64)
    if q.shape[-1] != 2:
        raise ValueError(f"ocam_cam2world_ref: pixels are [..., 2], got {q.shape}")
    m = model
    u, v = q[..., 0], q[..., 1]
    with np.errstate(all="ignore"):
        if m.ue_flip:
            v = m.yc * 2 - v
        invdet = 1.0 / (m.c - m.d * m.e)
        xp = invdet * ((u - m.xc) - m.d * (v - m.yc))
        yp = invdet * (-m.e * (u - m.xc) + m.c * (v - m.yc))
        r = np.sqrt(xp * xp + yp * yp)
        zp = _ocam_poly(m.pol, r)
        invnorm = 1.0 / np.sqrt(xp * xp + yp * yp + zp * zp)
        rx, ry, rz = invnorm * xp, invnorm * yp, invnorm * zp
        if m.ue_flip:
            ry, rz = ry * -1.0, rz * -1.0
    return np.stack([rx, ry, rz], axis=-1)


def stereo_pose_row0(preset: LiftPreset) -> int:
    """the row of the lifted pose that heatmap joint 0 is paired with: the heatmaps are gt_camera_2d[1:] (dataloader/data_loader.py:90), the pose
    target gt_local_pose with the head at row 0 when the head is estimated (UnrealEgo), gt_local_pose[1:] otherwise (:175); the loss pairs rows"""
    return 1 if preset.estimate_head else 0


def stereo_pixel_affine(model: OcamModel, S: int):
    """(ax, bx, ay, by): keypoints of the RGB / byte serving entries (pixels of the 4S x 4S input frame) -> the calibration's pixels.  The
    reference's maps are coord2d / 1024 * res with 1024 the calibration's image: size / (4S) per axis (size = (height, width))."""
    return (model.size[1] / (4.0 * S), 0.0, model.size[0] / (4.0 * S), 0.0)


STEREO_IDENTITY_AFFINE = ((1.0, 0.0, 1.0, 0.0),) * 2      # the sensor entry: its keypoints are already the calibrated sensor's pixels


def stereo_triangulate_ref(keypoints, left: OcamModel, right: OcamModel, t, R=None, affine=None, min_score=STEREO_MIN_SCORE, pose=None, pose_row0=0,
                           dtype="float32"):
    """The records egotap_stereo_triangulate writes, restated in float64 numpy: keypoints [B, 2, J, 4] (eye, joint, (x, y, score, index)) ->
    (joints3d float32 [B, J, 8], frame float32 [B, 8]).  ``t`` (3) and ``R`` (3 x 3, None: identity) are the right camera's origin and axes in
    the left camera's frame, ``affine`` [2, 4] = (ax, bx, ay, by) per eye from keypoint units to the calibration's pixels (None: identity).
    Per (frame, joint):

        seen  = both scores >= min_score (a NaN fails) and the four coordinates finite
        pL    = (ax x + bx, ay y + by);  dL = cam2world_L(pL);  dR = R cam2world_R(pR);  w0 = -t
        b = dL.dR   d = dL.w0   e = dR.w0   den = 1 - b^2   s = (b e - d) / den   u = (e - b d) / den
        PL = s dL   PR = t + u dR   X = (PL + PR) / 2   gap = |PL - PR|
        valid = seen and den > 0 and s > 0 and u > 0 and everything finite (with a pose: its row pose[pose_row0 + j] too)

    Per frame, summed over the valid joints in ascending order: n = #valid; with a pose [B, P, 3] and n >= 1,
    t_hat = sum X / n - sum pose[pose_row0 + j] / n and disagree_j = |X_j - pose[pose_row0 + j] - t_hat|.

        joints3d = (X, Y, Z, gap, den, s, disagree, valid);  an invalid joint is all zeros
        frame    = (t_hat x, y, z, n, rms disagree, max disagree, rms gap, max gap);  without a pose t_hat and the disagreements are 0; n = 0: zeros

    Each value is rounded once from float64 (``dtype="float64"``: not at all -- the records before that rounding)."""
    import numpy as np
    kp = np.asarray(keypoints, dtype=np.float64)
    if kp.ndim != 4 or kp.shape[1] != 2 or kp.shape[3] != 4:
        raise ValueError(f"stereo_triangulate_ref: keypoints are [B, 2, J, 4], got {kp.shape}")
    B, _, J, _ = kp.shape
    if not 1 <= J <= STEREO_MAX_JOINTS:
        raise ValueError(f"stereo_triangulate_ref: 1 .. {STEREO_MAX_JOINTS} joints, got {J}")
    t = np.asarray(t, dtype=np.float64).reshape(3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    a = np.asarray(STEREO_IDENTITY_AFFINE if affine is None else affine, dtype=np.float64).reshape(2, 4)
    ps = None
    if pose is not None:
        ps = np.asarray(pose, dtype=np.float64)
        if ps.ndim != 3 or ps.shape[0] != B or ps.shape[2] != 3 or pose_row0 < 0 or pose_row0 + J > ps.shape[1]:
            raise ValueError(f"stereo_triangulate_ref: pose is [B, P, 3] with pose_row0 + J <= P, got {ps.shape}, pose_row0 = {pose_row0}, J = {J}")
        ps = ps[:, pose_row0:pose_row0 + J]
    with np.errstate(all="ignore"):
        seen = (kp[:, 0, :, 2] >= min_score) & (kp[:, 1, :, 2] >= min_score) & np.isfinite(kp[:, :, :, :2]).all(axis=(1, 3))
        pix = [np.stack([a[e, 0] * kp[:, e, :, 0] + a[e, 1], a[e, 2] * kp[:, e, :, 1] + a[e, 3]], axis=-1) for e in range(2)]
        dL, r = ocam_cam2world_ref(pix[0], left), ocam_cam2world_ref(pix[1], right)
        dR = np.stack([R[k, 0] * r[..., 0] + R[k, 1] * r[..., 1] + R[k, 2] * r[..., 2] for k in range(3)], axis=-1)
        w0 = -t

        def dot(p, q):
            return p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]
        b, d, e = dot(dL, dR), dot(dL, w0[None, None]), dot(dR, w0[None, None])
        den = 1.0 - b * b
        s, u = (b * e - d) / den, (e - b * d) / den
        PL, PR = s[..., None] * dL, t + u[..., None] * dR
        X = (PL + PR) * 0.5
        df = PL - PR
        gap = np.sqrt(df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1] + df[..., 2] * df[..., 2])
        valid = seen & (den > 0) & (s > 0) & (u > 0) & np.isfinite(X).all(axis=-1) & np.isfinite(gap) & np.isfinite(den) & np.isfinite(s) & np.isfinite(u)
        if ps is not None:
            valid = valid & np.isfinite(ps).all(axis=-1)                                     # "everything finite": the joint's pose row too
        n = np.zeros(B)
        sx, sp = np.zeros((B, 3)), np.zeros((B, 3))
        for j in range(J):                                                                   # ascending joint order, as the kernel adds
            on = valid[:, j]
            n = n + on
            sx = np.where(on[:, None], sx + X[:, j], sx)
            if ps is not None:
                sp = np.where(on[:, None], sp + ps[:, j], sp)
        nn = np.where(n > 0, n, 1.0)
        that = np.zeros((B, 3)) if ps is None else sx / nn[:, None] - sp / nn[:, None]
        dis = np.zeros((B, J))
        if ps is not None:
            q = X - ps - that[:, None]
            dis = np.sqrt(q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1] + q[..., 2] * q[..., 2])
        s2d, s2g, mxd, mxg = np.zeros(B), np.zeros(B), np.zeros(B), np.zeros(B)
        for j in range(J):
            on = valid[:, j]
            s2d = np.where(on, s2d + dis[:, j] * dis[:, j], s2d)
            s2g = np.where(on, s2g + gap[:, j] * gap[:, j], s2g)
            mxd = np.where(on & (dis[:, j] > mxd), dis[:, j], mxd)
            mxg = np.where(on & (gap[:, j] > mxg), gap[:, j], mxg)
        rec = np.stack([X[..., 0], X[..., 1], X[..., 2], gap, den, s, dis, np.ones((B, J))], axis=-1)
        rec = np.where(valid[..., None], rec, 0.0)
        frame = np.stack([that[:, 0], that[:, 1], that[:, 2], n, np.sqrt(s2d / nn), mxd, np.sqrt(s2g / nn), mxg], axis=-1)
        frame = np.where((n > 0)[:, None], frame, 0.0)
    return rec.astype(dtype), frame.astype(dtype)


# ---- the lifted joints fused with the keypoint rays (egotap.h: egotap_stereo_fuse) ----------------------------------------------------------
FUSE_PRIOR, FUSE_USED, FUSE_GATED, FUSE_NOT_IN_FRONT, FUSE_FALLBACK = 1, (2, 4), (8, 16), (32, 64), 128      # the mode bits; pairs: (left, right)


@dataclass(frozen=True)
class FuseParams:
    """egotap.h egotap_fuse_params.  ``sigma_prior``: the standard deviation of a lifted joint, in the pose's units -- it carries a unit, the project
    knows no dataset's, so it has no default.  ``sigma_ray``: the angular standard deviation of a keypoint's ray in radians; 0.02 is about a third of a
    heatmap pixel on a 64-pixel map across a 180 degree lens.  ``max_sigma``: the gate in standard deviations, before and after the fit (+inf: none).
    ``min_joints``: fewest triangulated joints behind a t_hat that places a prior, as the tracker's.  Nobody has tuned any of these on real data."""
    sigma_prior: float
    sigma_ray: float = 0.02
    max_sigma: float = 3.0
    min_joints: int = 3

    def __post_init__(self):
        for name in ("sigma_prior", "sigma_ray"):
            v = float(getattr(self, name))
            if not (math.isfinite(v) and v > 0):
                raise ValueError(f"FuseParams: {name} must be finite and > 0, got {v}")
            object.__setattr__(self, name, v)
        v = float(self.max_sigma)
        if not v >= 0:
            raise ValueError(f"FuseParams: max_sigma must be >= 0 (+inf: no gate), got {v}")
        object.__setattr__(self, "max_sigma", v)
        n = int(self.min_joints)
        if n < 0:
            raise ValueError(f"FuseParams: min_joints must not be negative, got {n}")
        object.__setattr__(self, "min_joints", n)


def stereo_fuse_ref(keypoints, pose, frame, left: OcamModel, right: OcamModel, t, params: FuseParams, R=None, affine=None, min_score=STEREO_MIN_SCORE,
                    pose_row0=0, dtype="float32"):
    """The records egotap_stereo_fuse writes, restated in float64 numpy operation for operation (egotap.h holds the definition and its order):
    keypoints [B, 2, J, 4], pose [B, P, 3], frame [B, 8] (the triangulation's; t_hat and n are read) -> (pose_fused [B, P, 3], fused [B, J, 8] =
    (x, y, z, move, res left, res right, share, mode), stats [B, 8] = (priors, kept fits of both eyes, kept fits of one eye, eyes rejected, rms move,
    max move, rms res, max res)).  The rig arguments are ``stereo_triangulate_ref``'s.  pose_fused is float32 whatever ``dtype``: its untouched rows are
    the input's bits.  ``dtype="float64"``: fused and stats before their one rounding."""
    import numpy as np
    kp = np.asarray(keypoints, dtype=np.float64)
    if kp.ndim != 4 or kp.shape[1] != 2 or kp.shape[3] != 4:
        raise ValueError(f"stereo_fuse_ref: keypoints are [B, 2, J, 4], got {kp.shape}")
    B, _, J, _ = kp.shape
    if not 1 <= J <= STEREO_MAX_JOINTS:
        raise ValueError(f"stereo_fuse_ref: 1 .. {STEREO_MAX_JOINTS} joints, got {J}")
    if not isinstance(params, FuseParams):
        raise ValueError("stereo_fuse_ref: params is a spec.FuseParams (sigma_prior has no default)")
    p32 = np.ascontiguousarray(np.asarray(pose), dtype=np.float32)
    if p32.ndim != 3 or p32.shape[0] != B or p32.shape[2] != 3 or pose_row0 < 0 or pose_row0 + J > p32.shape[1]:
        raise ValueError(f"stereo_fuse_ref: pose is [B, P, 3] with pose_row0 + J <= P, got {p32.shape}, pose_row0 = {pose_row0}, J = {J}")
    fr = np.asarray(frame, dtype=np.float32).astype(np.float64)
    if fr.shape != (B, 8):
        raise ValueError(f"stereo_fuse_ref: frame is [B, 8] = {(B, 8)}, got {fr.shape}")
    t = np.asarray(t, dtype=np.float64).reshape(3)
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
    af = np.asarray(STEREO_IDENTITY_AFFINE if affine is None else affine, dtype=np.float64).reshape(2, 4)
    s_ray, s_pri, max_sigma = params.sigma_ray, params.sigma_prior, params.max_sigma

    def dot(p, q):
        return p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]

    with np.errstate(all="ignore"):
        that = fr[:, None, :3]
        root_ok = (fr[:, 3] >= params.min_joints) & np.isfinite(fr[:, :3]).all(axis=-1)
        q = p32[:, pose_row0:pose_row0 + J].astype(np.float64)
        prior = root_ok[:, None] & np.isfinite(q).all(axis=-1)
        x0 = q + that
        wp = 1.0 / (s_pri * s_pri)
        pix = [np.stack([af[e, 0] * kp[:, e, :, 0] + af[e, 1], af[e, 2] * kp[:, e, :, 1] + af[e, 3]], axis=-1) for e in range(2)]
        dL, r = ocam_cam2world_ref(pix[0], left), ocam_cam2world_ref(pix[1], right)
        dR = np.stack([R[k, 0] * r[..., 0] + R[k, 1] * r[..., 1] + R[k, 2] * r[..., 2] for k in range(3)], axis=-1)
        mode = np.where(prior, FUSE_PRIOR, 0)
        eyes = []
        for e, (d, o) in enumerate(((dL, np.zeros(3)), (dR, t))):
            score = kp[:, e, :, 2]
            seen = prior & (score >= min_score) & np.isfinite(kp[:, e, :, :2]).all(axis=-1)
            y0 = x0 - o
            a, rho = dot(d, y0), np.sqrt(dot(y0, y0))
            rr = y0 - a[..., None] * d
            sr = s_ray * rho
            sr2 = sr * sr
            g = np.sqrt(dot(rr, rr)) / np.sqrt(sr2 + s_pri * s_pri)
            front = (a > 0) & np.isfinite(g)
            used = seen & front & (g <= max_sigma)
            mode = mode + np.where(seen & ~front, FUSE_NOT_IN_FRONT[e], 0) + np.where(seen & front & ~(g <= max_sigma), FUSE_GATED[e], 0) + np.where(used, FUSE_USED[e], 0)
            eyes.append((used, d, o, score / sr2, sr))
        # the system: the upper triangle (A00, A01, A02, A11, A12, A22), left before right; the left origin is 0 and adds nothing to b
        zero = np.zeros((B, J))
        A = [zero + wp, zero, zero, zero + wp, zero, zero + wp]
        b = [wp * x0[..., k] for k in range(3)]
        sw = zero
        for e, (used, d, o, w, sr) in enumerate(eyes):
            m00, m01, m02 = 1.0 - d[..., 0] * d[..., 0], -(d[..., 0] * d[..., 1]), -(d[..., 0] * d[..., 2])
            m11, m12, m22 = 1.0 - d[..., 1] * d[..., 1], -(d[..., 1] * d[..., 2]), 1.0 - d[..., 2] * d[..., 2]
            A = [np.where(used, Ak + w * m, Ak) for Ak, m in zip(A, (m00, m01, m02, m11, m12, m22))]
            if e == 1:
                c = [(m00 * o[0] + m01 * o[1]) + m02 * o[2], (m01 * o[0] + m11 * o[1]) + m12 * o[2], (m02 * o[0] + m12 * o[1]) + m22 * o[2]]
                b = [np.where(used, bk + w * ck, bk) for bk, ck in zip(b, c)]
            sw = np.where(used, sw + w, sw)
        l10, l20 = A[1] / A[0], A[2] / A[0]
        D1, c21 = A[3] - l10 * A[1], A[4] - l20 * A[1]
        l21 = c21 / D1
        D2 = (A[5] - l20 * A[2]) - l21 * c21
        z1 = b[1] - l10 * b[0]
        z2 = (b[2] - l20 * b[0]) - l21 * z1
        y0, y1, y2 = b[0] / A[0], z1 / D1, z2 / D2
        x2 = y2
        x1 = y1 - l21 * x2
        xs = np.stack([(y0 - l10 * x1) - l20 * x2, x1, x2], axis=-1)
        tried = eyes[0][0] | eyes[1][0]
        keep = tried & np.isfinite(xs).all(axis=-1)
        res = []
        for used, d, o, w, sr in eyes:
            v = xs - o
            c = dot(v, d)
            pp = v - c[..., None] * d
            rs = np.sqrt(dot(pp, pp)) / sr
            keep = keep & (~used | ((rs <= max_sigma) & (c > 0)))
            res.append(np.where(used & np.isfinite(rs), rs, 0.0))
        mode = mode + np.where(tried & ~keep, FUSE_FALLBACK, 0)
        x = np.where(keep[..., None], xs, x0)
        dx = xs - x0
        move = np.where(keep, np.sqrt(dot(dx, dx)), 0.0)
        share = np.where(keep, sw / (wp + sw), 0.0)
        rec = np.stack([x[..., 0], x[..., 1], x[..., 2], move, res[0], res[1], share, mode.astype(np.float64)], axis=-1)
        rec = np.where(prior[..., None], rec, 0.0)
        pose_fused = p32.copy()
        rows = pose_fused[:, pose_row0:pose_row0 + J]
        rows[keep] = (xs - that)[keep].astype(np.float32)
        # the frame's statistics: ascending joint order, left before right
        n_prior, n_both, n_one, n_rej, n_res = (np.zeros(B) for _ in range(5))
        s2m, mxm, s2r, mxr = (np.zeros(B) for _ in range(4))
        for j in range(J):
            on, kj = prior[:, j], keep[:, j]
            uL, uR = eyes[0][0][:, j], eyes[1][0][:, j]
            n_prior = n_prior + on
            s2m = np.where(on, s2m + move[:, j] * move[:, j], s2m)
            mxm = np.where(on & (move[:, j] > mxm), move[:, j], mxm)
            rejected = sum(((mode[:, j] & bit) != 0).astype(np.float64) for bit in FUSE_GATED + FUSE_NOT_IN_FRONT)
            n_rej = n_rej + rejected + np.where(on & ~kj, uL.astype(np.float64) + uR, 0.0)
            n_both = n_both + (kj & uL & uR)
            n_one = n_one + (kj & (uL ^ uR))
            for u, rs in ((uL, res[0][:, j]), (uR, res[1][:, j])):
                inc = kj & u
                n_res = n_res + inc
                s2r = np.where(inc, s2r + rs * rs, s2r)
                mxr = np.where(inc & (rs > mxr), rs, mxr)
        some, some_res = n_prior > 0, n_res > 0
        stats = np.stack([n_prior, n_both, n_one, n_rej, np.where(some, np.sqrt(s2m / np.where(some, n_prior, 1.0)), 0.0), mxm,
                          np.where(some_res, np.sqrt(s2r / np.where(some_res, n_res, 1.0)), 0.0), mxr], axis=-1)
    return pose_fused, rec.astype(dtype), stats.astype(dtype)


# ---- a camera rig per stream (egotap.h: egotap_stereo_rig, egotap_stereo_triangulate_streams / egotap_stereo_fuse_streams) ---------------------
STEREO_MAX_STREAMS = 4096                      # egotap.h EGOTAP_MAX_STREAM_RIGS


@dataclass(frozen=True, eq=False)
class StereoRig:
    """One stream's camera rig, the arguments ``stereo_triangulate_ref`` takes about a rig: the two ``OcamModel``, ``t`` (3) and ``R`` (3 x 3, None:
    identity) the right camera's origin and axes in the left camera's frame, ``affine`` [2, 4] from keypoint units to the calibration's pixels (None:
    identity) and ``min_score``.  A table of rigs (egotap.h egotap_stereo_rig) is a list of these, stream s first to last."""
    left: OcamModel
    right: OcamModel
    t: tuple
    R: object = None
    affine: object = None
    min_score: float = STEREO_MIN_SCORE

    def __post_init__(self):
        for side in ("left", "right"):
            if not isinstance(getattr(self, side), OcamModel):
                raise ValueError(f"StereoRig: {side} is a spec.OcamModel, got {type(getattr(self, side)).__name__}")
        t = tuple(float(v) for v in self.t)
        if len(t) != 3:
            raise ValueError(f"StereoRig: t is the right camera's origin in the left frame, 3 values, got {len(t)}")
        object.__setattr__(self, "t", t)
        if self.R is not None:
            R = tuple(tuple(float(v) for v in row) for row in self.R)
            if len(R) != 3 or any(len(row) != 3 for row in R):
                raise ValueError("StereoRig: R is 3 x 3")
            object.__setattr__(self, "R", R)
        if self.affine is not None:
            a = tuple(tuple(float(v) for v in row) for row in self.affine)
            if len(a) != 2 or any(len(row) != 4 for row in a):
                raise ValueError("StereoRig: affine is [2, 4] = (ax, bx, ay, by) per eye")
            object.__setattr__(self, "affine", a)
        object.__setattr__(self, "min_score", float(self.min_score))


def _stream_rigs(who, rigs, B):
    rigs = list(rigs)
    if not 1 <= len(rigs) <= STEREO_MAX_STREAMS or not all(isinstance(r, StereoRig) for r in rigs):
        raise ValueError(f"{who}: rigs is a list of 1 .. {STEREO_MAX_STREAMS} spec.StereoRig, one per stream")
    if B % len(rigs):
        raise ValueError(f"{who}: the batch must be a multiple of the number of streams (frame b uses rig b % S), got B = {B}, S = {len(rigs)}")
    return rigs


def stereo_triangulate_streams_ref(keypoints, rigs, pose=None, pose_row0=0, dtype="float32"):
    """The records egotap_stereo_triangulate_streams writes: ``stereo_triangulate_ref`` on rows s, s + S, .. of a time-major batch (frame b = t * S + s)
    with rig s of ``rigs`` (a list of S ``StereoRig``).  No arithmetic of its own."""
    import numpy as np
    kp = np.asarray(keypoints)
    rigs = _stream_rigs("stereo_triangulate_streams_ref", rigs, kp.shape[0])
    S = len(rigs)
    ps = None if pose is None else np.asarray(pose)
    rec = frame = None
    for s, g in enumerate(rigs):
        r, f = stereo_triangulate_ref(kp[s::S], g.left, g.right, g.t, R=g.R, affine=g.affine, min_score=g.min_score, pose=None if ps is None else ps[s::S],
                                      pose_row0=pose_row0, dtype=dtype)
        if rec is None:
            rec, frame = np.empty((kp.shape[0],) + r.shape[1:], dtype=r.dtype), np.empty((kp.shape[0],) + f.shape[1:], dtype=f.dtype)
        rec[s::S], frame[s::S] = r, f
    return rec, frame


def stereo_fuse_streams_ref(keypoints, pose, frame, rigs, params: FuseParams, pose_row0=0, dtype="float32"):
    """The records egotap_stereo_fuse_streams writes: ``stereo_fuse_ref`` on rows s, s + S, .. with rig s of ``rigs``; one ``params`` for all streams.
    No arithmetic of its own."""
    import numpy as np
    kp, ps, fr = np.asarray(keypoints), np.asarray(pose), np.asarray(frame)
    rigs = _stream_rigs("stereo_fuse_streams_ref", rigs, kp.shape[0])
    S = len(rigs)
    out = None
    for s, g in enumerate(rigs):
        part = stereo_fuse_ref(kp[s::S], ps[s::S], fr[s::S], g.left, g.right, g.t, params, R=g.R, affine=g.affine, min_score=g.min_score, pose_row0=pose_row0,
                               dtype=dtype)
        if out is None:
            out = tuple(np.empty((kp.shape[0],) + a.shape[1:], dtype=a.dtype) for a in part)
        for whole, a in zip(out, part):
            whole[s::S] = a
    return out


# ---- frames from another lens -> the model camera's frame (egotap.h: egotap_lens_remap / egotap_predict_pose_lens) -----------------------
LENS_FRAC_BITS = 11                            # a map entry is a sensor pixel coordinate in Q11: the resize's weight precision
LENS_MAX_SIDE = 16384                          # H, W <= 16384, as for the resize: an entry stays below 2^25
LENS_INVALID = -1                              # both halves of an entry whose output pixel has no source: the kernel writes the fill bytes


@dataclass(frozen=True, eq=False)
class LensMap:
    """One eye's lens map (``lens_map`` builds it): ``taps`` int32 [S0, S0, 2], entry (Y, X) = (fx, fy), the Q11 pixel coordinates in the H x W
    sensor frame that output pixel (X, Y) of the S0 x S0 frame the stems read is sampled at, or (-1, -1) where it has none.  ``model_size`` is
    (h, w) of the model camera's calibration image -- the units keypoints come back in -- and ``mirror`` whether output column X shows the model
    camera's column S0 - 1 - X.  The array is read-only: a map is uploaded once and reused for every frame of the rig."""
    taps: object
    S0: int
    H: int
    W: int
    model_size: tuple
    mirror: bool = False

    def __post_init__(self):
        import numpy as np
        S0, H, W = int(self.S0), int(self.H), int(self.W)
        if S0 < 1 or not (1 <= H <= LENS_MAX_SIDE and 1 <= W <= LENS_MAX_SIDE):
            raise ValueError(f"LensMap: S0 must be positive and the frame height and width between 1 and {LENS_MAX_SIDE}, got S0 = {S0}, {H} x {W}")
        t = np.asarray(self.taps)
        if t.dtype != np.int32 or t.shape != (S0, S0, 2):
            raise ValueError(f"LensMap: taps are int32 [{S0}, {S0}, 2], got {t.dtype} {t.shape}")
        t = np.ascontiguousarray(t).copy()
        ok = t[..., 0] >= 0
        if np.any((t[..., 1] >= 0) != ok) or np.any(t[~ok] != LENS_INVALID):
            raise ValueError("LensMap: an entry is valid in both halves or (-1, -1)")
        if np.any(t[..., 0][ok] > (W - 1) << LENS_FRAC_BITS) or np.any(t[..., 1][ok] > (H - 1) << LENS_FRAC_BITS):
            raise ValueError(f"LensMap: an entry lies outside the {H} x {W} frame")
        t.setflags(write=False)
        size = tuple(int(v) for v in self.model_size)
        if len(size) != 2 or min(size) < 1:
            raise ValueError(f"LensMap: model_size is (h, w) of the model camera's calibration image, got {self.model_size}")
        for k, v in (("taps", t), ("S0", S0), ("H", H), ("W", W), ("model_size", size), ("mirror", bool(self.mirror))):
            object.__setattr__(self, k, v)

    @property
    def valid(self):
        """bool [S0, S0]: the output pixels that have a source"""
        return self.taps[..., 0] >= 0


def _lens_frame_size(who, sensor: OcamModel, frame_size):
    H, W = (int(v) for v in (sensor.size if frame_size is None else frame_size))
    if not (1 <= H <= LENS_MAX_SIDE and 1 <= W <= LENS_MAX_SIDE):
        raise ValueError(f"{who}: the frame height and width must be between 1 and {LENS_MAX_SIDE}, got {H} x {W}")
    return H, W


def _lens_chain(uv, model: OcamModel, sensor: OcamModel, R, frame):
    """model-camera calibration pixels [..., 2] -> (pixels of the sensor's H x W frame, pixels of the sensor's calibration image), float64"""
    import numpy as np
    ray = ocam_cam2world_ref(uv, model)
    if R is not None:
        R = np.asarray(R, dtype=np.float64)
        if R.shape != (3, 3):
            raise ValueError(f"lens map: R is 3 x 3 (the model camera's axes in the sensor camera's frame), got {R.shape}")
        with np.errstate(all="ignore"):
            ray = ray @ R.T
    cal = ocam_world2cam_ref(ray, sensor)
    H, W = frame
    with np.errstate(all="ignore"):
        xs = cal[..., 0] if W == sensor.size[1] else (cal[..., 0] + 0.5) * (W / sensor.size[1]) - 0.5
        ys = cal[..., 1] if H == sensor.size[0] else (cal[..., 1] + 0.5) * (H / sensor.size[0]) - 0.5
    return np.stack([xs, ys], axis=-1), cal


def lens_map(model: OcamModel, sensor: OcamModel, S0: int, R=None, frame_size=None, mirror: bool = False) -> LensMap:
    """The lens map of one eye, in float64 numpy on the host, once per rig: where in the SENSOR's frame each pixel of the S0 x S0 frame the stems
    read is sampled, so that the stems see what the MODEL camera (the lens the estimators were trained on) would have seen.

    For output pixel (X, Y), with X' = S0 - 1 - X if ``mirror`` else X:
        u = (X' + 0.5) * model.size[1] / S0 - 0.5,  v = (Y + 0.5) * model.size[0] / S0 - 0.5      (calibration pixel, align_corners=False)
        ray = ocam_cam2world_ref((u, v), model);  ray_s = R @ ray  (R 3 x 3: the model camera's axes in the sensor camera's frame; None: identity)
        (xs, ys) = ocam_world2cam_ref(ray_s, sensor)
    ``frame_size`` = (H, W) of the frames the sensor delivers, by default ``sensor.size``; another size scales the calibration pixels per axis by
    (p + 0.5) * ratio - 0.5.  The entry is valid when xs, ys are finite, 0 <= xs <= W - 1 and 0 <= ys <= H - 1, and -- for a model with
    ``radius`` > 0 -- (u, v) lies inside the model's image circle and the sensor's calibration pixel inside the sensor's.  THE IMAGE CIRCLES ARE
    THE ONLY GUARD against a polynomial that extrapolates outside its field of view: a calibration with radius 0 is believed wherever its
    polynomial lands inside the frame.  A valid entry is (floor(xs * 2048 + 0.5), floor(ys * 2048 + 0.5)) (Q11, below 2^25), an invalid one
    (-1, -1)."""
    import numpy as np
    S0 = int(S0)
    if S0 < 1:
        raise ValueError(f"lens_map: the output side must be positive, got {S0}")
    H, W = _lens_frame_size("lens_map", sensor, frame_size)
    X, Y = np.meshgrid(np.arange(S0, dtype=np.float64), np.arange(S0, dtype=np.float64))
    if mirror:
        X = S0 - 1 - X
    u = (X + 0.5) * (model.size[1] / S0) - 0.5
    v = (Y + 0.5) * (model.size[0] / S0) - 0.5
    pix, cal = _lens_chain(np.stack([u, v], axis=-1), model, sensor, R, (H, W))
    xs, ys = pix[..., 0], pix[..., 1]
    with np.errstate(all="ignore"):
        ok = np.isfinite(xs) & np.isfinite(ys) & (xs >= 0) & (xs <= W - 1) & (ys >= 0) & (ys <= H - 1)
        if model.radius > 0:
            ok &= np.hypot(u - model.xc, v - model.yc) <= model.radius
        if sensor.radius > 0:
            ok &= np.hypot(cal[..., 0] - sensor.xc, cal[..., 1] - sensor.yc) <= sensor.radius
    one = float(1 << LENS_FRAC_BITS)
    taps = np.stack([np.floor(np.where(ok, xs, 0.0) * one + 0.5), np.floor(np.where(ok, ys, 0.0) * one + 0.5)], axis=-1).astype(np.int32)
    taps[~ok] = LENS_INVALID
    return LensMap(taps, S0, H, W, tuple(model.size), bool(mirror))


def lens_map_points(points_xy, model: OcamModel, sensor: OcamModel, R=None, frame_size=None):
    """Model-camera calibration pixels [..., 2] -> pixels of the sensor's frame, float64, through the chain of ``lens_map`` (no validity test:
    a point outside either lens comes back wherever the polynomials put it, or NaN).  For drawing the keypoints a lens entry returns -- they are
    in the model camera's calibration pixels -- over the frame the sensor delivered.  Host only."""
    import numpy as np
    q = np.array(points_xy, dtype=np.float64)
    if q.shape[-1] != 2:
        raise ValueError(f"lens_map_points: points are [..., 2], got {q.shape}")
    return _lens_chain(q, model, sensor, R, _lens_frame_size("lens_map_points", sensor, frame_size))[0]


def lens_taps(lens: LensMap):
    """The integer taps the kernel derives from a map: int64 numpy arrays (valid, ix0, ix1, wx1, iy0, iy1, wy1), each [S0, S0]:
    ix0 = fx >> 11, wx1 = fx & 2047, ix1 = min(ix0 + 1, W - 1), likewise in y; zeros where the entry is invalid."""
    import numpy as np
    ok = lens.valid
    fx, fy = (np.where(ok, lens.taps[..., k], 0).astype(np.int64) for k in (0, 1))
    mask = (1 << LENS_FRAC_BITS) - 1
    ix0, iy0 = fx >> LENS_FRAC_BITS, fy >> LENS_FRAC_BITS
    return ok, ix0, np.minimum(ix0 + 1, lens.W - 1), fx & mask, iy0, np.minimum(iy0 + 1, lens.H - 1), fy & mask


def lens_remap_u8(frames, lens: LensMap, fill=(0, 0, 0)):
    """The whole remap, restated in integers on the host: frames uint8 [n, H, W, 3] (numpy array or torch tensor on any device) of the map's H x W
    -> uint8 [n, S0, S0, 3] of the same kind.  With the taps of ``lens_taps`` and wx0 = 2048 - wx1, wy0 = 2048 - wy1:

        out = (wy0 (wx0 p[iy0][ix0] + wx1 p[iy0][ix1]) + wy1 (wx0 p[iy1][ix0] + wx1 p[iy1][ix1]) + 2^21) >> 22        (``resize_u8``'s formula)

    and the ``fill`` bytes (R, G, B) where the entry is invalid.  This is what lens_remap_kernel computes, bit for bit.  For an NV12 / YUYV source
    the definition is ``lens_remap_u8(yuv_to_rgb_u8(frames, layout, colour), lens)``: nothing is interpolated in YUV."""
    import numpy as np
    import torch
    if not isinstance(lens, LensMap):
        raise ValueError(f"lens_remap_u8: the map is a spec.LensMap, got {type(lens).__name__}")
    is_np = isinstance(frames, np.ndarray)
    x = torch.from_numpy(frames) if is_np else frames
    if x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise ValueError(f"lens_remap_u8: frames are uint8 [n, H, W, 3], got {x.dtype} {tuple(x.shape)}")
    if (int(x.shape[1]), int(x.shape[2])) != (lens.H, lens.W):
        raise ValueError(f"lens_remap_u8: the map was built for {lens.H} x {lens.W} frames, got {int(x.shape[1])} x {int(x.shape[2])} "
                         "(build it with frame_size=(H, W))")
    fill = tuple(int(v) for v in fill)
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"lens_remap_u8: fill is three bytes (R, G, B), got {fill}")
    dev = x.device
    ok, ix0, ix1, wx1, iy0, iy1, wy1 = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in lens_taps(lens))
    wx1, wy1 = wx1.view(1, lens.S0, lens.S0, 1), wy1.view(1, lens.S0, lens.S0, 1)
    wx0, wy0 = RESIZE_WEIGHT_ONE - wx1, RESIZE_WEIGHT_ONE - wy1
    top = wx0 * x[:, iy0, ix0].to(torch.int64) + wx1 * x[:, iy0, ix1].to(torch.int64)
    bot = wx0 * x[:, iy1, ix0].to(torch.int64) + wx1 * x[:, iy1, ix1].to(torch.int64)
    out = ((wy0 * top + wy1 * bot + (1 << 21)) >> 22).to(torch.uint8)
    out = torch.where(ok.view(1, lens.S0, lens.S0, 1), out, torch.tensor(fill, dtype=torch.uint8, device=dev).view(1, 1, 1, 3))
    return out.numpy() if is_np else out


def lens_remap_streams_u8(frames, lenses, fill=(0, 0, 0)):
    """The remap of egotap_lens_remap_streams: ``lens_remap_u8`` on frames s, s + S, .. of a time-major batch with map s of ``lenses`` (one eye's S
    ``LensMap``, all of one S0 and frame size).  No arithmetic of its own; S = 1 is ``lens_remap_u8``."""
    import numpy as np
    lenses = list(lenses)
    if not lenses or not all(isinstance(m, LensMap) for m in lenses):
        raise ValueError("lens_remap_streams_u8: lenses is a list of spec.LensMap, one per stream")
    if len({(m.S0, m.H, m.W) for m in lenses}) != 1:
        raise ValueError("lens_remap_streams_u8: every stream's map must have one S0 and one frame size")
    S, n = len(lenses), int(frames.shape[0])
    if n % S:
        raise ValueError(f"lens_remap_streams_u8: the batch must be a multiple of the number of streams (frame b uses map b % S), got {n} frames, S = {S}")
    parts = [lens_remap_u8(frames[s::S], m, fill) for s, m in enumerate(lenses)]
    if isinstance(frames, np.ndarray):
        out = np.empty((n,) + parts[0].shape[1:], dtype=np.uint8)
    else:
        out = frames.new_empty((n,) + tuple(parts[0].shape[1:]))
    for s, a in enumerate(parts):
        out[s::S] = a
    return out


# ---- the pose, the root and the stereo joints filtered over time (egotap.h: egotap_pose_track) ---------------------------------------------
POSE_TRACK_STATE = 12                          # per track: x^ (3), v^ (3), m_prev (3), gap_t, age, live
POSE_TRACK_MAX_ROWS = 64                       # P and J: one lane each
TRACK_CLASSES = ("pose", "root", "joints")
TWO_PI = 6.283185307179586


@dataclass(frozen=True)
class TrackParams:
    """egotap.h egotap_track_params.  ``pose`` / ``root`` / ``joints``: (min_cutoff [Hz], beta [1 / (pose unit / s)], d_cutoff [Hz]) of the One-Euro
    filter per class of track -- 1.0, 0.007, 1.0 are the paper's starting values (Casiez et al. 2012).  ``max_disagree`` / ``max_gap``: the frame's rms
    disagree / rms gap above which the triangulation's t_hat is not accepted; ``max_joint_gap``: a joint's gap above which it is not; +inf: off.
    ``min_joints``: fewest triangulated joints behind an accepted t_hat (below 3 it is a mean of one or two points); ``max_hold``: most consecutive
    steps a track is held without an accepted sample before it is forgotten.  Nobody has tuned any of these on real data: there is no dataset here."""
    pose: tuple = (1.0, 0.007, 1.0)
    root: tuple = (1.0, 0.007, 1.0)
    joints: tuple = (1.0, 0.007, 1.0)
    max_disagree: float = math.inf
    max_gap: float = math.inf
    max_joint_gap: float = math.inf
    min_joints: int = 3
    max_hold: int = 8

    def __post_init__(self):
        for name in TRACK_CLASSES:
            c = tuple(float(v) for v in getattr(self, name))
            if len(c) != 3:
                raise ValueError(f"TrackParams: {name} is (min_cutoff, beta, d_cutoff), got {len(c)} values")
            if not (math.isfinite(c[0]) and c[0] > 0 and math.isfinite(c[2]) and c[2] > 0):
                raise ValueError(f"TrackParams: {name}: min_cutoff and d_cutoff must be finite and > 0, got {c[0]}, {c[2]}")
            if not (math.isfinite(c[1]) and c[1] >= 0):
                raise ValueError(f"TrackParams: {name}: beta must be finite and >= 0, got {c[1]}")
            object.__setattr__(self, name, c)
        for name in ("max_disagree", "max_gap", "max_joint_gap"):
            v = float(getattr(self, name))
            if not v >= 0:
                raise ValueError(f"TrackParams: {name} must be >= 0 (+inf: off), got {v}")
            object.__setattr__(self, name, v)
        for name in ("min_joints", "max_hold"):
            v = int(getattr(self, name))
            if v < 0:
                raise ValueError(f"TrackParams: {name} must not be negative, got {v}")
            object.__setattr__(self, name, v)

    @classmethod
    def uniform(cls, min_cutoff=1.0, beta=0.007, d_cutoff=1.0, **rest):
        """the same filter for the three classes"""
        c = (min_cutoff, beta, d_cutoff)
        return cls(pose=c, root=c, joints=c, **rest)


def _track_inputs(who, pose, state, dt_or_dts, params, frame, joints3d, streams):
    """the arguments of pose_track_ref / pose_track_world_ref read and checked -> (prm, S, T, P, J, state copy, dts [T], meas [T, S, K, 3], acc [T, S, K]):
    the camera-frame measurement of every track and whether it is accepted (finite, valid, the gates)"""
    import numpy as np
    prm = TrackParams() if params is None else params
    ps = np.asarray(pose, dtype=np.float64)
    S = int(streams)
    if ps.ndim != 3 or ps.shape[2] != 3 or S < 1 or ps.shape[0] < S or ps.shape[0] % S:
        raise ValueError(f"{who}: pose is [T * streams, P, 3] with T >= 1, got {ps.shape} for {S} streams")
    B, P, _ = ps.shape
    T = B // S
    J = 0
    j3 = None
    if joints3d is not None:
        j3 = np.asarray(joints3d, dtype=np.float64)
        if j3.ndim != 3 or j3.shape[0] != B or j3.shape[2] != 8 or j3.shape[1] < 1:
            raise ValueError(f"{who}: joints3d is [T * streams, J, 8] with J >= 1, got {j3.shape} for {B} frames")
        J = j3.shape[1]
    if not (1 <= P <= POSE_TRACK_MAX_ROWS and J <= POSE_TRACK_MAX_ROWS):
        raise ValueError(f"{who}: at most {POSE_TRACK_MAX_ROWS} pose rows and joints, got P = {P}, J = {J}")
    fr = None
    if frame is not None:
        fr = np.asarray(frame, dtype=np.float64)
        if fr.shape != (B, 8):
            raise ValueError(f"{who}: frame is [T * streams, 8], got {fr.shape} for {B} frames")
    K = P + 1 + J
    st = np.array(state, dtype=np.float64)
    if st.shape != (S, K, POSE_TRACK_STATE):
        raise ValueError(f"{who}: state is [streams, P + 1 + J, {POSE_TRACK_STATE}] = {(S, K, POSE_TRACK_STATE)}, got {st.shape}")
    if np.ndim(dt_or_dts) == 0:
        if not (math.isfinite(float(dt_or_dts)) and float(dt_or_dts) > 0):
            raise ValueError(f"{who}: dt must be finite and > 0, got {dt_or_dts}")
        dts = np.full(T, float(dt_or_dts))
    else:
        dts = np.asarray(dt_or_dts, dtype=np.float32).astype(np.float64)
        if dts.shape != (T,):
            raise ValueError(f"{who}: dts holds one value per time step, [{T}], got {dts.shape}")
    meas = np.zeros((T, S, K, 3))
    acc = np.zeros((T, S, K), dtype=bool)
    with np.errstate(all="ignore"):
        meas[:, :, :P] = ps.reshape(T, S, P, 3)
        acc[:, :, :P] = np.isfinite(meas[:, :, :P]).all(axis=-1)
        if fr is not None:
            f = fr.reshape(T, S, 8)
            meas[:, :, P] = f[..., 0:3]
            acc[:, :, P] = (f[..., 3] >= prm.min_joints) & np.isfinite(f[..., 0:3]).all(axis=-1) & (f[..., 4] <= prm.max_disagree) & (f[..., 6] <= prm.max_gap)
        if j3 is not None:
            q = j3.reshape(T, S, J, 8)
            meas[:, :, P + 1:] = q[..., 0:3]
            acc[:, :, P + 1:] = (q[..., 7] == 1) & np.isfinite(q[..., 0:3]).all(axis=-1) & (q[..., 3] <= prm.max_joint_gap)
    return prm, S, T, P, J, st, dts, meas, acc


def _track_run(prm, P, st, dts, meas, acc):
    """the T steps of every track: state [S, K, 12], dts [T], meas [T, S, K, 3] read only where acc [T, S, K] is set -> float64 (tracks [T, S, K, 8],
    placed [T, S, P, 3], with_root [T, S] = the root took part in placed, new_state)"""
    import numpy as np
    T, S, K = acc.shape
    cls = np.empty((K, 3))                                   # (min_cutoff, beta, d_cutoff) per track
    cls[:P], cls[P], cls[P + 1:] = prm.pose, prm.root, prm.joints
    c_min, c_beta, c_d = (cls[None, :, k] for k in range(3))

    def alpha(fc, te):
        r = (TWO_PI * fc) * te
        return r / (r + 1.0)
    x, v, mp = st[..., 0:3].copy(), st[..., 3:6].copy(), st[..., 6:9].copy()
    gap_t, age, live = st[..., 9].copy(), st[..., 10].copy(), st[..., 11] != 0
    tracks = np.zeros((T, S, K, 8))
    placed = np.zeros((T, S, P, 3))
    with_root = np.zeros((T, S), dtype=bool)
    with np.errstate(all="ignore"):
        for t in range(T):
            dt = dts[t]
            ok = bool(np.isfinite(dt) and dt > 0)
            a = acc[t]
            m = np.where(a[..., None], meas[t], 0.0)          # a rejected measurement is never read
            first = ~live & a
            upd = live & a & ok
            miss = live & ~upd
            # live, accepted, ok (computed everywhere, kept where upd)
            te = gap_t + dt
            ad = alpha(c_d, te)
            dx = (m - mp) / te[..., None]
            v_u = v + ad[..., None] * (dx - v)
            speed = np.sqrt(v_u[..., 0] * v_u[..., 0] + v_u[..., 1] * v_u[..., 1] + v_u[..., 2] * v_u[..., 2])
            fc = c_min + c_beta * speed
            ax = alpha(fc, te)
            x_u = x + ax[..., None] * (m - x)
            # live, otherwise
            age_m = age + 1.0
            gap_m = gap_t + dt if ok else gap_t
            expire = miss & (age_m > prm.max_hold)
            hold = miss & ~expire
            x = np.where(first[..., None], m, np.where(upd[..., None], x_u, np.where(expire[..., None], 0.0, x)))
            v = np.where(first[..., None] | expire[..., None], 0.0, np.where(upd[..., None], v_u, v))
            mp = np.where((first | upd)[..., None], m, np.where(expire[..., None], 0.0, mp))
            gap_t = np.where(first | upd | expire, 0.0, np.where(hold, gap_m, gap_t))
            age = np.where(first | upd | expire, 0.0, np.where(hold, age_m, age))
            live = (live | first) & ~expire
            status = np.where(first | upd, 1.0, np.where(hold, 2.0, 0.0))
            cutoff = np.where(first, c_min, np.where(upd, fc, 0.0))
            rec = np.concatenate([x, v, cutoff[..., None], status[..., None]], axis=-1)
            tracks[t] = np.where((status != 0)[..., None], rec, 0.0)
            root_on = status[:, P] != 0
            pl = np.where(root_on[:, None, None], x[:, :P] + x[:, P:P + 1], x[:, :P])
            placed[t] = np.where((status[:, :P] != 0)[..., None], pl, 0.0)
            with_root[t] = root_on
    new_state = np.concatenate([x, v, mp, gap_t[..., None], age[..., None], live[..., None].astype(np.float64)], axis=-1)
    return tracks, placed, with_root, new_state


def pose_track_ref(pose, state, dt_or_dts, params=None, frame=None, joints3d=None, streams=1, dtype="float32"):
    """The records and the state egotap_pose_track writes, restated in float64 numpy, operation for operation: pose [B, P, 3] with B = T * streams
    frames, time-major (frame b = t * streams + s); state [streams, K, 12] float64 with K = P + 1 + J (not modified); ``dt_or_dts`` a positive number for
    every step, or T values (rounded to float32 first: what the device reads); frame [B, 8] / joints3d [B, J, 8] the triangulation's records or None
    -> (tracks [B, K, 8], placed [B, P, 3], new_state [streams, K, 12]).  Per track and step, with measurement m, accept flag a, ok = dt finite and
    > 0, alpha(fc, te) = r / (r + 1), r = (6.283185307179586 fc) te:

        not live, a      x^ = m_prev = m; v^ = 0; gap_t = age = 0; live = 1                                     status 1, cutoff = min_cutoff
        not live, not a                                                                                         status 0, record all zeros
        live, a and ok   te = gap_t + dt; ad = alpha(d_cutoff, te); dx = (m - m_prev) / te; v^ = v^ + ad (dx - v^);
                         speed = sqrt(v^x v^x + v^y v^y + v^z v^z); fc = min_cutoff + beta speed; ax = alpha(fc, te);
                         x^ = x^ + ax (m - x^); m_prev = m; gap_t = age = 0                                     status 1, cutoff = fc
        live, otherwise  age += 1; if ok: gap_t += dt; age > max_hold: the state zeroed                         status 0, record all zeros
                                                       else x^, v^ unchanged                                    status 2, cutoff = 0

    a: a pose row is accepted when finite; the root (frame[:, 0:3]) when the frame is given, n >= min_joints, t_hat finite, rms disagree <=
    max_disagree and rms gap <= max_gap; a joint when valid == 1, X finite and gap <= max_joint_gap (every comparison false on a NaN).
    tracks = (x^, v^, cutoff, status); placed = x^_pose + x^_root (added in float64) while the root's status is 1 or 2, x^_pose alone otherwise, zeros
    for a pose row of status 0.  Each output is rounded once from float64 (``dtype="float64"``: not at all)."""
    prm, S, T, P, J, st, dts, meas, acc = _track_inputs("pose_track_ref", pose, state, dt_or_dts, params, frame, joints3d, streams)
    tracks, placed, _, new_state = _track_run(prm, P, st, dts, meas, acc)
    return tracks.reshape(T * S, -1, 8).astype(dtype), placed.reshape(T * S, P, 3).astype(dtype), new_state


# ---- the same filter in a world frame, from the rig's own pose (egotap.h: egotap_pose_track_world) ---------------------------------------
RIG_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)      # row-major 3 x 4 (R | t)


def rig_pose(t, R=None, quat=None):
    """The 12 values egotap_pose_track_world reads per frame: the row-major 3 x 4 (R | t) of the left camera in the world, x_w = R x_c + t, float64
    [..., 12].  ``t`` [..., 3] in the pose's units; the rotation as ``R`` [..., 3, 3] or as a quaternion ``quat`` [..., 4] = (w, x, y, z), which is
    normalised in float64 (a zero or non-finite norm is refused); neither: no rotation.  Leading dimensions broadcast."""
    import numpy as np
    t = np.asarray(t, dtype=np.float64)
    if t.ndim < 1 or t.shape[-1] != 3:
        raise ValueError(f"rig_pose: t is [..., 3], got {t.shape}")
    if R is not None and quat is not None:
        raise ValueError("rig_pose: give the rotation as R or as quat, not both")
    if quat is not None:
        q = np.asarray(quat, dtype=np.float64)
        if q.ndim < 1 or q.shape[-1] != 4:
            raise ValueError(f"rig_pose: quat is [..., 4] = (w, x, y, z), got {q.shape}")
        with np.errstate(all="ignore"):
            n = np.sqrt((q * q).sum(axis=-1, keepdims=True))
        if not (np.isfinite(n).all() and (n > 0).all()):
            raise ValueError("rig_pose: quat must have a finite, non-zero norm")
        w, x, y, z = np.moveaxis(q / n, -1, 0)
        R = np.stack([np.stack([1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)], axis=-1),
                      np.stack([2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)], axis=-1),
                      np.stack([2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)], axis=-1)], axis=-2)
    elif R is None:
        R = np.eye(3)
    R = np.asarray(R, dtype=np.float64)
    if R.ndim < 2 or R.shape[-2:] != (3, 3):
        raise ValueError(f"rig_pose: R is [..., 3, 3], got {R.shape}")
    lead = np.broadcast_shapes(R.shape[:-2], t.shape[:-1])
    out = np.empty(lead + (3, 4))
    out[..., :3] = R
    out[..., 3] = t
    return out.reshape(lead + (12,))


_rig_pose = rig_pose      # pose_track_world_ref's parameter of that name hides the function inside its body: this name does not


def rig_compose(a, b):
    """``b`` and then ``a``, both [..., 12] as ``rig_pose`` makes them: x -> R_a (R_b x + t_b) + t_a.  "Device in world o left camera in device" is
    rig_compose(device_in_world, camera_in_device)."""
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.ndim < 1 or b.ndim < 1 or a.shape[-1] != 12 or b.shape[-1] != 12:
        raise ValueError(f"rig_compose: two rig poses [..., 12], got {a.shape} and {b.shape}")
    A, Bm = a.reshape(a.shape[:-1] + (3, 4)), b.reshape(b.shape[:-1] + (3, 4))
    R = A[..., :3] @ Bm[..., :3]
    t = (A[..., :3] @ Bm[..., 3:4])[..., 0] + A[..., 3]
    return _rig_pose(t, R=R)


def pose_track_world_ref(pose, state, rig_pose, dt_or_dts, params=None, frame=None, joints3d=None, streams=1, ortho_tol=1e-6, dtype="float32"):
    """The records and the state egotap_pose_track_world writes, restated in float64 numpy, operation for operation.  The arguments of
    ``pose_track_ref`` and ``rig_pose`` [B, 12] float64, per frame the row-major 3 x 4 (R | t) of the left camera in the world
    -> (tracks [B, K, 8], placed_world [B, P, 3], placed_cam [B, P, 3], new_state [streams, K, 12]).

    A frame's rig pose is seen when its 12 values are finite, every |E_ij| <= ortho_tol with E_ij = ((r_i0 r_j0 + r_i1 r_j1) + r_i2 r_j2) - delta_ij,
    and det R = (r00 (r11 r22 - r12 r21) - r01 (r10 r22 - r12 r20)) + r02 (r10 r21 - r11 r20) > 0 (every comparison false on a NaN).  The
    acceptance tests of ``pose_track_ref`` apply to the camera-frame values; an accepted m enters ``pose_track_ref``'s step as
    ((R[r][0] m0 + R[r][1] m1) + R[r][2] m2), plus t[r] for the root and the joints (points; the pose rows are offsets).  A frame whose rig pose is
    not seen accepts no track: a missing sample.  placed_world is ``pose_track_ref``'s placed; placed_cam the same float64 value p back in the frame's
    camera, d = p - t where the root took part and d = p where not, out[c] = ((R[0][c] d0 + R[1][c] d1) + R[2][c] d2), zeros where placed_world is
    zeros and for a frame whose rig pose is not seen."""
    import numpy as np
    who = "pose_track_world_ref"
    prm, S, T, P, J, st, dts, meas, acc = _track_inputs(who, pose, state, dt_or_dts, params, frame, joints3d, streams)
    g = np.asarray(rig_pose, dtype=np.float64)
    if g.shape != (T * S, 12):
        raise ValueError(f"{who}: rig_pose is [T * streams, 12] = {(T * S, 12)}, got {g.shape}")
    tol = float(ortho_tol)
    if not tol >= 0:
        raise ValueError(f"{who}: ortho_tol must be >= 0, got {ortho_tol}")
    g = g.reshape(T, S, 3, 4)
    R, tr = g[..., :3], g[..., 3]
    with np.errstate(all="ignore"):
        seen = np.isfinite(g).all(axis=(-1, -2))
        for i in range(3):
            for j in range(i, 3):
                e = ((R[..., i, 0] * R[..., j, 0] + R[..., i, 1] * R[..., j, 1]) + R[..., i, 2] * R[..., j, 2]) - (1.0 if i == j else 0.0)
                seen &= np.abs(e) <= tol
        c0 = R[..., 1, 1] * R[..., 2, 2] - R[..., 1, 2] * R[..., 2, 1]
        c1 = R[..., 1, 0] * R[..., 2, 2] - R[..., 1, 2] * R[..., 2, 0]
        c2 = R[..., 1, 0] * R[..., 2, 1] - R[..., 1, 1] * R[..., 2, 0]
        seen &= (R[..., 0, 0] * c0 - R[..., 0, 1] * c1) + R[..., 0, 2] * c2 > 0.0
        acc = acc & seen[..., None]
        m = np.where(acc[..., None], meas, 0.0)               # a rejected measurement is never read
        Rk = R[:, :, None]                                    # [T, S, 1, 3, 3] against the K tracks
        rot = (Rk[..., 0] * m[..., 0:1] + Rk[..., 1] * m[..., 1:2]) + Rk[..., 2] * m[..., 2:3]
        point = np.arange(P + 1 + J) >= P
        m_w = np.where(point[:, None], rot + tr[:, :, None], rot)
        tracks, placed, with_root, new_state = _track_run(prm, P, st, dts, m_w, acc)
        d = np.where(with_root[..., None, None], placed - tr[:, :, None], placed)
        cam = (Rk[..., 0, :] * d[..., 0:1] + Rk[..., 1, :] * d[..., 1:2]) + Rk[..., 2, :] * d[..., 2:3]
        cam = np.where((tracks[..., :P, 7] != 0)[..., None] & seen[..., None, None], cam, 0.0)
    B = T * S
    return tracks.reshape(B, -1, 8).astype(dtype), placed.reshape(B, P, 3).astype(dtype), cam.reshape(B, P, 3).astype(dtype), new_state


# ---- a rigid skeleton and bone rotations from the tracked pose (egotap.h: egotap_skeleton_fit) -------------------------------------------
SKELETON_MAX_ROWS = 64                         # P: one lane each
SKELETON_STATE = 2                             # per row: (L^, n)
SKELETON_ANTIPARALLEL = -1.0 + 1e-12           # v . u above this: the shortest arc's regular branch
SKELETON_FRAME_ROWS = {"UnrealEgo": (1, 2, 3),       # neck_01, upperarm_l, upperarm_r
                       "EgoCap": (0, 9, 13)}         # neck, left_hip, right_hip (rows = the reference's joints 1 .. 17)
SKELETON_MIRROR = {"UnrealEgo": (-1, -1) + tuple(j ^ 1 for j in range(2, 16)),
                   "EgoCap": (-1,) + tuple(range(5, 9)) + tuple(range(1, 5)) + tuple(range(13, 17)) + tuple(range(9, 13))}


@dataclass(frozen=True)
class SkeletonParams:
    """egotap.h egotap_skeleton_params.  ``window``: a bone's length is the exact mean of its first ``window`` accepted samples, then an exponential
    average with alpha = 1 / window; ``min_samples``: below this many accepted samples every valid sample is taken; from then on one is taken when
    |l - L^| <= max_dev L^ (``max_dev`` relative, +inf: every one); ``freeze``: the lengths are used and no longer updated.  With min_samples = 0 an
    empty state never accepts a sample (|l - 0| <= max_dev 0 is false).  Nobody has tuned any of these on real data: there is no dataset here."""
    window: int = 120
    min_samples: int = 10
    max_dev: float = math.inf
    freeze: bool = False

    def __post_init__(self):
        w, m, d = int(self.window), int(self.min_samples), float(self.max_dev)
        if w < 1:
            raise ValueError(f"SkeletonParams: window must be at least 1, got {self.window}")
        if m < 0:
            raise ValueError(f"SkeletonParams: min_samples must not be negative, got {self.min_samples}")
        if not d >= 0:
            raise ValueError(f"SkeletonParams: max_dev must be >= 0 (+inf: off), got {self.max_dev}")
        for name, v in (("window", w), ("min_samples", m), ("max_dev", d), ("freeze", bool(self.freeze))):
            object.__setattr__(self, name, v)


def skeleton_parents(joint_preset):
    """The parent row of every pose row, -1 for the root row (utils/util.py:51-52).  "UnrealEgo": the 16 rows with the head as the root.  "EgoCap":
    joints 1 .. 17 as rows 0 .. 16, the neck the root row: the camera-to-neck bone is dropped, as the reference's loss drops it."""
    from .lib import KINEMATIC_PARENTS
    if joint_preset not in KINEMATIC_PARENTS:
        raise ValueError(f"skeleton_parents: joint_preset is {joint_preset!r}, expected one of {sorted(KINEMATIC_PARENTS)}")
    par = KINEMATIC_PARENTS[joint_preset]
    if joint_preset == "EgoCap":
        return tuple(p - 1 if j > 1 else -1 for j, p in enumerate(par) if j >= 1)
    return tuple(p if j > 0 else -1 for j, p in enumerate(par))


def _sk_norm3(d):
    return math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def _sk_cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sk_ok(n):
    return 0.0 < n <= 1.7976931348623157e308          # finite and > 0; false on a NaN


def skeleton_frame(xa, xb, xc):
    """the orthonormal frame of three points, rows (e0, e1, e2), or None where a norm in its construction is zero or not finite:
    e0 = normalize(xb - xc); w = xa - (xb + xc) / 2; e1 = normalize(w - (w . e0) e0); e2 = e0 x e1"""
    f = tuple(xb[i] - xc[i] for i in range(3))
    n0 = _sk_norm3(f)
    if not _sk_ok(n0):
        return None
    e0 = tuple(f[i] / n0 for i in range(3))
    w = tuple(xa[i] - 0.5 * (xb[i] + xc[i]) for i in range(3))
    p = (w[0] * e0[0] + w[1] * e0[1]) + w[2] * e0[2]
    g = tuple(w[i] - p * e0[i] for i in range(3))
    n1 = _sk_norm3(g)
    if not _sk_ok(n1):
        return None
    e1 = tuple(g[i] / n1 for i in range(3))
    return (e0, e1, _sk_cross(e0, e1))


def quat_sign(q):
    """the sign rule: w >= 0; at w == 0 the first non-zero of x, y, z is positive"""
    w, x, y, z = q
    neg = w < 0 or (w == 0 and (x < 0 or (x == 0 and (y < 0 or (y == 0 and z < 0)))))
    return (-w, -x, -y, -z) if neg else (w, x, y, z)


def quat_normalize(q):
    n = math.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return (q[0] / n, q[1] / n, q[2] / n, q[3] / n)


def quat_mul(a, b):
    """Hamilton's a (x) b on (w, x, y, z), each component added left to right"""
    return (((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3],
            ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2],
            ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1],
            ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0])


def quat_conj(q):
    return (q[0], -q[1], -q[2], -q[3])


def quat_rotate(q, v):
    """v' = (v + w t) + q_v x t with t = 2 (q_v x v)"""
    qv = q[1:]
    c = _sk_cross(qv, v)
    t = (2.0 * c[0], 2.0 * c[1], 2.0 * c[2])
    k = _sk_cross(qv, t)
    return tuple((v[i] + q[0] * t[i]) + k[i] for i in range(3))


def quat_from_frames(cur, rest):
    """quat(M_cur M_rest^T) of two frames given as rows (e0, e1, e2): R[i][j] = (e0c[i] e0r[j] + e1c[i] e1r[j]) + e2c[i] e2r[j], then Shepperd's rule,
    which divides by the largest of (trace, R00, R11, R22) only -- t = (R00 + R11) + R22:
        t > 0                     s = 2 sqrt(t + 1);                  (w, x, y, z) = (s / 4, (R21 - R12) / s, (R02 - R20) / s, (R10 - R01) / s)
        R00 >= R11 and R00 >= R22 s = 2 sqrt(((1 + R00) - R11) - R22); (w, x, y, z) = ((R21 - R12) / s, s / 4, (R01 + R10) / s, (R02 + R20) / s)
        R11 >= R22                s = 2 sqrt(((1 + R11) - R00) - R22); (w, x, y, z) = ((R02 - R20) / s, (R01 + R10) / s, s / 4, (R12 + R21) / s)
        otherwise                 s = 2 sqrt(((1 + R22) - R00) - R11); (w, x, y, z) = ((R10 - R01) / s, (R02 + R20) / s, (R12 + R21) / s, s / 4)
    then normalised and given its sign"""
    R = [[(cur[0][i] * rest[0][j] + cur[1][i] * rest[1][j]) + cur[2][i] * rest[2][j] for j in range(3)] for i in range(3)]
    t = (R[0][0] + R[1][1]) + R[2][2]
    if t > 0:
        s = math.sqrt(t + 1.0) * 2.0
        q = (0.25 * s, (R[2][1] - R[1][2]) / s, (R[0][2] - R[2][0]) / s, (R[1][0] - R[0][1]) / s)
    elif R[0][0] >= R[1][1] and R[0][0] >= R[2][2]:
        s = math.sqrt(max(((1.0 + R[0][0]) - R[1][1]) - R[2][2], 0.0)) * 2.0
        q = ((R[2][1] - R[1][2]) / s, 0.25 * s, (R[0][1] + R[1][0]) / s, (R[0][2] + R[2][0]) / s)
    elif R[1][1] >= R[2][2]:
        s = math.sqrt(max(((1.0 + R[1][1]) - R[0][0]) - R[2][2], 0.0)) * 2.0
        q = ((R[0][2] - R[2][0]) / s, (R[0][1] + R[1][0]) / s, 0.25 * s, (R[1][2] + R[2][1]) / s)
    else:
        s = math.sqrt(max(((1.0 + R[2][2]) - R[0][0]) - R[1][1], 0.0)) * 2.0
        q = ((R[1][0] - R[0][1]) / s, (R[0][2] + R[2][0]) / s, (R[1][2] + R[2][1]) / s, 0.25 * s)
    return quat_sign(quat_normalize(q))


def quat_shortest_arc(v, u):
    """the swing that takes the unit vector v to the unit vector u by the shortest arc, c = v . u: c > -1 + 1e-12: normalize(1 + c, v x u); otherwise
    (0, normalize(v x e_k)), k the lowest index of the smallest |v_k| (a half turn about an axis at right angles to v).  Not given a sign."""
    c = (v[0] * u[0] + v[1] * u[1]) + v[2] * u[2]
    if c > SKELETON_ANTIPARALLEL:
        x = _sk_cross(v, u)
        return quat_normalize((1.0 + c, x[0], x[1], x[2]))
    k = 0
    for i in (1, 2):
        if abs(v[i]) < abs(v[k]):
            k = i
    x = _sk_cross(v, tuple(1.0 if i == k else 0.0 for i in range(3)))
    n = _sk_norm3(x)
    return (0.0, x[0] / n, x[1] / n, x[2] / n)


@dataclass(frozen=True, eq=False)
class SkeletonRig:
    """egotap.h egotap_skeleton_rig, checked, with what the entry derives from it: ``rest_dir`` [P, 3] and ``rest_len`` [P] (zeros for root rows),
    ``rest_frame`` (the rows e0, e1, e2 of the rest pose's triangle) and ``depth`` [P].  Built by ``skeleton_rig``."""
    P: int
    parents: tuple
    rest_pos: object
    frame_rows: tuple
    mirror: object
    fixed_length: object
    rest_dir: object
    rest_len: object
    rest_frame: tuple
    depth: tuple


def skeleton_rig(parents, rest_pos, frame_rows, mirror=None, fixed_length=None):
    """The avatar a skeleton is fitted to: ``parents`` [P] (-1: a root row; otherwise 0 <= parent < row), ``rest_pos`` [P, 3] the rest pose in any
    unit, ``frame_rows`` (a, b, c) three distinct rows whose triangle orients the root rows, ``mirror`` [P] the row on the other side of the body or
    -1 (None: no row has one), ``fixed_length`` [P] the avatar's own bone lengths (None: calibrated from the data) -> a ``SkeletonRig``.  Refuses, by
    name, what egotap_skeleton_fit refuses."""
    import numpy as np
    who = "skeleton_rig"
    par = tuple(int(p) for p in parents)
    P = len(par)
    if not 1 <= P <= SKELETON_MAX_ROWS:
        raise ValueError(f"{who}: 1 .. {SKELETON_MAX_ROWS} rows, got {P}")
    if -1 not in par:
        raise ValueError(f"{who}: no root row (parent -1)")
    for j, p in enumerate(par):
        if p != -1 and not 0 <= p < j:
            raise ValueError(f"{who}: parent[{j}] = {p}: a parent is -1 (a root row) or an earlier row, 0 <= parent < row")
    rp = np.array(rest_pos, dtype=np.float64)
    if rp.shape != (P, 3):
        raise ValueError(f"{who}: rest_pos is [P, 3] = {(P, 3)}, got {rp.shape}")
    if not np.isfinite(rp).all():
        raise ValueError(f"{who}: rest_pos must be finite")
    fr = tuple(int(r) for r in frame_rows)
    if len(fr) != 3 or any(not 0 <= r < P for r in fr) or len(set(fr)) != 3:
        raise ValueError(f"{who}: frame_rows are three distinct rows 0 .. {P - 1}, got {fr}")
    rest_dir, rest_len, depth = np.zeros((P, 3)), np.zeros(P), [0] * P
    for j, p in enumerate(par):
        if p < 0:
            continue
        d = tuple(float(rp[j, i]) - float(rp[p, i]) for i in range(3))
        n = _sk_norm3(d)
        if not _sk_ok(n):
            raise ValueError(f"{who}: the rest bone of row {j} (to its parent {p}) has length {n}: a zero or non-finite rest bone has no direction")
        rest_dir[j], rest_len[j], depth[j] = [d[i] / n for i in range(3)], n, depth[p] + 1
    frame = skeleton_frame(*(tuple(float(v) for v in rp[r]) for r in fr))
    if frame is None:
        raise ValueError(f"{who}: the rest pose's triangle of rows {fr} is degenerate: it orients nothing")
    mir = None
    if mirror is not None:
        mir = tuple(int(m) for m in mirror)
        if len(mir) != P:
            raise ValueError(f"{who}: mirror holds one row per row, [{P}], got {len(mir)}")
        for j, m in enumerate(mir):
            if m == -1:
                continue
            if not 0 <= m < P or mir[m] != j:
                raise ValueError(f"{who}: mirror[{j}] = {m} is not an involution (mirror[mirror[j]] == j, or -1)")
            if par[j] < 0 or par[m] < 0:
                raise ValueError(f"{who}: mirror[{j}] = {m} pairs a root row, which has no bone")
    fixed = None
    if fixed_length is not None:
        fixed = np.array(fixed_length, dtype=np.float64)
        if fixed.shape != (P,):
            raise ValueError(f"{who}: fixed_length holds one length per row, [{P}], got {fixed.shape}")
        for j, p in enumerate(par):
            if p >= 0 and not _sk_ok(float(fixed[j])):
                raise ValueError(f"{who}: fixed_length[{j}] = {fixed[j]} must be finite and > 0")
        fixed = np.where(np.array(par) >= 0, fixed, 0.0)
        fixed.setflags(write=False)
    for a in (rp, rest_dir, rest_len):
        a.setflags(write=False)
    return SkeletonRig(P, par, rp, fr, mir, fixed, rest_dir, rest_len, frame, tuple(depth))


def skeleton_rig_from_pose(joint_preset, pose_rows, mirror=True, fixed_length=None):
    """One frame taken as the rest pose, the "stand in a T-pose" calibration: the preset's parents, frame rows and (``mirror=True``) left / right
    pairs, ``pose_rows`` [P, 3] relative to its root row"""
    import numpy as np
    par = skeleton_parents(joint_preset)
    ps = np.array(pose_rows.detach().cpu().numpy() if hasattr(pose_rows, "detach") else pose_rows, dtype=np.float64)
    if ps.shape != (len(par), 3):
        raise ValueError(f"skeleton_rig_from_pose: pose_rows is one frame [P, 3] = {(len(par), 3)} for {joint_preset}, got {ps.shape}")
    return skeleton_rig(par, ps - ps[par.index(-1)], SKELETON_FRAME_ROWS[joint_preset], mirror=SKELETON_MIRROR[joint_preset] if mirror else None,
                        fixed_length=fixed_length)


def _sk_div(a, b):
    """a / b as IEEE has it (a state the caller wrote may hold anything)"""
    import numpy as np
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def skeleton_fit_ref(points, state, rig, params=None, tracks=None, streams=1, dtype="float32"):
    """The records and the state egotap_skeleton_fit writes, restated in float64, operation for operation: points [B, P, 3] with B = T * streams frames,
    time-major (frame b = t * streams + s); state [streams, P, 2] float64 = (L^, n) per row (not modified; None with a ``fixed_length`` rig, which
    reads none); tracks [B, K, 8] (K >= P) the tracker's records or None -> (rigid [B, P, 4], rotations [B, P, 8], lengths [B, P, 2], new_state).
    One step of one stream, every comparison false on a NaN:

        seen        the row's three inputs are finite (and, with tracks, its status is 1 or 2)
        sample      non-root: d = x_j - x_p, l = sqrt((d0 d0 + d1 d1) + d2 d2); valid: both ends seen, l finite and > 0; u = d / l
        update      valid, not frozen, no fixed_length, and (n < min_samples or |l - L^| <= max_dev L^): n = min(n + 1, window), L^ = L^ + (l - L^) / n
        length L_j  fixed_length[j]; else, after every row's update: L^_j where n_j >= 1, (L^_j + L^_m) / 2 with a mirror m of n_m >= 1; else none
        rigid       a seen root row passes through; r_j = r_p + L_j u_j where the sample is valid, L_j exists and the parent is ok; else zeros
        rotation    root rows: quat_from_frames(skeleton_frame(x_a, x_b, x_c), rest frame) where a, b, c are seen and the frame is not degenerate;
                    others, with a valid sample and a parent whose rotation is ok: v = rotate(Q_p, rest_dir_j), s = quat_shortest_arc(v, u_j),
                    Q_j = sign(normalize(s (x) Q_p)), local_j = sign(conj(Q_p) (x) Q_j); else the identity (local = global for a root row)

    rigid = (x, y, z, 1 (position ok) + 2 (rotation ok)); rotations = (global wxyz, local wxyz); lengths = (L_j or 0, n_j), zeros for root rows.
    Each output is rounded once from float64 (``dtype="float64"``: not at all)."""
    return _skeleton_fit_walk("skeleton_fit_ref", points, state, rig, params, tracks, streams, dtype, None)


def _skeleton_fit_walk(who, points, state, rig, params, tracks, streams, dtype, twist):
    """the one body of skeleton_fit_ref (``twist`` None) and skeleton_fit_twist_ref (a checked SkeletonTwist of the same rig)"""
    import numpy as np
    if not isinstance(rig, SkeletonRig):
        raise ValueError(f"{who}: rig is a spec.SkeletonRig (spec.skeleton_rig builds one), got {type(rig).__name__}")
    prm = SkeletonParams() if params is None else params
    pts = np.asarray(points, dtype=np.float64)
    S, P = int(streams), rig.P
    if pts.ndim != 3 or pts.shape[1:] != (P, 3) or S < 1 or pts.shape[0] < S or pts.shape[0] % S:
        raise ValueError(f"{who}: points is [T * streams, P, 3] with T >= 1 and the rig's P = {P}, got {pts.shape} for {S} streams")
    B = pts.shape[0]
    T = B // S
    status = None
    if tracks is not None:
        tr = np.asarray(tracks, dtype=np.float64)
        if tr.ndim != 3 or tr.shape[0] != B or tr.shape[1] < P or tr.shape[2] != 8:
            raise ValueError(f"{who}: tracks is [T * streams, K, 8] with K >= P, got {tr.shape} for {B} frames of {P} rows")
        status = tr[:, :P, 7]
    fixed = rig.fixed_length is not None
    if fixed:
        st = None
    else:
        if state is None:
            raise ValueError(f"{who}: state is [streams, P, 2]; only a rig with fixed_length goes without one")
        st = np.array(state, dtype=np.float64)
        if st.shape != (S, P, SKELETON_STATE):
            raise ValueError(f"{who}: state is [streams, P, {SKELETON_STATE}] = {(S, P, SKELETON_STATE)}, got {st.shape}")
    par, mir = rig.parents, rig.mirror
    rest_dir = [tuple(float(v) for v in r) for r in rig.rest_dir]
    window, min_samples, max_dev = float(prm.window), float(prm.min_samples), prm.max_dev
    fa, fb, fc = rig.frame_rows
    hinge_g = None if twist is None else [tuple(float(v) for v in row) for row in twist.g]
    rigid, rot, lens = np.zeros((B, P, 4)), np.zeros((B, P, 8)), np.zeros((B, P, 2))
    ident = (1.0, 0.0, 0.0, 0.0)
    fin = math.isfinite
    for t in range(T):
        for s in range(S):
            b = t * S + s
            x = [tuple(float(v) for v in pts[b, j]) for j in range(P)]
            seen = [fin(x[j][0]) and fin(x[j][1]) and fin(x[j][2]) and (status is None or status[b, j] == 1 or status[b, j] == 2) for j in range(P)]
            valid, u, ell = [False] * P, [None] * P, [0.0] * P
            for j, p in enumerate(par):
                if p < 0 or not (seen[j] and seen[p]):
                    continue
                d = (x[j][0] - x[p][0], x[j][1] - x[p][1], x[j][2] - x[p][2])
                n = _sk_norm3(d)
                if _sk_ok(n):
                    valid[j], ell[j], u[j] = True, n, (d[0] / n, d[1] / n, d[2] / n)
            if not fixed and not prm.freeze:
                for j in range(P):
                    if not valid[j]:
                        continue
                    L, n = float(st[s, j, 0]), float(st[s, j, 1])
                    if n < min_samples or abs(ell[j] - L) <= max_dev * L:
                        n = n + 1.0 if n + 1.0 < window else window
                        st[s, j] = (L + _sk_div(ell[j] - L, n), n)
            frame = skeleton_frame(x[fa], x[fb], x[fc]) if seen[fa] and seen[fb] and seen[fc] else None
            q_root = quat_from_frames(frame, rig.rest_frame) if frame is not None else None
            r, Q, r_ok, q_ok = [None] * P, [ident] * P, [False] * P, [False] * P
            for j, p in enumerate(par):
                loc, t_ok = ident, False
                if p < 0:
                    r_ok[j], r[j] = seen[j], x[j]
                    if q_root is not None:
                        q_ok[j], Q[j] = True, q_root
                        loc = q_root
                else:
                    if fixed:
                        L, have, n = float(rig.fixed_length[j]), True, 0.0
                    else:
                        L, n = float(st[s, j, 0]), float(st[s, j, 1])
                        have = n >= 1
                        if have and mir is not None and mir[j] >= 0 and st[s, mir[j], 1] >= 1:
                            L = 0.5 * (L + float(st[s, mir[j], 0]))
                    lens[b, j] = (L if have else 0.0, n)
                    if valid[j] and have and r_ok[p]:
                        r_ok[j], r[j] = True, tuple(r[p][i] + L * u[j][i] for i in range(3))
                    if valid[j] and q_ok[p]:
                        v = quat_rotate(Q[p], rest_dir[j])
                        q_s = quat_normalize(quat_mul(quat_shortest_arc(v, u[j]), Q[p]))
                        if twist is not None and twist.pole[j] >= 0 and valid[twist.pole[j]]:
                            rolled = quat_twist(q_s, hinge_g[j], u[j], u[twist.pole[j]], twist.bend_lo, twist.bend_hi)
                            if rolled is not None:
                                q_s, t_ok = rolled, True
                        Q[j] = quat_sign(q_s)
                        loc = quat_sign(quat_mul(quat_conj(Q[p]), Q[j]))
                        q_ok[j] = True
                rigid[b, j] = ((r[j] if r_ok[j] else (0.0, 0.0, 0.0)) + (1.0 * r_ok[j] + 2.0 * q_ok[j] + 4.0 * t_ok,))
                rot[b, j] = Q[j] + loc
    return rigid.astype(dtype), rot.astype(dtype), lens.astype(dtype), st


# ---- bone twist from the bend plane of the child bone (egotap.h: egotap_skeleton_fit_twist) ----------------------------------------------
SKELETON_BEND_LO = 0.17364817766693033         # sin 10 deg: at or below this sine of the bend angle the twist is not observed
SKELETON_BEND_HI = 0.42261826174069944         # sin 25 deg: from here on the bend normal is fully taken.  Nobody has tuned either on data: there is no dataset here.
SKELETON_HINGE_MIN = 1e-6                      # a hinge's part at right angles to its rest bone is at least this long
# row j -> the row c whose bone bends against j's (rows are skeleton_parents' rows): upper arm -> forearm, thigh -> shank, shank -> foot.  The EgoCap
# wrists are left out: a hand flexes both ways, so the normal's sign is not stable there.
SKELETON_POLE = {"UnrealEgo": {4: 6, 5: 7, 10: 12, 11: 13, 12: 14, 13: 15},
                 "EgoCap": {2: 3, 6: 7, 10: 11, 14: 15, 11: 12, 15: 16}}


def _sk_dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def quat_twist(q_s, g, u, u_c, bend_lo, bend_hi):
    """egotap.h's twist step: ``q_s`` the swung rotation of a bone (unit, no sign), ``g`` its unit rest hinge at right angles to its rest direction,
    ``u`` the bone's direction, ``u_c`` its pole child's -> normalize(tw (x) q_s), not given a sign, or None where the twist is not observed:
        m = u x u_c, sigma = |m|; w = 0 unless sigma > bend_lo, 1 if sigma >= bend_hi, else t = (sigma - bend_lo) / (bend_hi - bend_lo), w = (t t)(3 - 2 t)
        w > 0: n = m / sigma; h = rotate(q_s, g), h' = normalize(h - (h . u) u); b = normalize((1 - w) h' + w n); a zero or non-finite norm: None
        k = h' . b; k > -1 + 1e-12: tw = normalize(1 + k, h' x b); otherwise tw = (0, u), the half turn about the bone"""
    m = _sk_cross(u, u_c)
    sigma = _sk_norm3(m)
    if not (sigma > bend_lo and _sk_ok(sigma)):
        return None
    if sigma >= bend_hi:
        w = 1.0
    else:
        t = (sigma - bend_lo) / (bend_hi - bend_lo)
        w = (t * t) * (3.0 - 2.0 * t)
    if not w > 0.0:
        return None
    n = (m[0] / sigma, m[1] / sigma, m[2] / sigma)
    h = quat_rotate(q_s, g)
    p = _sk_dot(h, u)
    hr = (h[0] - p * u[0], h[1] - p * u[1], h[2] - p * u[2])
    nh = _sk_norm3(hr)
    if not _sk_ok(nh):
        return None
    hp = (hr[0] / nh, hr[1] / nh, hr[2] / nh)
    w1 = 1.0 - w
    br = (w1 * hp[0] + w * n[0], w1 * hp[1] + w * n[1], w1 * hp[2] + w * n[2])
    nb = _sk_norm3(br)
    if not _sk_ok(nb):
        return None
    b = (br[0] / nb, br[1] / nb, br[2] / nb)
    k = _sk_dot(hp, b)
    if k > SKELETON_ANTIPARALLEL:
        x = _sk_cross(hp, b)
        tw = quat_normalize((1.0 + k, x[0], x[1], x[2]))
    else:
        tw = (0.0, u[0], u[1], u[2])
    return quat_normalize(quat_mul(tw, q_s))


@dataclass(frozen=True, eq=False)
class SkeletonTwist:
    """egotap.h egotap_skeleton_twist, checked against its rig, with what the entry derives from it: ``pole`` [P] (-1: none), ``hinge`` [P, 3] (zeros
    where the row has no pole), ``g`` [P, 3] = the hinge made orthogonal to rest_dir and normalised, the two thresholds.  Built by ``skeleton_twist``."""
    P: int
    pole: tuple
    hinge: object
    g: object
    bend_lo: float
    bend_hi: float


def _sk_pole_rows(who, rig, pole):
    """``pole`` as a tuple [P]: given as a mapping {row: child} or as one entry per row (-1: none); refuses what egotap_skeleton_fit_twist refuses"""
    if not isinstance(rig, SkeletonRig):
        raise ValueError(f"{who}: rig is a spec.SkeletonRig (spec.skeleton_rig builds one), got {type(rig).__name__}")
    P = rig.P
    if hasattr(pole, "items"):
        rows = [-1] * P
        for j, c in pole.items():
            if not 0 <= int(j) < P:
                raise ValueError(f"{who}: pole names row {j}: rows are 0 .. {P - 1}")
            rows[int(j)] = int(c)
    else:
        rows = [int(c) for c in pole]
        if len(rows) != P:
            raise ValueError(f"{who}: pole holds one row per row, [{P}], or is a mapping row -> child; got {len(rows)} entries")
    for j, c in enumerate(rows):
        if c == -1:
            continue
        if not 0 <= c < P:
            raise ValueError(f"{who}: pole[{j}] = {c} is -1 or a row 0 .. {P - 1}")
        if rig.parents[j] < 0:
            raise ValueError(f"{who}: pole[{j}] = {c} is set on a root row, which has no bone to roll")
        if rig.parents[c] != j:
            raise ValueError(f"{who}: pole[{j}] = {c}: the pole of a row is one of its children (parent[{c}] = {rig.parents[c]})")
    return tuple(rows)


def _sk_thresholds(who, bend_lo, bend_hi):
    lo, hi = float(bend_lo), float(bend_hi)
    if not (0.0 <= lo < hi <= 1.0):
        raise ValueError(f"{who}: 0 <= bend_lo < bend_hi <= 1, sines of the bend angle, got bend_lo = {bend_lo}, bend_hi = {bend_hi}")
    return lo, hi


def skeleton_twist(rig, pole, hinge=None, bend_lo=SKELETON_BEND_LO, bend_hi=SKELETON_BEND_HI):
    """The twist table of egotap_skeleton_fit_twist for ``rig``: ``pole`` a mapping {row j: the row c whose bone bends against j's} (``SKELETON_POLE``
    holds the presets') or one entry per row, -1 for none; ``hinge`` [P, 3] the hinge axis of every pole row IN THE REST POSE, the direction
    rest_dir_j x rest_dir_c would have if the joint were bent the way it anatomically bends (rows without a pole are not read), None: the rest pose's
    own rest_dir_j x rest_dir_c, which needs a rest pose bent by at least ``bend_hi`` at every pole joint; ``bend_lo`` / ``bend_hi`` sines of the bend
    angle (at or below the first the twist is not observed, from the second on it is fully taken; the defaults, sin 10 deg and sin 25 deg, have not
    been tuned on data) -> a ``SkeletonTwist``.  Refuses, by name, what the entry refuses."""
    import numpy as np
    who = "skeleton_twist"
    rows = _sk_pole_rows(who, rig, pole)
    lo, hi = _sk_thresholds(who, bend_lo, bend_hi)
    P = rig.P
    rest_dir = [tuple(float(v) for v in r) for r in rig.rest_dir]
    hg = np.zeros((P, 3))
    if hinge is not None:
        given = np.array(hinge, dtype=np.float64)
        if given.shape != (P, 3):
            raise ValueError(f"{who}: hinge is [P, 3] = {(P, 3)}, got {given.shape}")
    g = np.zeros((P, 3))
    for j, c in enumerate(rows):
        if c < 0:
            continue
        if hinge is None:
            h = _sk_cross(rest_dir[j], rest_dir[c])
            n = _sk_norm3(h)
            if not n >= hi:
                raise ValueError(f"{who}: the rest pose is straight at row {j}: |rest_dir[{j}] x rest_dir[{c}]| = {n} is below bend_hi = {hi}, so it has no "
                                 "hinge of its own (a T-pose has straight arms); take the hinges from a frame with bent elbows and knees "
                                 "(skeleton_hinges_from_pose) or give an explicit axis")
        else:
            h = tuple(float(v) for v in given[j])
            if not all(math.isfinite(v) for v in h):
                raise ValueError(f"{who}: hinge[{j}] is not finite")
        d = _sk_dot(h, rest_dir[j])
        gr = (h[0] - d * rest_dir[j][0], h[1] - d * rest_dir[j][1], h[2] - d * rest_dir[j][2])
        n = _sk_norm3(gr)
        if not (n >= SKELETON_HINGE_MIN and _sk_ok(n)):
            raise ValueError(f"{who}: hinge[{j}] is (nearly) parallel to the rest bone of row {j}: its part at right angles has norm {n} < {SKELETON_HINGE_MIN}")
        hg[j], g[j] = h, (gr[0] / n, gr[1] / n, gr[2] / n)
    for a in (hg, g):
        a.setflags(write=False)
    return SkeletonTwist(P, rows, hg, g, lo, hi)


def skeleton_hinges_from_pose(rig, pole, pose_rows, bend_hi=SKELETON_BEND_HI):
    """The "now bend your elbows and knees" calibration: one frame ``pose_rows`` [P, 3] in which every pole joint is bent the way it anatomically
    bends, by at least ``bend_hi`` (a sine) -> hinge [P, 3] for ``skeleton_twist``: the float64 swing walk of skeleton_fit_ref on that frame gives
    Q_s per row, the frame's bend normal is n_j = normalize(u_j x u_c), and hinge_j = rotate(conj(Q_s_j), n_j) -- the normal carried back into the rest
    pose; zeros for rows without a pole.  Refuses by name a frame in which a pole row or its child is missing or a joint is too straight."""
    import numpy as np
    who = "skeleton_hinges_from_pose"
    rows = _sk_pole_rows(who, rig, pole)
    hi = _sk_thresholds(who, 0.0, bend_hi)[1]
    ps = np.array(pose_rows.detach().cpu().numpy() if hasattr(pose_rows, "detach") else pose_rows, dtype=np.float64)
    if ps.shape != (rig.P, 3):
        raise ValueError(f"{who}: pose_rows is one frame [P, 3] = {(rig.P, 3)}, got {ps.shape}")
    state = None if rig.fixed_length is not None else np.zeros((1, rig.P, SKELETON_STATE))
    rigid, rot, _, _ = _skeleton_fit_walk(who, ps[None], state, rig, None, None, 1, "float64", None)
    hinge = np.zeros((rig.P, 3))
    for j, c in enumerate(rows):
        if c < 0:
            continue
        if rigid[0, j, 3] < 2 or rigid[0, c, 3] < 2:
            raise ValueError(f"{who}: row {j} or its pole child {c} has no rotation in this frame (a missing row, a zero-length bone or a degenerate triangle)")
        x = [tuple(float(v) for v in ps[k]) for k in (rig.parents[j], j, c)]
        dj, dc = tuple(x[1][i] - x[0][i] for i in range(3)), tuple(x[2][i] - x[1][i] for i in range(3))
        nj, nc = _sk_norm3(dj), _sk_norm3(dc)
        m = _sk_cross(tuple(v / nj for v in dj), tuple(v / nc for v in dc))
        sigma = _sk_norm3(m)
        if not sigma >= hi:
            raise ValueError(f"{who}: the frame is straight at row {j}: the sine of the bend between the bones of rows {j} and {c} is {sigma}, below bend_hi = {hi}; "
                             "bend the elbows and knees")
        hinge[j] = quat_rotate(quat_conj(tuple(float(v) for v in rot[0, j, :4])), tuple(v / sigma for v in m))
    return hinge


def skeleton_fit_twist_ref(points, state, rig, twist, params=None, tracks=None, streams=1, dtype="float32"):
    """The records and the state egotap_skeleton_fit_twist writes, restated in float64, operation for operation: skeleton_fit_ref's arguments and
    results with ``twist`` a ``SkeletonTwist`` of the same rig (``skeleton_twist`` builds one).  Every step is skeleton_fit_ref's but a non-root row's
    rotation: with q_s = normalize(s (x) Q_p) its swung rotation, a row j whose pole child c has a valid sample gets
    Q_j = sign(quat_twist(q_s, g_j, u_j, u_c, bend_lo, bend_hi)) and flags + 4 where that observes a twist, Q_j = sign(q_s) otherwise; descendants read
    the twisted Q_j.  rigid[..., :3], lengths and the state equal skeleton_fit_ref's in bits."""
    who = "skeleton_fit_twist_ref"
    if not isinstance(twist, SkeletonTwist):
        raise ValueError(f"{who}: twist is a spec.SkeletonTwist (spec.skeleton_twist builds one), got {type(twist).__name__}")
    if isinstance(rig, SkeletonRig):
        if twist.P != rig.P:
            raise ValueError(f"{who}: the twist table has P = {twist.P} rows, the rig {rig.P}")
        _sk_pole_rows(who, rig, twist.pole)
    return _skeleton_fit_walk(who, points, state, rig, params, tracks, streams, dtype, twist)


# ---- heatmaps, keypoints and bones drawn onto the frames (egotap.h: egotap_heat_u8 / egotap_overlay_u8) -----------------------------------
OVERLAY_MAX_MARKS = 64                         # M: prepared once per workgroup, one thread each
OVERLAY_MAX_BONES = 64                         # L
OVERLAY_MAX_SIDE = 16384                       # Hc, Wc <= 16384: a pixel centre 16 X + 8 stays below 2^18
OVERLAY_MAX_HEAT_SIDE = 4096                   # S <= 4096: a tap index fits the low 16 bits of a table entry
OVERLAY_MAX_R16 = 16384                        # r16, w16 <= 16384 (1024 pixels): a culling box stays inside int32
OVERLAY_MARK_LIMIT = 32768.0                   # |x|, |y| < 32768: |rint(16 x)| <= 2^19, so every product below stays under 2^42
OVERLAY_TAP_OUTSIDE = -1                       # a tap table entry whose canvas pixel lies outside the map's extent


def heat_u8(hm, c0: int, n: int, groups: int = 1):
    """The reference's picture of a heatmap stack (utils/util.py:160-175 tensor2im(is_heatmap=True)) per group of channels, restated in numpy: hm
    [B, C, S, S] (float32, or anything exactly representable in it -- bf16 values upcast) -> uint8 [B, groups, S, S].  Group g is channels
    c0 + g n/groups .. c0 + (g + 1) n/groups - 1; per pixel, in float32:

        v = the group's channels added in ascending order;  v = v > 0 ? (v < 1 ? v : 1) : 0  (a NaN gives 0);  byte = (uint8)(int)(v * 255.0f)

    truncated, as the reference's astype(np.uint8) truncates.  This is what heat_u8_kernel computes, bit for bit."""
    import numpy as np
    h = np.asarray(hm, dtype=np.float32)
    if h.ndim != 4 or h.shape[2] != h.shape[3]:
        raise ValueError(f"heat_u8: maps are [B, C, S, S], got {h.shape}")
    B, C, S, _ = h.shape
    c0, n, groups = int(c0), int(n), int(groups)
    if n < 1 or groups < 1 or n % groups or c0 < 0 or c0 + n > C:
        raise ValueError(f"heat_u8: channels {c0} .. {c0 + n - 1} in {groups} groups are not a slice of the {C} channels in equal groups")
    per = n // groups
    out = np.empty((B, groups, S, S), dtype=np.uint8)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in range(groups):
            v = h[:, c0 + g * per].copy()
            for k in range(1, per):
                v = (v + h[:, c0 + g * per + k]).astype(np.float32)
            v = np.where(v > 0, np.where(v < 1, v, np.float32(1)), np.float32(0)).astype(np.float32)
            out[:, g] = (v * np.float32(255.0)).astype(np.float32).astype(np.int32).astype(np.uint8)
    return out


def overlay_taps(a: float, b: float, S: int, L: int):
    """The tap table of one canvas axis of length L over a heat map of side S: int32 [L].  Canvas coordinate = a u + b with u the heat coordinate
    (heat pixel centres at i + 0.5, canvas pixel centres at X + 0.5; a < 0 is a mirror) -- one component, (ax, bx) or (ay, by), of the eye's keypoint
    affine.  In float64: u = (X + 0.5 - b) / a;  outside the map's extent (not 0 <= u <= S) the entry is -1;  otherwise p = max(u - 0.5, 0),
    i0 = floor(p) (<= S - 1, as u <= S), w1 = floor((p - i0) * 2048 + 0.5), entry = i0 | w1 << 16 -- ``resize_taps``' pair for a = L / S, b = 0.  The second tap is
    i1 = min(i0 + 1, S - 1), the first one's weight 2048 - w1.  Built once on the host; the device reads the table and never the affine."""
    import numpy as np
    a, b, S, L = float(a), float(b), int(S), int(L)
    if not (math.isfinite(a) and math.isfinite(b)) or a == 0.0:
        raise ValueError(f"overlay_taps: the affine component must be finite with a != 0, got ({a}, {b})")
    if not (1 <= S <= OVERLAY_MAX_HEAT_SIDE and 1 <= L <= OVERLAY_MAX_SIDE):
        raise ValueError(f"overlay_taps: the heat side is 1 .. {OVERLAY_MAX_HEAT_SIDE} and the canvas length 1 .. {OVERLAY_MAX_SIDE}, got {S}, {L}")
    u = (np.arange(L, dtype=np.float64) + 0.5 - b) / a
    inside = (u >= 0.0) & (u <= float(S))
    p = np.where(inside, np.maximum(u - 0.5, 0.0), 0.0)
    i0 = np.floor(p)
    w1 = np.floor((p - i0) * float(RESIZE_WEIGHT_ONE) + 0.5)
    entry = i0.astype(np.int64) | (w1.astype(np.int64) << 16)
    return np.where(inside, entry, OVERLAY_TAP_OUTSIDE).astype(np.int32)


@dataclass(frozen=True)
class OverlayStyle:
    """egotap.h egotap_overlay_style: what is drawn and how.  ``bones`` [L][2] indices into the marks, ``mark_rgba`` [M][4] and ``bone_rgba`` [L][4]
    bytes (alpha 0 draws nothing), ``r16`` / ``w16`` the marks' radius and the bones' half-width in sixteenths of a pixel, ``min_score`` the least score
    of a mark that is drawn, ``heat_rgba`` the heat layer's one colour and its alpha."""
    bones: tuple = ()
    mark_rgba: tuple = ()
    bone_rgba: tuple = ()
    r16: int = 40
    w16: int = 16
    min_score: float = STEREO_MIN_SCORE
    heat_rgba: tuple = (255, 255, 255, 160)

    def __post_init__(self):
        bones = tuple((int(i), int(j)) for i, j in self.bones)
        marks = tuple(tuple(int(v) for v in c) for c in self.mark_rgba)
        bcol = tuple(tuple(int(v) for v in c) for c in self.bone_rgba)
        heat = tuple(int(v) for v in self.heat_rgba)
        M, L = len(marks), len(bones)
        if M > OVERLAY_MAX_MARKS or L > OVERLAY_MAX_BONES:
            raise ValueError(f"OverlayStyle: at most {OVERLAY_MAX_MARKS} marks and {OVERLAY_MAX_BONES} bones, got {M} and {L}")
        if len(bcol) != L:
            raise ValueError(f"OverlayStyle: bone_rgba has one colour per bone, got {len(bcol)} for {L} bones")
        if any(not (0 <= i < M and 0 <= j < M) for i, j in bones):
            raise ValueError(f"OverlayStyle: a bone's ends are mark indices 0 .. {M - 1}, got {bones}")
        if any(len(c) != 4 or any(not 0 <= v <= 255 for v in c) for c in marks + bcol + (heat,)):
            raise ValueError("OverlayStyle: a colour is four bytes (R, G, B, alpha)")
        r16, w16, ms = int(self.r16), int(self.w16), float(self.min_score)
        if not (0 <= r16 <= OVERLAY_MAX_R16 and 0 <= w16 <= OVERLAY_MAX_R16):
            raise ValueError(f"OverlayStyle: r16 and w16 are 0 .. {OVERLAY_MAX_R16} sixteenths of a pixel, got {self.r16}, {self.w16}")
        if math.isnan(ms):
            raise ValueError("OverlayStyle: min_score must not be NaN")
        for name, v in (("bones", bones), ("mark_rgba", marks), ("bone_rgba", bcol), ("heat_rgba", heat), ("r16", r16), ("w16", w16), ("min_score", ms)):
            object.__setattr__(self, name, v)


OVERLAY_LEFT_RGBA = (64, 160, 255, 255)        # the lower row of a mirrored pair (SKELETON_MIRROR)
OVERLAY_RIGHT_RGBA = (255, 96, 64, 255)        # the higher row
OVERLAY_CENTRE_RGBA = (96, 255, 96, 255)       # a row without a mirror row


def overlay_style(joint_preset, r16: int = 40, w16: int = 16, min_score: float = STEREO_MIN_SCORE, heat_rgba=(255, 255, 255, 160)):
    """The style of a preset's keypoints: one mark per heatmap joint, a bone from every joint to its parent (``skeleton_parents``; the pose rows the
    joints are paired with start at ``stereo_pose_row0``, and a bone whose parent is the head UnrealEgo has no heatmap of is left out), the colours by
    body side from ``SKELETON_MIRROR`` (the lower row of a mirrored pair, the higher one, rows without a mirror row); a bone takes its child's colour.
    Nothing here was tuned on data."""
    p = lift_preset(joint_preset)
    row0, par, mir = stereo_pose_row0(p), skeleton_parents(joint_preset), SKELETON_MIRROR[joint_preset]

    def colour(row):
        return OVERLAY_CENTRE_RGBA if mir[row] < 0 else OVERLAY_LEFT_RGBA if row < mir[row] else OVERLAY_RIGHT_RGBA
    rows = range(row0, row0 + p.n_joints_hm)
    bones = tuple((par[r] - row0, r - row0) for r in rows if par[r] >= row0)
    return OverlayStyle(bones=bones, mark_rgba=tuple(colour(r) for r in rows), bone_rgba=tuple(colour(r) for r in rows if par[r] >= row0), r16=r16, w16=w16,
                        min_score=min_score, heat_rgba=heat_rgba)


def overlay_isqrt(n):
    """floor(sqrt(n)) of int64 values 0 <= n < 2^52: the float64 square root truncated, then one integer correction step each way"""
    import numpy as np
    n = np.asarray(n, dtype=np.int64)
    r = np.sqrt(n.astype(np.float64)).astype(np.int64)
    r = r - (r * r > n)
    return r + ((r + 1) * (r + 1) <= n)


def overlay_blend(c, colour, t):
    """one channel under one layer: (c (65536 - t) + colour t + 32768) >> 16 with t = coverage (0 .. 256) * alpha (0 .. 255); t = 0 returns c"""
    return (c * (65536 - t) + colour * t + 32768) >> 16


def overlay_eligible(marks, min_score):
    """which marks [..., 4] = (x, y, score, _) float32 are drawn: score >= min_score in float32 (false on a NaN), x and y finite, |x|, |y| < 32768"""
    import numpy as np
    m = np.asarray(marks, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (m[..., 2] >= np.float32(min_score)) & (np.abs(m[..., 0]) < np.float32(OVERLAY_MARK_LIMIT)) & (np.abs(m[..., 1]) < np.float32(OVERLAY_MARK_LIMIT))


def _overlay_coverage(d, half16):
    import numpy as np
    return np.clip(half16 + 8 - d, 0, 16) * 16


def overlay_u8(left8, right8, style: OverlayStyle, marks=None, heat8=None, taps=None):
    """What egotap_overlay_u8 writes, restated in numpy integers: canvases uint8 [B, Hc, Wc, 3] (``right8`` None: one eye, E = 1, else E = 2) -> the
    canvases with three layers blended on, in this order: the heat, the bones in ascending index, the marks in ascending index.  Every layer
    changes every channel by ``overlay_blend`` with t = coverage * alpha.

      heat   ``heat8`` uint8 [B, E, S, S] (``heat_u8``) and ``taps`` = per eye (x table int32 [Wc], y table int32 [Hc]) from ``overlay_taps``:  a pixel
             whose x or y entry is -1 is left alone;  otherwise A = (wy0 (wx0 p00 + wx1 p01) + wy1 (wx0 p10 + wx1 p11) + 2^21) >> 22 over the four
             taps (the sensor front ends' blend of one byte), t = A * heat alpha, the one heat colour
      marks  ``marks`` float32 [B, E, M, 4] = (x, y, score, _) in canvas pixels (pixel centres at X + 0.5), ``overlay_eligible``;  in sixteenths:
             mx = rint(16 x), my = rint(16 y) (ties to even), pixel centre (16 X + 8, 16 Y + 8), d = isqrt(dx^2 + dy^2) (a floor),
             coverage = clamp(r16 + 8 - d, 0, 16) * 16, colour and alpha of the mark's palette row
      bones  a bone (i, j) is drawn when both marks are eligible;  a, b their sixteenths, e = b - a, dd = e . e, s = (p - a) . e:
             dd == 0 or s <= 0: d = the distance to a as above;  s >= dd: to b;  otherwise d = |cross(p - a, e)| div isqrt(dd);
             coverage = clamp(w16 + 8 - d, 0, 16) * 16, colour and alpha of the bone's palette row
    Every intermediate is an integer below 2^42.  Returns (out_left, out_right or None) as numpy arrays."""
    import numpy as np
    eyes = [np.asarray(left8)] + ([np.asarray(right8)] if right8 is not None else [])
    E = len(eyes)
    for c in eyes:
        if c.dtype != np.uint8 or c.ndim != 4 or c.shape[3] != 3 or c.shape != eyes[0].shape:
            raise ValueError(f"overlay_u8: canvases are uint8 [B, Hc, Wc, 3] of one shape, got {[(str(e.dtype), e.shape) for e in eyes]}")
    B, Hc, Wc, _ = eyes[0].shape
    M, L = len(style.mark_rgba), len(style.bones)
    if marks is None:
        if M or L:
            raise ValueError("overlay_u8: the style has marks or bones and no marks are given")
    else:
        marks = np.asarray(marks, dtype=np.float32)
        if marks.shape != (B, E, M, 4):
            raise ValueError(f"overlay_u8: marks are [B, E, M, 4] = {(B, E, M, 4)}, got {marks.shape}")
    if heat8 is not None:
        heat8 = np.asarray(heat8)
        if heat8.dtype != np.uint8 or heat8.ndim != 4 or heat8.shape[:2] != (B, E) or heat8.shape[2] != heat8.shape[3]:
            raise ValueError(f"overlay_u8: heat8 is uint8 [B, E, S, S] with (B, E) = {(B, E)}, got {heat8.dtype} {heat8.shape}")
        if taps is None or len(taps) != E or any(np.asarray(tx).shape != (Wc,) or np.asarray(ty).shape != (Hc,) for tx, ty in taps):
            raise ValueError(f"overlay_u8: taps are per eye (x table [{Wc}], y table [{Hc}]) from overlay_taps")
    px = (16 * np.arange(Wc, dtype=np.int64) + 8).reshape(1, Wc)
    py = (16 * np.arange(Hc, dtype=np.int64) + 8).reshape(Hc, 1)

    def layer(acc, cov, rgba):
        t = (cov * rgba[3]).astype(np.int64)[..., None]
        return overlay_blend(acc, np.asarray(rgba[:3], dtype=np.int64), t)

    def dist(ax, ay):
        dx, dy = px - ax, py - ay
        return overlay_isqrt(dx * dx + dy * dy)

    outs = []
    for e, canvas in enumerate(eyes):
        out = np.empty_like(canvas)
        for b in range(B):
            acc = canvas[b].astype(np.int64)
            if heat8 is not None:
                S = heat8.shape[2]
                tx, ty = (np.asarray(t, dtype=np.int64) for t in taps[e])
                ok = (ty >= 0).reshape(Hc, 1) & (tx >= 0).reshape(1, Wc)
                ix0, wx1 = np.where(tx >= 0, tx & 0xffff, 0), np.where(tx >= 0, tx >> 16, 0)
                iy0, wy1 = np.where(ty >= 0, ty & 0xffff, 0), np.where(ty >= 0, ty >> 16, 0)
                ix1, iy1 = np.minimum(ix0 + 1, S - 1), np.minimum(iy0 + 1, S - 1)
                wx0, wy0 = (RESIZE_WEIGHT_ONE - wx1).reshape(1, Wc), (RESIZE_WEIGHT_ONE - wy1).reshape(Hc, 1)
                h = heat8[b, e].astype(np.int64)
                top = wx0 * h[iy0][:, ix0] + wx1.reshape(1, Wc) * h[iy0][:, ix1]
                bot = wx0 * h[iy1][:, ix0] + wx1.reshape(1, Wc) * h[iy1][:, ix1]
                A = (wy0 * top + wy1.reshape(Hc, 1) * bot + (1 << 21)) >> 22
                acc = layer(acc, np.where(ok, A, 0), style.heat_rgba)
            if M:
                m = marks[b, e]
                elig = overlay_eligible(m, style.min_score)
                with np.errstate(invalid="ignore", over="ignore"):
                    q = np.where(elig[:, None], np.rint(np.float32(16) * np.where(elig[:, None], m[:, :2], np.float32(0))), 0).astype(np.int64)
                for l, (i, j) in enumerate(style.bones):
                    if not (elig[i] and elig[j]):
                        continue
                    ax, ay, bx, by = int(q[i, 0]), int(q[i, 1]), int(q[j, 0]), int(q[j, 1])
                    ex, ey = bx - ax, by - ay
                    dd = ex * ex + ey * ey
                    if dd == 0:
                        d = dist(ax, ay)
                    else:
                        s = (px - ax) * ex + (py - ay) * ey
                        cross = np.abs((px - ax) * ey - (py - ay) * ex)
                        d = np.where(s <= 0, dist(ax, ay), np.where(s >= dd, dist(bx, by), cross // int(overlay_isqrt(dd))))
                    acc = layer(acc, _overlay_coverage(d, style.w16), style.bone_rgba[l])
                for j in range(M):
                    if elig[j]:
                        acc = layer(acc, _overlay_coverage(dist(int(q[j, 0]), int(q[j, 1])), style.r16), style.mark_rgba[j])
            out[b] = acc.astype(np.uint8)
        outs.append(out)
    return outs[0], (outs[1] if E == 2 else None)
