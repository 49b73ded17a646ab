"""Host-side mirror of the reference's network modules for the hot path.

Same class names, constructor arguments, forward signatures and ``state_dict`` keys as
``model/net_architecture.py`` in the reference, so ``train.py``/``test.py``-style callers and released
checkpoints work unchanged -- but the modules hold parameters only: every forward goes through the
C ABI of libegotap_hip.so (hand-written HIP for gfx950).  There is no PyTorch compute fallback; without
the HIP library or off the GPU these modules raise.
"""
from __future__ import annotations

import ctypes as C
import types

import torch
import torch.nn as nn

from . import lib as _lib
from . import session as _session
from . import spec as _spec
from .session import ptr, stream


class _Node(nn.Module):
    """Parameter container; the tree of _Nodes reproduces the reference's dotted state_dict keys."""

    def forward(self, *a, **k):  # pragma: no cover - containers are never called
        raise RuntimeError("parameter container: compute happens in libegotap_hip.so")


def _build_tree(root: nn.Module, entries):
    """Register (key, shape) entries as nn.Parameter / buffers under nested _Node children of root."""
    for key, shape in entries:
        parts = key.split(".")
        mod = root
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, _Node())
            mod = mod._modules[p]
        leaf = parts[-1]
        if leaf == "num_batches_tracked":
            mod.register_buffer(leaf, torch.zeros(shape, dtype=torch.long))
        elif _spec.is_buffer(key):
            mod.register_buffer(leaf, torch.ones(shape) if leaf == "running_var" else torch.zeros(shape))
        else:
            mod.register_parameter(leaf, nn.Parameter(torch.zeros(shape)))


def _kaiming_init_(module: nn.Module):
    """init_net(net, 'kaiming') of the reference (network_utils.py:37-58): kaiming-normal (fan_in) on every
    Conv/Linear weight, zero bias; everything else keeps its constructor default.  Uses torch's RNG."""
    for name, p in module.named_parameters():
        leaf = name.rsplit(".", 1)[-1]
        with torch.no_grad():
            if leaf == "weight" and p.dim() >= 2:
                nn.init.kaiming_normal_(p, a=0, mode="fan_in")
            elif leaf == "weight":            # LayerNorm / BatchNorm1d gain
                p.fill_(1.0)
            elif leaf == "bias":
                p.zero_()
            elif leaf in ("cls_token", "position_embeddings"):
                nn.init.trunc_normal_(p, mean=0.0, std=0.02)
            elif leaf == "mask_token":
                p.zero_()


class _FrozenWeights:
    """Opt-in frozen-weight serving in the "bf16" mode (egotap.h, frozen-weight serving): ``freeze_weights()`` prepares every weight once, in one
    launch, into an arena the module owns; the eval-mode forwards then read the arena and launch no weight preparation -- same bits.

    Staleness: ``.train()`` and ``set_precision`` unfreeze.  Every frozen forward compares ``data_ptr()`` and ``_version`` of the frozen tensors
    with what it recorded at the freeze and re-runs the one launch (into the same arena) when one moved: optimizer steps, ``load_state_dict``,
    ``copy_``, ``mul_`` ... all bump ``_version``.  Writes through ``.data`` (and raw device writes) do NOT: call ``refresh_frozen_weights()``
    after those.  Subclasses give _frozen_tensors(), _frozen_bytes(), _frozen_launch(arena, dev) and _frozen_release()."""

    _frozen_sig = None          # None: not frozen; else ((data_ptr, _version), ...) of the frozen tensors at the last freeze
    _frozen_arena = None
    _frozen_list = None

    @property
    def weights_frozen(self) -> bool:
        return self._frozen_sig is not None

    def _frozen_device(self):
        dev = next(self.parameters()).device
        if dev.type != "cuda":
            raise _lib.EgotapError("freeze_weights: the module is on the CPU; the prepared weights live on the GPU (no CPU fallback)")
        return dev

    def freeze_weights(self, *args, **kwargs):
        dev = self._frozen_device()
        if self.training:
            raise _lib.EgotapError("freeze_weights: the module is in train mode (training never reads the prepared weights): call .eval() first")
        if self.precision != "bf16":
            raise _lib.EgotapError(f"freeze_weights: nothing to freeze in precision {self.precision!r}: only 'bf16' prepares "
                                   "weights per forward (f32 / bf16x3 read the live parameters)")
        with torch.cuda.device(dev):
            self._frozen_prepare(*args, **kwargs)
            self._bind(dev)
            need = self._frozen_bytes()
            if self._frozen_arena is None or self._frozen_arena.numel() != need or self._frozen_arena.device != dev:
                self._frozen_arena = torch.empty(need, dtype=torch.uint8, device=dev)
            self._frozen_run(dev)
        return self

    def _frozen_prepare(self):
        pass

    def _frozen_run(self, dev):
        if self._frozen_arena.device != dev:
            self._frozen_arena = torch.empty(self._frozen_arena.numel(), dtype=torch.uint8, device=dev)
        self._frozen_list = self._frozen_tensors()
        self._frozen_launch(self._frozen_arena, dev)
        self._frozen_sig = tuple((t.data_ptr(), t._version) for t in self._frozen_list)

    def refresh_frozen_weights(self):
        """prepare the weights again from the live parameters, into the same arena (a graph captured while frozen stays valid)"""
        if not self.weights_frozen:
            raise _lib.EgotapError("refresh_frozen_weights: the module is not frozen")
        dev = self._frozen_device()
        with torch.cuda.device(dev):
            self._bind(dev)
            self._frozen_run(dev)
        return self

    def unfreeze_weights(self):
        if self._frozen_sig is not None:
            if self._abi is not None:
                self._frozen_release()
            self._frozen_sig = self._frozen_arena = self._frozen_list = None
        return self

    def _frozen_check(self, dev):
        """every frozen eval forward, after _bind: one tuple compare; the one launch again when a frozen tensor moved or was written"""
        if self._frozen_sig != tuple((t.data_ptr(), t._version) for t in self._frozen_list):
            self._frozen_run(dev)

    def train(self, mode: bool = True):
        if mode:
            self.unfreeze_weights()
        return super().train(mode)


class _AbiModule(_FrozenWeights):
    """What both network modules do with the C ABI, on one session.Handle of their own (created at the first use): binding, the grow-only
    workspace ``_ws``, the precision mode and views of the last forward's intermediates.  Subclasses give ``_net`` (the net id their
    tensors are bound under), ``_intermediate_query`` (the ABI's query by name), _new_handle() and _bound_tensors()."""

    def __init__(self):
        super().__init__()
        self._abi = None
        self._ws = None
        self.precision = "f32"

    def _ensure_handle(self):
        if self._abi is None:
            self._abi = self._new_handle()
        return self._abi.h

    def _bind(self, device):
        self._ensure_handle()
        return self._abi.bind(self._net, self._bound_tensors(), device)

    def set_precision(self, mode: str = "f32"):
        if mode not in _lib.PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_lib.PRECISIONS)}")
        self.unfreeze_weights()        # prepared weights belong to a mode (the library unfreezes the handle too)
        _lib.check(_lib.load().egotap_set_precision(self._ensure_handle(), _lib.PRECISIONS[mode]))
        self.precision = mode
        return self

    def intermediate(self, name: str, B: int):
        """View of an intermediate of the LAST forward inside the workspace (parity tests)."""
        self._ensure_handle()
        return self._abi.intermediate(getattr(_lib.load(), self._intermediate_query), self._ws, B, name=name)


class EgoTAPAutoEncoder(_AbiModule, nn.Module):
    """Heatmaps -> 3D pose lifting head (reference: model/net_architecture.py:579-758).

    forward(input[B, 6J, S, S]) -> (pose[B, J(+1), 3], rot zeros[B, 3J], indep_pos zeros[B, 6J],
    reconstructed-heatmap zeros[B, 6J, S, S]) -- the last three are all-zero in the reference too
    (net_architecture.py:718-719, 756); they are returned as cached / broadcast zeros, not re-allocated.
    """
    _net = _lib.NET_LIFT
    _intermediate_query = "egotap_lift_intermediate"

    def __init__(self, opt, input_channel_scale: int = 2, fc_dim: int = 16384):
        super().__init__()
        if input_channel_scale != 2:
            raise NotImplementedError("only the stereo presets (UnrealEgo, EgoCap) are built")
        if not getattr(opt, "patched_heatmap_ae", True) or getattr(opt, "skel_layer", "PU") != "PU":
            raise NotImplementedError("only --patched_heatmap_ae --skel_layer PU (the shipped configuration) is built")
        if getattr(opt, "heatmap_type", "sin") != "sin":
            raise NotImplementedError("only --heatmap_type sin is built")
        hm = list(getattr(opt, "load_size_heatmap", [64, 64]))
        if hm[0] != hm[1]:
            raise ValueError("load_size_heatmap must be square")
        self.preset = _spec.lift_preset(opt.joint_preset, hm[0], getattr(opt, "ae_hidden_size", 128))
        if opt.num_heatmap != self.preset.n_joints_hm or opt.num_rot_heatmap != self.preset.n_joints_hm:
            raise ValueError("num_heatmap / num_rot_heatmap must match the joint preset")
        p = self.preset
        self.joint_preset = opt.joint_preset
        self.hidden_size = p.hidden
        self.num_joints = p.out_joints
        self.num_pos_heatmap = self.num_rot_heatmap = p.n_joints_hm
        self.channels_heatmap = p.in_channels
        self.W = self.H = p.hm_size
        self.rot_dim = 3 * p.n_joints_hm
        _build_tree(self, _spec.lift_state_spec(p))
        _kaiming_init_(self)
        self._zeros = {}
        # several processes on one GPU (rehearsals, tests): per-step propagation-unit kernels instead of the one-launch recurrence.  An OPTION of the
        # model (opt.shared_device); the EGOTAP_SHARED_DEVICE=1 environment switch remains for launchers that cannot reach opt
        self._shared_device = bool(getattr(opt, "shared_device", False))

    # -- C-ABI plumbing ---------------------------------------------------------------------------
    def _new_handle(self):
        return _session.Handle(self.preset, shared_device=self._shared_device)      # several processes on one GPU: see set_pu_chain

    def _bound_tensors(self):
        sd = dict(self.named_parameters())
        sd.update(self.named_buffers())
        return sd

    def set_pu_chain(self, enable: bool = True):
        """The propagation units' recurrence as one launch per layer (default; its workgroups wait for each other, so the process must
        have the GPU to itself while a forward runs) or as one kernel per step (enable = False: safe on a shared device, same bits).
        EGOTAP_SHARED_DEVICE=1 in the environment selects the per-step kernels for every module of the process."""
        _lib.check(_lib.load().egotap_set_pu_chain(self._ensure_handle(), int(bool(enable))))
        return self

    def pu_chain_status(self):
        """(enabled, faults): whether this module still runs the recurrence as one launch per layer, and how many of its launches had
        to be redone on the device because their workgroups were not co-resident (egotap.h egotap_pu_chain_status; results were
        right every time -- the library switches itself to the per-step kernels after the first).  Exact after a synchronise."""
        en, nf = C.c_int(), C.c_int()
        _lib.check(_lib.load().egotap_pu_chain_status(self._ensure_handle(), C.byref(en), C.byref(nf)))
        return bool(en.value), nf.value

    # -- frozen-weight serving (see _FrozenWeights) --------------------------------------------------
    def _frozen_tensors(self):
        """what egotap_lift_freeze keeps a prepared copy of: the weights of the patch projection, of the ViT blocks' six Linear layers and of the
        two fc1 (bf16 copies), and the q / k / v biases (fused per block)"""
        return [t for k, t in self.named_parameters()
                if ".attention.attention." in k or (".encoder.layer." in k and k.endswith("dense.weight"))
                or k.endswith("patch_embeddings.projection.weight") or k.endswith("_heatmap_encoder.fc1.fc.weight")]

    def _frozen_bytes(self):
        need = _session.nbytes(_lib.load().egotap_lift_frozen_bytes, self._ensure_handle())
        if need == 0:
            raise _lib.EgotapError(f"freeze_weights: nothing to freeze: the bf16-storage forward needs a sequence that is a multiple of 32 tokens "
                                   f"(heatmap side {self.preset.hm_size}: {self.preset.seq} tokens run on fp32 tensors, which read the live parameters)")
        return need

    def _frozen_launch(self, arena, dev):
        _lib.check(_lib.load().egotap_lift_freeze(self._ensure_handle(), ptr(arena), arena.numel(), stream(dev)))

    def _frozen_release(self):
        _lib.check(_lib.load().egotap_lift_unfreeze(self._abi.h))

    def _workspace_bytes(self, B):
        return _session.nbytes(_lib.load().egotap_lift_workspace_bytes, self._ensure_handle(), B)

    def _workspace(self, B, device):
        _session.grown(self, "_ws", self._workspace_bytes(B), device)      # (the new block while the old one is held: their addresses differ)
        self._act_scratch(B, device)
        return self._ws

    def _act_scratch(self, B, device):
        """bf16 mode: scratch for the bf16 copy of a GEMM's activation operand (egotap_set_act_scratch), sized for the ViT MLP's
        hidden activations [B * seq, 4 * D] and grown with the batch"""
        if self.precision != "bf16" or device.type != "cuda":
            return
        if B * self.preset.seq >= 4096:      # the bf16-storage forward (egotap_lift_forward at batches that fill the chip) converts nothing
            return
        cur = getattr(self, "_ascratch", None)
        buf = _session.grown(self, "_ascratch", 2 * B * self.preset.seq * 4 * self.preset.vit_dim, device)
        if buf is not cur:
            _lib.check(_lib.load().egotap_set_act_scratch(self._ensure_handle(), ptr(buf), buf.numel()))

    def _reducer(self):
        """the overlapped gradient reducer of this module's training Function (egotap_amd.parallel.GradReducer; a no-op for one rank)"""
        if getattr(self, "_grad_reducer", None) is None:
            from .parallel import GradReducer
            self._grad_reducer = GradReducer()
        return self._grad_reducer

    def set_precision(self, mode: str = "f32"):
        """Arithmetic of the large GEMMs (egotap.h egotap_set_precision): "f32" = exact fp32 MFMA (default),
        "bf16x3" = fp32 operands split into hi + lo bf16, three bf16 MFMAs per product, fp32 accumulate (opt-in fast mode)."""
        super().set_precision(mode)
        if mode == "bf16":             # scratch for the bf16 copy of a GEMM's weights (largest: fc1 of the position encoder)
            dev = next(self.parameters()).device
            if dev.type == "cuda" and (getattr(self, "_wscratch", None) is None or self._wscratch.device != dev):
                need = 2 * max(p.numel() for p in self.parameters() if p.dim() >= 2)
                self._wscratch = torch.empty(need, dtype=torch.uint8, device=dev)
            if getattr(self, "_wscratch", None) is not None:
                _lib.check(_lib.load().egotap_set_weight_scratch(self._ensure_handle(), ptr(self._wscratch), self._wscratch.numel()))
        else:                          # the activation scratch is (re)attached by the next forward in bf16 mode (_act_scratch)
            self._ascratch = None
            _lib.check(_lib.load().egotap_set_act_scratch(self._ensure_handle(), None, 0))
        return self

    # -- reference API ----------------------------------------------------------------------------
    def predict_pose(self, input, input_rgb_left=None, input_rgb_right=None):
        return self.forward(input, input_rgb_left, input_rgb_right, pose_only=True)

    def _check_heatmaps(self, input):
        p = self.preset
        if not input.is_cuda:
            raise _lib.EgotapError("EgoTAPAutoEncoder runs on the GPU only (no CPU fallback); move the input to cuda")
        if input.dim() != 4 or tuple(input.shape[1:]) != (p.in_channels, p.hm_size, p.hm_size):
            raise ValueError(f"expected input [B, {p.in_channels}, {p.hm_size}, {p.hm_size}], got {tuple(input.shape)}")

    def forward(self, input, input_rgb_left=None, input_rgb_right=None, pose_only=False):
        p = self.preset
        self._check_heatmaps(input)
        if self.training:
            from .training import lift_train_forward          # training mode: batch-statistics BatchNorm, differentiable
            pose = lift_train_forward(self, input)
            return pose if pose_only else (pose,) + self._zero_outputs(input.shape[0], input.device)[1:]
        hm = input.detach()
        if hm.dtype != torch.float32:
            hm = hm.float()
        hm = hm.contiguous()
        B = hm.shape[0]
        dev = hm.device
        pose = torch.empty((B, p.out_joints, 3), dtype=torch.float32, device=dev)
        if B > 0:
            with torch.cuda.device(dev):
                self._bind(dev)
                if self._frozen_sig is not None:
                    self._frozen_check(dev)
                ws = self._workspace(B, dev)
                # predict_pose: the pose-only entry (same bits; the last ViT layer skips the rows fc1 never reads), forward(): every intermediate
                entry = _lib.load().egotap_lift_predict_pose if pose_only else _lib.load().egotap_lift_forward
                _lib.check(entry(self._ensure_handle(), ptr(hm), B, ptr(pose), ptr(ws), ws.numel(), stream(dev)))
        if pose_only:
            return pose
        return (pose,) + self._zero_outputs(B, dev)[1:]

    def predict_pose_graphed(self, input):
        """predict_pose through a captured HIP graph (serving at small batches, where the ~130 launches of a forward cost more than
        the kernels): the forward is captured once per (batch, device, precision, parameter pointers, frozen arena) with a static input
        and output buffer and replayed afterwards -- same kernels, same bits (tests/test_gpu_lift.py).  [r6] Captures the pose-only entry
        (egotap_lift_predict_pose), as predict_pose runs it.  Eval mode only; the returned
        tensor is the graph's static output buffer (valid until the next call with the same batch)."""
        if self.training:
            raise RuntimeError("predict_pose_graphed is an inference path: call .eval() first")
        self._check_heatmaps(input)
        dev = input.device
        self._bind(dev)
        if self._frozen_sig is not None:               # stale prepared weights are redone here, into the same arena, ahead of the replay
            with torch.cuda.device(dev):
                self._frozen_check(dev)
        B = input.shape[0]
        # the frozen state (and its arena) is part of the key: a graph captured while frozen holds no preparation kernels and reads that arena
        key = (B, str(dev), self.precision, self._abi.bound[self._net], self._frozen_arena.data_ptr() if self.weights_frozen else None)

        def build():
            # Every pointer a captured launch takes is baked into the graph, so the graph OWNS what it replays into: a workspace of
            # its own (the module's grow-only self._ws is replaced -- and the old one handed back to the allocator -- as soon as a
            # larger batch arrives) and references to the bf16 scratch buffers attached to the handle at capture time (replaced, not
            # resized, when they grow; their contents are transient within one launch, so sharing them between graphs is fine).
            lib, h = _lib.load(), self._ensure_handle()
            static_in = input.detach().float().contiguous().clone()
            static_out = torch.empty((B, self.preset.out_joints, 3), dtype=torch.float32, device=dev)
            self.predict_pose(static_in)                   # eager once: lazy occupancy queries and allocations happen here
            ws = torch.empty(self._workspace_bytes(B), dtype=torch.uint8, device=dev)
            self._act_scratch(B, dev)
            keep = (ws, getattr(self, "_ascratch", None), getattr(self, "_wscratch", None), self._frozen_arena if self.weights_frozen else None)
            return (lambda: _lib.check(lib.egotap_lift_predict_pose(h, ptr(static_in), B, ptr(static_out), ptr(ws), ws.numel(), stream(dev))),
                    (static_in, static_out), keep)
        with torch.cuda.device(dev):
            graph, (static_in, static_out), _ = _session.captured(self.__dict__.setdefault("_graphs", {}), key, build)
        static_in.copy_(input)
        graph.replay()
        return static_out

    def _zero_outputs(self, B, dev):
        """(None, rot, indep_pos, reconstructed heatmaps): the reference's all-zero outputs, cached / broadcast"""
        p = self.preset
        key = (B, str(dev))
        if key not in self._zeros:
            z = torch.zeros((), dtype=torch.float32, device=dev)
            self._zeros = {key: (torch.zeros((B, self.rot_dim), device=dev), torch.zeros((B, 6 * p.n_joints_hm), device=dev),
                                 z.expand(B, p.in_channels, p.hm_size, p.hm_size))}
        rot, indep, out_hm = self._zeros[key]
        return None, rot, indep, out_hm


class HeatMap_UnrealEgo_Shared(_AbiModule, nn.Module):
    """Stereo heatmap estimator (reference: model/net_architecture.py:25-173 over torchvision resnet18).

    forward(left[B,3,256,256], right[B,3,256,256]) -> [B, 2*n_hm, 64, 64] (left maps then right maps); in eval mode any heatmap side S
    that is a multiple of 16 runs ([B,3,4S,4S] -> [B, 2*n_hm, S, S]), train mode and the batch-statistics forward at S = 64 / 128.
    The state_dict has the reference's 258 keys, including the duplicate ``backbone.backbone.layerK.*`` views of
    the ResNet tensors (the same nn.Parameter objects registered under both paths, as in the reference).
    ``forward_into(left, right, out)`` writes the result into a channel slice of a larger tensor instead
    (used by the wrapper to build the lifting head's input without torch.cat).
    """
    _intermediate_query = "egotap_hm_intermediate"

    def __init__(self, opt, model_name: str = "resnet18", input_channel_scale: int = 2):
        super().__init__()
        self.model_name = model_name
        # resnet18 / resnet34 (BasicBlocks: one-call C forward, bf16 modes, stage-1 training) or resnet50 / resnet101 (Bottleneck blocks,
        # feature_scale 4: fp32 eval forward composed from the operator entry points, _forward_bottleneck)
        self.bottleneck = _spec.hm_is_bottleneck(model_name)
        self.blocks = _spec.hm_all_blocks(model_name)
        if input_channel_scale != 2:
            raise NotImplementedError("only the stereo presets are built")
        limb = {"none": 0, "sin": 2, "limb": 1}[getattr(opt, "heatmap_type", "none")]
        self.num_heatmap = opt.num_heatmap + opt.num_rot_heatmap * limb
        hm = list(getattr(opt, "load_size_heatmap", [64, 64]))
        self.hm_size = hm[0]
        self.preset = _spec.lift_preset(opt.joint_preset, hm[0], getattr(opt, "ae_hidden_size", 128))
        self._rgb_opt = types.SimpleNamespace(rgb_mean=getattr(opt, "rgb_mean", None), rgb_std=getattr(opt, "rgb_std", None))
        J = self.preset.n_joints_hm
        if self.num_heatmap == J:
            self._net = _lib.NET_HM_POS
        elif self.num_heatmap == 2 * J:
            self._net = _lib.NET_HM_ROT
        else:
            raise ValueError("heatmap estimator must be the position net (num_rot_heatmap=0) or the sin/cos net (num_heatmap=0)")
        entries = _spec.hm_state_spec(self.num_heatmap, model_name)
        _build_tree(self, [(k, s) for k, s, a in entries if a is None])
        for k, s, a in entries:                      # aliases: same Parameter / buffer object under a second path
            if a is None:
                continue
            src_mod, src_leaf = self._locate(a)
            parts = k.split(".")
            mod = self
            for part in parts[:-1]:
                if part not in mod._modules:
                    mod.add_module(part, _Node())
                mod = mod._modules[part]
            if src_leaf in src_mod._parameters:
                mod.register_parameter(parts[-1], src_mod._parameters[src_leaf])
            else:
                mod.register_buffer(parts[-1], src_mod._buffers[src_leaf])
        self._aliases = [(k, a) for k, s, a in entries if a is not None]
        _kaiming_init_(self)

    def _apply(self, fn, *args, **kwargs):
        """Module._apply (.to / .cuda / .float ...) replaces every registered BUFFER by fn(buffer) -- once per registration, so the
        ``backbone.backbone.layerK.*`` aliases of the BatchNorm statistics would stop being the tensors the forward updates (parameters keep
        their identity: torch swaps .data).  In the reference the aliases are the same nn.BatchNorm2d MODULES (net_architecture.py:68-73), so they
        can never drift apart, and its load_state_dict reads the alias keys LAST: a checkpoint written with stale aliases would load stale
        statistics there.  Re-tie them after every _apply."""
        super()._apply(fn, *args, **kwargs)
        for k, a in getattr(self, "_aliases", ()):
            src_mod, src_leaf = self._locate(a)
            mod, leaf = self._locate(k)
            if src_leaf in src_mod._buffers:
                mod._buffers[leaf] = src_mod._buffers[src_leaf]
        if self._abi is not None:
            self._abi.bound.pop(self._net, None)
        if self._frozen_sig is not None:
            self._frozen_sig = ()          # the buffers are new objects: the next frozen forward lists the tensors again and re-freezes
        return self

    def set_precision(self, mode: str = "f32"):
        """Arithmetic of the 3x3 stride-1 convolutions with >= 128 output channels (88 % of the FLOPs): "f32" exact (default),
        "bf16x3" split operands, "bf16" rounded operands; everything else stays fp32 (egotap.h egotap_set_precision)."""
        if self.bottleneck and mode in _lib.PRECISIONS and mode != "f32":
            raise NotImplementedError(f"backbone {self.model_name!r} runs in fp32 only (the bf16 modes cover resnet18 / resnet34)")
        return super().set_precision(mode)

    def _locate(self, key):
        parts = key.split(".")
        mod = self
        for part in parts[:-1]:
            mod = mod._modules[part]
        return mod, parts[-1]

    # -- frozen-weight serving (see _FrozenWeights) --------------------------------------------------
    def freeze_weights(self, batch: int = 1):
        """Keep this estimator's packed convolution weights, padded biases and folded BatchNorms (running statistics) for ``forward_into`` /
        the eval forward.  The packed layout depends on the batch (which convolutions run split over K): the arena is built for ``batch``;
        a forward at a batch with another layout packs per call as if not frozen (the library decides per call; same bits either way)."""
        if self.bottleneck:
            raise _lib.EgotapError(f"freeze_weights: nothing to freeze: backbone {self.model_name!r} runs in fp32 only (no bf16 mode, no packed weights)")
        return super().freeze_weights(batch)

    def _frozen_prepare(self, batch: int = 1):
        if int(batch) < 1:
            raise ValueError("freeze_weights: batch must be positive")
        self._frozen_batch = int(batch)

    def _frozen_tensors(self):
        """everything pack_all_bf16s_kernel reads: every convolution weight / bias and BatchNorm tensor except the stem's (read live); the
        ResNet's classifier (fc) is never read at all"""
        sd = self.state_dict(keep_vars=True)
        bb = "backbone.backbone.backbone."
        seen = {id(t) for k, t in sd.items() if k.startswith((bb + "conv1.", bb + "bn1.", bb + "fc."))}
        out = []
        for k, t in sd.items():
            if id(t) not in seen and t.dtype == torch.float32:
                seen.add(id(t))
                out.append(t)
        return out

    def _frozen_bytes(self):
        need = _session.nbytes(_lib.load().egotap_hm_frozen_bytes, self._ensure_handle(), self._net, self._frozen_batch)
        if need == 0:
            raise _lib.EgotapError(f"freeze_weights: nothing to freeze at heatmap side {self.hm_size}: the bf16 channels-last path exists at sides "
                                   "64 and 128; every other side runs the exact-fp32 path, which reads the live parameters")
        return need

    def _frozen_launch(self, arena, dev):
        _lib.check(_lib.load().egotap_hm_freeze(self._ensure_handle(), self._net, self._frozen_batch, ptr(arena), arena.numel(), stream(dev)))

    def _frozen_release(self):
        _lib.check(_lib.load().egotap_hm_unfreeze(self._abi.h, self._net))

    def _new_handle(self):
        # Bottleneck nets never bind to the handle's one-call forward (it only carries the operator calls): default block counts
        return _session.Handle(self.preset, hm_blocks=(2, 2, 2, 2) if self.bottleneck else self.blocks)

    def _bound_tensors(self):
        return self.state_dict(keep_vars=True)          # the ``backbone.backbone.layerK.*`` aliases under both names

    def _workspace(self, B, device):
        need = _session.nbytes(_lib.load().egotap_hm_workspace_bytes, self._ensure_handle(), B)
        return _session.grown(self, "_ws", need, device, drop_first=True)

    def _check_stereo_io(self, left, right, out, channel_offset):
        """left / right [B, 3, 4S, 4S] and an `out` that holds channels [channel_offset, channel_offset + 2 n_hm) of B maps; returns B"""
        for t in (left, right, out):
            if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
                raise _lib.EgotapError("heatmap estimator needs contiguous float32 CUDA tensors (no CPU fallback)")
        B, S = left.shape[0], 4 * self.hm_size
        if tuple(left.shape) != (B, 3, S, S) or tuple(right.shape) != (B, 3, S, S):
            raise ValueError(f"expected left/right [B, 3, {S}, {S}], got {tuple(left.shape)} / {tuple(right.shape)}")
        if out.dim() != 4 or out.shape[0] != B or out.shape[2] != self.hm_size or out.shape[3] != self.hm_size \
                or channel_offset + 2 * self.num_heatmap > out.shape[1]:
            raise ValueError("output tensor does not hold the requested channel slice")
        return B

    def _out_slice(self, out, channel_offset):
        """(address of out[0, channel_offset], elements between two frames of out) as the estimator entries take them"""
        hw = self.hm_size * self.hm_size
        return ptr(out, 4 * channel_offset * hw), out.shape[1] * hw

    def forward_into(self, left, right, out, channel_offset: int = 0, workspace=None):
        """Write this net's [B, 2*n_hm, S, S] output into out[:, channel_offset : channel_offset + 2*n_hm]."""
        if self.training:
            raise NotImplementedError("forward_into writes the eval-mode result (folded BatchNorm) into a caller's slice; in train mode call the module itself (differentiable path) or .eval() first")
        B = self._check_stereo_io(left, right, out, channel_offset)
        if B == 0:
            return out
        dev = left.device
        if self.bottleneck:
            with torch.cuda.device(dev):
                self._forward_bottleneck(left, right, out, channel_offset)
            return out
        with torch.cuda.device(dev):
            self._bind(dev)
            if self._frozen_sig is not None:
                self._frozen_check(dev)
            ws = workspace if workspace is not None else self._workspace(B, dev)
            self._ws = ws
            _lib.check(_lib.load().egotap_hm_forward(self._ensure_handle(), self._net, ptr(left), ptr(right), B, *self._out_slice(out, channel_offset),
                                                     ptr(ws), ws.numel(), stream(dev)))
        return out

    def camera_table(self, device):
        """the fp32 [3, 256] value table of the byte entries on `device` (spec.rgb_u8_table with this net's opt.rgb_mean / opt.rgb_std): one
        small tensor the module owns -- the library allocates nothing.  The statistics are read ONCE, when the module is constructed (a module keeps no
        opt); a model that changes them builds a new estimator, or goes through EgoTAPAutoEncoderModel.camera_table, which follows its opt"""
        t = self.__dict__.get("_camera_table")
        if t is None or t.device != device:
            t = self._camera_table = torch.from_numpy(_spec.rgb_u8_table(self._rgb_opt)).to(device)
        return t

    @torch.no_grad()
    def forward_from_camera(self, left8, right8):
        """The eval forward from camera bytes (egotap.h egotap_hm_forward_u8): left8 / right8 uint8 [B, 4S, 4S, 3] (HWC, RGB) -> [B, 2*n_hm, S, S],
        bit for bit the eval forward on the normalised frames table[c][byte].  At sides 64 / 128 the stem kernels stage the bytes themselves; at
        every other side the library converts them into a workspace slice first.  Eval mode only (the train-mode forwards keep their fp32 source).
        resnet50 / resnet101 (composed on the host): egotap_rgb_u8_to_f32, then the module forward -- by name."""
        if self.training:
            raise NotImplementedError("forward_from_camera is the eval-mode forward (folded BatchNorm); .eval() first -- training reads normalised fp32 frames")
        S0 = 4 * self.hm_size
        B = _lib.check_camera_frames("forward_from_camera", left8, right8, S0)
        dev = left8.device
        out = torch.empty((B, 2 * self.num_heatmap, self.hm_size, self.hm_size), dtype=torch.float32, device=dev)
        if B == 0:
            return out
        table = self.camera_table(dev)
        if self.bottleneck:
            left, right = _lib.rgb_u8_to_f32(left8, right8, table)
            return self.forward_into(left, right, out)
        lib = _lib.load()
        with torch.cuda.device(dev):
            self._bind(dev)
            if self._frozen_sig is not None:
                self._frozen_check(dev)
            need = _session.nbytes(lib.egotap_hm_forward_u8_workspace_bytes, self._ensure_handle(), B)
            ws = self._ws = _session.grown(self, "_ws", need, dev, drop_first=True)
            _lib.check(lib.egotap_hm_forward_u8(self._ensure_handle(), self._net, ptr(left8), ptr(right8), B, ptr(table), *self._out_slice(out, 0),
                                                ptr(ws), ws.numel(), stream(dev)))
        return out

    @torch.no_grad()
    def forward_bnbatch_into(self, left, right, out, channel_offset: int = 0, chunk: int = 256, workspace=None):
        """forward_into with BATCH-statistics BatchNorm2d and no graph (egotap.h egotap_hm_forward_bnbatch): what a FROZEN estimator computes
        while the lifting head trains under train.py:91 model.train() -- per-eye statistics, running_mean / running_var /
        num_batches_tracked of every BatchNorm updated twice (left, right).  bf16 precision only (the bf16 channels-last kernels); the
        backbone runs over the whole batch, the decoder in pieces of `chunk` frames.  The module's own .training flag is not consulted."""
        if self.bottleneck:
            raise NotImplementedError(f"backbone {self.model_name!r}: no batch-statistics forward (resnet18 / resnet34 have one)")
        _spec.hm_check_batch_stats_side(self.hm_size, "forward_bnbatch_into (batch-statistics BatchNorm)")
        if self.precision != "bf16":
            raise _lib.EgotapError("forward_bnbatch_into runs on the bf16 channels-last kernels: set_precision('bf16') first "
                                   "(fp32 / bf16x3: hm_training.hm_train_forward_nograd)")
        B = self._check_stereo_io(left, right, out, channel_offset)
        if B < 2:
            raise ValueError("batch-statistics BatchNorm needs at least two frames")
        dev = left.device
        chunk = B if chunk is None or chunk <= 0 else min(int(chunk), B)
        with torch.cuda.device(dev):
            self._bind(dev)
            ws = workspace
            if ws is None or ws.numel() < self._bnbatch_bytes(B, chunk) or ws.device != dev:
                ws = self.bnbatch_workspace(B, chunk, dev)
            _lib.check(_lib.load().egotap_hm_forward_bnbatch(self._ensure_handle(), self._net, ptr(left), ptr(right), B, *self._out_slice(out, channel_offset),
                                                             chunk, ptr(ws), ws.numel(), stream(dev)))
            if self._frozen_sig is not None:
                self._frozen_sig = ()      # the kernels moved the running statistics without a _version bump: the next frozen forward folds them again
        return out

    def bnbatch_intermediate(self, name: str, B: int, chunk: int, ws=None):
        """bf16 view [B * s * s, 2 C] of a backbone map of the LAST forward_bnbatch_into inside its workspace (parity tests)"""
        self._ensure_handle()
        return self._abi.intermediate(_lib.load().egotap_hm_forward_bnbatch_intermediate, ws if ws is not None else self._ws_bn, B,
                                      min(chunk, B) if chunk else B, name=name, dtype=torch.bfloat16)

    def _bnbatch_bytes(self, B, chunk):
        return _session.nbytes(_lib.load().egotap_hm_forward_bnbatch_workspace_bytes, self._ensure_handle(), B, min(chunk, B) if chunk else B)

    def bnbatch_workspace(self, B, chunk, device):
        """scratch of forward_bnbatch_into for (B, chunk), kept on the module (both estimators of a wrapper can share one)"""
        return _session.grown(self, "_ws_bn", self._bnbatch_bytes(B, chunk), device, drop_first=True)

    @torch.no_grad()
    def _forward_bottleneck(self, left, right, out, channel_offset):
        """Eval forward of the resnet50 / resnet101 estimators (net_architecture.py:45-51 backbone once per eye, :75-85 pyramid, :139-173
        decoder on the channel-concatenated eyes), composed from the library's operator entry points: every convolution is one
        conv_f32 kernel launch with its BatchNorm (eval) / bias, residual and ReLU in the epilogue; images n = 2b + eye, so a stage output
        [2B, C, s, s] IS the stereo concat [B, 2C, s, s]; upsamples and 1x1 skips write channel slices of the concat buffers in place."""
        from . import hm_ops as H
        h = self._ensure_handle()
        sd = self._bound_tensors()
        _session.check_bindable(sd, left.device)
        BB, AB = "backbone.backbone.backbone.", "after_backbone."
        bn = lambda k: (sd[k + ".weight"], sd[k + ".bias"], sd[k + ".running_mean"], sd[k + ".running_var"])       # noqa: E731
        B, S0, dev = left.shape[0], left.shape[2], left.device
        N2 = 2 * B
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)     # noqa: E731
        l0 = new(N2, 64, S0 // 2, S0 // 2)
        H.stem_bn_fwd(left, right, sd[BB + "conv1.weight"], bn(BB + "bn1"), l0)
        x = new(N2, 64, S0 // 4, S0 // 4)
        H.maxpool_fwd(l0, x)
        del l0
        side, pyr = S0 // 4, []
        for i, (c, st) in enumerate(_spec.HM_STAGES, start=1):
            for b in range(self.blocks[i - 1]):
                k = f"{BB}layer{i}.{b}."
                stride = st if b == 0 else 1
                so = side // stride
                t1 = new(N2, c, side, side)
                H.conv_bn_fwd(h, x, sd[k + "conv1.weight"], bn(k + "bn1"), t1, taps=1)
                t2 = new(N2, c, so, so)
                H.conv_bn_fwd(h, t1, sd[k + "conv2.weight"], bn(k + "bn2"), t2, taps=9, stride=stride)
                idt = x
                if (k + "downsample.0.weight") in sd:
                    idt = new(N2, 4 * c, so, so)
                    H.conv_bn_fwd(h, x, sd[k + "downsample.0.weight"], bn(k + "downsample.1"), idt, taps=1, stride=stride, relu=False)
                y = new(N2, 4 * c, so, so)
                H.conv_bn_fwd(h, t2, sd[k + "conv3.weight"], bn(k + "bn3"), y, res=idt, taps=1)
                x, side = y, so
            pyr.append(x)
        L = [t.view(B, 2 * t.shape[1], t.shape[2], t.shape[3]) for t in pyr]
        f = 2 * _spec.hm_feature_scale(self.model_name)
        wb = lambda name: (sd[AB + name + ".weight"], sd[AB + name + ".bias"])      # noqa: E731
        s64, s32, s16, s8 = (t.shape[2] for t in L)
        w, bias = wb("layer4_1x1.0")
        u4 = new(B, 512 * f, s8, s8)
        H.conv_fwd(h, L[3], w, u4, bias=bias, taps=1, relu=True)
        cat3 = new(B, (512 + 258) * f, s16, s16)
        H.upsample_fwd(u4, H.View(cat3, 0, 512 * f))
        w, bias = wb("layer3_1x1.0")
        H.conv_fwd(h, L[2], w, H.View(cat3, 512 * f, 258 * f), bias=bias, taps=1, relu=True)
        x3 = new(B, 512 * f, s16, s16)
        w, bias = wb("conv_up3.0")
        H.conv_fwd(h, cat3, w, x3, bias=bias, taps=9, relu=True)
        del cat3, u4
        cat2 = new(B, (512 + 128) * f, s32, s32)
        H.upsample_fwd(x3, H.View(cat2, 0, 512 * f))
        w, bias = wb("layer2_1x1.0")
        H.conv_fwd(h, L[1], w, H.View(cat2, 512 * f, 128 * f), bias=bias, taps=1, relu=True)
        x2 = new(B, 256 * f, s32, s32)
        w, bias = wb("conv_up2.0")
        H.conv_fwd(h, cat2, w, x2, bias=bias, taps=9, relu=True)
        del cat2, x3
        cat1 = new(B, (256 + 64) * f, s64, s64)
        H.upsample_fwd(x2, H.View(cat1, 0, 256 * f))
        w, bias = wb("layer1_1x1.0")
        H.conv_fwd(h, L[0], w, H.View(cat1, 256 * f, 64 * f), bias=bias, taps=1, relu=True)
        x1 = new(B, 256 * f, s64, s64)
        w, bias = wb("conv_up1.0")
        H.conv_fwd(h, cat1, w, x1, bias=bias, taps=9, relu=True)
        w, bias = wb("conv_heatmap")
        H.conv_fwd(h, x1, w, H.View(out, channel_offset, 2 * self.num_heatmap), bias=bias, taps=1, relu=False)
        return out

    def forward(self, *inputs):
        if len(inputs) != 2:
            raise NotImplementedError("stereo input (left, right) expected")
        if not inputs[0].is_cuda:
            raise _lib.EgotapError("HeatMap_UnrealEgo_Shared runs on the GPU only (no CPU fallback)")
        if self.bottleneck and self.training:
            raise NotImplementedError(f"backbone {self.model_name!r}: the eval forward is built (fp32); train-mode BatchNorm / stage-1 training cover "
                                      "resnet18 and resnet34 -- call .eval() (the stage-2 wrapper keeps frozen estimators in eval mode)")
        if self.training and torch.is_grad_enabled():
            from .hm_training import hm_train_forward          # train mode: batch-statistics BatchNorm2d, differentiable
            return hm_train_forward(self, inputs[0], inputs[1])
        left, right = (t.detach().float().contiguous() for t in inputs)
        out = torch.empty((left.shape[0], 2 * self.num_heatmap, self.hm_size, self.hm_size), dtype=torch.float32,
                          device=left.device)
        return self.forward_into(left, right, out)
