"""The host side of one C-ABI session, each piece once: the pointer / stream casts, grow-only device buffers, the library handle with its
parameter binding and workspace views, graph capture, and the state of the one-call serving entry.  networks.py, models.py and the
operator wrappers are built on these; nothing here launches a kernel of its own."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import lib as _lib
from .lib import ptr, stream          # noqa: F401  (the two casts: defined next to the operators that use them, re-exported here)


# ----------------------------------------------------------------------------------------- grow-only buffers
def grown(owner, name, nbytes, device, floor=0, drop_first=False):
    """The uint8 buffer kept as ``owner.name``, replaced when it is missing, smaller than `nbytes` or on another device (never shrunk);
    a new one has max(nbytes, floor) bytes.  By default the new block is allocated while the old one is still held (the two never
    share an address: a captured graph or a test may tell them apart); ``drop_first`` lets go of the old block before allocating,
    which keeps the peak at one buffer."""
    buf = getattr(owner, name, None)
    if buf is None or buf.numel() < nbytes or buf.device != device:
        if drop_first:
            buf = None
            setattr(owner, name, None)
        buf = torch.empty(max(nbytes, floor), dtype=torch.uint8, device=device)
        setattr(owner, name, buf)
    return buf


class Scratch:
    """Grow-only device scratch of the operator wrappers (split-M slabs, column-sum partials ...): ``get`` returns ``buf``, at least
    `floor` bytes, reused by every call"""

    def __init__(self, floor: int = 64 << 20):
        self.buf, self.floor = None, floor

    def get(self, nbytes: int, device):
        return grown(self, "buf", nbytes, device, floor=self.floor)


# ----------------------------------------------------------------------------------------- the library handle
def nbytes(query_fn, *args):
    """a size the ABI reports through a trailing size_t*: query_fn(*args, &bytes)"""
    need = C.c_size_t()
    _lib.check(query_fn(*args, C.byref(need)))
    return need.value


def _abi_dtype(key, t, device):
    """egotap_bind_param's dtype code for one tensor; the one wording of what the ABI can bind"""
    dt = _lib.F32 if t.dtype == torch.float32 else (_lib.I64 if t.dtype == torch.long else None)
    if t.device != device or dt is None or not t.is_contiguous():
        raise _lib.EgotapError(f"parameter {key}: need a contiguous fp32 tensor (or int64 counter) on {device}; it is "
                               f"{t.dtype} on {t.device}{'' if t.is_contiguous() else ', not contiguous'}")
    return dt


def check_bindable(named_tensors, device):
    """every tensor of {key: tensor} is something the ABI can bind on `device`, or EgotapError"""
    for k, t in named_tensors.items():
        _abi_dtype(k, t, device)


class Handle:
    """One egotap handle (egotap_create ... egotap_destroy): ``h`` is what the ABI takes.  Built from a lift preset, the estimators'
    ResNet block counts (None: the library's default, resnet18) and ``shared_device``: with it, or with EGOTAP_SHARED_DEVICE=1 in the
    environment, the propagation units run as per-step kernels (egotap_set_pu_chain(0): several processes on one GPU)."""

    def __init__(self, preset, hm_blocks=None, shared_device=False):
        p = preset
        cfg = _lib.EgotapConfig(C.sizeof(_lib.EgotapConfig), p.n_joints_hm, int(p.estimate_head), p.hm_size, p.hidden, p.vit_dim, p.vit_heads,
                                p.vit_layers, p.patch, p.pu_hidden, *(() if hm_blocks is None else ((C.c_int32 * 4)(*hm_blocks),)))
        self.h = None
        self.bound = {}                # net id -> ((key, data_ptr), ...) of the tensors last bound
        h = C.c_void_p()
        _lib.check(_lib.load().egotap_create(C.byref(cfg), C.byref(h)))
        self.h = h
        if shared_device or os.environ.get("EGOTAP_SHARED_DEVICE", "0") == "1":
            _lib.check(_lib.load().egotap_set_pu_chain(h, 0))

    def __del__(self):
        try:                           # (at interpreter shutdown the library module may be gone already)
            if self.h is not None:
                h, self.h = self.h, None
                _lib.load().egotap_destroy(h)
        except Exception:
            pass

    def bind(self, net_id, named_tensors, device):
        """egotap_bind_param for every tensor of {key: tensor} -- unless the same keys at the same addresses are what this net was bound to
        last.  Every tensor is checked (device, dtype, contiguity) before the first one is bound; afterwards the forward must miss
        nothing (egotap_unbound_count).  True when anything was (re)bound."""
        sig = tuple((k, t.data_ptr()) for k, t in named_tensors.items())
        if sig == self.bound.get(net_id):
            return False
        dts = [_abi_dtype(k, t, device) for k, t in named_tensors.items()]
        lib = _lib.load()
        for (k, t), dt in zip(named_tensors.items(), dts):
            _lib.check(lib.egotap_bind_param(self.h, net_id, k.encode(), ptr(t), t.numel(), dt))
        n = C.c_int()
        _lib.check(lib.egotap_unbound_count(self.h, net_id, C.byref(n)))
        if n.value:
            raise _lib.EgotapError(f"{n.value} parameters the forward needs are not bound")
        self.bound[net_id] = sig
        return True

    def intermediate(self, query_fn, ws, *args, name, dtype=torch.float32):
        """typed view of the intermediate `name` inside the workspace `ws`: query_fn(h, *args, name, &offset, &numel) is the ABI's query"""
        off, n = C.c_size_t(), C.c_int64()
        _lib.check(query_fn(self.h, *args, name.encode(), C.byref(off), C.byref(n)))
        return ws[off.value: off.value + dtype.itemsize * n.value].view(dtype)


# ----------------------------------------------------------------------------------------- graph capture
def captured(cache, key, build, limit=8):
    """The entry (graph, statics, keep) of `cache` under `key`.  On a miss ``build()`` returns (run, statics, keep): `run` launches what
    is to be replayed, `statics` are the buffers it reads and writes (the caller copies inputs in and hands outputs out), `keep`
    everything else whose address a captured launch holds.  `run` goes once eagerly on a side stream (occupancy queries and kernel
    attributes are settled there), then into the capture; beyond `limit` entries the oldest is dropped.  Call under the device's
    ``torch.cuda.device``."""
    g = cache.get(key)
    if g is None:
        run, statics, keep = build()
        cur, side = torch.cuda.current_stream(), torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            run()
        cur.wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run()
        if len(cache) >= limit:
            cache.pop(next(iter(cache)))
        g = cache[key] = (graph, statics, keep)
    return g


# ----------------------------------------------------------------------------------------- one-call serving
class Serving:
    """What the one-call serving entry (egotap_predict_pose_rgb) keeps between calls: ONE handle with all three networks bound, the
    eager workspace and the chunk it was laid out for, and what is attached to the handle right now -- precision, the head's bf16
    scratch buffers, per network the frozen arena it reads -- plus the captured graphs."""

    def __init__(self, handle):
        self.handle = handle
        self.ws = self.chunk = self.precision = self.wscratch = self.ascratch = None
        self.frozen = [None, None, None]
        self.graphs = {}

    def __getitem__(self, name):       # tests and tools reach the state by name: m._rgb["ws"], m._rgb["graphs"]
        return getattr(self, name)
