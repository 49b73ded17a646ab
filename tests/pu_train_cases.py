"""The PU chain + pose head of the lifting head's training step as ONE case, shared by tests/test_gpu_train_ops.py, tests/test_gpu_pu_train_batches.py
and tests/test_pu_train_cases_cpu.py: the inputs, the oracle (``reference``), the C ABI run (``run_gpu``), the error measure and the gates.

Every tensor a run returns is compared: "skel" [J, B, H] (the PU output), "pose", "dposz", "drotz" and one gradient per weight of
skel_sequential_layer.*, pose_mlp.* and global_mlp.* (state_dict keys).  Importable without a GPU; nothing here is collected by pytest."""
import ctypes as C
import functools

import torch

PREFIXES = ("skel_sequential_layer.", "pose_mlp.", "global_mlp.")
PU_ORDER = ("0.x2f", "0.x2h", "0.b2h", "0.h2h", "1.x2f", "1.x2h", "1.h2h")          # the order of egotap_train_pu_bwd's grads argument
PU_PRE = "skel_sequential_layer.lstm_custom.layers."
DATA = ("skel", "pose", "dposz", "drotz")
TAIL_SCALE = 8.0      # the upstream gradient of the LAST sample is this much larger: a lost tail row cannot hide in a sum over hundreds of rows

# gates: e(k) = max|got - ref64| / max|ref64| per tensor; fp32: e(k) <= F32_FACTOR * max(e32(k), F32_FLOOR) with e32 the same
# oracle run in float32 on the CPU; bf16x3: BF16X3_FACTOR times that bound (the ratio between test_attention_fwd_bwd and its bf16x3 twin)
F32_FACTOR, F32_FLOOR, BF16X3_FACTOR = 8.0, 2.5e-7, 10.0
BF16_REL_L2, BF16_COS, BF16_FWD = 0.2, 0.98, 3e-2


def preset(name):
    from egotap_amd import spec
    return spec.lift_preset(name)


@functools.lru_cache(maxsize=None)
def weights(name):
    """float64 {key: tensor} of the stage's weights (the hash-RNG values lift_net loads: one hash per key, so only these keys are drawn)"""
    from egotap_amd import spec
    from egotap_amd.synthetic import synth_state_dict
    entries = [(k, shp) for k, shp in spec.lift_state_spec(preset(name)) if k.startswith(PREFIXES)]
    return {k: torch.from_numpy(v).double() for k, v in synth_state_dict(entries).items()}


def _rand(shape, seed, lo=-1.0, hi=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).float()


@functools.lru_cache(maxsize=None)
def inputs(name, B):
    """posz, rotz [B*2J, hid] and the upstream gradient dpose [B, out_joints, 3], fp32: every batch row its own random values"""
    p = preset(name)
    posz, rotz = _rand((B * 2 * p.n_joints_hm, p.hidden), 61), _rand((B * 2 * p.n_joints_hm, p.hidden), 62)
    dpose = _rand((B, p.out_joints, 3), 63)
    dpose[B - 1] *= TAIL_SCALE
    return posz, rotz, dpose


def _oracle(name, B, dtype, tree=False, drop_last=False):
    from oracle import lift_ref as O
    p = preset(name)
    posz, rotz, dpose = inputs(name, B)
    if drop_last:
        dpose = dpose.clone()
        dpose[B - 1] = 0.0
    leaves = {k: v.to(dtype).clone().requires_grad_(True) for k, v in weights(name).items()}
    pz, rz = posz.to(dtype).clone().requires_grad_(True), rotz.to(dtype).clone().requires_grad_(True)
    pos_j, rot_j = O.stereo_interleave(pz, B, p), O.stereo_interleave(rz, B, p)
    parents = None
    if tree:                                   # the kinematic parent lists of egotap_train_pose_loss (utils/util.py:51-52)
        parents = [0, 0, 1, 1, 2, 3, 4, 5, 2, 3, 8, 9, 10, 11, 12, 13] if p.estimate_head else [0, 0, 1, 2, 3, 4, 1, 6, 7, 8, 2, 10, 11, 12, 6, 14, 15, 16]
    skel = O.pu_chain(pos_j.transpose(0, 1), rot_j.transpose(0, 1), leaves, hidden=p.pu_hidden, tree_parents=parents)
    pose = O.pose_head(pos_j, skel, leaves, p)
    pose.backward(dpose.to(dtype))
    out = {"skel": skel.detach(), "pose": pose.detach(), "dposz": pz.grad, "drotz": rz.grad}
    out.update({k: v.grad for k, v in leaves.items()})
    return out


@functools.lru_cache(maxsize=None)
def reference(name, B, dtype=torch.float64):
    """autograd of the oracle (oracle.lift_ref: stereo_interleave, pu_chain, pose_head) in ``dtype`` on the CPU: {name: tensor}.  Computed once per
    (preset, B, dtype) and shared between tests, so nobody writes into it."""
    return _oracle(name, B, dtype)


def wrong_results(name, B):
    """three results a subtly wrong kernel would give, built from the float64 oracle: {what: (result, tensors that must miss the gate)}"""
    r64 = reference(name, B, torch.float64)
    p = preset(name)
    dropped = dict(r64)
    dropped.update({k: v for k, v in _oracle(name, B, torch.float64, drop_last=True).items() if k not in DATA})
    swapped = dict(r64)
    swapped["dposz"] = r64["dposz"].view(B, 2, p.n_joints_hm, -1).flip(1).reshape(r64["dposz"].shape)
    tree = _oracle(name, B, torch.float64, tree=True)
    return {"the last sample left out of the weight-gradient sums": (dropped, set(r64) - set(DATA)),
            "dposz with the two eyes swapped": (swapped, {"dposz"}),
            "a kinematic-tree propagation in place of the chain": (tree, {"skel", "pose"})}


def rel_err(got, ref64):
    """e(k): the maximum error normalised by the tensor's own scale"""
    got, ref64 = got.detach().cpu().double(), ref64.double()
    assert got.shape == ref64.shape, (tuple(got.shape), tuple(ref64.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float((got - ref64).abs().max() / ref64.abs().max())


@functools.lru_cache(maxsize=None)
def f32_bounds(name, B):
    """{tensor: (bound, e32)}: the fp32 gate of every tensor, from the float32 oracle's own error against the float64 one"""
    r64, r32 = reference(name, B, torch.float64), reference(name, B, torch.float32)
    e32 = {k: rel_err(r32[k], r64[k]) for k in r64}
    return {k: (F32_FACTOR * max(e, F32_FLOOR), e) for k, e in e32.items()}


def f32_gate_failures(got, name, B, factor=1.0, report=None):
    """the tensors of ``got`` that miss ``factor`` x the fp32 gate, as [(tensor, e, bound)]; report(line) gets every figure before anything is asserted"""
    r64, bad = reference(name, B, torch.float64), []
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    for k, (bound, e32) in f32_bounds(name, B).items():
        e = rel_err(got[k], r64[k])
        if report:
            report(f"{name} B={B} {k}: e = {e:.3e}, e32 = {e32:.3e}, e / max(e32, floor) = {e / max(e32, F32_FLOOR):.2f}, bound = {factor * bound:.3e}")
        if not e <= factor * bound:
            bad.append((k, e, factor * bound))
    return bad


def bf16_gate_failures(got, name, B, report=None):
    """relative L2 <= 20 % and cosine >= 0.98 per gradient tensor, the forward outputs within 3e-2 * max|ref|"""
    r64, bad = reference(name, B, torch.float64), []
    assert set(got) == set(r64), sorted(set(got) ^ set(r64))
    for k, ref in r64.items():
        a, b = got[k].detach().cpu().double().reshape(-1), ref.double().reshape(-1)
        if k in ("skel", "pose"):
            e = rel_err(got[k], ref)
            if report:
                report(f"{name} B={B} {k}: max err / max|ref| = {e:.3e}")
            if not e <= BF16_FWD:
                bad.append((k, e, BF16_FWD))
            continue
        rel, cos = float((a - b).norm() / b.norm()), float(a @ b / (a.norm() * b.norm()))
        if report:
            report(f"{name} B={B} {k}: rel L2 = {rel:.3e}, cos = {cos:.6f}")
        if not (rel <= BF16_REL_L2 and cos >= BF16_COS):
            bad.append((k, rel, cos))
    return bad


# ------------------------------------------------------------------------------------------------------------------ the C ABI run
def handle(name):
    from gpu_util import lift_net
    net, _, p = lift_net(name)
    net._bind(torch.device("cuda", 0))
    return net._ensure_handle(), net, p


def routes(name, B):
    from egotap_amd import lib as L
    return L.pu_train_routes(handle(name)[0], B)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _forward(h, p, B, pc, rc, st):
    """egotap_train_pu_fwd into a saved buffer whose every byte starts as 0xFF (NaN patterns: nothing stale from an earlier run can stand in
    for a value this run should have written).  Returns (saved, hs1 view [J*B*H])."""
    from egotap_amd import lib as L, train_ops as T
    lib = L.load()
    J, H = p.n_joints_hm, p.pu_hidden
    nb, off = C.c_size_t(), C.c_size_t()
    L.check(lib.egotap_train_pu_saved_bytes(h, B, C.byref(nb), C.byref(off)))
    saved = torch.full((nb.value,), 0xFF, dtype=torch.uint8, device="cuda")
    L.check(lib.egotap_train_pu_fwd(h, T._p(pc), T._p(rc), B, T._p(saved), saved.numel(), st))
    return saved, saved[off.value: off.value + 4 * J * B * H].view(torch.float32)


def run_gpu(name, B, mode="f32", accumulate=0, chain=True):
    """egotap_train_pu_fwd, egotap_train_pose_head_fwd / _bwd and egotap_train_pu_bwd on the preset's cached handle.  Every output starts as NaN
    (accumulate = 0: the gradients too; accumulate = 1: the gradient buffers start as random values, returned under "prefill" -- the caller
    compares with prefill + reference).  Returns the tensors of ``reference`` on the CPU.  Precision and chain switch
    are restored whatever happens."""
    from egotap_amd import lib as L, train_ops as T
    h, net, p = handle(name)
    lib = L.load()
    J, H = p.n_joints_hm, p.pu_hidden
    posz, rotz, dpose = inputs(name, B)
    keys = sorted(weights(name))
    try:
        if mode != "f32":
            net.set_precision(mode)
        if not chain:
            net.set_pu_chain(False)
        pc, rc, dpose_dev = posz.cuda(), rotz.cuda(), dpose.cuda()          # (kept alive: the calls take raw pointers)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        saved, hs1 = _forward(h, p, B, pc, rc, st)
        pose = _nan(B, p.out_joints, 3)
        L.check(lib.egotap_train_pose_head_fwd(h, T._p(pc), T._p(hs1), B, T._p(pose), st))
        dposz, dhs1, drotz = _nan(*pc.shape), _nan(J * B * H), _nan(*rc.shape)
        sd = net.state_dict()
        if accumulate:
            prefill = {k: _rand(tuple(sd[k].shape), 900 + i) for i, k in enumerate(keys)}
            g = {k: v.cuda() for k, v in prefill.items()}
        else:
            prefill = None
            g = {k: _nan(*sd[k].shape) for k in keys}
        gp = lambda k: T._p(g[k]) if k in g else None                        # EgoCap has no global_mlp: null dWg / dbg
        L.check(lib.egotap_train_pose_head_bwd(h, T._p(pc), T._p(hs1), T._p(dpose_dev), B, T._p(dposz), T._p(dhs1),
                                               gp("pose_mlp.pose_fcs.0.weight"), gp("pose_mlp.pose_fcs.0.bias"),
                                               gp("global_mlp.pose_fcs.0.weight"), gp("global_mlp.pose_fcs.0.bias"), accumulate, st))
        wsb = C.c_size_t()
        L.check(lib.egotap_train_pu_bwd_ws_bytes(h, B, C.byref(wsb)))
        ws = torch.full((wsb.value,), 0xFF, dtype=torch.uint8, device="cuda")
        ptrs = (C.c_void_p * 14)()
        for i, nme in enumerate(PU_ORDER):
            ptrs[2 * i] = g[f"{PU_PRE}{nme}.weight"].data_ptr()
            ptrs[2 * i + 1] = g[f"{PU_PRE}{nme}.bias"].data_ptr()
        L.check(lib.egotap_train_pu_bwd(h, T._p(pc), T._p(rc), B, T._p(saved), T._p(dhs1), T._p(dposz), T._p(drotz), ptrs, accumulate, T._p(ws),
                                        ws.numel(), st))
        torch.cuda.synchronize()
        out = {"skel": hs1.reshape(J, B, H).cpu().clone(), "pose": pose.cpu(), "dposz": dposz.cpu(), "drotz": drotz.cpu()}
        out.update({k: g[k].cpu() for k in keys})
        if prefill is not None:
            out["prefill"] = prefill
        assert bool(torch.isfinite(dhs1).all()), "dhs1: a NaN of the prefill survived egotap_train_pose_head_bwd"
        return out
    finally:
        if not chain:
            net.set_pu_chain(True)
        if mode != "f32":
            net.set_precision("f32")


def pose_aligned_and_unaligned(name, B):
    """pose_head_kernel on hs1 as the forward leaves it (16-byte aligned: the vector path) and on a copy one float into a larger buffer
    (4-byte aligned: the scalar loop).  Returns (aligned, unaligned) on the CPU."""
    from egotap_amd import lib as L, train_ops as T
    h, _, p = handle(name)
    lib = L.load()
    posz, rotz, _ = inputs(name, B)
    pc, rc = posz.cuda(), rotz.cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _, hs1 = _forward(h, p, B, pc, rc, st)
    backing = _nan(hs1.numel() + 8)
    view = backing[1:1 + hs1.numel()]
    view.copy_(hs1)
    assert hs1.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4
    poses = []
    for src in (hs1, view):
        pose = _nan(B, p.out_joints, 3)
        L.check(lib.egotap_train_pose_head_fwd(h, T._p(pc), T._p(src), B, T._p(pose), st))
        poses.append(pose)
    torch.cuda.synchronize()
    return poses[0].cpu(), poses[1].cpu()
