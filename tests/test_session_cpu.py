"""egotap_amd/session.py on the host: the bind cache, its refusals, the grow-only buffer helper and the handle's lifetime.  No kernel runs:
the library's egotap_bind_param stores addresses only, so CPU tensors bind (as tests/test_abi_cpu.py binds made-up addresses)."""
import ctypes as C
import gc
import weakref

import pytest
import torch

from egotap_amd import lib as L
from egotap_amd import networks, session

CPU = torch.device("cpu")


def _head():
    from egotap_amd.options import preset_defaults
    return networks.EgoTAPAutoEncoder(preset_defaults("UnrealEgo", 64), input_channel_scale=2).eval()


def _estimator():
    from egotap_amd.options import preset_defaults
    opt = preset_defaults("UnrealEgo", 64)
    opt.num_rot_heatmap = 0
    return networks.HeatMap_UnrealEgo_Shared(opt, "resnet18", 2).eval()


@pytest.fixture
def calls(monkeypatch):
    """counts (and records) the library calls that create, bind and destroy"""
    lib = L.load()
    seen = {"egotap_bind_param": [], "egotap_create": [], "egotap_destroy": []}
    for name, log in seen.items():
        def wrapped(*args, _fn=getattr(lib, name), _log=log):
            _log.append(args)
            return _fn(*args)
        monkeypatch.setattr(lib, name, wrapped)
    return seen


def _unbound(net):
    n = C.c_int()
    L.check(L.load().egotap_unbound_count(net._ensure_handle(), net._net, C.byref(n)))
    return n.value


@pytest.mark.parametrize("make", [_head, _estimator])
def test_bind_cache(make, calls):
    net = make()
    binds = calls["egotap_bind_param"]
    sd = net.state_dict(keep_vars=True)
    assert net._bind(CPU) is True
    assert sorted(a[2].decode() for a in binds) == sorted(sd)          # every state_dict tensor, once, under its own name
    assert all(a[3].value == sd[a[2].decode()].data_ptr() for a in binds)
    assert _unbound(net) == 0
    if make is _estimator:                                             # the aliases of the ResNet tensors: one address under both names
        bound = {a[2].decode(): a[3].value for a in binds}
        assert len(net._aliases) == 120 and any(k.startswith("backbone.backbone.layer4.") for k, _ in net._aliases)
        for k, a in net._aliases:
            assert bound[k] == bound[a], (k, a)
        assert len(bound) == 258
    del binds[:]
    assert net._bind(CPU) is False and not binds                       # nothing moved: no ABI call
    net.load_state_dict({k: v.detach().clone() for k, v in sd.items()})
    assert net._bind(CPU) is False and not binds                       # load_state_dict copies into the same storages
    name, prm = next(iter(net.named_parameters()))
    prm.data = prm.data.clone()
    assert net._bind(CPU) is True
    assert {a[2].decode(): a[3].value for a in binds}[name] == prm.data_ptr()
    assert _unbound(net) == 0


@pytest.mark.parametrize("make", [_head, _estimator])
@pytest.mark.parametrize("fault", ["float64", "non-contiguous", "other device"])
def test_bind_refuses_before_the_first_bind_call(make, fault, calls):
    net = make()
    prm = [p for p in net.parameters() if p.dim() >= 2][-1]           # a late one: everything before it would have been bound already
    if fault == "float64":
        prm.data = prm.data.double()
    elif fault == "non-contiguous":
        prm.data = prm.data.transpose(0, 1).contiguous().transpose(0, 1)
        assert not prm.is_contiguous()
    with pytest.raises(L.EgotapError, match="contiguous fp32"):
        net._bind(torch.device("meta") if fault == "other device" else CPU)
    assert not calls["egotap_bind_param"]
    if fault == "other device":
        assert net._bind(CPU) is True                                  # a refused bind records nothing: the right device binds everything


def test_forward_bottleneck_validates_through_the_same_check():
    sd = {"w": torch.zeros(4, 4), "n": torch.zeros((), dtype=torch.long)}
    session.check_bindable(sd, CPU)
    for bad in (torch.zeros(4, 4, dtype=torch.float64), torch.zeros(4, 4).t()[:, :2], torch.zeros(2, dtype=torch.int32)):
        with pytest.raises(L.EgotapError, match="parameter w"):
            session.check_bindable({"w": bad}, CPU)
    with pytest.raises(L.EgotapError, match="parameter w"):
        session.check_bindable(sd, torch.device("meta"))


class _Owner:
    pass


def test_grow_only_buffer():
    o = _Owner()
    a = session.grown(o, "buf", 100, CPU)
    assert a is o.buf and a.dtype == torch.uint8 and a.numel() == 100
    assert session.grown(o, "buf", 100, CPU) is a and session.grown(o, "buf", 1, CPU) is a      # the need does not exceed the size
    b = session.grown(o, "buf", 101, CPU)
    assert b is not a and b is o.buf and b.numel() == 101                                        # grown
    c = session.grown(o, "buf", 1, torch.device("meta"))
    assert c is not b and c.device.type == "meta" and o.buf is c                                 # another device
    assert session.grown(_Owner(), "buf", 10, CPU, floor=64).numel() == 64                       # the floor
    assert session.grown(_Owner(), "buf", 100, CPU, floor=64).numel() == 100
    s = session.Scratch(floor=32)
    assert s.buf is None and s.get(8, CPU).numel() == 32 and s.get(16, CPU) is s.buf and s.get(40, CPU).numel() == 40
    from egotap_amd import train_ops
    assert train_ops.Scratch is session.Scratch and session.Scratch().floor == 64 << 20


@pytest.mark.parametrize("drop_first", [False, True])
def test_grow_only_buffer_allocation_order(drop_first, monkeypatch):
    """drop_first: the old block is gone before the new one is allocated (peak of one buffer); otherwise both exist for a moment"""
    o = _Owner()
    old = weakref.ref(session.grown(o, "buf", 16, CPU))
    alive, empty = [], torch.empty

    def watched(*a, **k):
        alive.append(old() is not None)
        return empty(*a, **k)
    monkeypatch.setattr(torch, "empty", watched)
    session.grown(o, "buf", 32, CPU, drop_first=drop_first)
    assert alive == [not drop_first]
    assert old() is None and o.buf.numel() == 32


@pytest.mark.parametrize("make", [_head, _estimator])
def test_handle_is_created_once_and_destroyed_once(make, calls):
    net = make()
    assert not calls["egotap_create"]                                  # lazily: a module that never runs holds no handle
    h = net._ensure_handle()
    assert net._ensure_handle() is h and isinstance(h, C.c_void_p) and h.value
    assert len(calls["egotap_create"]) == 1
    net._bind(CPU)
    value = h.value
    del net, h
    gc.collect()
    assert [a[0].value for a in calls["egotap_destroy"]] == [value]


def test_handle_applies_the_shared_device_rule_in_one_place(monkeypatch):
    lib, seen = L.load(), []
    monkeypatch.setattr(lib, "egotap_set_pu_chain", lambda h, on, _fn=lib.egotap_set_pu_chain: seen.append(on) or _fn(h, on))
    monkeypatch.delenv("EGOTAP_SHARED_DEVICE", raising=False)
    preset = _head().preset
    session.Handle(preset)
    assert seen == []
    session.Handle(preset, shared_device=True)
    assert seen == [0]
    monkeypatch.setenv("EGOTAP_SHARED_DEVICE", "1")
    session.Handle(preset, hm_blocks=(3, 4, 6, 3))
    assert seen == [0, 0]


def test_casts():
    t = torch.zeros(8)
    assert session.ptr(None).value is None and session.ptr(t).value == t.data_ptr() and session.ptr(t, 12).value == t.data_ptr() + 12
    from egotap_amd import bf16s, hm_ops, train_ops
    assert L._ptr is session.ptr is train_ops._p is bf16s._p is hm_ops._p
    assert L._stream is session.stream is train_ops._s is bf16s._s is hm_ops._s
