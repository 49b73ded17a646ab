"""Host side of egotap_predict_pose_rgb (stereo RGB -> pose in one call): exported, declared, sized and refusing by name -- no kernel is
launched here (every refusal comes before the first launch; the pointers below are never dereferenced)."""
import ctypes as C
import os
import re

import pytest

from egotap_amd import lib as L
from egotap_amd import spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1


def _handle(bind=(L.NET_LIFT, L.NET_HM_POS, L.NET_HM_ROT), hm=64):
    lib = L.load()
    cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, hm, 128, 1024, 8, 3, 16, 512)
    h = C.c_void_p()
    assert lib.egotap_create(C.byref(cfg), C.byref(h)) == 0
    fake = C.c_void_p(0x100000)
    specs = {L.NET_LIFT: [(k, s) for k, s in spec.lift_state_spec(spec.lift_preset("UnrealEgo", hm))],
             L.NET_HM_POS: [(k, s) for k, s, _ in spec.hm_state_spec(15)], L.NET_HM_ROT: [(k, s) for k, s, _ in spec.hm_state_spec(30)]}
    for net in bind:
        for key, shape in specs[net]:
            n = 1
            for d in shape:
                n *= d
            dt = L.I64 if key.endswith("num_batches_tracked") else L.F32
            assert lib.egotap_bind_param(h, net, key.encode(), fake, n, dt) == 0, key
        left = C.c_int()
        assert lib.egotap_unbound_count(h, net, C.byref(left)) == 0 and left.value == 0
    return lib, h


def test_symbols_are_exported_and_declared():
    lib = L.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egotap.h")).read(), flags=re.S)
    debug = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "egotap_debug.h")).read(), flags=re.S)
    for name in ("egotap_predict_pose_rgb", "egotap_predict_pose_rgb_workspace_bytes"):
        assert hasattr(lib, name) and name in L.exported_symbols()
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for name in ("egotap_debug_predict_pose_rgb_form", "egotap_debug_predict_pose_rgb_intermediate"):
        assert hasattr(lib, name) and name in L.exported_symbols()
        assert re.search(r"\bint\s+" + name + r"\s*\(", debug), name
    assert lib.egotap_abi_version() == 2               # additive: the version stays


@pytest.mark.parametrize("hm", [64, 128, 32])
def test_workspace_bytes(hm):
    lib, h = _handle(bind=(), hm=hm)
    try:
        def rgb(B, chunk):
            v = C.c_size_t()
            assert lib.egotap_predict_pose_rgb_workspace_bytes(h, B, chunk, C.byref(v)) == 0
            return v.value

        def part(fn, B):
            v = C.c_size_t()
            assert fn(h, B, C.byref(v)) == 0
            return v.value
        prev = 0
        for B in (1, 2, 3, 8, 37, 64, 256, 300):
            v = rgb(B, 0)
            assert v > 0 and v % 256 == 0 and v >= prev, (B, v, prev)
            prev = v
            assert v >= max(part(lib.egotap_hm_workspace_bytes, B), part(lib.egotap_lift_workspace_bytes, B))
        prev = 0
        for chunk in (1, 2, 4, 16, 64, 256):
            v = rgb(300, chunk)
            assert v > 0 and v % 256 == 0 and v >= prev, (chunk, v, prev)
            prev = v
            assert v >= max(part(lib.egotap_hm_workspace_bytes, chunk), part(lib.egotap_lift_workspace_bytes, 300))
        assert rgb(300, 0) == rgb(300, 300) == rgb(300, 1000) >= prev      # 0 and anything past B: the whole batch
        # the chunk bounds the estimators' scratch: a chunked B = 300 needs less than the whole batch at once
        assert rgb(300, 16) < rgb(300, 0)
        bad = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, -1, 0, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 4, -1, C.byref(bad)) == INVALID
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 4, 0, None) == INVALID
        assert lib.egotap_predict_pose_rgb_workspace_bytes(None, 4, 0, C.byref(bad)) == INVALID
        assert b"egotap_predict_pose_rgb_workspace_bytes" in lib.egotap_last_error()
    finally:
        lib.egotap_destroy(h)


def test_refusals_come_by_name_and_before_any_launch():
    lib, h = _handle()
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 4, 0, C.byref(need)) == 0
        le, ri, pose, hm, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x500000, 0x600000))
        f = lib.egotap_predict_pose_rgb

        def refused(*args, word):
            assert f(*args) == INVALID, args
            msg = lib.egotap_last_error()
            assert b"egotap_predict_pose_rgb" in msg and word in msg, msg
        refused(None, le, ri, 4, pose, hm, 0, ws, need.value, None, word=b"null handle")
        refused(h, None, ri, 4, pose, hm, 0, ws, need.value, None, word=b"null argument")
        refused(h, le, None, 4, pose, hm, 0, ws, need.value, None, word=b"null argument")
        refused(h, le, ri, 4, None, hm, 0, ws, need.value, None, word=b"null argument")
        refused(h, le, ri, 4, pose, hm, 0, None, need.value, None, word=b"null argument")
        refused(h, le, ri, 0, pose, hm, 0, ws, need.value, None, word=b"batch must be positive")
        refused(h, le, ri, -3, pose, hm, 0, ws, need.value, None, word=b"batch must be positive")
        refused(h, le, ri, 4, pose, hm, -1, ws, need.value, None, word=b"chunk")
        refused(h, le, ri, 4, pose, hm, 0, ws, need.value - 1, None, word=b"workspace too small")
        refused(h, le, ri, 4, pose, None, 0, ws, need.value - 1, None, word=b"workspace too small")      # the size does not depend on `heatmaps`
        refused(h, le, ri, 4, pose, hm, 0, ws, 0, None, word=b"workspace too small")
        refused(h, le, ri, 4, pose, hm, 0, C.c_void_p(0x600010), need.value, None, word=b"aligned")          # ws: 256 bytes
        refused(h, C.c_void_p(0x200004), ri, 4, pose, hm, 0, ws, need.value, None, word=b"aligned")
        refused(h, le, ri, 4, pose, C.c_void_p(0x500008), 0, ws, need.value, None, word=b"aligned")
        # a chunked call needs the chunked size only
        small = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 300, 16, C.byref(small)) == 0
        refused(h, le, ri, 300, pose, hm, 16, ws, small.value - 256, None, word=b"workspace too small")
        form = C.c_int(-1)
        assert lib.egotap_debug_predict_pose_rgb_form(h, C.byref(form)) == 0 and form.value == 0          # nothing ran
    finally:
        lib.egotap_destroy(h)


@pytest.mark.parametrize("missing,word", [(L.NET_LIFT, b"lifting head"), (L.NET_HM_POS, b"position estimator"), (L.NET_HM_ROT, b"limb estimator")])
def test_unbound_network_is_refused_by_name(missing, word):
    lib, h = _handle(bind=[n for n in (L.NET_LIFT, L.NET_HM_POS, L.NET_HM_ROT) if n != missing])
    try:
        need = C.c_size_t()
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 2, 0, C.byref(need)) == 0
        le, ri, pose, ws = (C.c_void_p(a) for a in (0x200000, 0x300000, 0x400000, 0x600000))
        assert lib.egotap_predict_pose_rgb(h, le, ri, 2, pose, None, 0, ws, need.value, None) == INVALID
        msg = lib.egotap_last_error()
        assert b"egotap_predict_pose_rgb" in msg and b"unbound parameter" in msg and word in msg and b"not bound" in msg, msg
    finally:
        lib.egotap_destroy(h)


def test_debug_intermediate_names_the_heatmap_slot():
    lib, h = _handle(bind=())
    try:
        need, off, num = C.c_size_t(), C.c_size_t(), C.c_int64()
        assert lib.egotap_predict_pose_rgb_workspace_bytes(h, 5, 2, C.byref(need)) == 0
        for name in (b"heatmaps", b"handoff"):
            assert lib.egotap_debug_predict_pose_rgb_intermediate(h, 5, 2, name, C.byref(off), C.byref(num)) == 0
            assert off.value % 256 == 0 and num.value == 5 * 90 * 64 * 64 and off.value + 4 * num.value <= need.value
        assert lib.egotap_debug_predict_pose_rgb_intermediate(h, 5, 2, b"tokens", C.byref(off), C.byref(num)) == INVALID
        assert b"unknown intermediate" in lib.egotap_last_error()
    finally:
        lib.egotap_destroy(h)
