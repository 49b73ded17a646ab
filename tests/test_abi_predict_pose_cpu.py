"""Host-side argument checks of the pose-only entry egotap_lift_predict_pose (no kernel is launched here): it refuses what
egotap_lift_forward refuses, with its own name in the message."""
import ctypes as C

from egotap_amd import lib as L
from egotap_amd import spec


def _bound_handle():
    lib = L.load()
    cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, 64, 128, 1024, 8, 3, 16, 512)
    h = C.c_void_p()
    assert lib.egotap_create(C.byref(cfg), C.byref(h)) == 0
    fake = C.c_void_p(0x100000)                   # never dereferenced: every check below fails before a launch
    for key, shape in spec.lift_state_spec(spec.lift_preset("UnrealEgo", 64)):
        n = 1
        for d in shape:
            n *= d
        lib.egotap_bind_param(h, L.NET_LIFT, key.encode(), fake, n, L.F32)
    n = C.c_int()
    assert lib.egotap_unbound_count(h, L.NET_LIFT, C.byref(n)) == 0 and n.value == 0
    return lib, h


def test_predict_pose_refusals():
    lib, h = _bound_handle()
    need = C.c_size_t()
    assert lib.egotap_lift_workspace_bytes(h, 4, C.byref(need)) == 0
    hm, pose, ws = C.c_void_p(0x200000), C.c_void_p(0x300000), C.c_void_p(0x400000)
    f = lib.egotap_lift_predict_pose
    assert f(h, hm, 0, pose, ws, need.value, None) == 0                        # empty batch: nothing to do
    assert f(None, hm, 4, pose, ws, need.value, None) == 1
    for args in ((None, pose, ws), (hm, None, ws), (hm, pose, None)):
        assert f(h, args[0], 4, args[1], args[2], need.value, None) == 1
        assert b"egotap_lift_predict_pose" in lib.egotap_last_error()
    assert f(h, hm, -1, pose, ws, need.value, None) == 1
    assert f(h, C.c_void_p(0x200004), 4, pose, ws, need.value, None) == 1   # hm not 16-byte aligned
    assert f(h, hm, 4, pose, C.c_void_p(0x400010), need.value, None) == 1   # ws not 256-byte aligned
    assert b"aligned" in lib.egotap_last_error()
    assert f(h, hm, 4, pose, ws, need.value - 1, None) == 4                  # workspace too small
    assert b"workspace too small" in lib.egotap_last_error()
    lib.egotap_destroy(h)

