"""Host-side argument checks of egotap_lift_backward_dhm (no kernel is launched here): it refuses what egotap_lift_backward refuses and a
dhm that is misaligned or overlaps hm, with its own name in the message, before any launch."""
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
        if not spec.is_buffer(key) and key not in spec.LIFT_DEAD_KEYS:
            assert lib.egotap_bind_grad(h, key.encode(), fake, n) == 0
    return lib, h


def test_lift_backward_dhm_refusals():
    lib, h = _bound_handle()
    B = 4
    sb, wb = C.c_size_t(), C.c_size_t()
    assert lib.egotap_lift_train_bytes(h, B, C.byref(sb), C.byref(wb)) == 0
    hm, dpose, saved, ws = (C.c_void_p(a) for a in (0x10000000, 0x20000000, 0x30000000, 0x40000000))
    dhm_bytes = B * 90 * 64 * 64 * 4
    dhm = C.c_void_p(0x50000000)
    f = lib.egotap_lift_backward_dhm

    def call(hm_=hm, dpose_=dpose, B_=B, saved_=saved, sbytes=sb.value, ws_=ws, wbytes=wb.value, dhm_=dhm, n_events=0):
        return f(h, hm_, dpose_, B_, saved_, sbytes, ws_, wbytes, None, n_events, None, dhm_)

    def refused(rc, *words):
        msg = lib.egotap_last_error()
        assert rc != 0 and b"egotap_lift_backward_dhm" in msg, (rc, msg)
        for w in words:
            assert w in msg, msg

    # bad arguments
    refused(call(hm_=None))
    refused(call(dpose_=None))
    refused(call(saved_=None))
    refused(call(ws_=None))
    refused(call(B_=0))
    refused(call(B_=-1))
    refused(call(n_events=3), b"bucket events")
    assert f(None, hm, dpose, B, saved, sb.value, ws, wb.value, None, 0, None, dhm) != 0
    # dhm: 16-byte aligned, not overlapping the input
    refused(call(dhm_=C.c_void_p(0x50000004)), b"aligned")
    refused(call(dhm_=hm), b"overlap")
    refused(call(dhm_=C.c_void_p(0x10000000 + dhm_bytes - 16)), b"overlap")
    refused(call(dhm_=C.c_void_p(0x10000000 - dhm_bytes + 16)), b"overlap")
    # buffers too small
    refused(call(wbytes=wb.value - 1), b"workspace too small")
    refused(call(sbytes=sb.value - 1), b"saved buffer too small")
    # and with dhm == NULL the same checks hold, still under this entry's name
    refused(call(dhm_=None, wbytes=wb.value - 1), b"workspace too small")
    # the plain entry keeps its own name
    assert lib.egotap_lift_backward(h, hm, dpose, B, saved, sb.value, ws, wb.value - 1, None, 0, None) != 0
    msg = lib.egotap_last_error()
    assert b"egotap_lift_backward:" in msg and b"workspace too small" in msg
    lib.egotap_destroy(h)


def test_scatter_operators_refuse_bad_shapes():
    """the operator entries of the two products check their shapes before any launch"""
    lib, h = _bound_handle()
    x, w, dhm = C.c_void_p(0x10000000), C.c_void_p(0x20000000), C.c_void_p(0x30000000)
    nt = lib.egotap_train_gemm_nt
    TE_SCATTER_PATCH, TE_SCATTER_ROT = 7, 8
    seq, T, D, S = 576, 30, 1024, 64
    for epi, M, N, K in ((TE_SCATTER_PATCH, 2 * seq + 1, 256, D), (TE_SCATTER_PATCH, 2 * seq, 512, D), (TE_SCATTER_PATCH, 2 * seq, 256, 512),
                         (TE_SCATTER_ROT, 2 * T + 1, 2 * S * S, 2048), (TE_SCATTER_ROT, 2 * T, S * S, 2048), (TE_SCATTER_ROT, 2 * T, 2 * S * S, 1024)):
        assert nt(h, 0, x, 0, None, w, None, dhm, M, N, K, epi, None, None, 0, None) != 0
        assert b"scatter" in lib.egotap_last_error()
    assert nt(h, 2, x, 0, None, w, None, dhm, 2 * T, 2 * S * S, 2048, TE_SCATTER_ROT, None, None, 0, None) != 0          # plain rows only
    assert nt(h, 0, x, 0, None, w, None, C.c_void_p(0x30000008), 2 * T, 2 * S * S, 2048, TE_SCATTER_ROT, None, None, 0, None) != 0
    assert b"aligned" in lib.egotap_last_error()
    assert lib.egotap_bf16_fc1_dgrad_rot(h, x, w, C.c_void_p(0x30000008), 2, None) != 0
    assert lib.egotap_bf16_patch_dgrad(h, x, w, None, 2, None) != 0
    assert lib.egotap_bf16_patch_dgrad(h, x, w, dhm, 0, None) != 0
    lib.egotap_destroy(h)
