"""The one-call serving workspace, as exact equalities between the three size queries and the two scratch queries they are made of:
[ scratch = max(estimator scratch of a chunk, head scratch of the batch) | heatmaps | converter slice (bytes, where no stem reads them) | resized bytes
(sensor) ].  No GPU: the queries only compute."""
import ctypes as C

import pytest

from egotap_amd import lib as L
from egotap_amd import spec


def _al256(n):
    return (n + 255) // 256 * 256


def _q(fn, *args):
    v = C.c_size_t()
    assert fn(*args, C.byref(v)) == 0, L.load().egotap_last_error()
    return v.value


@pytest.mark.parametrize("hm", [32, 64])
def test_the_three_sizes_are_the_layout(hm):
    lib = L.load()
    cfg = L.EgotapConfig(C.sizeof(L.EgotapConfig), 15, 1, hm, 128, 1024, 8, 3, 16, 512)
    h = C.c_void_p()
    assert lib.egotap_create(C.byref(cfg), C.byref(h)) == 0
    try:
        channels, S0 = spec.lift_preset("UnrealEgo", hm).in_channels, 4 * hm
        for B, chunk in ((1, 0), (4, 0), (5, 2), (300, 16)):
            c = chunk if 0 < chunk <= B else B
            scratch = _al256(max(_q(lib.egotap_hm_workspace_bytes, h, c), _q(lib.egotap_lift_workspace_bytes, h, B)))
            rgb = _q(lib.egotap_predict_pose_rgb_workspace_bytes, h, B, chunk)
            u8 = _q(lib.egotap_predict_pose_rgb_u8_workspace_bytes, h, B, chunk)
            sensor = _q(lib.egotap_predict_pose_sensor_u8_workspace_bytes, h, B, 37, 53, chunk)
            assert rgb == scratch + _al256(B * channels * hm * hm * 4), (B, chunk)
            assert u8 == rgb + (c * 2 * 3 * S0 * S0 * 4 if hm == 32 else 0), (B, chunk)
            assert sensor == u8 + c * 2 * 3 * S0 * S0, (B, chunk)
            offset, numel = C.c_size_t(), C.c_int64()
            assert lib.egotap_debug_predict_pose_rgb_intermediate(h, B, chunk, b"heatmaps", C.byref(offset), C.byref(numel)) == 0
            assert offset.value == scratch, (B, chunk)                 # the heatmaps sit right behind the scratch, whichever the source
    finally:
        lib.egotap_destroy(h)
