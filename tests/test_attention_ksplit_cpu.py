"""The key-split planner of the exact-fp32 attention (attention_f32_ksplit, csrc/attention_f32.h), through its host-only hook
egotap_debug_attention_f32_ksplit: no device call, no GPU needed.  The expected counts are re-derived here from the rule the launcher documents,
not read back from the library."""
import pytest

from egotap_amd import lib as L

SCRATCH = 1 << 24          # the forward's split-K scratch, in floats


def _tiles(N):
    return (N + 31) // 32


def _per_split(B, N, heads):
    """floats of one split's partials: ctx [B * N, heads * 128] and its log-sum-exps [B * heads * N]"""
    return B * N * heads * 128 + B * heads * N


def _admissible(B, N, heads, k, scratch, cu):
    """the documented rule: whole key tiles per range, B x heads x query groups x k workgroups within 4.5 per compute unit, partials within scratch"""
    wgs = B * heads * ((_tiles(N) + 1) // 2)
    return _tiles(N) % k == 0 and 2 * wgs * k <= 9 * cu and k * _per_split(B, N, heads) <= scratch


def _expected(B, N, heads, scratch, cu):
    return next((k for k in range(8, 1, -1) if _admissible(B, N, heads, k, scratch, cu)), 1)


@pytest.mark.parametrize("B,k", [(1, 6), (2, 6), (4, 3), (8, 2), (16, 1)])
def test_documented_table(B, k):
    """the table above attention_f32_launch: 576 tokens, 8 heads, 256 CUs, the forward's scratch"""
    assert L.attention_f32_ksplit(B, 576, 8, SCRATCH, 256) == k


@pytest.mark.parametrize("N", [32, 36, 64, 100, 144, 192, 224, 256, 288, 324, 576, 1296])
@pytest.mark.parametrize("cu", [1, 8, 64, 256, 304])
def test_count_divides_the_tiles_fits_and_is_the_largest_admissible(N, cu):
    for B, heads in ((1, 1), (2, 2), (1, 8), (3, 8), (16, 8)):
        for scratch in (0, _per_split(B, N, heads), 3 * _per_split(B, N, heads), SCRATCH, 1 << 30):
            k = L.attention_f32_ksplit(B, N, heads, scratch, cu)
            assert 1 <= k <= 8 and _tiles(N) % k == 0, (N, B, heads, cu, scratch, k)
            assert k == 1 or k * _per_split(B, N, heads) <= scratch, (N, B, heads, cu, scratch, k)
            assert k == _expected(B, N, heads, scratch, cu), (N, B, heads, cu, scratch, k)


@pytest.mark.parametrize("N,k,below", [(192, 6, 3), (192, 3, 2), (192, 2, 1), (256, 8, 4), (256, 4, 2), (224, 7, 1), (144, 5, 1), (64, 2, 1), (36, 2, 1), (576, 6, 3)])
@pytest.mark.parametrize("B,heads", [(1, 1), (2, 2)])
def test_one_float_short_gives_the_next_smaller_admissible_count(N, k, below, B, heads):
    need = k * _per_split(B, N, heads)
    assert L.attention_f32_ksplit(B, N, heads, need, 256) == k
    assert L.attention_f32_ksplit(B, N, heads, need - 1, 256) == below


@pytest.mark.parametrize("N,tiles", [(324, 11), (416, 13), (1296, 41), (532, 17)])
def test_prime_tile_count_above_eight_is_never_split(N, tiles):
    assert _tiles(N) == tiles
    for B, heads in ((1, 1), (1, 8), (2, 8)):
        assert L.attention_f32_ksplit(B, N, heads, 1 << 30, 256) == 1


def test_wrapper_raises_on_refused_arguments():
    with pytest.raises(L.EgotapError, match="num_cu=0"):
        L.attention_f32_ksplit(1, 64, 8, SCRATCH, 0)
    with pytest.raises(L.EgotapError, match="bad shape"):
        L.attention_f32_ksplit(1, 30, 8, SCRATCH, 256)
