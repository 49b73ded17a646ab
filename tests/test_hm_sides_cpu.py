"""Which heatmap sides the estimators' batch-statistics paths accept (no GPU): 64 and 128; every other side is refused by name."""
import pytest

from egotap_amd import spec


def test_batch_statistics_sides_are_64_and_128():
    assert spec.HM_BATCH_STATS_SIDES == (64, 128)
    for s in (64, 128):
        spec.hm_check_batch_stats_side(s, "stage-1 training")


def test_the_backward_is_built_at_side_64_only():
    """the weight-gradient kernels stop at map width 64: a differentiable forward at 128 is refused by name (the forward alone is not)"""
    assert spec.HM_TRAIN_SIDES == (64,)
    spec.hm_check_train_side(64, "stage-1 training")
    with pytest.raises(NotImplementedError, match="stage-1 training is built at heatmap side 64 only .*not 128.*hm_train_forward_nograd.*64 and 128"):
        spec.hm_check_train_side(128, "stage-1 training")
    with pytest.raises(NotImplementedError, match="64 and 128 only .*not 32"):
        spec.hm_check_train_side(32, "stage-1 training")


@pytest.mark.parametrize("side", [16, 32, 48, 80, 96, 112])
def test_other_sides_are_refused_by_name(side):
    with pytest.raises(NotImplementedError, match=f"stage-1 training is built at heatmap sides 64 and 128 only .*not {side}"):
        spec.hm_check_batch_stats_side(side, "stage-1 training")
