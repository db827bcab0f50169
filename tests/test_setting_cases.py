"""CPU: tests/setting_cases.py imports without a GPU, and sequence() has the three properties the split-chain tests rely on, from the
formula alone."""
import pytest

from tests import setting_cases as SC


def test_settings_are_named_functions():
    assert SC.NAMES == ["off", "sym", "col", "rf_accept", "rf_fallback", "all"]
    assert all(callable(s) for s in SC.SETTINGS)
    assert len(SC.POOL_NAMES) == 12 and len(set(SC.POOL_NAMES)) == 12


@pytest.mark.parametrize("n,parts", [(128, 2), (256, 4)])
def test_sequence_properties(n, parts):
    assert n >= 64 * parts                                # host.hip.inc: the batch splits
    seq = SC.sequence(n, parts)
    assert len(seq) == n and all(0 <= k < len(SC.POOL_NAMES) for k in seq)
    distorted = [p for p in range(n) if seq[p] not in SC.CLEAN]
    fb = SC.FALLS_BACK[66]
    # both sides of every part boundary are distorted; a falling-back frame on the earlier side of one boundary and on the later side of one
    earlier = later = False
    for q in range(1, parts):
        lo = n * q // parts
        assert lo - 1 in distorted and lo in distorted, q
        earlier |= seq[lo - 1] == fb
        later |= seq[lo] == fb
    assert earlier and later
    # the ends are distorted
    assert 0 in distorted and n - 1 in distorted
    # at most one position in eight, or the next batch would not split (mostly_flood wants a quarter; the margin is the issue's)
    assert 8 * len(distorted) <= n
    # ... and fewer than 16, or a batch that certifies none of them would switch the certifying pass off for the batch after it
    assert len(distorted) < 16
    # every distorted pool frame turns up
    assert set(seq) == set(range(len(SC.POOL_NAMES)))


def test_short_sequence_holds_the_whole_pool():
    seq = SC.short_sequence(16)
    assert len(seq) == 16 and set(seq) == set(range(len(SC.POOL_NAMES)))
