"""The one scan that turns the sorted keys into bin starts and slots (prims.hip: prim_bins_scan, in harc_dict_build) against the table's contract
(tests/index_ref.py), through harc_amd_selftest_index: sizes at every power of two from 64 to 65 536 and one to either side -- the edges of the scan's
tiles, whatever their size --, a chain of slots that every tile hands to the next, and a maximum that has to cross tiles in which no bin begins.  At 2
and 4 slots per read, sorted on the library's choice of top bits and on all 64."""
import numpy as np
import pytest

from tests import index_ref as ix
from tests import index_sets as sx

pytestmark = pytest.mark.gpu

SORT_BITS = (None, "64")


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    h = harc_amd.HarcAmd(harc_amd.default_params(100))
    yield h
    h.close()


def _build_and_check(ctx, monkeypatch, keys, m, what):
    for k in ("HARC_AMD_TABLE_FILL", "HARC_AMD_CAPMULT"):
        monkeypatch.delenv(k, raising=False)
    for sb in SORT_BITS:
        if sb is None:
            monkeypatch.delenv("HARC_AMD_SORT_BITS", raising=False)
        else:
            monkeypatch.setenv("HARC_AMD_SORT_BITS", sb)
        cap, nbins, slots, ids, lst = ctx.selftest_index(keys, slots_per_read=m, bigthresh=16, want_large=True)
        assert cap == ix.cap_for(keys.size, m), what
        try:
            ix.check_table(keys, cap, nbins, slots, ids, 16, lst)
        except ix.ContractError as e:
            raise ix.ContractError("%s m=%d SORT_BITS=%s: %s" % (what, m, sb, e)) from None


def _uniform_with_duplicates(n, seed):
    """n keys drawn from 0.6 n random scrambled values: single bins, small bins and heads at every distance"""
    rng = np.random.default_rng(seed)
    pool = sx._rand_h(rng, max(1, (6 * n) // 10))
    return sx.unscramble(pool[rng.integers(0, pool.size, size=n)])


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("k", range(6, 17))
def test_sizes_around_every_power_of_two(k, m, ctx, monkeypatch):
    for n in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        _build_and_check(ctx, monkeypatch, _uniform_with_duplicates(n, 7000 + n), m, "uniform keys with duplicates, n = %d" % n)


def _slot_of(ref_slots, h):
    at = np.flatnonzero((ref_slots["key"] == np.uint64(h)) & ((ref_slots["count"] & ix.SLOT_CNT_MASK) != 0))
    assert at.size == 1
    return int(at[0])


def _in_bucket(b, cap, count):
    """`count` distinct scrambled keys with their home in bucket b, spread over the whole bucket"""
    lo, hi = ix.first_h(b, cap), ix.first_h(b + 1, cap)
    step = (hi - lo) // (count + 1)
    assert step >= 1
    return [lo + 1 + j * step for j in range(count)]


@pytest.mark.parametrize("m", [2, 4])
def test_carry_that_crosses_many_tiles(m, ctx, monkeypatch):
    """20 000 distinct keys whose home is ONE bucket, an eighth into the table: every slot is the slot before it + 1, so what the scan carries from
    tile to tile grows by one per bin to the very end"""
    n = 20000
    cap = ix.cap_for(n, m)
    b = cap // 32
    hs = _in_bucket(b, cap, n)
    keys = sx._deal([(h, 1) for h in hs])
    assert (ix.home(ix.scramble(keys), cap) == 4 * b).all()
    nbins, ref_slots, _, _, wrapped = ix.build_ref(keys, cap)
    assert nbins == n and wrapped == 0 and _slot_of(ref_slots, max(hs)) - 4 * b >= n - 1
    _build_and_check(ctx, monkeypatch, keys, m, "20 000 bins homed in one bucket")


def _three_groups(h, cap):
    """5 000 distinct keys homed in bucket h, ONE key of bucket h + 1 30 000 times, 5 000 distinct keys of bucket h + 2: 35 000 sorted places in a row
    in which no bin begins, and behind them bins whose slot is still decided by the first group"""
    g1, g2, g3 = _in_bucket(h, cap, 5000), _in_bucket(h + 1, cap, 1), _in_bucket(h + 2, cap, 5000)
    return sx._deal([(x, 1) for x in g1] + [(g2[0], 30000)] + [(x, 1) for x in g3]), g3


N3 = 5000 + 30000 + 5000


@pytest.mark.parametrize("m", [2, 4])
def test_max_carried_across_tiles_without_a_head(m, ctx, monkeypatch):
    cap = ix.cap_for(N3, m)
    h = cap // 32
    keys, g3 = _three_groups(h, cap)
    assert keys.size == N3
    nbins, ref_slots, _, _, wrapped = ix.build_ref(keys, cap, 16)
    assert nbins == 10001 and wrapped == 0
    assert all(_slot_of(ref_slots, x) // 4 != h + 2 for x in (g3[0], g3[1], g3[2499], g3[-1]))      # the third group is not at home
    assert _slot_of(ref_slots, g3[0]) == 4 * h + 5001 and _slot_of(ref_slots, g3[-1]) == 4 * h + 10000
    _build_and_check(ctx, monkeypatch, keys, m, "three groups, 30 000 copies between them")


@pytest.mark.parametrize("m", [2, 4])
def test_max_carried_across_tiles_at_the_table_end(m, ctx, monkeypatch):
    """the same set with its three buckets the table's last: the pushed bins pass the end of the table and the wrapping pass places them"""
    cap = ix.cap_for(N3, m)
    h = cap // 4 - 3
    keys, g3 = _three_groups(h, cap)
    assert keys.size == N3
    nbins, ref_slots, _, _, wrapped = ix.build_ref(keys, cap, 16)
    assert nbins == 10001 and wrapped >= 10001 - 12
    assert all(_slot_of(ref_slots, x) // 4 != h + 2 for x in (g3[0], g3[1], g3[2499], g3[-1]))
    _build_and_check(ctx, monkeypatch, keys, m, "three groups at the table's end")
