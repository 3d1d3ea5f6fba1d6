"""The crafted key sets of tests/test_gpu_index.py and tests/test_index_ref.py.  Each is made in the space of SCRAMBLED keys (the high word picks the
bucket) and unscrambled; `m` = slots per read.  crafted_sets(m) is built once per process."""
import functools

import numpy as np

from tests.index_ref import MIXED_BUDGET, TP_SPAN, cap_for, first_h, scramble, sort_bits, unscramble      # noqa: F401


# A set is a list of (h, copies); the keys are dealt out in a shuffled order so that the copies of a bin are interleaved with the others.
def _deal(bins, seed=1):
    hs = np.array([b[0] for b in bins], dtype=np.uint64)
    assert np.unique(hs).size == hs.size, "crafted bins must be distinct"
    h = np.repeat(hs, [b[1] for b in bins])
    return unscramble(np.random.default_rng(seed).permutation(h))


def _sized(make, m):
    """bins depend on cap and cap on n: make(cap) must return the same number of keys for every cap"""
    n = sum(c for _, c in make(cap_for(1000, m)))
    return make(cap_for(n, m))


def _rand_h(rng, k):
    return rng.integers(0, 1 << 63, size=k, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=k, dtype=np.uint64)


def set_uniform(nbins, m, seed=3):
    return unscramble(_rand_h(np.random.default_rng(seed), nbins))


def set_equal(n, m):
    return np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)


H1 = 0xFFFFFFFF00000000                                           # home: the last bucket of any table


def set_table_end(nend, copies, m, variant):
    """nend bins in the last bucket.  variant "run": 13 more bins with their home three buckets before the end (they fill the last three buckets and one of
    THEM is pushed past the end); "start": 4 more bins that fill bucket 0 exactly, without a flag: the wrapped bins must pass it; "both": the two together"""
    def make(cap):
        nb = cap // 4
        bins = [(H1 + 7 * j, copies) for j in range(nend)]
        if variant in ("run", "both"):
            bins += [(first_h(nb - 3, cap) + 5 * j, copies) for j in range(13)]
        if variant in ("start", "both"):
            bins += [(first_h(0, cap) + 3 * j + 1, copies) for j in range(4)]
        return bins + [(first_h(nb // 2, cap) + j, 1) for j in range(3)]
    return _deal(_sized(make, m))


def set_overflow(nhome_b, next_in_b1, m, fill=100):
    """nhome_b bins with their home in bucket b (three quarters into the table), then one bin with its home in b + 1 when next_in_b1; `fill` single bins
    in the first quarter, so that the table has room for the chain behind b"""
    def make(cap):
        nb = cap // 4
        b = overflow_bucket(cap)
        bins = [(first_h(b, cap) + 11 * j, 1 + j % 2) for j in range(nhome_b)]
        if next_in_b1:
            bins.append((first_h(b + 1, cap) + 5, 1))
        return bins + [(first_h((j * (nb // 4)) // fill, cap) + 9 + j, 1) for j in range(fill)]
    return _deal(_sized(make, m))


def overflow_bucket(cap):
    return 3 * (cap // 4) // 4


def set_two_bins(n, m):
    """two bins in a table of m * n slots: the stretch between them is far longer than TP_SPAN"""
    return _deal([(0x4000000000000123, n // 2), (0xC000000000000456, n - n // 2)])


def set_one_block_span(over, m):
    """256 bins, one workgroup, in a table of exactly TP_SPAN slots (over = False) or one bucket more"""
    n = next(x for x in range(256, 4 * TP_SPAN) if cap_for(x, m) == TP_SPAN + (4 if over else 0))
    rng = np.random.default_rng(5)
    h = _rand_h(rng, 256)
    return unscramble(rng.permutation(np.concatenate([h, h[rng.integers(0, 256, size=n - 256)]])))


def set_first_block_span(over, m):
    """the 256 bins of the first workgroup end in the last bucket inside TP_SPAN slots (over = False) or in the first beyond; more bins behind them"""
    copies, tail = (1, 344) if m == 4 else (3, 60)                # enough keys for a table longer than TP_SPAN at either capacity

    def make(cap):
        endb = TP_SPAN // 4 - 1 + (1 if over else 0)
        nb = cap // 4
        bins = [(first_h((j * (endb - 1)) // 255, cap) + j, copies) for j in range(255)] + [(first_h(endb, cap) + 1, copies + 1)]
        return bins + [(first_h(endb + 1 + (j * (nb - endb - 2)) // tail, cap) + j, 1 + (j % 3 == 0)) for j in range(tail)]
    return _deal(_sized(make, m))


def set_mixed(n, runs, seed=7):
    """runs: list of (top, length): `length` distinct scrambled keys that share the top sort_bits(n) bits `top` and differ below them, 1 - 3 copies each;
    random single keys fill up to n.  (n must keep sort_bits: the caller asserts it on the result)"""
    sb = sort_bits(n)
    rng = np.random.default_rng(seed)
    bins = []
    for top, length in runs:
        low = rng.choice(1 << 20, size=length, replace=False).astype(np.uint64) * np.uint64(1 << (64 - sb - 20) if 64 - sb > 20 else 1)
        bins += [((top << (64 - sb)) | int(x), 1 + j % 3) for j, x in enumerate(low)]
    used = sum(c for _, c in bins)
    tops = {t for t, _ in runs}
    fill = [int(x) for x in _rand_h(rng, n - used) if (int(x) >> (64 - sb)) not in tops]
    return _deal(bins + [(x, 1) for x in sorted(set(fill))], seed)


def mixed_places(keys, sb=None):
    """places where a key follows a DIFFERENT key with the same top bits after a stable sort on those bits alone (what k_mixed_find lists), and the
    number of those where the two are out of order"""
    h = scramble(keys)
    sb = sb or sort_bits(h.size)
    s = h[np.argsort(h >> np.uint64(64 - sb), kind="stable")]
    same_top = (s[1:] >> np.uint64(64 - sb)) == (s[:-1] >> np.uint64(64 - sb))
    return int((same_top & (s[1:] != s[:-1])).sum()), int((same_top & (s[1:] < s[:-1])).sum())


def set_fallback(n, m):
    """n distinct scrambled keys that share their top 32 bits, handed over in DESCENDING order: one stretch, longer than MIXED_BUDGET"""
    cap = cap_for(n, m)
    hi = first_h(cap // 32, cap) >> 32                            # home an eighth into the table: the chain of n slots ends inside it
    return unscramble(np.uint64(hi << 32) + np.arange(n, 0, -1, dtype=np.uint64) * np.uint64(3))


def set_counts(counts, seed=11):
    rng = np.random.default_rng(seed)
    return _deal([(int(x), c) for x, c in zip(_rand_h(rng, len(counts)), counts)], seed)


def set_random(seed):
    """uniform keys with duplicates: n from 1 to 70 000 (log-uniform), duplicate rate 0 - 90 %"""
    rng = np.random.default_rng(1000 + seed)
    n = 1 if seed == 0 else 70000 if seed == 1 else int(round(70000 ** rng.random()))
    pool = _rand_h(rng, max(1, int(n * (1.0 - 0.9 * rng.random()))))
    return unscramble(pool[rng.integers(0, pool.size, size=n)])


def set_loud(nbins):
    return unscramble(np.uint64(H1) + np.arange(nbins, dtype=np.uint64) * np.uint64(13))


@functools.lru_cache(maxsize=None)
def crafted_sets(m):
    """(name, keys, properties) of the small crafted sets at m slots per read.  Properties: wrap = whether bins must lie past the end of the table
    (None: not the point of the set), mixed = the top-bits sort alone does not decide the order, bigthresh / large = what to ask the build for"""
    out = []

    def add(name, keys, wrap=None, mixed=False, bigthresh=0, large=False):
        out.append((name, keys, dict(wrap=wrap, mixed=mixed, bigthresh=bigthresh, large=large)))
    for n in (1, 2, 4, 5, 255, 256, 257, 511, 513, 767, 769):
        add("distinct%d" % n, set_uniform(n, m, seed=n))
    add("equal1000", set_equal(1000, m))
    for variant in ("plain", "run", "start", "both"):
        for nend in (1, 4, 5, 9, 300):
            for copies in (1, 2, 20):
                add("end_%s_%d_x%d" % (variant, nend, copies), set_table_end(nend, copies, m, variant), wrap=nend > 4 or variant in ("run", "both"))
    add("ovf_4_then_next_bucket", set_overflow(4, True, m))
    add("ovf_5_same_bucket", set_overflow(5, False, m))
    for chain in (2, 3, 40):
        add("ovf_chain%d" % chain, set_overflow(4 * chain + 1, False, m, fill=400 if chain == 40 else 100))
    add("gap_two_bins_40000_slots", set_two_bins(40000 // m, m))
    for over in (False, True):
        add("gap_one_block_%s" % ("over" if over else "under"), set_one_block_span(over, m))
        add("gap_first_block_%s" % ("over" if over else "under"), set_first_block_span(over, m))
    sb = sort_bits(3000)
    top = (1 << sb) - 1
    add("mixed_pairs_triples_run", set_mixed(3000, [(0x123456 & top, 2), (0x2468AC & top, 3), (0x400000 & top, 50), (0x7FFFFF & top, 2)]), mixed=True)
    add("mixed_adjacent_groups", set_mixed(3000, [(0x555555 & top, 50), ((0x555555 & top) + 1, 50)]), mixed=True)
    add("mixed_first_and_last", set_mixed(3000, [(0, 50), (top, 2)]), mixed=True)
    add("mixed_last_run_wraps", set_mixed(3000, [(0, 3), (top, 50)]), mixed=True)
    add("big_999_1000_1001", set_counts([999, 1000, 1001, 1, 2, 3]), bigthresh=1000)
    add("large_16_17_5000", set_counts([16, 17, 5000, 1, 1, 2, 15, 18]), large=True)
    add("large_and_big", set_counts([16, 17, 40, 1001, 1, 2]), bigthresh=1000, large=True)
    return out
