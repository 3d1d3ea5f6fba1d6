"""The contract of the index (the bucketed key -> bin table of harc_dict_build and its ids[] array), restated in plain numpy.

Nothing here comes from the library: the scramble, the home bucket, the probe rule, the checker and a small sequential reference builder are
written out again from the comments in harc_amd/csrc (devutil.h: key_scramble, bucket_slot; stage1.hip: the slot rule and the overflow flag;
stage2.hip: dict_lookup_b).  Only the constants are read from the sources, so that they cannot drift.

The contract does not say WHICH slot a bin gets: it says that the probe rule finds it.  A builder with another valid layout stays inside it.
tests/test_index_ref.py proves that check_table can fail; tests/test_gpu_index.py holds the GPU build to it, on the key sets of tests/index_sets.py."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLOT = np.dtype([("key", "<u8"), ("start", "<u4"), ("count", "<u4")])       # HashSlot, 16 bytes
M32 = np.uint64(0xFFFFFFFF)


def _const(name, *files):
    for f in files:
        m = re.search(r"^\s*#\s*define\s+%s\s+\(?\s*(0x[0-9A-Fa-f]+|\d+)[uU]?" % name, open(os.path.join(ROOT, "harc_amd", "csrc", f)).read(), re.M)
        if m:
            return int(m.group(1), 0)
    raise KeyError(name)


SLOT_DEAD, SLOT_EMB, SLOT_BIG, SLOT_OVF, SLOT_CNT_MASK = (_const(n, "internal.h") for n in ("SLOT_DEAD", "SLOT_EMB", "SLOT_BIG", "SLOT_OVF", "SLOT_CNT_MASK"))
LARGEBIN = _const("HARC_LARGEBIN", "stage1.hip", "internal.h")
TP_SPAN = _const("TP_SPAN", "stage1.hip")
MIXED_BUDGET = _const("MIXED_BUDGET", "stage1.hip")


class ContractError(AssertionError):
    pass


def _need(ok, clause, what):
    if not ok:
        raise ContractError("index contract, clause %s: %s" % (clause, what))


# ---- key_scramble: three 32-bit Feistel rounds; each round xors one half with a function of the other, so the rounds run backwards invert it
_C = (np.uint32(0x9E3779B1), np.uint32(0x85EBCA77), np.uint32(0xC2B2AE3D))
_S = (np.uint32(15), np.uint32(13), np.uint32(16))


def _halves(k):
    k = np.atleast_1d(np.asarray(k, dtype=np.uint64))
    return (k & M32).astype(np.uint32), (k >> np.uint64(32)).astype(np.uint32)


def _join(a, b):
    return (b.astype(np.uint64) << np.uint64(32)) | a.astype(np.uint64)


def _f(x, r):
    y = x * _C[r]                                                 # uint32 arrays wrap
    return y ^ (y >> _S[r])


def scramble(k):
    a, b = _halves(k)
    b = b ^ _f(a, 0)
    a = a ^ _f(b, 1)
    b = b ^ _f(a, 2)
    return _join(a, b)


def unscramble(h):
    a, b = _halves(h)
    b = b ^ _f(a, 2)
    a = a ^ _f(b, 1)
    b = b ^ _f(a, 0)
    return _join(a, b)


# ---- geometry
def cap_for(n, m):
    """slots of a table over n keys at m slots per read (harc_dict_alloc)"""
    return ((m * n + 4) + 3) & ~3


def home(h, cap):
    """bucket_slot: first slot of the 4-slot bucket of a scrambled key; the high word decides, monotonically"""
    h = np.asarray(h, dtype=np.uint64)
    return (((h >> np.uint64(32)) * np.uint64(cap // 4)) >> np.uint64(32)) * np.uint64(4)


def first_h(b, cap):
    """smallest scrambled key whose home is bucket b (b == cap / 4: 2^64)"""
    nb = cap // 4
    return (-((-b << 32) // nb)) << 32


def sort_bits(n):
    """top bits the build's first sort looks at (harc_dict_build, without HARC_AMD_SORT_BITS)"""
    lg = 1
    while (1 << lg) < n:
        lg += 1
    return min(64, 8 * ((lg + 8 + 7) // 8))


# ---- the probe rule
def lookup(slots, cap, h):
    """slot index of scrambled key h, or -1: the literal probe rule"""
    h = int(h)
    b = int(home(h, cap)) // 4
    for _ in range(cap // 4 + 1):
        for j in range(4):
            s = slots[4 * b + j]
            if int(s["count"]) == 0:
                return -1
            if int(s["key"]) == h:
                return 4 * b + j
        if not int(slots[4 * b]["count"]) & SLOT_OVF:
            return -1
        b = b + 1 if 4 * (b + 1) < cap else 0
    raise ContractError("index contract, clause 5: the search for %#x does not terminate (every bucket full and flagged)" % h)


def lookup_many(slots, cap, hs):
    """lookup for an array of keys, without walking: a search from bucket b runs through the buckets that are full and flagged and ends in the first
    one that is not; the key is found when it sits in that stretch, in front of the first empty slot of its bucket.  Keys in the table must be
    distinct (check_table looks at that first)."""
    hs = np.asarray(hs, dtype=np.uint64)
    nb = cap // 4
    cnt = slots["count"].reshape(nb, 4)
    empty = cnt == 0
    first_empty = np.where(empty.any(axis=1), empty.argmax(axis=1), 4)
    goes_on = (first_empty == 4) & ((cnt[:, 0] & SLOT_OVF) != 0)
    stops = np.flatnonzero(~goes_on)
    if stops.size == 0:
        raise ContractError("index contract, clause 5: no search terminates (every bucket full and flagged)")
    b = (home(hs, cap) // np.uint64(4)).astype(np.int64)
    j = np.searchsorted(stops, b)
    dist = np.where(j < stops.size, stops[np.minimum(j, stops.size - 1)], stops[0] + nb) - b      # buckets walked beyond the first
    live = np.flatnonzero(cnt.reshape(-1) != 0)
    tk = slots["key"][live]
    o = np.argsort(tk, kind="stable")
    tk, tp = tk[o], live[o]
    at = np.minimum(np.searchsorted(tk, hs), max(tk.size - 1, 0))
    if tk.size == 0:
        return np.full(hs.size, -1, dtype=np.int64)
    pos = np.where(tk[at] == hs, tp[at], -1).astype(np.int64)
    pb = pos // 4
    ok = (pos >= 0) & (((pb - b) % nb) <= dist) & ((pos % 4) < first_empty[np.maximum(pb, 0)])
    return np.where(ok, pos, -1)


def absent_probes(hu, cap):
    """UNSCRAMBLED keys that are not in the table and whose search runs where searches can go wrong: h +- 1 of the present values, and the first and
    last h of every bucket that holds the home of a present key"""
    hu = np.asarray(hu, dtype=np.uint64)
    one = np.uint64(1)
    b = np.unique((home(hu, cap) // np.uint64(4)).astype(np.int64))
    edge = [first_h(int(x), cap) for x in b] + [first_h(int(x) + 1, cap) - 1 for x in b]
    c = np.concatenate([hu + one, hu - one, np.array(edge, dtype=np.uint64)])      # (wraps at both ends of the key space: still a key)
    c = np.unique(c)
    return unscramble(c[~np.isin(c, hu)])


def _groups(keys):
    h = scramble(keys)
    order = np.argsort(h, kind="stable")                          # positions grouped by scrambled key, ascending inside a group
    hu, first, counts = np.unique(h[order], return_index=True, return_counts=True)
    return h, order, hu, first, counts


def check_table(keys, cap, nbins, slots, ids, bigthresh, large, tag=1):
    """raises ContractError naming the clause the table (cap, nbins, slots[cap], ids[n], large list or None) breaks for the unscrambled `keys`"""
    keys = np.asarray(keys, dtype=np.uint64)
    n = keys.size
    h, order, hu, first, counts = _groups(keys)
    # 1
    _need(cap % 4 == 0 and cap >= hu.size and len(slots) == cap, 1, "cap %d for %d distinct keys" % (cap, hu.size))
    _need(nbins == hu.size, 1, "nbins %d, distinct keys %d" % (nbins, hu.size))
    # 2
    live = (slots["count"] & SLOT_CNT_MASK) != 0
    _need(int(live.sum()) == nbins, 2, "%d slots hold a bin, nbins %d" % (int(live.sum()), nbins))
    _need(np.unique(slots["key"][live]).size == int(live.sum()), 2, "two slots hold the same key")
    stale = ~live & ((slots["key"] != 0) | (slots["start"] != 0) | (slots["count"] != 0))
    _need(not stale.any(), 2, "%d empty slots are not 16 zero bytes, the first at %d" % (int(stale.sum()), int(stale.argmax())))
    # 4 (before 3: a bin's id list is read through ids)
    _need(len(ids) == n and np.array_equal(np.sort(ids), np.arange(n, dtype=ids.dtype)), 4, "ids is not a permutation of 0 .. n-1")
    # 3
    pos = lookup_many(slots, cap, hu)
    miss = pos < 0
    _need(not miss.any(), 3, "%d keys are not found by the probe rule, the first %#x (home slot %d)" % (int(miss.sum()), int(hu[miss.argmax()]), int(home(hu[miss.argmax()], cap)) if miss.any() else 0))
    c = slots["count"][pos]
    st = slots["start"][pos].astype(np.int64)
    bad = (c & SLOT_CNT_MASK) != counts
    _need(not bad.any(), 3, "live count of key %#x is %d, it occurs %d times" % (int(hu[bad.argmax()]), int(c[bad.argmax()] & SLOT_CNT_MASK), int(counts[bad.argmax()])))
    _need(not (c & SLOT_DEAD).any(), 3, "SLOT_DEAD is set")
    one = counts == 1
    bad = ((c & SLOT_EMB) != 0) != one
    _need(not bad.any(), 3, "SLOT_EMB of key %#x does not match its count %d" % (int(hu[bad.argmax()]), int(counts[bad.argmax()])))
    bad = one & (st != order[first])
    _need(not bad.any(), 3, "single-key bin %#x carries id %d, the key is at %d" % (int(hu[bad.argmax()]), int(st[bad.argmax()]), int(order[first][bad.argmax()])))
    mst, mfirst, mcnt = st[~one], first[~one], counts[~one]
    _need(not (mst + mcnt > n).any(), 3, "a bin's ids[start : start + count] runs past n")
    if mcnt.size:
        off = np.arange(int(mcnt.sum())) - np.repeat(np.cumsum(mcnt) - mcnt, mcnt)
        got, want = ids[np.repeat(mst, mcnt) + off], order[np.repeat(mfirst, mcnt) + off]
        bad = got != want
        _need(not bad.any(), 3, "ids of a bin are not the ascending positions of its key: ids[%d] = %d, expected %d" % (int((np.repeat(mst, mcnt) + off)[bad.argmax()]), int(got[bad.argmax()]), int(want[bad.argmax()])))
    big = (counts > bigthresh) if bigthresh else np.zeros(counts.size, dtype=bool)
    bad = ((c & SLOT_BIG) != 0) != big
    _need(not bad.any(), 3, "SLOT_BIG of key %#x (count %d, bigthresh %d)" % (int(hu[bad.argmax()]), int(counts[bad.argmax()]), bigthresh))
    # the vectorised rule against the literal one, on a sample (long chains are walked in Python: a budget of bucket steps)
    budget = 20000
    for x in np.unique(np.concatenate([np.linspace(0, hu.size - 1, min(hu.size, 32)).astype(np.int64), np.arange(max(0, hu.size - 16), hu.size)]))[::-1]:      # the table's end first
        cost = int((pos[x] - int(home(hu[x], cap))) % cap) // 4 + 1
        if cost > budget:
            continue
        budget -= cost
        _need(lookup(slots, cap, hu[x]) == pos[x], 3, "the literal probe rule disagrees for %#x" % int(hu[x]))
    # 5
    ab = scramble(absent_probes(hu, cap))
    _need(not (lookup_many(slots, cap, ab) >= 0).any(), 5, "an absent key is found")
    for x in ab[np.unique(np.concatenate([np.linspace(0, ab.size - 1, min(ab.size, 32)).astype(np.int64), np.arange(max(0, ab.size - 16), ab.size)]))] if budget > 0 and hu.size < 5000 else []:
        _need(lookup(slots, cap, x) == -1, 5, "the literal probe rule finds the absent key %#x" % int(x))
    # 6
    if large is not None:
        want = np.sort((pos[counts > LARGEBIN].astype(np.uint64) << np.uint64(1)) | np.uint64(tag))
        got = np.sort(np.asarray(large, dtype=np.uint64))
        _need(np.array_equal(got, want), 6, "large list %s, expected %s" % (got[:8].tolist(), want[:8].tolist()))


# ---- sequential reference builder: a plain restatement, one bin after the other in the order of their scrambled keys.  The slot of a bin is
# max(its home, the slot behind the bin before it); a bin whose slot falls past the end takes the first free slot from 0.  The flags come from
# their DEFINITION, not from a rule about neighbours: bucket b is flagged when a bin whose home is b or an earlier bucket sits beyond b.
def build_ref(keys, cap, bigthresh=0, tag=1):
    """(nbins, slots, ids, large, wrapped): wrapped = how many bins lie past the end of the table"""
    h, order, hu, first, counts = _groups(np.asarray(keys, dtype=np.uint64))
    nb = cap // 4
    homes = home(hu, cap).astype(np.int64).tolist()
    place, prev = [], -1
    for hm in homes:
        prev = max(hm, prev + 1)
        place.append(prev)
    taken = np.zeros(cap, dtype=bool)
    taken[[s for s in place if s < cap]] = True
    free = wrapped = 0
    for i, s in enumerate(place):
        if s >= cap:
            while taken[free]:
                free += 1
            place[i], taken[free], wrapped = free, True, wrapped + 1
    passed = np.zeros(nb + 1, dtype=np.int64)                     # +1 where a stretch of buckets that a bin has left begins, -1 behind it
    for hm, s in zip(homes, place):
        if s >= hm:
            passed[hm // 4] += 1                                  # buckets home .. (its own - 1)
            passed[s // 4] -= 1
        else:
            passed[hm // 4] += 1                                  # wrapped: home .. the last bucket, then 0 .. (its own - 1)
            passed[0] += 1
            passed[s // 4] -= 1
    flagged = np.flatnonzero(np.cumsum(passed[:nb]) > 0)
    place = np.array(place, dtype=np.int64)
    slots = np.zeros(cap, dtype=SLOT)
    slots["key"][place] = hu
    slots["start"][place] = np.where(counts == 1, order[first], first)
    slots["count"][place] = np.where(counts == 1, 1 | SLOT_EMB, counts | np.where((counts > bigthresh) & (bigthresh > 0), SLOT_BIG, 0))
    slots["count"][4 * flagged] |= SLOT_OVF
    large = np.sort((place[counts > LARGEBIN].astype(np.uint64) << np.uint64(1)) | np.uint64(tag))
    return hu.size, slots, order.astype(np.uint32), large, wrapped
