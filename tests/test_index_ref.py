"""The index contract's checker can fail (no GPU): tests/index_ref.py's sequential reference builder makes tables for the crafted key sets of
tests/test_gpu_index.py, check_table accepts them, and rejects every single mutation with a message that names the clause."""
import numpy as np
import pytest

from tests import index_ref as ix
from tests import index_sets as sx


def test_scramble_round_trips_and_matches_the_written_out_rounds():
    rng = np.random.default_rng(0)
    k = np.concatenate([sx._rand_h(rng, 5000), np.array([0, 1, 0xFFFFFFFF, 1 << 32, (1 << 64) - 1], dtype=np.uint64)])
    assert np.array_equal(ix.unscramble(ix.scramble(k)), k) and np.array_equal(ix.scramble(ix.unscramble(k)), k)
    assert np.unique(ix.scramble(k)).size == np.unique(k).size
    for key in (0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF, 1):      # devutil.h key_scramble, in Python integers
        a, b, M = key & 0xFFFFFFFF, key >> 32, 0xFFFFFFFF
        y = a * 0x9E3779B1 & M; b ^= y ^ (y >> 15)
        y = b * 0x85EBCA77 & M; a ^= y ^ (y >> 13)
        y = a * 0xC2B2AE3D & M; b ^= y ^ (y >> 16)
        assert int(ix.scramble(key)[0]) == (b << 32) | a


def test_home_is_monotone_and_first_h_is_the_bucket_edge():
    for cap in (8, 20, 1280, 280004):
        nb = cap // 4
        for b in (0, 1, nb // 2, nb - 1):
            lo, hi = ix.first_h(b, cap), ix.first_h(b + 1, cap) - 1
            assert int(ix.home(lo, cap)) == 4 * b == int(ix.home(hi, cap))
            assert b == 0 or int(ix.home(lo - 1, cap)) == 4 * (b - 1)
    assert int(ix.home(sx.H1, 20)) == 16 and ix.first_h(5, 20) == 1 << 64
    assert ix.sort_bits(3000) == 24 and ix.sort_bits(210000) == 32 and ix.sort_bits(1) == 16 and ix.sort_bits(65536) == 24 and ix.sort_bits(65537) == 32


@pytest.mark.parametrize("m", [2, 4])
def test_reference_builder_satisfies_the_contract_on_every_crafted_set(m):
    for name, keys, p in sx.crafted_sets(m):
        cap = ix.cap_for(keys.size, m)
        nbins, slots, ids, large, wrapped = ix.build_ref(keys, cap, p["bigthresh"])
        if p["wrap"] is not None:
            assert (wrapped > 0) == p["wrap"], (name, wrapped)
        if p["mixed"]:
            assert ix.sort_bits(keys.size) == 24 and sx.mixed_places(keys)[1] > 0, name
        ix.check_table(keys, cap, nbins, slots, ids, p["bigthresh"], large)
        hu = np.unique(ix.scramble(keys))
        ab = np.sort(ix.scramble(ix.absent_probes(hu, cap)))
        for some in (hu[:64], hu[-64:], ab[:32], ab[-64:]):       # the table's end, where the wrapped bins and their absent neighbours are, included
            got = ix.lookup_many(slots, cap, some)
            assert [ix.lookup(slots, cap, x) for x in some] == got.tolist() and ((got >= 0) == np.isin(some, hu)).all(), name


def test_overflow_boundary_sets_are_what_they_claim():
    for m in (2, 4):
        by = {name: keys for name, keys, _ in sx.crafted_sets(m)}
        for name, flagged in (("ovf_4_then_next_bucket", False), ("ovf_5_same_bucket", True), ("ovf_chain40", True)):
            cap = ix.cap_for(by[name].size, m)
            slots = ix.build_ref(by[name], cap)[1]
            b = sx.overflow_bucket(cap)
            assert (slots["count"][4 * b:4 * b + 4] != 0).all() and bool(slots["count"][4 * b] & ix.SLOT_OVF) == flagged, name
        cap = ix.cap_for(by["ovf_chain40"].size, m)
        slots, b = ix.build_ref(by["ovf_chain40"], cap)[1], sx.overflow_bucket(cap)
        assert all(slots["count"][4 * (b + j)] & ix.SLOT_OVF for j in range(40)) and slots["count"][4 * (b + 40) + 1] == 0


def _table(name, m=4):
    keys, p = next((k, p) for n, k, p in sx.crafted_sets(m) if n == name)
    cap = ix.cap_for(keys.size, m)
    nbins, slots, ids, large, _ = ix.build_ref(keys, cap, p["bigthresh"])
    return [keys, cap, nbins, slots.copy(), ids.copy(), p["bigthresh"], large.copy()]


def _rejects(t, clause):
    with pytest.raises(ix.ContractError, match="clause %s" % clause):
        ix.check_table(*t)


@pytest.mark.parametrize("name", ["ovf_5_same_bucket", "ovf_chain3", "end_plain_9_x2", "end_both_5_x1"])
def test_a_needed_overflow_flag_cleared_is_rejected(name):
    t = _table(name)
    flagged = np.flatnonzero(t[3]["count"] & ix.SLOT_OVF)
    assert flagged.size
    for s in flagged:                                             # every flag the reference builder sets is needed
        u = _table(name)
        u[3]["count"][s] &= ~np.uint32(ix.SLOT_OVF)
        _rejects(u, 3)


def test_a_never_ending_search_is_rejected():
    keys = sx.set_uniform(8, 4)
    slots = np.zeros(8, dtype=ix.SLOT)
    slots["key"], slots["count"], slots["start"] = np.sort(ix.scramble(keys)), 1 | ix.SLOT_EMB, 0
    slots["count"][::4] |= ix.SLOT_OVF
    with pytest.raises(ix.ContractError, match="clause 5"):
        ix.lookup(slots, 8, 12345)
    with pytest.raises(ix.ContractError, match="clause 5"):
        ix.lookup_many(slots, 8, [12345])


def test_single_mutations_are_rejected():
    name = "large_and_big"
    t = _table(name)
    live = np.flatnonzero(t[3]["count"])
    empty = np.flatnonzero(t[3]["count"] == 0)
    u = _table(name); u[3][live[2]] = (0, 0, 0); _rejects(u, 2)                                  # a bin removed
    u = _table(name); u[3][empty[-1]] = u[3][live[0]]; _rejects(u, 2)                           # a bin duplicated into an empty slot
    u = _table(name); u[3]["key"][empty[0]] = 0xA5A5A5A5A5A5A5A5; _rejects(u, 2)               # an empty slot holding stale bytes
    u = _table(name); u[3]["start"][empty[1]] = 7; _rejects(u, 2)
    u = _table(name); u[3]["count"][empty[2]] = ix.SLOT_OVF; _rejects(u, 2)
    multi = next(s for s in live if (t[3]["count"][s] & ix.SLOT_CNT_MASK) >= 16)
    st = int(t[3]["start"][multi])
    u = _table(name); u[4][[st, st + 1]] = u[4][[st + 1, st]]; _rejects(u, 3)                   # two ids swapped inside a bin
    two = next(s for s in live if (t[3]["count"][s] & ix.SLOT_CNT_MASK) == 2)
    u = _table(name); u[3]["count"][two] |= ix.SLOT_EMB; _rejects(u, 3)                         # SLOT_EMB on a bin of two
    u = _table(name); u[2] += 1; _rejects(u, 1)                                                  # nbins off by one
    u = _table(name); u[2] -= 1; _rejects(u, 1)
    u = _table(name); u[6][0] ^= np.uint64(2); _rejects(u, 6)                                    # a large-list entry naming the wrong slot
    u = _table(name); u[6] = u[6][1:]; _rejects(u, 6)
    u = _table(name); u[6] = np.concatenate([u[6], u[6][:1]]); _rejects(u, 6)
    big = next(s for s in live if t[3]["count"][s] & ix.SLOT_BIG)
    u = _table(name); u[3]["count"][big] &= ~np.uint32(ix.SLOT_BIG); _rejects(u, 3)
    u = _table(name); u[3]["count"][multi] |= ix.SLOT_BIG if multi != big else 0; u[3]["count"][two] |= ix.SLOT_BIG; _rejects(u, 3)
    u = _table(name); u[3]["count"][two] |= ix.SLOT_DEAD; _rejects(u, 3)
    u = _table(name); u[4][0] = u[4][1]; _rejects(u, 4)                                          # ids not a permutation
    u = _table(name); u[3]["count"][two] += 1; _rejects(u, 3)                                    # a wrong count
    one = next(s for s in live if t[3]["count"][s] & ix.SLOT_EMB)
    u = _table(name); u[3]["start"][one] ^= 1; _rejects(u, 3)                                    # a single-key bin naming another id
    u = _table(name); u[1] += 4; _rejects(u, 1)                                                  # cap and slots disagree


def test_a_bin_moved_in_front_of_its_home_is_rejected():
    t = _table("distinct257")
    live = np.flatnonzero(t[3]["count"])
    s = next(int(x) for x in live if x >= 8 and not t[3]["count"][x - 8:x - 4].any())
    t[3][s - 8], t[3][s] = t[3][s].copy(), (0, 0, 0)
    _rejects(t, 3)
