"""Stage II's contig structure (stage2.hip: contig_structure; prims.hip: prim_contig_scan) against a numpy model of its definitions, through
harc_amd_selftest_contigs: the one scan that makes head, cid, gstart and chead from flag[] and pos[], and the passes that take its place when a read
lies more than `cut` reads behind the last flag-'0' read or shard start before it.  A wave walks a segment of 2048 reads (more from 32 M reads on),
64 reads a trip: the sizes are the edges of both, the heads sit on either side of both, and the cut is small enough to be met."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEG = 2048          # reads a wave walks at the sizes used here
ZERO, ONE = ord("0"), ord("1")


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    h = harc_amd.HarcAmd(harc_amd.default_params(100))
    yield h
    h.close()


def model(flag, pos, L, q, cut):
    M = flag.size
    i = np.arange(M, dtype=np.int64)
    head1 = (flag == ZERO) | (i % q == 0)
    r = i - np.maximum.accumulate(np.where(head1, i, 0))
    head = head1 | ((r > 0) & (r % (cut + 1) == 0))
    cid = np.cumsum(head) - head
    d = np.where(head, np.where(i == 0, 0, L), pos.astype(np.int64))
    gstart = np.cumsum(d.astype(np.uint64), dtype=np.uint64)
    return head.astype(np.uint8), cid.astype(np.uint32), gstart, np.flatnonzero(head).astype(np.uint32), int(head.sum()), int(gstart[-1]) + L, bool(r.max() > cut)


def check(ctx, flag, pos, L, q, cut, what, fellback=None):
    flag = np.asarray(flag, dtype=np.uint8)
    pos = np.asarray(pos, dtype=np.uint8)
    want = model(flag, pos, L, q, cut)
    got = ctx.selftest_contigs(flag, pos, L, q, cut)
    if fellback is not None:
        assert want[6] == fellback, what + ": the case does not do what it was made for"
    for name, g, w in zip(("head", "cid", "gstart", "chead"), got[:4], want[:4]):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs first at %s" % (what, name, np.flatnonzero(g != w)[:4] if g.shape == w.shape else "its length")
    assert got[4:] == want[4:], "%s: (contigs, columns, fell back) = %r, the model %r" % (what, got[4:], want[4:])


def random_case(M, seed, p_head=0.05):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(M) < p_head, ZERO, ONE).astype(np.uint8), rng.integers(0, 256, size=M).astype(np.uint8)


def flags_with_heads(M, heads):
    f = np.full(M, ONE, dtype=np.uint8)
    f[np.asarray(heads, dtype=np.int64)] = ZERO
    return f


@pytest.mark.parametrize("M", [1, 63, 64, 65])
def test_smallest_sizes(M, ctx):
    flag, pos = random_case(M, 100 + M, 0.2)
    for q in (1, 7, M):
        check(ctx, flag, pos, 100, q, 10000000, "M = %d, q = %d" % (M, q), fellback=False)


@pytest.mark.parametrize("k", range(7, 18))
def test_sizes_around_every_power_of_two(k, ctx):
    for M in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        flag, pos = random_case(M, 9000 + M)
        check(ctx, flag, pos, 100, 1 + (M - 1) // 8, 10000000, "random heads, M = %d" % M, fellback=False)


M5 = 5 * SEG + 100


def test_heads_at_the_edges_of_segments_and_trips(ctx):
    rng = np.random.default_rng(5)
    pos = rng.integers(0, 256, size=M5).astype(np.uint8)
    edges = [63, 64, 127, 128, SEG - 1, SEG, SEG + 63, SEG + 64, 2 * SEG - 1, 3 * SEG, 5 * SEG - 1, 5 * SEG, M5 - 1]
    check(ctx, flags_with_heads(M5, edges), pos, 100, M5, 10000000, "heads at the edges", fellback=False)
    check(ctx, flags_with_heads(M5, edges[::2]), pos, 37, M5, 10000000, "every other edge", fellback=False)


def test_segments_without_a_head(ctx):
    rng = np.random.default_rng(6)
    pos = rng.integers(0, 256, size=M5).astype(np.uint8)
    check(ctx, flags_with_heads(M5, [5, 4 * SEG + 5]), pos, 100, M5, 10000000, "three segments without a head", fellback=False)


def test_all_heads_and_only_read_0(ctx):
    rng = np.random.default_rng(7)
    pos = rng.integers(0, 256, size=M5).astype(np.uint8)
    check(ctx, np.full(M5, ZERO, dtype=np.uint8), pos, 100, M5, 10000000, "all heads", fellback=False)
    check(ctx, np.full(M5, ONE, dtype=np.uint8), pos, 100, M5, 10000000, "only read 0 a head", fellback=False)


@pytest.mark.parametrize("q", [1, 2, 63, 64, 100, 127, 128, 129, 2048, 3000, M5 - 1, M5])
def test_shard_lengths(q, ctx):
    """q = 1, q = M, and lengths that do not divide M, on either side of the 128 from which on a trip holds one shard start at most"""
    flag, pos = random_case(M5, 300 + q, 0.01)
    check(ctx, flag, pos, 100, q, 10000000, "q = %d" % q, fellback=False)
    if q > 1:
        check(ctx, np.full(M5, ONE, dtype=np.uint8), pos, 100, q, 10000000, "q = %d, no flag '0'" % q, fellback=False)


@pytest.mark.parametrize("value", [0, 255])
def test_pos_at_its_ends(value, ctx):
    flag, _ = random_case(M5, 11)
    check(ctx, flag, np.full(M5, value, dtype=np.uint8), 255, 1 + (M5 - 1) // 3, 10000000, "every pos %d" % value, fellback=False)


def test_columns_beyond_32_bits(ctx):
    """17 M reads of 255 columns each: gstart passes 2^32 (no smaller input does: a read adds 255 columns at most)"""
    M = 17000000
    rng = np.random.default_rng(12)
    flag = np.where(rng.random(M) < 0.001, ZERO, ONE).astype(np.uint8)
    want_total = model(flag, np.full(M, 255, dtype=np.uint8), 255, 1 + (M - 1) // 8, 10000000)[5]
    assert want_total > 1 << 32
    check(ctx, flag, np.full(M, 255, dtype=np.uint8), 255, 1 + (M - 1) // 8, 10000000, "columns beyond 2^32", fellback=False)


def gap_case(M, a, g):
    """every read a head but reads a + 1 .. a + g: the longest distance to a head is g"""
    f = np.full(M, ZERO, dtype=np.uint8)
    f[a + 1:a + 1 + g] = ONE
    return f


@pytest.mark.parametrize("cut", [5, 1000])
def test_longest_gap_at_the_cut_and_one_beyond(cut, ctx):
    rng = np.random.default_rng(cut)
    pos = rng.integers(0, 256, size=M5).astype(np.uint8)
    starts = {"inside a segment": SEG + 100, "inside a trip": 64 * 3 + 1 if cut == 5 else 64 * 3, "over a segment's end": 2 * SEG - 3, "at the first read": 0,
              "to the last read": M5 - 1 - cut - 1}
    for where, a in starts.items():
        if where != "to the last read":
            check(ctx, gap_case(M5, a, cut), pos, 100, M5, cut, "gap of cut = %d %s" % (cut, where), fellback=False)
        else:
            check(ctx, gap_case(M5, a + 1, cut), pos, 100, M5, cut, "gap of cut = %d %s" % (cut, where), fellback=False)
        check(ctx, gap_case(M5, a, cut + 1), pos, 100, M5, cut, "gap of cut + 1 = %d %s" % (cut + 1, where), fellback=True)


@pytest.mark.parametrize("cut", [5, 1000])
def test_gaps_over_several_segments(cut, ctx):
    rng = np.random.default_rng(50 + cut)
    pos = rng.integers(0, 256, size=M5).astype(np.uint8)
    check(ctx, gap_case(M5, SEG - 10, 3 * SEG + 7), pos, 100, M5, cut, "a gap over three segments, cut %d" % cut, fellback=True)
    check(ctx, np.full(M5, ONE, dtype=np.uint8), pos, 100, M5, cut, "no head but read 0, cut %d" % cut, fellback=True)
    # shard starts end a gap as a flag '0' does: shards of cut + 1 reads never reach the cut, shards of cut + 2 do
    check(ctx, np.full(M5, ONE, dtype=np.uint8), pos, 100, cut + 1, cut, "shards of cut + 1 reads", fellback=False)
    check(ctx, np.full(M5, ONE, dtype=np.uint8), pos, 100, cut + 2, cut, "shards of cut + 2 reads", fellback=True)
    flag, pos2 = random_case(M5, 60 + cut, 0.3 / cut)
    check(ctx, flag, pos2, 100, 1 + (M5 - 1) // 3, cut, "random heads, a few gaps beyond the cut %d" % cut, fellback=True)
