"""The index build (harc_dict_build: k_table_place, the top-bits sort with k_mixed_*, the two fill paths) against the table's contract as
tests/index_ref.py restates it, through harc_amd_selftest_index: crafted key sets at the table's end, at the overflow-flag boundary, with long
gaps, with keys that share the sorted top bits, at the workgroup edges of the placement, and uniform keys.  Every set is made by choosing
scrambled values and unscrambling them; the slot array holds a non-zero byte pattern before every build."""
import time

import numpy as np
import pytest

from tests import index_ref as ix
from tests import index_sets as sx

pytestmark = pytest.mark.gpu

NAMES = [name for name, _, _ in sx.crafted_sets(4)]             # (built once per process, shared with tests/test_index_ref.py)
FILLS = (None, "0", "1")


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    h = harc_amd.HarcAmd(harc_amd.default_params(100))
    yield h
    h.close()


def _env(monkeypatch, fill=None, sort_bits=None):
    for k, v in (("HARC_AMD_TABLE_FILL", fill), ("HARC_AMD_SORT_BITS", sort_bits)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    monkeypatch.delenv("HARC_AMD_CAPMULT", raising=False)


def _build_and_check(ctx, keys, m, bigthresh=0, large=False, what=""):
    cap, nbins, slots, ids, lst = ctx.selftest_index(keys, slots_per_read=m, bigthresh=bigthresh, want_large=large)
    assert cap == ix.cap_for(keys.size, m), what
    try:
        ix.check_table(keys, cap, nbins, slots, ids, bigthresh, lst)
    except ix.ContractError as e:
        raise ix.ContractError("%s: %s" % (what, e)) from None
    return cap, slots


def _precondition(name, keys, m, p):
    cap = ix.cap_for(keys.size, m)
    ref_nbins, ref_slots, _, _, wrapped = ix.build_ref(keys, cap, p["bigthresh"])
    if p["wrap"] is not None:
        assert (wrapped > 0) == p["wrap"], "%s: %d bins past the end of the table" % (name, wrapped)
    if p["mixed"]:
        assert ix.sort_bits(keys.size) == 24 and sx.mixed_places(keys)[1] > 0
    if name == "gap_two_bins_40000_slots":
        assert ref_nbins == 2 and cap >= 40000 > 30 * ix.TP_SPAN
    if name.startswith("gap_one_block"):
        assert ref_nbins == 256 and (cap > ix.TP_SPAN) == name.endswith("over") and abs(cap - ix.TP_SPAN) <= 4
    if name.startswith("gap_first_block"):
        last = int(np.flatnonzero(ref_slots["count"])[255])       # slot of the first workgroup's last bin: the stretch is [0, last]
        assert ref_nbins > 256 and wrapped == 0 and (last + 1 > ix.TP_SPAN) == name.endswith("over") and abs(last + 1 - ix.TP_SPAN) <= 4


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("name", NAMES)
def test_crafted_set_satisfies_the_contract(name, m, ctx, monkeypatch):
    """every crafted set, with the table cleared by a memset, by the placement, or as the library chooses; sorted on the library's choice of top bits and
    on all 64.  The set's own precondition (bins past the end of the table, keys that share the sorted top bits, a stretch
    longer than the LDS tile) is asserted with the reference builder before the GPU is asked"""
    keys, p = next((k, p) for n, k, p in sx.crafted_sets(m) if n == name)
    _precondition(name, keys, m, p)
    for fill in FILLS:
        for sb in (None, "64"):                                  # (on the mixed sets the 64-bit sort is the table k_mixed_fix's has to equal in every contract clause)
            _env(monkeypatch, fill, sb)
            _build_and_check(ctx, keys, m, p["bigthresh"], p["large"], "%s m=%d TABLE_FILL=%s SORT_BITS=%s" % (name, m, fill, sb))


@pytest.mark.parametrize("m", [2, 4])
def test_overflow_boundary_every_key_and_every_neighbour_resolves(m, ctx, monkeypatch):
    """four bins fill bucket b and the fifth has its home in b + 1: nothing whose home is b or earlier lies beyond b.  With the fifth's home in b the
    bucket needs its flag.  Either way the bins of b and b + 1, their neighbours h +- 1 and the edges of both buckets resolve by the LITERAL probe rule"""
    _env(monkeypatch)
    for name in ("ovf_4_then_next_bucket", "ovf_5_same_bucket", "ovf_chain2", "ovf_chain3", "ovf_chain40"):
        keys = next(k for n, k, _ in sx.crafted_sets(m) if n == name)
        cap, slots = _build_and_check(ctx, keys, m, what=name)
        b = sx.overflow_bucket(cap)
        hu = np.unique(ix.scramble(keys))
        near = hu[(ix.home(hu, cap) >= 4 * b) & (ix.home(hu, cap) <= 4 * b + 4)]
        assert near.size >= 5
        for h in near:
            s = ix.lookup(slots, cap, h)
            assert s >= 4 * b and int(slots["key"][s]) == int(h), name
        present = set(int(x) for x in hu)
        for h in [int(x) + d for x in near for d in (-1, 1)] + [ix.first_h(b, cap), ix.first_h(b + 1, cap) - 1, ix.first_h(b + 1, cap), ix.first_h(b + 2, cap) - 1]:
            assert h in present or ix.lookup(slots, cap, h) == -1, name


@pytest.mark.parametrize("m", [2, 4])
def test_one_bin_of_70000_keys(m, ctx, monkeypatch):
    for fill in FILLS:
        for sb in (None, "64"):
            _env(monkeypatch, fill, sb)
            _build_and_check(ctx, sx.set_equal(70000, m), m, bigthresh=16, large=True, what="70000 equal keys TABLE_FILL=%s SORT_BITS=%s" % (fill, sb))


@pytest.mark.parametrize("m", [2, 4])
@pytest.mark.parametrize("seed", range(20))
def test_uniform_keys_with_duplicates(seed, m, ctx, monkeypatch):
    """with TABLE_FILL = 1 a natural table in which some workgroups of the placement stage their stretch in LDS and others (many copies, long gaps) do not;
    with 0 uniform keys behind a memset; unset, the library's rule picks between them by the share of distinct keys"""
    keys = sx.set_random(seed)
    for fill in FILLS:
        for sb in (None, "64"):
            _env(monkeypatch, fill, sb)
            _build_and_check(ctx, keys, m, bigthresh=16, large=True, what="seed %d (n = %d) TABLE_FILL=%s SORT_BITS=%s" % (seed, keys.size, fill, sb))


@pytest.mark.parametrize("m", [2, 4])
def test_stretch_beyond_the_budget_falls_back_to_the_full_sort(m, ctx, monkeypatch, capfd):
    """210 000 distinct keys that share the 32 top bits the first sort looks at, in descending order: one stretch, longer than MIXED_BUDGET.  The build
    has to notice, sort again on all 64 bits, and still satisfy the contract (a chain of 210 000 slots behind one home bucket an eighth into the table:
    it ends inside the table at either capacity)"""
    monkeypatch.setenv("HARC_AMD_TRACE", "1")
    n = 210000
    keys = sx.set_fallback(n, m)
    assert n > ix.MIXED_BUDGET and ix.sort_bits(n) == 32 and np.unique(ix.scramble(keys) >> np.uint64(32)).size == 1 and sx.mixed_places(keys) == (n - 1, n - 1)
    assert ix.build_ref(keys, ix.cap_for(n, m))[4] == 0
    for fill in FILLS:
        _env(monkeypatch, fill)
        capfd.readouterr()
        _build_and_check(ctx, keys, m, what="fallback m=%d TABLE_FILL=%s" % (m, fill))
        err = capfd.readouterr().err
        assert "sort on the top 32 bits" in err and "too many or too long, sorting on all bits" in err and "sort on the top 64 bits" in err


def test_bins_far_beyond_the_end_fail_loudly_and_leave_the_context_usable(ctx, monkeypatch):
    """20 000 bins whose home is the last bucket at 4 slots per read: 79 workgroups of bins, those of the first 15 lie beyond the reach of the pass that
    wraps bins round (the last 64 workgroups).  An error decided by a counter: HARC_AMD_EINVAL, and the next build on the same context is right.
    Measured on an MI355X: the failing build takes 0.145 s (pass 1's serial walk from slot 0 over 16 160 bins included), so the case stays at 20 000 bins."""
    import harc_amd
    _env(monkeypatch)
    keys = sx.set_loud(20000)
    assert (ix.home(ix.scramble(keys), ix.cap_for(keys.size, 4)) == ix.cap_for(keys.size, 4) - 4).all() and (20000 + 255) // 256 > 64 + 1
    t0 = time.time()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        ctx.selftest_index(keys, slots_per_read=4)
    print("failing build of 20000 bins beyond the end: %.3f s" % (time.time() - t0))
    assert e.value.code == -1 and "beyond the end of the table" in str(e.value)
    for name in ("distinct769", "end_both_9_x2", "large_and_big"):
        keys, p = next((k, p) for n, k, p in sx.crafted_sets(4) if n == name)
        _build_and_check(ctx, keys, 4, p["bigthresh"], p["large"], "after the failed build: " + name)


def test_hook_refuses_bad_arguments_and_stays_usable(ctx, monkeypatch):
    import ctypes as C
    import harc_amd
    _env(monkeypatch)
    keys = sx.set_uniform(100, 4)
    cap, l = C.c_uint64(0), harc_amd.lib()
    assert l.harc_amd_selftest_index(ctx._ctx, keys.ctypes.data, 100, 5, 0, 0, C.byref(cap), None, None, None, None, 0, None) == -1
    assert l.harc_amd_selftest_index(ctx._ctx, keys.ctypes.data, 0, 4, 0, 0, C.byref(cap), None, None, None, None, 0, None) == -1
    assert l.harc_amd_selftest_index(ctx._ctx, keys.ctypes.data, 100, 4, 0, 0, C.byref(cap), None, None, None, None, 0, None) == 0 and cap.value == 404
    nb, buf, ids = C.c_uint32(0), np.zeros(400, dtype=ix.SLOT), np.zeros(100, dtype=np.uint32)
    cap.value = 400                                               # room for fewer slots than the table has
    assert l.harc_amd_selftest_index(ctx._ctx, keys.ctypes.data, 100, 4, 0, 0, C.byref(cap), C.byref(nb), buf.ctypes.data, ids.ctypes.data, None, 0, None) == -1
    assert not buf["count"].any()
    for m, want in ((0, None), (2, 204), (3, 304), (4, 404)):
        c2, nbins, slots, ids, _ = ctx.selftest_index(keys, slots_per_read=m)
        assert want is None or c2 == want
        ix.check_table(keys, c2, nbins, slots, ids, 0, None)


# ---- the kernels' own lookups on tables whose bins wrap round the end, against the oracle: k_succ / k_steps on stage I's, dict_lookup_b on stage II's
_BASE_CODE = np.zeros(256, dtype=np.uint64)
for _i, _ch in enumerate(b"AGCT"):
    _BASE_CODE[_ch] = _i


def _dict_keys(clean, start):
    """the 64-bit key of bases [start, start + 32) of every read: base j at bits 2j, A 0 G 1 C 2 T 3"""
    return (_BASE_CODE[clean[:, start:start + 32]] << (np.uint64(2) * np.arange(32, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


@pytest.fixture(scope="module")
def table_end_reads(oracle, tmp_path_factory):
    from tests import gen
    from tests.test_gpu_parity import _oracle_pipeline
    txt, planted = gen.reads_text_table_end(5)
    want = {}
    for K, S, E in ((1, 16, 1), (8, 16, 3)):
        want[K, S, E] = _oracle_pipeline(oracle, txt, 100, K, E, tmp_path_factory.mktemp("o%d" % K), S)[:3]
    return txt, planted, want


@pytest.mark.parametrize("succ", [None, "0"])
@pytest.mark.parametrize("capmult", [None, "2"])
@pytest.mark.parametrize("K,S,E", [(1, 16, 1), (8, 16, 3)])
def test_reads_whose_kmers_wrap_round_the_table_end_match_oracle(K, S, E, capmult, succ, table_end_reads, tmp_path, monkeypatch):
    """twelve k-mers whose home is the last bucket of both STAGE-I dictionaries, read at shifts -6 .. 6 and in both orientations: eight and more of the bins
    lie past the end of either table and wrap to its start, where k_succ / k_steps have to find them (stage II's tables hold other keys: the test below).
    All files equal the oracle's and the decoder returns the input multiset."""
    import harc_amd
    from tests import oracle_lib as ol
    from tests.test_gpu_parity import assert_same
    txt, planted, want = table_end_reads
    inputs, s1, s2 = want[K, S, E]
    rows = [l for l in txt.split(b"\n") if l]
    clean = np.frombuffer(b"".join(l for l in rows if b"N" not in l), dtype=np.uint8).reshape(-1, 100)
    for start in (18, 50):                                        # the point of the input: bins past the end of both tables at this capacity
        keys = _dict_keys(clean, start)
        assert np.isin(planted, keys).all()
        assert ix.build_ref(keys, ix.cap_for(keys.size, int(capmult or 4)))[4] >= 8
    for k, v in (("HARC_AMD_CAPMULT", capmult), ("HARC_AMD_SUCC", succ)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    base = ol.stage_dir(tmp_path, {k: inputs[k] for k in ["input_clean.dna", "numreads.bin", "input_N.dna", "read_order_N.bin"]})
    what = "K=%d S=%d E=%d CAPMULT=%s SUCC=%s" % (K, S, E, capmult, succ)
    harc_amd.reorder(base, 100, num_chains=K, num_steps=S)
    assert_same(ol.read_dir(base), s1, ol.STAGE1_FILES, what + ": stage I vs oracle")
    harc_amd.encoder(base, 100, num_thr=E)
    assert_same(ol.read_dir(base), s2, ol.stage2_files(E), what + ": stage II vs oracle")
    harc_amd.decoder(base, E)
    assert sorted(ol.read_dir(base)["output.dna"].split()) == sorted(rows)


@pytest.fixture(scope="module")
def table_end_reads_stage2(oracle, tmp_path_factory):
    from tests import gen
    from tests.test_gpu_parity import _oracle_pipeline
    txt, mers = gen.reads_text_table_end_stage2(9)
    want = {}
    for K, S, E in ((1, 16, 1), (8, 16, 3)):
        want[K, S, E] = _oracle_pipeline(oracle, txt, 100, K, E, tmp_path_factory.mktemp("p%d" % K), S)[:3]
    return txt, mers, want


def _lines(b):
    rows = [l for l in b.split(b"\n") if l]
    return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)


@pytest.mark.parametrize("capmult", [None, "2"])
@pytest.mark.parametrize("K,S,E", [(1, 16, 1), (8, 16, 3)])
def test_candidates_whose_kmers_wrap_round_the_stage2_table_end_match_oracle(K, S, E, capmult, table_end_reads_stage2, tmp_path, monkeypatch):
    """stage II's dictionaries are built over the singletons and the reads with N, keyed by the 3-bit-coded bases 0-20 and 21-41.  Twelve 42-mers whose two
    keys have their home in the last bucket of either table begin three reads with N each: nine and more bins of each table lie past its end and wrap to
    its start, where dict_lookup_b has to find them when the consensus passes -- and does, in the oracle: most of the 36 reads are aligned.  All files
    equal the oracle's and the decoder returns the input multiset."""
    import harc_amd
    from tests import gen, oracle_lib as ol
    from tests.test_gpu_parity import assert_same
    txt, mers, want = table_end_reads_stage2
    inputs, s1, s2 = want[K, S, E]
    cand = np.concatenate([_lines(s1["temp.dna.singleton"]), _lines(s1["input_N.dna"])])       # the candidates, from the oracle's stage-I output
    cap = ix.cap_for(cand.shape[0], int(capmult or 4))
    assert cap // 4 <= 2048                                       # the generator's max_buckets: its k-mers are in the last bucket of any smaller table
    for start in (0, 21):                                         # the point of the input: bins past the end of both stage-II tables at this capacity
        keys = gen.keys3(cand, start)
        assert np.isin(gen.keys3(mers, start), keys).all()
        assert ix.build_ref(keys, cap)[4] >= 8
    left = _lines(s2["input_N.dna"])
    n_left = int(sum((left[:, :42] == p).all(axis=1).sum() for p in mers))
    assert n_left <= 12, "%d of the 36 planted reads stay unaligned in the oracle: the lookups that find them are not made" % n_left
    for k, v in (("HARC_AMD_CAPMULT", capmult),):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    base = ol.stage_dir(tmp_path, {k: inputs[k] for k in ["input_clean.dna", "numreads.bin", "input_N.dna", "read_order_N.bin"]})
    what = "K=%d S=%d E=%d CAPMULT=%s" % (K, S, E, capmult)
    harc_amd.reorder(base, 100, num_chains=K, num_steps=S)
    assert_same(ol.read_dir(base), s1, ol.STAGE1_FILES, what + ": stage I vs oracle")
    harc_amd.encoder(base, 100, num_thr=E)
    assert_same(ol.read_dir(base), s2, ol.stage2_files(E), what + ": stage II vs oracle")
    harc_amd.decoder(base, E)
    assert sorted(ol.read_dir(base)["output.dna"].split()) == sorted(l for l in txt.split(b"\n") if l)
