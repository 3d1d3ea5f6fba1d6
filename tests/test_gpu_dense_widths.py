"""The DENSE chain kernels against the CPU oracle at every packed-read width (run with -m gpu).

Stage I's k_steps is compiled once per width W = ceil(2L/64), W = 1 ... 8, and a run of more than 16 384 chains -- every BASELINE-sized run -- takes one
of its three dense forms: the lanes scanning their own bins (k_steps<W, false, false>), the wave-uniform scan (SEQ) and the specialised SEQ kernel
(SPEC: W >= 4, 64-bit keys, bitmap lines by minimizer).  Their column counts live in LDS (ConsState<W, true>), their register and wave budget depends on
W, SEQ has a candidate test, a slot search and a lazy application of the counts of its own.  A dense kernel with a subtly wrong Hamming window, consensus
column or key still decodes losslessly and is still deterministic, so only a comparison with the schedule of DESIGN.md section 2 (the oracle) can tell.

Part A forces every dense form (as test_gpu_parity.py::test_kernel_variants_same_bytes does at L = 100) on small inputs at both sides of every 64-bit
boundary of the 2-bit store: the smallest and the largest L of every W, plus the headline lengths.  L = 97 ... 99 have 62-bit keys (SPEC falls back to the
general kernel), L >= 100 has 64-bit keys (SPEC is taken from W = 4 on); below 100 bp the minimizer lines have other window counts than 17.
Part B is the regime itself: 20 000 chains (k_reseed_mg, S by the index rule, the back-off, the dense launch by the library's own rule) at W = 2, 4, 5, 8.

Every stage-I and every stage-II file of the HIP path must be the oracle's, byte for byte; then the streams are decoded (the oracle's restatement of
decoder.cpp) and compared with the input as a multiset, which tells a wrong schedule (other bytes, lossless) from a wrong encoder."""
import concurrent.futures as cf

import numpy as np
import pytest

from tests import gen
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

S1_STREAMS = {"temp.dna": "S1_DNA", "temp.dna.singleton": "S1_DNA_SINGLETON", "read_rev.txt": "S1_RC", "tempflag.txt": "S1_FLAG", "temppos.txt": "S1_POS",
              "read_order.bin": "S1_ORDER", "read_order.bin.singleton": "S1_ORDER_SINGLETON"}              # files.cpp write_stage1
S2_SHARD_STREAMS = {"read_seq.txt.%d": "S2_SEQ", "read_seq.txt.%d.tail": "S2_SEQ_TAIL", "read_pos.txt.%d": "S2_POS", "read_noise.txt.%d": "S2_NOISE",
                    "read_noisepos.txt.%d": "S2_NOISEPOS", "read_rev.txt.%d": "S2_REV", "read_rev.txt.%d.tail": "S2_REV_TAIL"}
S2_STREAMS = {"read_order.bin": "S2_ORDER", "read_order_N_pe.bin": "S2_ORDER_N_PE", "input_N.dna": "S2_INPUT_N", "read_meta.txt": "S2_META",
              "read_singleton.txt": "S2_SINGLETON", "read_singleton.txt.tail": "S2_SINGLETON_TAIL"}        # files.cpp write_stage2
assert sorted(S1_STREAMS) == sorted(ol.STAGE1_FILES)

_DENSE_VARS = ("HARC_AMD_QUAD", "HARC_AMD_SEQ", "HARC_AMD_SPEC", "HARC_AMD_LAZY", "HARC_AMD_S1BLOOM_MZMB", "HARC_AMD_SEQ_REMEASURE", "HARC_AMD_BATCHSYNC")


def _diff(name, a, b):
    if a == b:
        return None
    n = min(len(a), len(b))
    first = next((i for i in range(n) if a[i] != b[i]), n)
    return f"{name}: len {len(a)} vs {len(b)}, first difference at byte {first}: {a[first:first+16]!r} vs {b[first:first+16]!r}"


def _diffs(got, want, files):
    """as assert_same of test_gpu_parity.py reports them: file, lengths, first differing byte"""
    return [d for d in (_diff(f, got.get(f, b"<missing>"), want[f]) for f in files) if d]


def _set_env(monkeypatch, env):
    for v in _DENSE_VARS:                                              # nothing inherited: the case alone says which kernel runs
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _matched_share(s1):
    """share of the clean reads that stage I put behind another read (tempflag.txt: one character per read, '1' = matched)"""
    return s1["tempflag.txt"].count(b"1") / max(1, len(s1["tempflag.txt"]))


def _oracle_run(oracle, d, txt, L, K, S, E):
    """-> (preprocessed inputs, stage-I files, stage-II files) of the oracle"""
    base = ol.stage_dir(d, {})
    assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
    inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna")}
    assert oracle.harc_oracle_reorder(base.encode(), L, K, S, None, None) == 0
    s1 = {f: v for f, v in ol.read_dir(base).items() if f in ol.STAGE1_FILES}
    assert oracle.harc_oracle_encoder(base.encode(), L, E, None, None) == 0
    s2 = {f: v for f, v in ol.read_dir(base).items() if f in ol.stage2_files(E)}
    for f in (d / "output").iterdir():
        f.unlink()
    return inputs, s1, s2


def _load(h, inputs, L):
    clean, withN = inputs["input_clean.dna"], inputs["input_N.dna"]
    h.set_reads_ascii(clean, len(clean) // (L + 1), L + 1)
    h.set_nreads_ascii(withN, len(withN) // (L + 1), L + 1)


def _gpu_run(h, E):
    """reorder + encode on the context -> (stage-I files, stage-II files) as files.cpp would write them"""
    h.reorder()
    s1 = {f: h.stream(s) for f, s in S1_STREAMS.items()}
    h.encode()
    s2 = {f: h.stream(s) for f, s in S2_STREAMS.items()}
    for e in range(E):
        s2.update({fmt % e: h.stream(s, e) for fmt, s in S2_SHARD_STREAMS.items()})
    assert sorted(s2) == sorted(ol.stage2_files(E))
    return s1, s2


def _roundtrip_error(oracle, d, s2, E, txt, L):
    """the HIP path's own streams through the oracle's decoder: None when they hold exactly the reads of the input"""
    base = ol.stage_dir(d, s2)
    if oracle.harc_oracle_decoder(base.encode(), E) != 0:
        return "the streams do not decode"
    out = np.frombuffer(ol.read_dir(base)["output.dna"], dtype=np.uint8)
    want = np.frombuffer(txt, dtype=np.uint8)
    if out.size != want.size:
        return f"the streams decode to {out.size} bytes, the input has {want.size}"
    v = np.dtype((np.void, L + 1))
    if not np.array_equal(np.sort(out.view(v)), np.sort(want.view(v))):
        return "the streams decode to OTHER reads than the input's"
    return None


def _check(oracle, d, got, want, E, txt, L, what):
    errs = _diffs(got[0], want[0], ol.STAGE1_FILES) + _diffs(got[1], want[1], ol.stage2_files(E))
    rt = _roundtrip_error(oracle, d, got[1], E, txt, L)
    if errs and not rt:
        errs.append("(these streams decode to the input's reads: another schedule, not a broken encoder)")
    if rt:
        errs.append("round trip: " + rt)
    assert not errs, what + "\n" + "\n".join(errs)


# ------------------------------------------------------------------------------------------------ part A
# both sides of every 64-bit boundary of the 2-bit store (W = 1 ... 8 at its smallest and its largest L) and the headline lengths 99 / 101 / 150
LENGTHS = [32, 33, 64, 65, 96, 97, 99, 101, 128, 129, 150, 160, 161, 192, 193, 224, 225, 255]
assert {(2 * L + 63) // 64 for L in LENGTHS} == set(range(1, 9))
FORMS = {
    "lanes": {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "0"},                                            # k_steps<W, false, false>
    "seq": {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1"},                                              # k_steps<W, false, false, 4, true>, hashed bitmap lines
    "seq_spec": {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1", "HARC_AMD_S1BLOOM_MZMB": "0"},           # SPEC where its conditions hold, else SEQ with lines by minimizer
    "seq_nospec": {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1", "HARC_AMD_S1BLOOM_MZMB": "0", "HARC_AMD_SPEC": "0"},      # the general kernel under SPEC's conditions
    "seq_eager": {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1", "HARC_AMD_LAZY": "0"},                  # every step applies its column counts
}
N_READS = 20000
INPUTS_A = {
    "iid": lambda L: gen.reads_text(2000 + L, N_READS, L, N_READS * L // 15, err=0.005),            # i.i.d. genome at 15x, 0.5 % errors, reads with N
    "rich": lambda L: gen.reads_text_lowcomplexity(3000 + L, N_READS, L, 50000, err=0.004),         # repeat copies and poly-A runs: bins of more than 16 reads
}


def schedule_a(L):
    """(K, S, E) drawn from L.  K fills more than one workgroup of four chains (61: a partly filled last one); S mostly 16 / 32, a few 1 and 64"""
    rs = np.random.RandomState(L)
    return int(rs.choice([24, 61, 300])), int(rs.choice([16, 32, 16, 32, 1, 64])), int(rs.choice([1, 3]))


@pytest.fixture(scope="module")
def oracle_a(oracle, tmp_path_factory):
    """the oracle's run of an (L, input) -- one per pair, not one per form"""
    root = tmp_path_factory.mktemp("dense_widths_a")
    cache = {}

    def get(L, name):
        if (L, name) not in cache:
            txt = INPUTS_A[name](L)
            K, S, E = schedule_a(L)
            d = root / f"L{L}_{name}"
            d.mkdir()
            cache[(L, name)] = (txt,) + _oracle_run(oracle, d, txt, L, K, S, E)
        return cache[(L, name)]
    return get




@pytest.mark.parametrize("L,name,form", [pytest.param(L, name, form, id=f"L{L}-{name}-{form}") for L in LENGTHS for name in INPUTS_A for form in FORMS])
def test_forced_dense_forms_match_oracle_at_every_width(L, name, form, oracle, oracle_a, tmp_path, monkeypatch):
    """a dense form forced on 20 000 reads with a few dozen to a few hundred chains: every file is the oracle's, the streams decode to the input, and
    the case is not vacuous -- the oracle matched more than 80 % of the reads (93 - 99 % on these inputs), the dense kernel walked steps, and on the
    repeat-rich input the cooperative kernel (with k_compact_bins) walked steps at this width too"""
    import harc_amd
    K, S, E = schedule_a(L)
    txt, inputs, s1, s2 = oracle_a(L, name)
    assert _matched_share(s1) > 0.80
    _set_env(monkeypatch, FORMS[form])
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        _load(h, inputs, L)
        got = _gpu_run(h, E)
        c = h.counters()
        dense_steps, coop_steps = int(c.dense_steps), int(c.coop_steps)
    _check(oracle, tmp_path, got, (s1, s2), E, txt, L, f"L={L} (W={(2 * L + 63) // 64}) {name} K={K} S={S} E={E} under {FORMS[form]!r}: HIP path vs oracle")
    assert dense_steps > 0
    if name == "rich":
        assert coop_steps > 0


# ------------------------------------------------------------------------------------------------ part B
LENGTHS_B = [64, 101, 150, 250]                                        # W = 2, 4, 5, 8
N_B, K_B, E_B = 300000, 20000, 4
INPUTS_B = {
    # name: (maker, steps per super-round the index rule must pick, first-dictionary k-mers of their own: more (True) or less (False) than 88 % of the reads)
    "clean": (lambda L: gen.lines_of(gen.reads_array_big(60 + L, N_B, L, N_B * L // 12, err=0.003)), 32, True),
    "rich": (lambda L: gen.reads_text_lowcomplexity(99, N_B, L, 750000, n_repeat=450, n_polya=12, err=0.004), 16, False),
}
CASES_B = {
    # name: (input, environment, super-rounds per look of the host at the counters)
    # the wave-uniform scan by the library's own rule.  (The oracle needs 7 super-rounds for these inputs: the run is over inside the first batch of eight,
    # the one that starts the measurement of the two scans, so nothing but the wave-uniform scan runs here ...
    "clean-auto": ("clean", {}, 8),
    # ... and this one does measure: batches of two super-rounds -- two with the wave-uniform scan, two with the lanes' own, the faster one from there on --
    # so both SEQ settings run in one job, and the second run on the context starts from the kept choice.)
    "clean-measure": ("clean", {"HARC_AMD_BATCHSYNC": "2"}, 2),
    "clean-mzmb0": ("clean", {"HARC_AMD_S1BLOOM_MZMB": "0"}, 8),     # lines by minimizer (a 300 k-read bitmap is too small for them otherwise): SPEC from 100 bp on
    "rich-auto": ("rich", {}, 8),                                      # the lanes' own scan next to the cooperative kernel and the back-off
    "rich-seq": ("rich", {"HARC_AMD_SEQ": "1", "HARC_AMD_S1BLOOM_MZMB": "0"}, 8),      # the wave-uniform form (SPEC from 100 bp on) on the same input
}


def _own_kmer_share(clean, L):
    """distinct first-dictionary k-mers / clean reads: stage1_run_w starts a dense run with the wave-uniform scan where it is above 0.88"""
    a = np.frombuffer(clean, dtype=np.uint8).reshape(-1, L + 1)
    w = 32 if L >= 100 else L * 32 // 100                              # harc:57-58
    return np.unique(np.ascontiguousarray(a[:, L // 2 - w:L // 2]), axis=0).shape[0] / a.shape[0]


@pytest.fixture(scope="module")
def oracle_b(oracle, tmp_path_factory):
    """{(L, input): (reads, preprocessed inputs, S, stage-I files, stage-II files, the oracle's super-rounds, k-mer share)}: the oracle's eight runs side by side in
    threads before the first comparison (ctypes releases the GIL, the oracle keeps no global state)"""
    import ctypes as C
    root = tmp_path_factory.mktemp("dense_widths_b")

    def one(key):
        L, name = key
        txt = INPUTS_B[name][0](L)
        d = root / f"L{L}_{name}"
        d.mkdir()
        base = ol.stage_dir(d, {})
        assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
        inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna")}
        S = gen.auto_steps(inputs["input_clean.dna"], K_B)
        stats = (C.c_uint64 * 4)()
        assert oracle.harc_oracle_reorder(base.encode(), L, K_B, S, None, stats) == 0
        s1 = {f: v for f, v in ol.read_dir(base).items() if f in ol.STAGE1_FILES}
        assert oracle.harc_oracle_encoder(base.encode(), L, E_B, None, None) == 0
        s2 = {f: v for f, v in ol.read_dir(base).items() if f in ol.stage2_files(E_B)}
        for f in (d / "output").iterdir():
            f.unlink()
        return key, (txt, inputs, S, s1, s2, int(stats[0]), _own_kmer_share(inputs["input_clean.dna"], L))
    with cf.ThreadPoolExecutor(max_workers=8) as ex:
        return dict(ex.map(one, [(L, name) for L in LENGTHS_B for name in INPUTS_B]))


@pytest.mark.parametrize("L,case", [pytest.param(L, case, id=f"L{L}-{case}") for L in LENGTHS_B for case in CASES_B])
def test_20000_chains_match_oracle_at_other_widths(L, case, oracle, oracle_b, tmp_path, monkeypatch):
    """K = 20 000 on 300 000 reads, num_steps = 0: the dense launch, S and the back-off by the library's own rules.  Two runs on one context (the second
    starts from the scan the first one measured): both give the oracle's bytes for the S of the index rule"""
    import harc_amd
    name, env, batch = CASES_B[case]
    txt, inputs, S, s1, s2, rounds, share = oracle_b[(L, name)]
    # the case is the one it is meant to be (a later change of a generator cannot silently move it to another kernel)
    assert S == INPUTS_B[name][1]                                      # 32: no bins of more than 16 reads to speak of; 16: such bins hold more than 2 % of N entries, and with 20 000 chains the back-off
    assert (share > 0.88) == INPUTS_B[name][2] and abs(share - 0.88) > 0.02
    if case == "clean-measure":
        assert rounds > 2 * batch                                      # a batch with each scan, and rounds after them for the faster one
    assert _matched_share(s1) > 0.80
    _set_env(monkeypatch, env)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E_B, num_chains=K_B, num_steps=0)) as h:
        _load(h, inputs, L)
        runs = []
        for rep in range(2):
            runs.append(_gpu_run(h, E_B))
            c = h.counters()
            assert int(c.chains) == K_B and int(c.dense_steps) > 0
            if name == "rich":
                assert int(c.coop_steps) > 0
    what = f"L={L} (W={(2 * L + 63) // 64}) {case} K={K_B} S=0 (oracle: {S}) E={E_B}"
    errs = _diffs(runs[0][0], s1, ol.STAGE1_FILES) + _diffs(runs[0][1], s2, ol.stage2_files(E_B))
    assert not errs, what + ", first run: HIP path vs oracle\n" + "\n".join(errs)
    _check(oracle, tmp_path, runs[1], (s1, s2), E_B, txt, L, what + ", second run on the same context: HIP path vs oracle")
