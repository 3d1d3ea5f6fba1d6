"""Stage II and everything else on the 3-bit read store against the CPU oracle at every width of that store (run with -m gpu).

Reads with N and stage I's singletons live in a store of three bits a base: W3 = ceil(3L/64) = 1 ... 12 words, whose boundaries (L = 21|22, 42|43, 64|65,
85|86, 106|107, 128|129, 149|150, 170|171, 192|193, 213|214, 234|235) lie elsewhere than those of the 2-bit store the other width modules walk along.
Every third or so field of that store straddles two words, and k_cand3_from2, k_key3, k_cand2_from3, k_ev_windows, final_words, k_left_emit(_w),
k_ingest_pack3, k_bucket3 and k_sig_packed3 each put such a field together by hand; k_realign_propose1<W, NWIN>, k_realign_propose<W> and
k_noise<W, EMIT> are compiled for W = 1 ... 8 and k_realign_block<NW> for 5 / 8 / 12 window words.  A wrong field in most of them still round-trips or
still is deterministic: only the oracle's bytes can tell.  LENGTHS holds both sides of every W3 boundary and the longest read.

Part A forces the forms of stage II other than its window passes on gen.reads_text_edge_N: 6000 reads of which three in ten carry one to three N, all
at the columns where the 3-bit store has an edge; reads with N and singletons are both aligned and left over at every length.  Part B forces the forms of
the window passes on gen.reads_text_bigbin_stage2_at: 3000 reads with N in one bin of either dictionary, above maxsearch.  Part C feeds the Part A reads
as FASTQ (k_ingest_pack3, k_classify) and takes the signature of the packed input (k_sig_packed3).  tests/test_stage2_inputs.py checks, without a GPU,
that the inputs have what the cases take for granted.

The contract is the dense-width module's, through its helpers: every stage-I and stage-II file is the oracle's, the HIP path's streams decode (the
oracle's decoder) to the input as a multiset, and no case is vacuous: the library aligned as many singletons and reads with N as the oracle did."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from tests import gen
from tests import oracle_lib as ol
from tests import test_gpu_dense_widths as dw
from tests.test_gpu_parity import _set_sched

pytestmark = pytest.mark.gpu

LENGTHS = [21, 22, 42, 43, 64, 65, 85, 86, 106, 107, 128, 129, 149, 150, 170, 171, 192, 193, 213, 214, 234, 235, 255]
N_EDGE = 6000
_CLEARED = ("HARC_AMD_S2_BLOCK", "HARC_AMD_S2_TWOKERNELS", "HARC_AMD_S2_ONEKERNEL", "HARC_AMD_S2_FLATPASSES", "HARC_AMD_S2_NOCHASE", "HARC_AMD_S2_RANK0",
            "HARC_AMD_S2_RANGE", "HARC_AMD_S2_EBOT", "HARC_AMD_S2_COMPACT", "HARC_AMD_S2_PIPE", "HARC_AMD_S2BLOOM_TILED", "HARC_AMD_S2BLOOM_VERIFY",
            "HARC_AMD_BLOOM1", "HARC_AMD_BLOOM4_HASHED", "HARC_AMD_BLOOMBITS", "HARC_AMD_LEFT_ALL", "HARC_AMD_MAXEVENTS")


def windows(L):
    """the bases of stage II's two dictionary windows (encoder.cpp:132-145)"""
    if L > 50:
        return 21, 21
    return 20 * L // 50 + 1, 41 * L // 50 - 20 * L // 50


def proposer(L):
    """the kernel the library takes by itself: windows of unequal width have a bitmap each (k_realign_propose<W>), equal ones share one
    (k_realign_propose1<W, NWIN>) whose lines go by minimizer where the windows are 21 bases wide"""
    w0, w1 = windows(L)
    return "propose" if w0 != w1 else "propose1-minimizer" if w0 == 21 else "propose1-hashed"


def edge_genome_len(L):
    """12x coverage; 8x for reads of at most 24 bases, where thresh_s = 24 lets every read with one whole window align and too few would be left over"""
    return N_EDGE * L // (12 if L > 24 else 8)


INPUTS = {
    "edge_N": lambda L: gen.reads_text_edge_N(7000 + L, N_EDGE, L, edge_genome_len(L)),
    "bigbin": lambda L: gen.reads_text_bigbin_stage2_at(11 + L, L),
}


def schedule(L, name="edge_N"):
    """(K, S, E) drawn from L; E among 1, 2, 3, 8: the cuts between the shards fall inside the data.  The deep bins keep the few chains they were measured
    with (a long contig over the shared window)"""
    rs = np.random.RandomState(L)
    K, S, E = int(rs.choice([2, 7, 24])), int(rs.choice([16, 32, 4])), int(rs.choice([1, 2, 3, 8]))
    return (2, 16, E) if name == "bigbin" else (K, S, E)


def _set_env(monkeypatch, env):
    for v in _CLEARED:                                                 # nothing inherited: the case alone says which kernel runs
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def oracle_run(oracle, d, txt, L, K, S, E):
    """-> dict: the preprocessed inputs, the stage-I and stage-II files of the oracle and what harc_oracle_encoder counted"""
    base = ol.stage_dir(d, {})
    assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
    inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna", "read_order_N.bin")}
    assert oracle.harc_oracle_reorder(base.encode(), L, K, S, None, None) == 0
    s1 = {f: v for f, v in ol.read_dir(base).items() if f in ol.STAGE1_FILES}
    ms, mn = C.c_uint32(0), C.c_uint32(0)
    assert oracle.harc_oracle_encoder(base.encode(), L, E, C.byref(ms), C.byref(mn)) == 0
    s2 = {f: v for f, v in ol.read_dir(base).items() if f in ol.stage2_files(E)}
    for f in (d / "output").iterdir():
        f.unlink()
    n_N = len(inputs["input_N.dna"]) // (L + 1)
    return dict(txt=txt, inputs=inputs, s1=s1, s2=s2, n_N=n_N, aligned_N=int(mn.value), left_N=len(s2["input_N.dna"]) // (L + 1),
                singletons=len(s1["read_order.bin.singleton"]) // 4, aligned_singletons=int(ms.value))


@pytest.fixture(scope="module")
def oracle_runs(oracle, tmp_path_factory):
    """the oracle's run of an (L, input) at the schedule of L -- one per pair, whatever the number of forms compared with it"""
    root = tmp_path_factory.mktemp("stage2_widths")
    cache = {}
    spent = [0.0]

    def get(L, name):
        if (L, name) not in cache:
            d = root / f"L{L}_{name}"
            d.mkdir()
            t0 = time.perf_counter()
            cache[(L, name)] = oracle_run(oracle, d, INPUTS[name](L), L, *schedule(L, name))
            spent[0] += time.perf_counter() - t0
        return cache[(L, name)]
    yield get
    print(f"\n[stage2_widths] {len(cache)} oracle runs: {spent[0]:.1f} s")


def _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, name, env, sched=None):
    """-> (the oracle's run, the HIP run's stage-II files, its counters) after every file was compared with the oracle's, the streams were decoded and the
    counts of aligned reads were compared"""
    import harc_amd
    K, S, E = schedule(L, name)
    o = oracle_runs(L, name)
    _set_env(monkeypatch, env)
    if sched is not None:
        _set_sched(monkeypatch, sched)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, o["inputs"], L)
        got = dw._gpu_run(h, E)
        c = h.counters()
        counters = {f: int(getattr(c, f)) for f in ("aligned_singletons", "aligned_N", "bins_over_maxsearch")}
    what = f"L={L} (W={(2 * L + 63) // 64}, W3={(3 * L + 63) // 64}, {proposer(L)}) {name} K={K} S={S} E={E} under {env!r} {sched or ''}: HIP path vs oracle"
    dw._check(oracle, tmp_path, got, (o["s1"], o["s2"]), E, o["txt"], L, what)
    assert (counters["aligned_singletons"], counters["aligned_N"]) == (o["aligned_singletons"], o["aligned_N"]), what
    return o, got[1], counters


# ------------------------------------------------------------------------------------------------ part A: the forms beside the window passes
_TILED = {"HARC_AMD_S2BLOOM_TILED": "1", "HARC_AMD_S2BLOOM_VERIFY": "1"}
FORMS_A = {
    # name: (environment, where the variable changes the kernel that runs)
    "auto": ({}, lambda L: True),
    "bloom1": ({"HARC_AMD_BLOOM1": "1"}, lambda L: proposer(L) != "propose"),             # k_realign_propose<W>; where the windows differ `auto` is that kernel
    "hashed": ({"HARC_AMD_BLOOM4_HASHED": "1"}, lambda L: windows(L) == (21, 21)),       # k_realign_propose1<W, 0> in place of the lines by minimizer
    "tiled": (_TILED, lambda L: proposer(L) != "propose"),                                # the shared bitmap from sorted items, compared with the atomics' word for word
    "tiled-hashed": (dict(_TILED, HARC_AMD_BLOOM4_HASHED="1"), lambda L: windows(L) == (21, 21)),
    "left-all": ({"HARC_AMD_LEFT_ALL": "1"}, lambda L: True),                             # k_left_emit over all candidates in place of k_left_emit_w over the list
    "maxev": ({"HARC_AMD_MAXEVENTS": "7"}, lambda L: True),                               # the event buffer grows and the proposal runs again
}
CASES_A = [(L, form) for L in LENGTHS for form, (_, applies) in FORMS_A.items() if applies(L)]


def _decoders_give_the_input_back(oracle, d, o, got_s2, L, E):
    """the GPU decoder on the HIP path's own files: output.dna is the oracle decoder's, and after pack_order the -p chain gives the input file"""
    import harc_amd
    (d / "o").mkdir(); (d / "g").mkdir()
    bo = ol.stage_dir(d / "o", o["s2"])
    assert oracle.harc_oracle_decoder(bo.encode(), E) == 0
    want = ol.read_dir(bo)["output.dna"]
    bg = ol.stage_dir(d / "g", dict(got_s2, **{f: o["inputs"][f] for f in ("read_order_N.bin", "numreads.bin")}))
    harc_amd.decoder(bg, E)
    assert ol.read_dir(bg)["output.dna"] == want, f"L={L} E={E}: the GPU decoder's output.dna is not the oracle decoder's"
    os.remove(os.path.join(bg, "output", "output.dna"))
    harc_amd.pack_order(bg, L)
    harc_amd.decoder(bg, E, preserve_order=True)
    assert ol.read_dir(bg)["output.dna"] == o["txt"], f"L={L} E={E}: the -p decoder does not give the input file back"


@pytest.mark.parametrize("L,form", [pytest.param(L, form, id=f"L{L}-{form}") for L, form in CASES_A])
def test_stage2_forms_match_oracle_at_every_width(L, form, oracle, oracle_runs, tmp_path, monkeypatch):
    """a form of stage II on reads whose N sit at the edges of the 3-bit store: every file is the oracle's, the streams decode to the input, and the
    library aligned the oracle's number of singletons and of reads with N (tests/test_stage2_inputs.py: both are aligned and left over at every length).
    The library's own form also goes through the GPU decoder, plain and -p"""
    o, got_s2, _ = _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, "edge_N", FORMS_A[form][0])
    if form == "auto":
        _decoders_give_the_input_back(oracle, tmp_path, o, got_s2, L, schedule(L)[2])


# ------------------------------------------------------------------------------------------------ part B: the window passes
SCHEDS_B = ["", "wave", "two", "rank0=1", "flat", "nochase,wave", "nocompact,noebot", "two,norange", "auto"]      # "": k_realign_block forced (_set_sched)
CASES_B = [(L, sched, 0) for L in LENGTHS for sched in SCHEDS_B] + [(L, "", 7) for L in LENGTHS]


@pytest.mark.parametrize("L,sched,maxev", [pytest.param(L, s, m, id=f"L{L}-{s or 'block'}" + ("-maxev" if m else "")) for L, s, m in CASES_B])
def test_window_passes_match_oracle_at_every_width(L, sched, maxev, oracle, oracle_runs, tmp_path, monkeypatch):
    """a form of the passes over bins above maxsearch (k_realign_block<5 / 8 / 12>, k_realign_big, the two-kernel form; k_ev_windows cuts the windows
    they compare): 3000 reads with N in one bin of either dictionary -- every file is the oracle's, and the library saw both bins"""
    env = {"HARC_AMD_MAXEVENTS": str(maxev)} if maxev else {}
    o, _, c = _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, "bigbin", env, sched)
    assert c["bins_over_maxsearch"] >= 2


# ------------------------------------------------------------------------------------------------ part C: FASTQ ingest and the input's signature
@pytest.mark.parametrize("L", LENGTHS)
def test_fastq_ingest_and_signature_match_oracle_at_every_width(L, oracle, oracle_runs, tmp_path, monkeypatch):
    """the Part A reads as a FASTQ file: the ingest on the GPU packs reads with N into the 3-bit store itself (k_ingest_pack3 behind k_classify) -- the
    N order, the read counts and every stage-II file are those of the oracle behind its own preprocess; and the signature of the packed input
    (k_sig_packed3 for the reads with N) is the numpy restatement's over the text"""
    import harc_amd
    from tests.bucket_ref import reads_signature
    K, S, E = schedule(L)
    o = oracle_runs(L, "edge_N")
    _set_env(monkeypatch, {})
    reads = o["txt"].split()
    fq = tmp_path / "in.fastq"
    fq.write_bytes(b"".join(b"@T.%d\n%s\n+\n%s\n" % (i, r, b"H" * L) for i, r in enumerate(reads)))
    base = ol.stage_dir(tmp_path, {})
    harc_amd.compress_fastq(str(fq), base, L, num_thr=E, num_chains=K, num_steps=S)
    got = ol.read_dir(base)
    want = dict(o["s2"], **{f: o["inputs"][f] for f in ("read_order_N.bin", "numreads.bin")})
    errs = dw._diffs(got, want, ["read_order_N.bin", "numreads.bin"] + ol.stage2_files(E))
    assert not errs, f"L={L} (W3={(3 * L + 63) // 64}) K={K} S={S} E={E}: FASTQ -> streams vs oracle\n" + "\n".join(errs)
    clean, withN = o["inputs"]["input_clean.dna"], o["inputs"]["input_N.dna"]
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        h.set_reads_ascii(clean, len(clean) // (L + 1), L + 1)
        h.set_nreads_ascii(withN, len(withN) // (L + 1), L + 1)
        assert h.input_signature() == reads_signature(reads)
