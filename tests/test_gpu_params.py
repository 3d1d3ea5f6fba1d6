"""Stage I and stage II against the CPU oracle under OTHER parameters than harc_amd_default_params derives from the read length (run with -m gpu).

harc_amd_params is "fill with harc_amd_default_params, then override"; harc_amd_create accepts maxmatch 0 .. min(128, L), any maxsearch >= 1, any thresh and
thresh_s >= 0 and two dictionary windows of 1 .. 32 bases anywhere in the read.  The kernels carry code only these fields reach: the scan window that closes
inside a small bin (exactwin, maxsearch below 16), the specialised dense kernel and the successor lists switching themselves off, the cooperative scans'
not-`fast` form and their start rot = hash mod min(live, maxsearch), k_compact_huge's stretch of maxsearch unclaimed entries, stage II's bigthresh =
min(maxsearch, 32) with nearly every bin going through the window passes, thresh_s in every 3-bit Hamming test, keys narrower than 64 bits at W >= 4,
windows that straddle a word of the packed read, probe tables of other shapes.  A kernel that is subtly wrong there still decodes losslessly and
deterministically; only the schedule's bytes tell.

The cases are tests/param_cases.py (tests/test_param_inputs.py shows on the CPU that each reaches what it is for); the oracle's own handling of the fields is
pinned to the reference by tests/golden/p_*.tar.xz.  Oracle and library get their parameters from ONE dict of overrides (oracle_lib.both_params).  Every
stage-I and stage-II file must be the oracle's byte for byte; then the streams go through the oracle's decoder, which tells another schedule from a broken
encoder."""
import ctypes as C

import pytest

from tests import oracle_lib as ol
from tests import param_cases as pc
from tests import test_gpu_dense_widths as dw
from tests import test_gpu_stage2_widths as s2w

pytestmark = pytest.mark.gpu

S = 16
_CLEARED = tuple(dw._DENSE_VARS) + tuple(s2w._CLEARED) + ("HARC_AMD_SUCC", "HARC_AMD_COOP_WAVES", "HARC_AMD_CARRY", "HARC_AMD_S1BLOOM", "HARC_AMD_S1BLOOM_M",
                                                         "HARC_AMD_FIRSTMAX", "HARC_AMD_WEEDMIN", "HARC_AMD_RESEED_MG", "HARC_AMD_FUSED_RR")


def _set_env(monkeypatch, env):
    for v in _CLEARED:                                                 # nothing inherited: the case alone says which kernel runs
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------------ stage I
_LANES = {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "0"}
_SEQ = {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1", "HARC_AMD_S1BLOOM_MZMB": "0"}      # lines by minimizer: SPEC where its conditions hold; it must fall back by itself where not
FORMS_S1 = {
    # name: (chains, encoder shards, environment)
    "auto-K6": (6, 2, {}),                                             # the library's own choice: QUAD with few chains
    "auto-K200": (200, 2, {}),
    "lanes-K6": (6, 2, _LANES),                                        # k_steps<W, false, false>
    "lanes-K200": (200, 2, _LANES),
    "seq-K6": (6, 2, _SEQ),                                            # the wave-uniform scan
    "seq-K200": (200, 2, _SEQ),
    "succ-K1": (1, 1, {"HARC_AMD_SUCC": "1"}),                         # successor lists asked for; declined with the same bytes where maxsearch < 16 or thresh > 127
}
FORMS_COOP = {f"coop{w}-K6": (6, 2, {"HARC_AMD_COOP_WAVES": str(w)}) for w in (1, 2, 4)}      # cases with bins of more than 16 reads
CASES_S1 = [(n, f) for n in pc.STAGE1 for f in list(FORMS_S1) + (list(FORMS_COOP) if pc.BY_NAME[n]["big"] else [])]


@pytest.fixture(scope="module")
def oracle_s1(oracle, tmp_path_factory):
    """the oracle's run of a (case, K, E) -- one per triple, not one per form"""
    root = tmp_path_factory.mktemp("params_s1")
    cache, texts = {}, {}

    def get(name, K, E):
        if (name, K, E) not in cache:
            c = pc.BY_NAME[name]
            if name not in texts:
                texts[name] = pc.reads_text(c)
            d = root / f"{name}_K{K}_E{E}"
            d.mkdir()
            cache[(name, K, E)] = (texts[name],) + pc.oracle_run(oracle, d, texts[name], ol.oracle_params(c["L"], c["overrides"]), K, S, E)
        return cache[(name, K, E)]
    return get


@pytest.mark.parametrize("name,form", [pytest.param(n, f, id=f"{n}-{f}") for n, f in CASES_S1])
def test_stage1_forms_match_oracle_under_overridden_parameters(name, form, oracle, oracle_s1, tmp_path, monkeypatch):
    import harc_amd
    c = pc.BY_NAME[name]
    L = c["L"]
    K, E, env = {**FORMS_S1, **FORMS_COOP}[form]
    txt, inputs, s1, s2 = oracle_s1(name, K, E)
    _set_env(monkeypatch, env)
    _, p = ol.both_params(L, c["overrides"], num_thr=E, num_chains=K, num_steps=S)
    with harc_amd.HarcAmd(p) as h:
        dw._load(h, inputs, L)
        got = dw._gpu_run(h, E)
        cn = h.counters()
        dense_steps, coop_steps, chains = int(cn.dense_steps), int(cn.coop_steps), int(cn.chains)
    dw._check(oracle, tmp_path, got, (s1, s2), E, txt, L, f"{name} L={L} {c['overrides']!r} K={K} S={S} E={E} under {env!r}: HIP path vs oracle")
    assert chains == K
    if env.get("HARC_AMD_QUAD") == "0" and p.maxmatch > 0 and "every_bin_above" not in c["reach"]:      # (no probe, or every bin the cooperative kernel's: no dense step)
        assert dense_steps > 0
    if c["big"]:
        assert coop_steps > 0


# ------------------------------------------------------------------------------------------------ stage II
FORMS_S2 = {"wave": {"HARC_AMD_S2_BLOCK": "0"}, "block": {"HARC_AMD_S2_BLOCK": "1"}, "nocompact": {"HARC_AMD_S2_COMPACT": "0"}}
K_S2 = 2


@pytest.fixture(scope="module")
def oracle_s2(oracle, tmp_path_factory):
    root = tmp_path_factory.mktemp("params_s2")
    cache, texts = {}, {}

    def get(name, E):
        if (name, E) not in cache:
            c = pc.BY_NAME[name]
            if name not in texts:
                texts[name] = pc.reads_text(c)
            d = root / f"{name}_E{E}"
            d.mkdir()
            cache[(name, E)] = (texts[name],) + pc.oracle_run(oracle, d, texts[name], ol.oracle_params(c["L"], c["overrides"]), K_S2, S, E)
        return cache[(name, E)]
    return get


@pytest.mark.parametrize("name,E,form", [pytest.param(n, E, f, id=f"{n}-E{E}-{f}") for n in pc.STAGE2 for E in (1, 3) for f in FORMS_S2])
def test_stage2_forms_match_oracle_under_overridden_parameters(name, E, form, oracle, oracle_s2, tmp_path, monkeypatch):
    """stage II alone: the stage-I streams are the oracle's (harc_amd_set_stage1_streams), so a difference is stage II's"""
    import harc_amd
    c = pc.BY_NAME[name]
    L = c["L"]
    txt, inputs, s1, s2 = oracle_s2(name, E)
    _set_env(monkeypatch, FORMS_S2[form])
    _, p = ol.both_params(L, c["overrides"], num_thr=E, num_chains=K_S2, num_steps=S)
    with harc_amd.HarcAmd(p) as h:
        h.set_stage1_streams(s1["temp.dna"], s1["tempflag.txt"], s1["temppos.txt"], s1["read_order.bin"], s1["read_rev.txt"],
                             s1["temp.dna.singleton"], s1["read_order.bin.singleton"])
        withN = inputs["input_N.dna"]
        h.set_nreads_ascii(withN, len(withN) // (L + 1), L + 1)
        h.encode()
        got = {f: h.stream(s) for f, s in dw.S2_STREAMS.items()}
        for e in range(E):
            got.update({fmt % e: h.stream(s, e) for fmt, s in dw.S2_SHARD_STREAMS.items()})
        big = int(h.counters().bins_over_maxsearch)
    what = f"{name} L={L} {c['overrides']!r} E={E} under {FORMS_S2[form]!r}: stage II on the oracle's stage-I streams vs oracle"
    errs = dw._diffs(got, s2, ol.stage2_files(E))
    rt = dw._roundtrip_error(oracle, tmp_path, got, E, txt, L)
    assert not errs and not rt, what + "\n" + "\n".join(errs + ([f"round trip: {rt}"] if rt else []))
    if "maxsearch" in c["overrides"]:
        want = pc.stage2_bins_over_maxsearch(s1, withN, L, c["overrides"]["maxsearch"])
        assert big == want and big > 0, f"{what}: the library counted {big} bins above maxsearch, the input has {want}"


# ------------------------------------------------------------------------------------------------ the file entry points honour the struct
@pytest.mark.parametrize("name", pc.FILE_CASES)
def test_file_entry_points_take_the_overridden_struct(name, oracle, tmp_path):
    """harc_amd_compress_files + pack_order + the -p decoder with the overridden struct: the files are the oracle's under the same overrides (not under
    the driver's parameters), and the output is the input text"""
    import harc_amd
    c = pc.BY_NAME[name]
    L, K, E = c["L"], 3, 2
    txt = pc.reads_text(c)
    (tmp_path / "o").mkdir(); (tmp_path / "g").mkdir()
    inputs, s1, s2 = pc.oracle_run(oracle, tmp_path / "o", txt, ol.oracle_params(L, c["overrides"]), K, S, E)
    base = ol.stage_dir(tmp_path / "g", inputs)
    _, p = ol.both_params(L, c["overrides"], num_thr=E, num_chains=K, num_steps=S)
    lib = harc_amd.lib()
    harc_amd.api._check(lib.harc_amd_compress_files(C.byref(p), base.encode()))
    got = ol.read_dir(base)
    errs = dw._diffs(got, s2, ol.stage2_files(E))
    assert not errs, f"{name}: harc_amd_compress_files with {c['overrides']!r} vs oracle\n" + "\n".join(errs)
    harc_amd.api._check(lib.harc_amd_pack_order_files(C.byref(p), base.encode()))
    harc_amd.decoder(base, E, preserve_order=True)
    assert ol.read_dir(base)["output.dna"] == txt, f"{name}: the -p decoder does not give the input file back"
