"""The rest of stage I's walk against the CPU oracle at every packed-read width (run with -m gpu): the cooperative kernel in its one-, two- and four-wave
forms, the scan of bins above maxsearch, k_compact_huge, and the steps by successor list.

tests/test_gpu_dense_widths.py holds the dense forms of k_steps to the oracle at W = ceil(2L/64) = 1 ... 8.  The kernels here are compiled per W too, and
were compared with the oracle at L = 100 (W = 4) only:
  * k_steps<W, true, true, NWV>, the cooperative kernel, with NWV = 1 (wg_scan_sk: the scan by sketch, with a dword choice of its own per W) and NWV = 2
    (wg_scan with the exchange between the two waves); the dense module reaches it in its four-wave form only;
  * the scan that is not `fast`: a bin above maxsearch = 1000, where the window closes, exact ranks apply and the scan has two segments;
  * k_compact_huge<W>: bins of more than 512 reads, its partial-top path a bin of more than 4096, and the mirror copy of W words per entry;
  * k_succ<W> and the walk by successor list, with one chain (exact mode) and with many (rollbacks).
Such a kernel with a subtly wrong sketch, rank or mirror word still writes a lossless, deterministic archive: only the oracle's bytes can tell.

Part A forces the cooperative kernel's forms on two inputs: the dense module's repeat-rich one (bins of 17 to a few hundred reads, the `fast` scan) and
gen.reads_text_hugebin_families (one bin of about 5200 reads in each dictionary, mates inside and beyond the maxsearch window).  Part B walks by successor
list.  tests/test_large_bin_inputs.py checks, without a GPU, that the inputs have the bins the cases are meant to meet.

The contract is the dense module's, through its own helpers: every stage-I and stage-II file is the oracle's, the HIP path's streams decode (the oracle's
decoder) to the input as a multiset, and a failure says whether it met another schedule or a broken encoder."""
import time

import pytest

from tests import gen
from tests import test_gpu_dense_widths as dw

pytestmark = pytest.mark.gpu

LENGTHS = dw.LENGTHS
_CLEARED = dw._DENSE_VARS + ("HARC_AMD_COOP_WAVES", "HARC_AMD_SUCC")
INPUTS = {
    "iid": dw.INPUTS_A["iid"],
    "rich": dw.INPUTS_A["rich"],
    "families": lambda L: gen.reads_text_hugebin_families(4000 + L, L),
}
# the oracle's matched share a case must have to mean anything: the dense module's floor for its own inputs; families: tests/test_large_bin_inputs.py
MATCHED_FLOOR = {"iid": 0.80, "rich": 0.80, "families": 0.60}


def _set_env(monkeypatch, env):
    for v in _CLEARED:                                                 # nothing inherited: the case alone says which kernel runs
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def oracle_runs(oracle, tmp_path_factory):
    """the oracle's run of an (L, input, K, S, E) -- one per tuple, whatever the number of forms that are compared with it; with -s the module's last
    line says how long the oracle took"""
    root = tmp_path_factory.mktemp("large_bin_widths")
    cache = {}
    spent = [0.0]

    def get(L, name, K, S, E):
        key = (L, name, K, S, E)
        if key not in cache:
            txt = INPUTS[name](L)
            d = root / f"L{L}_{name}_K{K}_S{S}_E{E}"
            d.mkdir()
            t0 = time.perf_counter()
            cache[key] = (txt,) + dw._oracle_run(oracle, d, txt, L, K, S, E)
            spent[0] += time.perf_counter() - t0
        return cache[key]
    yield get
    print(f"\n[large_bin_widths] {len(cache)} oracle runs: {spent[0]:.1f} s")


def _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, name, K, S, E, env):
    """-> the counters of the HIP run, after every file was compared with the oracle's and the streams were decoded"""
    import harc_amd
    txt, inputs, s1, s2 = oracle_runs(L, name, K, S, E)
    assert dw._matched_share(s1) > MATCHED_FLOOR[name]
    _set_env(monkeypatch, env)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, inputs, L)
        got = dw._gpu_run(h, E)
        c = h.counters()
        counters = {f: int(getattr(c, f)) for f in ("coop_steps", "coop_candidates", "dense_steps", "chains")}
    dw._check(oracle, tmp_path, got, (s1, s2), E, txt, L, f"L={L} (W={(2 * L + 63) // 64}) {name} K={K} S={S} E={E} under {env!r}: HIP path vs oracle")
    return counters


# ------------------------------------------------------------------------------------------------ part A: the cooperative kernel's forms
_Q0 = {"HARC_AMD_QUAD": "0"}
FORMS = {
    "w1": {"HARC_AMD_COOP_WAVES": "1"},                                               # k_steps<W, true, true, 1>: wg_scan_sk
    "w2": {"HARC_AMD_COOP_WAVES": "2"},                                               # two waves: wg_scan with the exchange
    "w4": {"HARC_AMD_COOP_WAVES": "4"},                                               # four waves: wg_scan, whole reads
    "w1-seq": dict(_Q0, HARC_AMD_COOP_WAVES="1", HARC_AMD_SEQ="1"),                   # the sketch scan behind the wave-uniform dense kernel
    "w2-lanes": dict(_Q0, HARC_AMD_COOP_WAVES="2", HARC_AMD_SEQ="0"),                 # two waves behind the lanes' own scans
}
# rich x four waves is the dense module's (all of its forms reach the cooperative kernel with the library's four waves)
CASES_A = [(L, name, form) for L in LENGTHS for name in ("rich", "families") for form in FORMS if not (name == "rich" and form == "w4")]


@pytest.mark.parametrize("L,name,form", [pytest.param(L, name, form, id=f"L{L}-{name}-{form}") for L, name, form in CASES_A])
def test_cooperative_forms_match_oracle_at_every_width(L, name, form, oracle, oracle_runs, tmp_path, monkeypatch):
    """a form of the cooperative kernel forced on bins of more than 16 reads (rich) and on bins above maxsearch and above 4096 (families): every file is
    the oracle's, the streams decode to the input, and the case is not vacuous -- the cooperative kernel walked steps and tested candidates, behind a
    forced dense kernel that one walked steps too, and on `families` more candidates were tested than one maxsearch window holds"""
    K, S, E = dw.schedule_a(L)
    c = _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, name, K, S, E, FORMS[form])
    assert c["coop_steps"] > 0 and c["coop_candidates"] > 0
    if "HARC_AMD_QUAD" in FORMS[form]:
        assert c["dense_steps"] > 0
    if name == "families":
        assert c["coop_candidates"] > 1000


# ------------------------------------------------------------------------------------------------ part B: steps by successor list
_SUCC = {"HARC_AMD_SUCC": "1"}
CASES_B = {
    "iid": ("iid", False),                                             # K of the schedule: where it is above 1, the list walk with chains that lose bids and are rolled back
    "iid-exact": ("iid", True),                                        # K = 1, S = 64: exact mode, the oracle is the reference at -t 1
    "rich": ("rich", False),                                           # lists next to the cooperative kernel
}


@pytest.mark.parametrize("L,case", [pytest.param(L, case, id=f"L{L}-{case}") for L in LENGTHS for case in CASES_B])
def test_steps_by_successor_list_match_oracle_at_every_width(L, case, oracle, oracle_runs, tmp_path, monkeypatch):
    """HARC_AMD_SUCC=1: k_succ<W> finds the candidates of every (read, orientation) beforehand and the few-chains kernel steps through its lists (the
    conditions of stage1_run_w hold for all of these: few chains, lazy counts, default maxsearch) -- every file is the oracle's"""
    name, exact = CASES_B[case]
    K, S, E = dw.schedule_a(L)
    if exact:
        K, S = 1, 64
    c = _run_and_check(oracle, oracle_runs, tmp_path, monkeypatch, L, name, K, S, E, _SUCC)
    assert c["chains"] == K
    if name == "rich":
        assert c["coop_steps"] > 0
