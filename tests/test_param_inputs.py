"""CPU checks of the parameter cases (tests/param_cases.py): every case reaches what it is in the table for, before tests/test_gpu_params.py holds the HIP
path to the oracle on it.  For every case
  - the oracle's files under the overrides differ from its files under the driver's parameters on the same input (stage-I files for the stage-I cases,
    stage-II files for thresh_s and the stage-II maxsearch cases): the overridden value decides bytes;
  - the case's stated targets hold (TARGETS below: counted from the input with numpy where the target is about the input, read off the parameters or
    the oracle's files where it is about the schedule);
  - the oracle's decoder gives the input back as a multiset.
These are conditions: a case that misses one gets another input, never a skip."""
import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import param_cases as pc

K, S, E = 1, 16, 1


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    root = tmp_path_factory.mktemp("param_inputs")
    cache = {}

    def get(name):
        if name not in cache:
            c = pc.BY_NAME[name]
            txt = pc.reads_text(c)
            d = root / name
            d.mkdir()
            (d / "x").mkdir(); (d / "d").mkdir()
            cache[name] = dict(txt=txt, over=pc.oracle_run(oracle, d / "x", txt, ol.oracle_params(c["L"], c["overrides"]), K, S, E),
                               dflt=pc.oracle_run(oracle, d / "d", txt, ol.oracle_params(c["L"]), K, S, E))
        return cache[name]
    return get


def _matched(s1):
    return s1["tempflag.txt"].count(b"1")


def _shifts(s1):
    """shift of every read stage I put behind another one"""
    f, p = np.frombuffer(s1["tempflag.txt"], dtype=np.uint8), np.frombuffer(s1["temppos.txt"], dtype=np.uint8)
    return p[f == ord("1")]


def _aligned(s1, s2, inputs, L):
    """singletons and reads with N that stage II put into a contig"""
    left = len(s2["read_singleton.txt"]) * 4 + len(s2["read_singleton.txt.tail"])
    return (len(s1["temp.dna.singleton"]) // (L + 1) - left // L) + (len(inputs["input_N.dna"]) - len(s2["input_N.dna"])) // (L + 1)


def check_target(c, r, target, arg):
    L, p = c["L"], ol.params_dict(c["L"], c["overrides"])
    inputs, s1, s2 = r["over"]
    d_inputs, d_s1, d_s2 = r["dflt"]
    ds, de = p["dict_start"], p["dict_end"]
    if target == "s1_bins_over_maxsearch":      # bins that hold more reads, all unclaimed at the start, than a scan may look at
        assert int((pc.stage1_bins(c, r["txt"]) > p["maxsearch"]).sum()) >= arg
    elif target == "s1_bin_above":
        assert int(pc.stage1_bins(c, r["txt"]).max()) > arg
    elif target == "every_bin_above":
        assert int(pc.stage1_bins(c, r["txt"]).min()) > arg
    elif target == "s2_bins_over_maxsearch":    # more than maxsearch singletons / reads with N share a stage-II bin
        assert pc.stage2_bins_over_maxsearch(s1, inputs["input_N.dna"], L, p["maxsearch"]) >= arg
        assert (np.frombuffer(inputs["input_N.dna"], dtype=np.uint8).reshape(-1, L + 1)[:, :42] == ord("N")).sum() == 0
    elif target == "matched":
        assert _matched(s1) < _matched(d_s1) if arg == "fewer" else _matched(s1) > _matched(d_s1)
        assert _matched(s1) > 0 or p["thresh"] == 0
    elif target == "aligned":
        a, b = _aligned(s1, s2, inputs, L), _aligned(d_s1, d_s2, d_inputs, L)
        assert a < b if arg == "fewer" else a > b
    elif target == "max_shift":
        sh = _shifts(s1)
        assert (sh.size == 0 and _matched(s1) == 0) if arg < 0 else (sh.size > 100 and int(sh.max()) == arg)
    elif target == "shift_at_least":            # reads found at shifts the driver's maxmatch = L / 2 never tries
        assert int((_shifts(s1) >= arg).sum()) >= 20 and int(_shifts(d_s1).max()) < L // 2
    elif target == "key_bits":
        assert tuple(2 * (de[l] - ds[l] + 1) for l in range(2)) == tuple(arg)
    elif target == "straddles":                 # the window's bits lie in two 64-bit words of the packed read
        assert (2 * ds[arg]) // 64 != (2 * de[arg] + 1) // 64
    elif target == "swapped":
        assert ds[0] > de[1]
    elif target == "overlap":
        assert min(de) - max(ds) + 1 == arg
    elif target == "no_reverse_probes":         # reorder.cpp:585: a reverse probe needs dict_start > shift
        assert ds[arg] == 0
    elif target == "forward_probes_at_shift0_only":     # reorder.cpp:520: a forward probe needs dict_end + shift < readlen
        assert de[arg] == L - 1
    else:
        raise KeyError(target)


@pytest.mark.parametrize("name", [c["name"] for c in pc.CASES])
def test_case_reaches_what_it_is_for(name, oracle, runs, tmp_path):
    c, r = pc.BY_NAME[name], runs(name)
    L = c["L"]
    n = len(r["txt"]) // (L + 1)
    assert (300 <= n <= 500) if name in ("mm0_L100", "dict_w1_1") else (1500 <= n <= 4000), n
    files = ol.STAGE1_FILES if c["stage"] == "s1" else ol.stage2_files(E)
    over, dflt = r["over"][1 if c["stage"] == "s1" else 2], r["dflt"][1 if c["stage"] == "s1" else 2]
    assert any(over[f] != dflt[f] for f in files), f"{name}: the overridden parameters decide no byte on this input"
    if c["stage"] == "s2":
        assert all(r["over"][1][f] == r["dflt"][1][f] for f in ol.STAGE1_FILES) or "maxsearch" in c["overrides"]
    assert c["reach"], name
    for target, arg in c["reach"].items():
        check_target(c, r, target, arg)
    # lossless: the oracle's own decoder gives the input back as a multiset
    base = ol.stage_dir(tmp_path, r["over"][2])
    assert oracle.harc_oracle_decoder(base.encode(), E) == 0
    out = np.frombuffer(ol.read_dir(base)["output.dna"], dtype=np.uint8)
    want = np.frombuffer(r["txt"], dtype=np.uint8)
    v = np.dtype((np.void, L + 1))
    assert out.size == want.size and np.array_equal(np.sort(out.view(v)), np.sort(want.view(v)))


def test_table_covers_the_axes():
    vals = lambda f, stage: sorted({c["overrides"][f] for c in pc.CASES if f in c["overrides"] and c["stage"] == stage})
    assert vals("maxsearch", "s1") == [1, 3, 15, 16, 17] and vals("maxsearch", "s2") == [1, 3, 31, 32, 33]
    assert vals("thresh", "s1") == [0, 1, 12, 127, 128, 300] and vals("thresh_s", "s2") == [0, 1, 60, 200]
    assert vals("maxmatch", "s1") == [0, 1, 25, 100, 128]
    assert sum("dict_start" in c["overrides"] and "maxmatch" not in c["overrides"] for c in pc.CASES) == 11
    assert {c["L"] for c in pc.CASES if "maxsearch" in c["overrides"] and c["stage"] == "s1"} == {100, 150}
    assert all(n in pc.BY_NAME for n in pc.FILE_CASES)


NEIGHBOURS = [(c["name"], f) for c in pc.CASES for f, top in (("maxsearch", 33), ("thresh", 1), ("thresh_s", 1)) if f in c["overrides"] and c["overrides"][f] <= top]


@pytest.mark.parametrize("name,field", NEIGHBOURS)
def test_the_next_value_gives_other_bytes(name, field, oracle, runs, tmp_path):
    """the small values sit at edges (maxsearch 15 / 16 / 17 around HARC_LARGEBIN, 31 / 32 / 33 around stage II's bigthresh, thresh 0 / 1): on the case's
    input the oracle with the value plus one writes other files, so a kernel that is off by one at the edge cannot pass the case"""
    c, r = pc.BY_NAME[name], runs(name)
    nxt = dict(c["overrides"], **{field: c["overrides"][field] + 1})
    (tmp_path / "n").mkdir()
    other = pc.oracle_run(oracle, tmp_path / "n", r["txt"], ol.oracle_params(c["L"], nxt), K, S, E)
    i = 1 if c["stage"] == "s1" else 2
    files = ol.STAGE1_FILES if c["stage"] == "s1" else ol.stage2_files(E)
    assert any(other[i][f] != r["over"][i][f] for f in files)
