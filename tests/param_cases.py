"""The parameter axis: one table of cases for tests/test_param_inputs.py (CPU: every case reaches what it is for) and tests/test_gpu_params.py (the HIP path
against the oracle under the same overrides).  harc_amd_params is "fill with harc_amd_default_params, then override" (include/harc_amd.h); the reference takes
the same quantities from the config.h it regenerates for every run (harc:52-63).  The oracle's handling of them is pinned to the reference by
tests/golden/p_*.tar.xz (tests/test_oracle_golden.py).

A case: name, L, overrides ({field: value} of tests/oracle_lib.PARAM_FIELDS), stage ("s1": stage-I files decide, "s2": stage-II files), gen (function of
tests/gen.py + kwargs -> the reads), reach ({target: argument}, checked by test_param_inputs.py; see TARGETS), big (bins of more than 16 reads: the
cooperative kernel runs)."""
import numpy as np

from tests import gen
from tests import oracle_lib as ol


def _per_start(seed, L, n_start=220, big=(40, 40, 30, 30, 24, 20, 1400), windows=None, **kw):
    return ("reads_array_per_start", dict(seed=seed, L=L, n_start=n_start, big=big, windows=windows, err=0.006, **kw))


def _iid(seed, L, n, cov, err=0.01, n_frac=0.25):
    return ("reads_array", dict(seed=seed, n=n, L=L, genome_len=max(2 * L, n * L // cov), err=err, n_frac=n_frac))


def _bigbin2(seed, L, n_clean=1500, n_dupN=500):
    return ("reads_text_bigbin_stage2_at", dict(seed=seed, L=L, n_clean=n_clean, n_dupN=n_dupN, genome_len=3000))


def _win(L, w0, w1):
    """overrides for window 0 = bases w0[0]..w0[1], window 1 = w1[0]..w1[1]"""
    return dict(dict_start=[w0[0], w1[0]], dict_end=[w0[1], w1[1]])


CASES = []


def _add(name, L, overrides, stage, g, reach, big=False):
    CASES.append(dict(name=name, L=L, overrides=overrides, stage=stage, gen=g, reach=reach, big=big))


# ---- maxsearch, stage I: 4 - 10 reads per start position (bins of 2 - 12 reads once a share is reverse-complemented), half of them failing every Hamming
#      test; six bins of 20 - 40 reads and one start with 1400 reads (a bin above the 512 of k_compact_huge).  15 / 16 / 17: both sides of HARC_LARGEBIN, where the scan window
#      closes inside a SMALL bin (exactwin), SPEC and the successor lists switch off (maxsearch < 16)
for L in (100, 150):
    for ms in (1, 3, 15, 16, 17):
        _add(f"ms{ms}_L{L}", L, dict(maxsearch=ms), "s1", _per_start(300 + L + ms, L),
             dict(s1_bins_over_maxsearch=50 if ms <= 3 else 6, s1_bin_above=512), big=True)

# ---- maxsearch, stage II: 500 reads with N in one bin of either stage-II dictionary, half of them failing the test; bigthresh = min(maxsearch, 32)
for ms in (1, 3, 31, 32, 33):
    _add(f"s2ms{ms}_L100", 100, dict(maxsearch=ms), "s2", _bigbin2(400 + ms, 100), dict(s2_bins_over_maxsearch=2))

# ---- thresh: 2 % substitutions (a pair of overlapping reads differs in about four bases: 4 - 8 bits of the 2-bit store); 127 / 128: both sides of the
#      successor lists' limit; 300 at L = 255 (no Hamming distance of a 255-base overlap at the tested shifts is refused by much)
for t, L in ((0, 100), (1, 100), (12, 100), (127, 150), (128, 150), (300, 255)):
    _add(f"t{t}_L{L}", L, dict(thresh=t), "s1", _iid(500 + t, L, 2500 if L < 255 else 1500, 20, err=0.02), dict(matched="fewer" if t < 4 else "more"))

# ---- thresh_s: half of the errors N -> a fifth of the reads go to stage II with N, besides the singletons.  Above the driver's 24 the input needs reads
#      that fail at 24: the stage-II big-bin input, whose failing half carries 33 substitutions behind the dictionary windows (up to 66 bits of the 3-bit store)
for ts in (0, 1):
    _add(f"ts{ts}_L100", 100, dict(thresh_s=ts), "s2", _iid(600 + ts, 100, 2500, 20, err=0.02, n_frac=0.5), dict(aligned="fewer"))
for ts in (60, 200):
    _add(f"ts{ts}_L100", 100, dict(thresh_s=ts), "s2", _bigbin2(600 + ts, 100), dict(aligned="more"))

# ---- maxmatch.  With the driver's windows only ONE shift exists beyond L / 2 - 1 whatever maxmatch says (reorder.cpp:520: a forward probe needs
#      dict_end + shift < readlen, :585: a reverse probe dict_start > shift: the first window's forward probe at shift L / 2; at L = 100 that is 137
#      probes a step for every maxmatch > 50, not 4 maxmatch).  So the values above L / 2 come twice: alone ("plain": shift L / 2 is reached, with
#      2 maxmatch mask rows in LDS), and with the windows at the two ends of the read, where shifts up to L - 33 are probed -- both on low coverage, where
#      the nearest read often starts more than L / 2 bases further on
_add("mm0_L100", 100, dict(maxmatch=0), "s1", _iid(700, 100, 400, 20), dict(max_shift=-1))
_add("mm1_L100", 100, dict(maxmatch=1), "s1", _iid(701, 100, 2500, 20), dict(max_shift=0))
_add("mm25_L100", 100, dict(maxmatch=25), "s1", _iid(702, 100, 2500, 6), dict(max_shift=24))
_add("mm100_L100_plain", 100, dict(maxmatch=100), "s1", _iid(703, 100, 2500, 3), dict(max_shift=50))
_add("mm128_L150_plain", 150, dict(maxmatch=128), "s1", _iid(704, 150, 2000, 3), dict(max_shift=75))
_add("mm100_L100", 100, dict(maxmatch=100, **_win(100, (0, 31), (68, 99))), "s1", _iid(703, 100, 2500, 2), dict(shift_at_least=50))
_add("mm128_L150", 150, dict(maxmatch=128, **_win(150, (0, 31), (118, 149))), "s1", _iid(704, 150, 2000, 2), dict(shift_at_least=75))

# ---- dictionary windows (L = 150: the driver's are 43..74 and 75..106)
_D = 150
_add("dict_w8_8", _D, _win(_D, (67, 74), (75, 82)), "s1", _iid(800, _D, 2000, 20), dict(key_bits=(16, 16)))
_add("dict_w16_16", _D, _win(_D, (59, 74), (75, 90)), "s1", _iid(801, _D, 2000, 20), dict(key_bits=(32, 32)))
_add("dict_w32_20", _D, _win(_D, (43, 74), (75, 94)), "s1", _iid(802, _D, 2000, 20), dict(key_bits=(64, 40)))
_add("dict_straddle", _D, _win(_D, (17, 48), (75, 106)), "s1", _iid(803, _D, 2000, 20), dict(straddles=0))
_add("dict_swapped", _D, _win(_D, (75, 106), (43, 74)), "s1", _iid(804, _D, 2000, 20), dict(swapped=True))
_add("dict_overlap10", _D, _win(_D, (43, 74), (65, 96)), "s1", _iid(805, _D, 2000, 20), dict(overlap=10))
_add("dict_identical", _D, _win(_D, (59, 90), (59, 90)), "s1", _iid(806, _D, 2000, 20), dict(overlap=32))
_add("dict_from0", _D, _win(_D, (0, 31), (75, 106)), "s1", _iid(807, _D, 2000, 20), dict(no_reverse_probes=0))
_add("dict_toend", _D, _win(_D, (43, 74), (118, 149)), "s1", _iid(808, _D, 2000, 20), dict(forward_probes_at_shift0_only=1))
_add("dict_L63_narrow_unequal", 63, _win(63, (20, 30), (35, 41)), "s1", _iid(809, 63, 2500, 20), dict(key_bits=(22, 14)))
_add("dict_w1_1", _D, _win(_D, (74, 74), (75, 75)), "s1", _iid(810, _D, 400, 20), dict(key_bits=(2, 2), every_bin_above=16), big=True)

BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
STAGE1 = [c["name"] for c in CASES if c["stage"] == "s1"]
STAGE2 = [c["name"] for c in CASES if c["stage"] == "s2"]
# the two most unusual parameter sets: through the file entry points too
FILE_CASES = ["dict_w1_1", "ms1_L100"]


def reads_text(case):
    """the case's reads as lines (bytes)"""
    fn, kw = case["gen"]
    r = getattr(gen, fn)(**kw)
    return r if isinstance(r, (bytes, bytearray)) else gen.lines_of(r)


def clean_array(txt, L):
    """the reads without N ([n, L] uint8): what stage I sees"""
    a = np.frombuffer(txt, dtype=np.uint8).reshape(-1, L + 1)[:, :L]
    return a[~(a == ord("N")).any(axis=1)]


def bin_sizes(reads, first, last):
    """sizes of the bins of a dictionary over bases first..last of `reads` ([n, L] uint8)"""
    if reads.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    return np.unique(np.ascontiguousarray(reads[:, first:last + 1]), axis=0, return_counts=True)[1]


def stage1_bins(case, txt):
    """bin sizes of both stage-I dictionaries of the case (its windows), one array"""
    p = ol.params_dict(case["L"], case["overrides"])
    a = clean_array(txt, case["L"])
    return np.concatenate([bin_sizes(a, p["dict_start"][l], p["dict_end"][l]) for l in range(2)])


def stage2_bins_over_maxsearch(s1_files, input_N, L, maxsearch):
    """bins of stage II's two dictionaries (encoder.cpp:132-145: bases 0..20 and 21..41 above 50 bp) over the singletons stage I left and the reads
    with N, that hold more than maxsearch reads: what harc_amd_counters.bins_over_maxsearch counts"""
    both = s1_files["temp.dna.singleton"] + input_N
    a = np.frombuffer(both, dtype=np.uint8).reshape(-1, L + 1)[:, :L]
    w = [(0, 20), (21, 41)] if L > 50 else [(0, 20 * L // 50), (20 * L // 50 + 1, 41 * L // 50)]
    return int(sum((bin_sizes(a, f, l) > maxsearch).sum() for f, l in w))


def oracle_run(oracle, d, txt, op, K, S, E, stats=None):
    """the oracle under the parameters op (ol.OracleParams; None: the driver's) -> (preprocessed inputs, stage-I files, stage-II files)"""
    import ctypes as C
    L = op.L
    base = ol.stage_dir(d, {})
    assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
    inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna", "read_order_N.bin")}
    assert oracle.harc_oracle_reorder_ex(base.encode(), C.byref(op), K, S, None, stats) == 0
    s1 = {f: v for f, v in ol.read_dir(base).items() if f in ol.STAGE1_FILES}
    assert oracle.harc_oracle_encoder_ex(base.encode(), C.byref(op), E, None, None) == 0
    s2 = {f: v for f, v in ol.read_dir(base).items() if f in ol.stage2_files(E)}
    for f in (d / "output").iterdir():
        f.unlink()
    return inputs, s1, s2
