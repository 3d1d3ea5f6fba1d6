"""The key kernel of the index build (k_keygen2: both dictionaries' keys scrambled and rotated for the sort where they are made, the keys' bitmap items
or bitmap bits made from the same scramble) against the CPU oracle at every packed-read width (run with -m gpu).

One small stage-I run per read length of tests/test_gpu_dense_widths.py (W = 1 ... 8 at the smallest and the largest L of each), every stage-I file the
oracle's, under three settings:
  * the bitmap built by tiles from the kernel's items and compared word for word (HARC_AMD_S1BLOOM_VERIFY) with the one built with atomics from RAW
    keys made over again -- two independent computations;
  * the same with the bitmap's lines chosen by minimizer (HARC_AMD_S1BLOOM_MZMB=0);
  * the sort on the top 8 bits only, where nearly every stretch of the sorted keys is mixed and a key rotated by the wrong count sorts elsewhere.
A wrong key, item or rotation gives a table or a bitmap in which k-mers are not found: a valid archive with another read order, which only the oracle's
bytes can tell -- or a bitmap that differs from the reference, which fails the run."""
import pytest

from tests import gen
from tests import oracle_lib as ol
from tests import test_gpu_dense_widths as dw

pytestmark = pytest.mark.gpu

LENGTHS = dw.LENGTHS
N_READS = 6000
_TILED = {"HARC_AMD_S1BLOOM_TILED": "1", "HARC_AMD_S1BLOOM_VERIFY": "1"}
SETTINGS = {
    "tiled-verify": _TILED,
    "tiled-verify-minimizer": dict(_TILED, HARC_AMD_S1BLOOM_MZMB="0"),
    "sort-bits-8": {"HARC_AMD_SORT_BITS": "8"},
}
_CLEARED = dw._DENSE_VARS + ("HARC_AMD_S1BLOOM_TILED", "HARC_AMD_S1BLOOM_VERIFY", "HARC_AMD_S1BLOOM", "HARC_AMD_S1BLOOM_M", "HARC_AMD_SORT_BITS", "HARC_AMD_CAPMULT",
                             "HARC_AMD_TABLE_FILL", "HARC_AMD_COOP_WAVES", "HARC_AMD_SUCC")


@pytest.fixture(scope="module")
def oracle_stage1(oracle, tmp_path_factory):
    """the oracle's stage I of a read length: one run, whatever the number of settings compared with it"""
    root = tmp_path_factory.mktemp("keys_fused")
    cache = {}

    def get(L):
        if L not in cache:
            K, S, _ = dw.schedule_a(L)
            txt = gen.reads_text(5000 + L, N_READS, L, N_READS * L // 15, err=0.005)
            d = root / f"L{L}"
            d.mkdir()
            base = ol.stage_dir(d, {})
            assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
            inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna")}
            assert oracle.harc_oracle_reorder(base.encode(), L, K, S, None, None) == 0
            cache[L] = (inputs, {f: v for f, v in ol.read_dir(base).items() if f in ol.STAGE1_FILES}, K, S)
        return cache[L]
    return get


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("L", LENGTHS)
def test_stage1_files_match_oracle_at_every_width(L, setting, oracle_stage1, monkeypatch):
    import harc_amd
    inputs, want, K, S = oracle_stage1(L)
    assert dw._matched_share(want) > 0.80                               # the index is what finds the matches: a run without them would prove nothing
    for v in _CLEARED:
        monkeypatch.delenv(v, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=1, num_chains=K, num_steps=S)) as h:
        dw._load(h, inputs, L)
        h.reorder()
        got = {f: h.stream(s) for f, s in dw.S1_STREAMS.items()}
    errs = dw._diffs(got, want, ol.STAGE1_FILES)
    assert not errs, f"L={L} (W={(2 * L + 63) // 64}) K={K} S={S} under {SETTINGS[setting]!r}: stage I vs oracle\n" + "\n".join(errs)
