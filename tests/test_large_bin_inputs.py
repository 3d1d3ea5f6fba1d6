"""What tests/test_gpu_large_bin_widths.py takes for granted about its inputs, checked on the generators and the CPU oracle alone (no GPU): a later change
of a generator cannot quietly move a case off the path it is meant to take.

`families` (gen.reads_text_hugebin_families): both dictionaries hold a bin of more than 4096 clean reads -- above HARC_LARGEBIN = 16 (the cooperative
kernel), above 512 (k_compact_huge), above maxsearch = 1000 (the scan whose window closes) and above the 4096 entries k_compact_huge looks at per pass; the
oracle matches most reads (mates are found) and leaves singletons (mates beyond the window are not: the window does close).
`rich` (the dense module's): bins of more than 16 reads, the `fast` scan; none is required above maxsearch."""
import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import test_gpu_dense_widths as dw
from tests import test_gpu_large_bin_widths as lb


def _bin_sizes(clean, L):
    """the bin sizes of the two dictionaries (harc:57-60) over the clean reads, as gen.auto_steps counts them"""
    a = np.frombuffer(clean, dtype=np.uint8).reshape(-1, L + 1)
    w = 32 if L >= 100 else L * 32 // 100
    out = []
    for ds, de in ((L // 2 - w, L // 2 - 1), (L // 2, L // 2 + w - 1)):
        _, cnt = np.unique(np.ascontiguousarray(a[:, ds:de + 1]), axis=0, return_counts=True)
        out.append(cnt)
    return out


def _preprocess(oracle, d, txt, L):
    base = ol.stage_dir(d, {})
    assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
    return base, ol.read_dir(base)["input_clean.dna"]


@pytest.mark.parametrize("L", lb.LENGTHS)
def test_families_input_has_a_bin_above_4096_in_both_dictionaries_and_a_window_that_closes(L, oracle, tmp_path):
    """matched share above 0.6: measured 0.72 ... 0.83 on the oracle at L = 33, 100, 255, the floor leaves room for the other lengths; at least 100
    singletons: 383 ... 2017 were measured -- reads whose mates all lie beyond the maxsearch window of their bin"""
    txt = lb.INPUTS["families"](L)
    base, clean = _preprocess(oracle, tmp_path, txt, L)
    d1, d2 = _bin_sizes(clean, L)
    K, S, E = dw.schedule_a(L)
    assert oracle.harc_oracle_reorder(base.encode(), L, K, S, None, None) == 0
    files = ol.read_dir(base)
    share = dw._matched_share(files)
    singletons = len(files["read_order.bin.singleton"]) // 4
    print(f"L={L} K={K} S={S}: largest bins {int(d1.max())} / {int(d2.max())}, matched share {share:.3f}, {singletons} singletons")
    assert d1.max() > 4096 and d2.max() > 4096
    assert share > lb.MATCHED_FLOOR["families"] >= 0.6
    assert singletons >= 100


@pytest.mark.parametrize("L", lb.LENGTHS)
def test_rich_input_has_bins_of_more_than_16_reads(L, oracle, tmp_path):
    """what the case needs is a bin above HARC_LARGEBIN = 16 in either dictionary (a walk that meets one goes through the cooperative kernel); the twelve
    poly-A runs of 150 bp alone give one of a few hundred reads in each (A...A forward, T...T reversed), the 60 copies of the 300-bp element a few more.
    Measured at these lengths: 7 ... 29 bins of more than 16 reads, the largest of about 350, none above maxsearch"""
    txt = lb.INPUTS["rich"](L)
    _, clean = _preprocess(oracle, tmp_path, txt, L)
    d1, d2 = _bin_sizes(clean, L)
    n16 = int((d1 > 16).sum() + (d2 > 16).sum())
    print(f"L={L}: largest bins {int(d1.max())} / {int(d2.max())}, {n16} bins of more than 16 reads, {int((d1 > 1000).sum() + (d2 > 1000).sum())} above 1000")
    assert d1.max() > 16 and d2.max() > 16
