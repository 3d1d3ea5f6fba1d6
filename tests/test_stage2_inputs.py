"""What tests/test_gpu_stage2_widths.py takes for granted about its lengths and inputs, checked on the generators and the CPU oracle alone (no GPU): a
later change of a generator or of a schedule cannot quietly move a case off the path it is meant to take.

`edge_N` (gen.reads_text_edge_N): every column at which the 3-bit store has an edge carries an N in some read; of the reads with N and of stage I's
singletons the oracle aligns a good part and leaves a good part, so k_noise's and k_left_emit_w's branches both run over such fields.
`bigbin` (gen.reads_text_bigbin_stage2_at): 3000 reads with N in one bin of either stage-II dictionary, three windows deep; from 64 bases on some are
taken and some never are, below that the free columns are too few to fail the Hamming test and the window slides over more than maxsearch claims."""
import numpy as np
import pytest

from tests import gen
from tests import test_gpu_stage2_widths as sw

BOUNDARIES = [(21, 22), (42, 43), (64, 65), (85, 86), (106, 107), (128, 129), (149, 150), (170, 171), (192, 193), (213, 214), (234, 235)]


def test_lengths_hold_both_sides_of_every_boundary_of_the_3bit_store_and_every_compiled_width():
    w3 = lambda L: (3 * L + 63) // 64
    assert BOUNDARIES == [(L, L + 1) for L in range(1, 255) if w3(L) != w3(L + 1)]
    assert sorted(sw.LENGTHS) == sorted({L for pair in BOUNDARIES for L in pair} | {255})
    assert {w3(L) for L in sw.LENGTHS} == set(range(1, 13))                                        # W3 = 1 ... 12
    assert {(2 * L + 63) // 64 for L in sw.LENGTHS} == set(range(1, 9))                            # k_realign_propose*, k_noise: W = 1 ... 8
    assert {5 if w3(L) <= 5 else 8 if w3(L) <= 8 else 12 for L in sw.LENGTHS} == {5, 8, 12}        # k_realign_block<NW>
    # each proposer is the library's own choice somewhere, by the window formulas of encoder.cpp:132-145
    assert (sw.windows(22), sw.windows(43), sw.windows(64)) == ((9, 10), (18, 18), (21, 21))
    assert {sw.proposer(L) for L in sw.LENGTHS} == {"propose", "propose1-hashed", "propose1-minimizer"}
    # and every form of part A runs at both sides of a boundary at least
    for form, (_, applies) in sw.FORMS_A.items():
        assert sum(applies(L) for L in sw.LENGTHS) >= 19, form
    assert {L for L in sw.LENGTHS if not sw.FORMS_A["bloom1"][1](L)} == {22, 42}                   # there `auto` is k_realign_propose<W> already


def test_edge_columns_are_where_the_3bit_store_has_an_edge():
    assert gen.edge_columns_3bit(21) == [0, 20]
    assert gen.edge_columns_3bit(22) == [0, 21]                                                    # base 21: bits 63 ... 65
    assert gen.edge_columns_3bit(100) == [0, 21, 31, 32, 42, 63, 64, 85, 99]
    for L in sw.LENGTHS:
        cols = gen.edge_columns_3bit(L)
        assert [b for b in range(L) if 3 * b // 64 != (3 * b + 2) // 64] == [b for b in cols if 3 * b % 64 > 61]      # every straddling field


@pytest.mark.parametrize("L", sw.LENGTHS)
def test_edge_N_input_has_N_at_every_edge_and_both_branches_of_stage2(L, oracle, tmp_path):
    """the floors are conditions on the input: a quarter of the reads with N on either side, and 5 (L = 21, 22) or 20 singletons on either side.  Measured
    on the oracle at these lengths and schedules: 1696 ... 1873 reads with N, 39 ... 62 % of them aligned; 360 ... 1630 singletons, 30 ... 55 % of them aligned"""
    txt = sw.INPUTS["edge_N"](L)
    a = np.frombuffer(txt, dtype=np.uint8).reshape(-1, L + 1)
    assert a.shape[0] == sw.N_EDGE
    ncols = np.nonzero((a[:, :L] == ord("N")).any(0))[0].tolist()
    assert ncols == gen.edge_columns_3bit(L)                                                       # every edge column, and no other
    K, S, E = sw.schedule(L)
    o = sw.oracle_run(oracle, tmp_path, txt, L, K, S, E)
    left_s = o["singletons"] - o["aligned_singletons"]
    print(f"L={L} K={K} S={S} E={E}: {o['n_N']} reads with N, {o['aligned_N']} aligned, {o['left_N']} left; {o['singletons']} singletons, {o['aligned_singletons']} aligned, {left_s} left")
    assert o["n_N"] == int((a == ord("N")).any(1).sum()) == o["aligned_N"] + o["left_N"]
    assert o["aligned_N"] >= 0.25 * o["n_N"] and o["left_N"] >= 0.25 * o["n_N"]
    floor = 5 if L <= 22 else 20
    assert o["aligned_singletons"] >= floor and left_s >= floor
    assert len(o["s2"]["read_singleton.txt"]) * 4 + len(o["s2"]["read_singleton.txt.tail"]) == left_s * L


@pytest.mark.parametrize("L", sw.LENGTHS)
def test_bigbin_input_has_a_bin_above_maxsearch_in_both_dictionaries_at_every_length(L, oracle, tmp_path):
    """measured: 1940 ... 2137 of the 3000 left from 64 bases on, 1000 at L = 21, none at 22, 42 and 43"""
    txt = sw.INPUTS["bigbin"](L)
    a = np.frombuffer(txt, dtype=np.uint8).reshape(-1, L + 1)[:, :L]
    withN = a[(a == ord("N")).any(1)]
    w0, w1 = sw.windows(L)
    assert withN.shape[0] == 3000 and np.unique(withN[:, :w0 + w1], axis=0).shape[0] == 1         # one bin of 3000 > maxsearch in either dictionary
    K, S, E = sw.schedule(L, "bigbin")
    o = sw.oracle_run(oracle, tmp_path, txt, L, K, S, E)
    print(f"L={L} K={K} S={S} E={E}: {o['aligned_N']} of {o['n_N']} reads with N aligned, {o['left_N']} left")
    assert len(o["s2"]["read_order_N_pe.bin"]) // 4 == 3000
    if L >= 64:
        assert 100 < o["left_N"] < 2900                                                            # some were taken, some never are
    else:
        assert o["aligned_N"] > 1000                                                               # more than one window holds: it has slid
