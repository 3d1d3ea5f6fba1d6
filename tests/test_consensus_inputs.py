"""What tests/test_gpu_consensus_strips.py takes for granted about its inputs, checked on the generators and the CPU oracle alone (no GPU): a later
change of a generator or of a schedule cannot quietly move a case off the path it is meant to take.

The depth of a pile is the oracle's own AVERAGE: reads in contigs x L / consensus columns.  A column of the pile holds at least that many reads, so
the bound on the average is a bound on the counter the kernel must carry: past an 8-bit field, past a 16-bit one."""
import pytest

from tests import test_gpu_consensus_strips as cs


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    root = tmp_path_factory.mktemp("consensus_inputs")
    cache = {}

    def get(name):
        if name not in cache:
            make, L, (K, S, E) = cs.CASES[name]
            d = root / name
            d.mkdir()
            cache[name] = cs.sw.oracle_run(oracle, d, make(), L, K, S, E)
        return cache[name]
    return get


def test_lengths_hold_both_sides_of_every_word_boundary_and_every_width():
    w = lambda L: (2 * L + 63) // 64
    assert {L for L in range(1, 255) if w(L) != w(L + 1)} | {L + 1 for L in range(1, 255) if w(L) != w(L + 1)} <= set(cs.LENGTHS)
    assert {w(L) for L in cs.LENGTHS} == set(range(1, 9))
    assert {21, 22, 255} <= set(cs.LENGTHS)                                                       # hardly longer than a strip of 16; the longest
    assert {cs.sw.schedule(L)[2] for L in cs.LENGTHS} >= {2, 3, 8}                                # shard cuts inside tiles


def test_consensus_of_the_boundary_cases_ends_inside_a_strip_and_spans_tiles(runs):
    """measured: 20 539 ... 190 163 columns (ten tiles and more), consensus length mod 32 != 0 at every length"""
    odd = 0
    for L in cs.LENGTHS:
        name = f"bounds-L{L}"
        al, cols = cs.oracle_stats(runs(name), L, cs.CASES[name][2][2])
        print(f"{name}: {al} reads in contigs, {cols} columns, mod 32 = {cols % 32}, mod 2048 = {cols % 2048}")
        assert al >= 0.5 * cs.N_BOUNDS and cols > 2 * 2048
        assert cols % 2048 != 0
        odd += cols % 32 != 0
    assert 2 * odd >= len(cs.LENGTHS)


@pytest.mark.parametrize("name", ["ties-3x", "ties-12x"])
def test_tie_cases_have_reads_that_differ_from_their_consensus(name, runs):
    """measured: 319 substitutions at 3x (169 reads in contigs: at 5 % errors few reads find a neighbour), 2200 at 12x (732 reads)"""
    _, L, (K, S, E) = cs.CASES[name]
    o = runs(name)
    noise = sum(o["s2"]["read_noise.txt.%d" % e].count(b"0") + o["s2"]["read_noise.txt.%d" % e].count(b"1") + o["s2"]["read_noise.txt.%d" % e].count(b"2")
                + o["s2"]["read_noise.txt.%d" % e].count(b"3") for e in range(E))
    al, cols = cs.oracle_stats(o, L, E)
    print(f"{name}: {al} reads in contigs on {cols} columns, {noise} substitutions against the consensus")
    assert noise > 100
    assert b"N" not in o["txt"]


@pytest.mark.parametrize("name,floor", [("pile-255", 255), ("pile-64k", 65535)])
def test_piles_are_deeper_than_the_counter_fields(name, floor, runs):
    """measured: 326 and 68 923 reads a column on average"""
    _, L, (K, S, E) = cs.CASES[name]
    al, cols = cs.oracle_stats(runs(name), L, E)
    print(f"{name}: {al} reads x {L} / {cols} columns = {al * L / cols:.0f}")
    assert al * L > floor * cols


def test_partitioned_case_cuts_the_columns_inside_a_tile(runs):
    o = runs("part")
    col1 = 4 * len(o["s2"]["read_seq.txt.0"]) + len(o["s2"]["read_seq.txt.0.tail"])
    assert col1 > 2048 and col1 % 2048 != 0 and o["s2"]["read_pos.txt.1"]
