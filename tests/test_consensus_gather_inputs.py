"""What tests/test_gpu_consensus_gather.py takes for granted about its inputs, checked on the generators and the CPU oracle alone (no GPU).

The first column of every reordered read follows from the oracle's stage-I files (tempflag.txt, temppos.txt, read_rev.txt: starts() of the GPU
module restates encoder.cpp:171-180 and :219-230); a tile is 2048 columns.  In the gathering form of k_consensus the tile a read starts in writes
its words and every tile it reaches gathers it, so each bounds input must hold a read on the last and on the first column of a tile, reads across a
tile's edge -- one of them reverse-complemented -- and enough reads of each orientation."""
import pytest

from tests import test_gpu_consensus_gather as cg


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    root = tmp_path_factory.mktemp("consensus_gather_inputs")
    cache = {}

    def get(name):
        if name not in cache:
            make, L, (K, S, E) = cg.CASES[name]
            d = root / name
            d.mkdir()
            cache[name] = cg.sw.oracle_run(oracle, d, make(), L, K, S, E)
        return cache[name]
    return get


def test_lengths_cover_every_width_and_the_lengths_of_the_issue():
    w = lambda L: (2 * L + 63) // 64
    assert {32, 33, 64, 65, 100, 150, 161, 255} <= set(cg.LENGTHS)
    assert {w(L) for L in cg.LENGTHS} == set(range(1, 9))
    assert {(2 * L) % 64 == 0 for L in cg.LENGTHS} == {True, False}
    assert {64 % w(L) == 0 for L in cg.LENGTHS} == {True, False}                                  # reads a wave with and without idle lanes


@pytest.mark.parametrize("L", cg.LENGTHS)
def test_bounds_inputs_have_reads_on_and_across_the_edges_of_tiles(L, runs):
    """measured: 1 ... 4 reads on the last column of a tile, 1 ... 4 on the first, 67 ... 293 across an edge of which 27 ... 118 reversed, 38 ... 49 %
    of the reads reversed, 11 ... 100 tiles"""
    name = f"bounds-L{L}"
    c = cg.tile_conditions(runs(name)["s1"], L, cg.CASES[name][2][2])
    print(name, c)
    assert c["tiles"] >= 10
    assert c["last_col"] >= 1 and c["first_col"] >= 1
    assert c["spans"] >= 1 and c["spans_rev"] >= 1
    assert 0.1 <= c["rev_share"] <= 0.9


def test_small_inputs_have_the_read_counts_they_are_named_for(runs):
    per_wave = 64 // ((2 * cg.FEW["L"] + 63) // 64)
    few, mod1 = len(runs("few")["s1"]["tempflag.txt"]), len(runs("mod1")["s1"]["tempflag.txt"])
    print("few:", few, "mod1:", mod1)
    assert 0 < few < per_wave
    assert mod1 > 4 * per_wave and mod1 % per_wave == 1


def test_pile_255_goes_through_lds_in_many_pieces(runs):
    """all reordered reads of pile-255 touch the one or two tiles of a 1000-base genome's contigs: more than ten pieces of 256 reads a tile"""
    _, L, (K, S, E) = cg.CASES["pile-255"]
    c = cg.tile_conditions(runs("pile-255")["s1"], L, E)
    print("pile-255", c)
    assert c["reads"] > 10 * 256 * c["tiles"]
