"""k_consensus counts its columns bit-sliced: a lane owns a strip of 16 columns and adds a read's 32-bit window of 2-bit codes into counter planes
with word-wide logic (run with -m gpu).  What can go wrong there is held to the CPU oracle through the helpers of the stage-II width module: every
stage-I and stage-II file is the oracle's and the HIP path's streams decode (the oracle's decoder) to the input as a multiset.

bounds  the window is cut from two 32-bit halves of the read's words by a funnel shift and clipped by the read's start, its end and the end of the
        consensus: L on both sides of every boundary of the 2-bit words and the extremes, 6000 reads at 12x (8x up to 24 bases: thresh_s = 24 lets
        every read with one whole window align), 1 % errors.  The consensus spans several tiles of 2048 columns and ends inside a strip and a tile;
        the schedules are those of the width module (E = 2, 3, 8: shard cuts inside tiles).  L = 21, 22: reads hardly longer than a strip.
ties    L = 100 at 3x with 5 % substitutions and no N, as the issue names it, and the same at 12x where many more reads align: columns at 1 : 1 and
        2 : 2 between C and G (adjacent rows, swapped codes) and the other pairs.  The first strict maximum in ROW order A C G T must come out.
piles   counts past the low planes, past 8 bits, past the 12 planes of the kernel every tile goes through (4095: the tile is counted again by the
        kernel with 32 planes) and past 16 bits.  pile-4000 is the issue's 4000 reads of 100 bases on 1000 (1 % errors cut the
        contigs: the oracle's average is 92 a column); pile-255 the same genome with 6000 reads at 0.2 % errors, whose AVERAGE is 326 a column;
        pile-64k 140 000 error-free reads of 64 bases on a 66-base genome with K = 2.  The issue's 70 000 reads on 200 bases reach 6531 a column and
        on 66 bases 34 729, because each of the two chains builds a contig of its own; twice the reads give 68 923 on both.  The oracle needs half
        a second for it.  tests/test_consensus_inputs.py asserts these figures (> 255, > 65 535) from the oracle's files without a GPU.
part    stage II partitioned over two ranks (HARC_AMD_S2_PART=2, the mailbox transport of tests/test_gpu_replicate.py): the second rank's first
        column lies in tile 18, not at a tile's edge, and its pieces put together are the oracle's files."""
import numpy as np
import pytest

from tests import gen
from tests import oracle_lib as ol
from tests import test_gpu_dense_widths as dw
from tests import test_gpu_stage2_widths as sw

pytestmark = pytest.mark.gpu

LENGTHS = [21, 22, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 255]
N_BOUNDS = 6000
PART = dict(n=6000, L=100, K=7, S=16, E=2)


def bounds_genome_len(L):
    return N_BOUNDS * L // (12 if L > 24 else 8)


# name: (reads as text, L, (K, S, E))
CASES = {f"bounds-L{L}": (lambda L=L: gen.reads_text(9000 + L, N_BOUNDS, L, bounds_genome_len(L), err=0.01), L, sw.schedule(L)) for L in LENGTHS}
CASES.update({
    "ties-3x": (lambda: gen.reads_text(2, 6000, 100, 200000, err=0.05, n_frac=0.0), 100, (7, 16, 2)),
    "ties-12x": (lambda: gen.reads_text(2, 6000, 100, 50000, err=0.05, n_frac=0.0), 100, (7, 16, 2)),
    "pile-4000": (lambda: gen.reads_text(1, 4000, 100, 1000, err=0.01, n_frac=0.0), 100, (2, 16, 1)),
    "pile-255": (lambda: gen.reads_text(1, 6000, 100, 1000, err=0.002, n_frac=0.0), 100, (2, 16, 1)),
    "pile-64k": (lambda: gen.reads_text(3, 140000, 64, 66, err=0.0), 64, (2, 16, 1)),
    "part": (lambda: gen.reads_text(4, PART["n"], PART["L"], PART["n"] * PART["L"] // 12, err=0.01), PART["L"], (PART["K"], PART["S"], PART["E"])),
})


def oracle_stats(o, L, E):
    """-> (reads in contigs, consensus columns) of an oracle run: every read that is not left over as a singleton or with its N sits in a contig"""
    s2 = o["s2"]
    n = len(o["txt"]) // (L + 1)
    left = (4 * len(s2["read_singleton.txt"]) + len(s2["read_singleton.txt.tail"])) // L + o["left_N"]
    cols = sum(4 * len(s2["read_seq.txt.%d" % e]) + len(s2["read_seq.txt.%d.tail" % e]) for e in range(E))
    return n - left, cols


@pytest.fixture(scope="module")
def oracle_runs(oracle, tmp_path_factory):
    """the oracle's run of a case: one per case"""
    root = tmp_path_factory.mktemp("consensus_strips")
    cache = {}

    def get(name):
        if name not in cache:
            make, L, (K, S, E) = CASES[name]
            d = root / name
            d.mkdir()
            cache[name] = sw.oracle_run(oracle, d, make(), L, K, S, E)
        return cache[name]
    return get


def _run_and_check(name, oracle, oracle_runs, tmp_path, monkeypatch):
    import harc_amd
    _, L, (K, S, E) = CASES[name]
    o = oracle_runs(name)
    sw._set_env(monkeypatch, {})
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, o["inputs"], L)
        got = dw._gpu_run(h, E)
    al, cols = oracle_stats(o, L, E)
    what = f"{name}: L={L} (W={(2 * L + 63) // 64}) K={K} S={S} E={E}, {al} reads on {cols} consensus columns ({cols % 2048} in the last tile): HIP path vs oracle"
    dw._check(oracle, tmp_path, got, (o["s1"], o["s2"]), E, o["txt"], L, what)
    return o, got


@pytest.mark.parametrize("L", LENGTHS)
def test_word_and_strip_boundaries_match_oracle(L, oracle, oracle_runs, tmp_path, monkeypatch):
    """reads that start and end at every offset of a strip, windows that straddle the 32-bit halves and the 64-bit words of a read at every width
    W = 1 ... 8, a consensus that ends inside a strip: every file is the oracle's"""
    _run_and_check(f"bounds-L{L}", oracle, oracle_runs, tmp_path, monkeypatch)


@pytest.mark.parametrize("name", ["ties-3x", "ties-12x"])
def test_ties_go_to_the_first_row_not_the_first_code(name, oracle, oracle_runs, tmp_path, monkeypatch):
    """equal counts between two bases: the byte of the consensus is the earlier of A C G T (the packed codes run A G C T) -- read_seq and, through
    the consensus every read is coded against, the noise streams are the oracle's"""
    _run_and_check(name, oracle, oracle_runs, tmp_path, monkeypatch)


@pytest.mark.parametrize("name", ["pile-4000", "pile-255", "pile-64k"])
def test_deep_piles_count_exactly(name, oracle, oracle_runs, tmp_path, monkeypatch):
    """hundreds and tens of thousands of reads on one column: the carries run up the main planes, past bit 8 and, in pile-64k, out of the 12 planes
    of k_consensus<12> (the tile is counted again by k_consensus<32>) and past bit 16"""
    _run_and_check(name, oracle, oracle_runs, tmp_path, monkeypatch)


def test_rank_partitioned_stage2_starts_inside_a_tile(oracle, oracle_runs, tmp_path, monkeypatch):
    """two ranks, stage II partitioned by encoder shard: rank 1 launches its tiles from the one that holds its first column on and writes only
    its own columns.  Its first column is past the first tile and not on a tile's edge; the ranks' pieces put together are the oracle's files"""
    from tests import shard_model
    from tests import test_gpu_replicate as rp
    _, L, (K, S, E) = CASES["part"]
    o = oracle_runs("part")
    col1 = 4 * len(o["s2"]["read_seq.txt.0"]) + len(o["s2"]["read_seq.txt.0.tail"])          # shard 0's columns = the first column of rank 1
    assert col1 > 2048 and col1 % 2048 != 0, col1
    sw._set_env(monkeypatch, {"HARC_AMD_S2_PART": "2", "HARC_AMD_MAILBOX_TIMEOUT": "180"})
    arr = np.frombuffer(o["txt"], dtype=np.uint8).reshape(-1, L + 1)[:, :L].copy()
    mbox = tmp_path / "mbox"
    mbox.mkdir()
    res = rp._ranks(2, shard_model.slices_of(arr, 2), L, E, K, S, str(mbox))
    got = rp._assemble(res, E, L)
    assert all(res[r]["files"]["read_pos.txt.%d" % r] for r in range(2)), "each rank owns one shard"
    assert set(got) == set(ol.stage2_files(E)) - {"read_meta.txt"}                            # the read length: no stream of a rank
    errs = dw._diffs(got, o["s2"], sorted(got))
    assert not errs, f"L={L} K={K} S={S} E={E}, stage II partitioned over two ranks from column {col1} (tile {col1 // 2048}) on: vs oracle\n" + "\n".join(errs)
