"""read_seq is packed from the packed consensus (stage2.hip: k_consensus stores a strip's 16 columns as half a word of cons2, k_pack_seq shifts
cons2's words to each shard's first column, all shards in one launch), held to the CPU oracle through the helpers of
tests/test_gpu_consensus_strips.py: every stage-I and stage-II file is the oracle's and the streams decode to the input.

What can go wrong is decided by where a shard's first column falls in a word of 32 columns, so the seeds were chosen for that from the oracle's
own files (test_shard_starts_cover_the_shifts asserts it without a GPU).  First columns modulo 32, and the consensus' length modulo 32:
    L100-E2  seed  8   0 30                     18
    L100-E3  seed  2   0 31  5                  18
    L100-E8  seed 27   0  2 31  9  8  0 31  1    6
    L24-E3   seed  1   0 29  6                  17
    L24-E8   seed 57   0  0 29 30 29  5 18  3    2
all four residues modulo 4 (a byte holds four columns); 29, 30 and 31, where nearly a whole word comes from the next one; 0 in a shard other than
the first (L100-E8 shard 5, L24-E8 shard 1), where nothing may come from the next word; every consensus ends inside a word.  6000 reads at 12x
(8x for 24 bases), 1 % errors, K = 7, S = 16.

pile-64k of the strips module (68 923 reads a column: tests/test_consensus_inputs.py) sends its tile through k_consensus<32>, which takes its
tiles from the list k_consensus<12> appends to."""
import pytest

from tests import gen
from tests import test_gpu_consensus_strips as cs

N_READS = 6000
# name: (seed, L, E)
SEEDS = {"L100-E2": (8, 100, 2), "L100-E3": (2, 100, 3), "L100-E8": (27, 100, 8), "L24-E3": (1, 24, 3), "L24-E8": (57, 24, 8)}
SEQ_CASES = {name: (lambda seed=seed, L=L: gen.reads_text(seed, N_READS, L, N_READS * L // (12 if L > 24 else 8), err=0.01), L, (7, 16, E)) for name, (seed, L, E) in SEEDS.items()}
ALL_CASES = dict(SEQ_CASES, **{"pile-64k": cs.CASES["pile-64k"]})


@pytest.fixture(scope="module")
def runs(oracle, tmp_path_factory):
    """the oracle's run of a case: one per case"""
    root = tmp_path_factory.mktemp("seq_pack")
    cache = {}

    def get(name):
        if name not in cache:
            make, L, (K, S, E) = ALL_CASES[name]
            d = root / name
            d.mkdir()
            cache[name] = cs.sw.oracle_run(oracle, d, make(), L, K, S, E)
        return cache[name]
    return get


def _run_and_check(name, oracle, runs, tmp_path, monkeypatch):
    import harc_amd
    _, L, (K, S, E) = ALL_CASES[name]
    o = runs(name)
    cs.sw._set_env(monkeypatch, {})
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        cs.dw._load(h, o["inputs"], L)
        got = cs.dw._gpu_run(h, E)
    al, cols = cs.oracle_stats(o, L, E)
    cs.dw._check(oracle, tmp_path, got, (o["s1"], o["s2"]), E, o["txt"], L, f"{name}: L={L} K={K} S={S} E={E}, {al} reads on {cols} consensus columns: HIP path vs oracle")
    return o


def shard_starts(o, E):
    """-> (first column of every shard, columns of the consensus) from the oracle's read_seq files"""
    cols = [4 * len(o["s2"]["read_seq.txt.%d" % e]) + len(o["s2"]["read_seq.txt.%d.tail" % e]) for e in range(E)]
    return [sum(cols[:e]) for e in range(E)], sum(cols)


def test_shard_starts_cover_the_shifts(runs):
    firsts, later = [], []
    for name, (make, L, (K, S, E)) in SEQ_CASES.items():
        st, total = shard_starts(runs(name), E)
        print(f"{name}: first columns mod 32 = {[s % 32 for s in st]}, {total} columns, mod 32 = {total % 32}")
        assert total % 32 != 0, name
        assert all(b > a for a, b in zip(st, st[1:])), name
        firsts += st
        later += st[1:]
    assert {s % 4 for s in firsts} == {0, 1, 2, 3}
    assert any(s % 32 >= 29 for s in firsts)
    assert any(s % 32 == 0 for s in later)
    assert {L for _, L, _ in SEQ_CASES.values()} == {100, 24} and {k[2] for _, _, k in SEQ_CASES.values()} == {2, 3, 8}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SEQ_CASES))
def test_read_seq_of_every_shard_matches_oracle(name, oracle, runs, tmp_path, monkeypatch):
    _run_and_check(name, oracle, runs, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_tile_counted_again_comes_from_the_list(oracle, runs, tmp_path, monkeypatch):
    """more than 4095 reads on a column: k_consensus<12> appends the tile to its list, k_consensus<32> finds it there"""
    name = "pile-64k"
    o = _run_and_check(name, oracle, runs, tmp_path, monkeypatch)
    _, L, (K, S, E) = ALL_CASES[name]
    al, cols = cs.oracle_stats(o, L, E)
    assert al * L > 4095 * cols
