"""k_consensus gathers its reads itself: a tile stages read order[i] from the clean reads, reverse-complemented where rc[i] == 'r', and the tile a
read starts in writes the read's words to the oriented copy (temp.dna in HBM) that k_noise and HARC_AMD_S1_DNA read (run with -m gpu).  Every case runs
in the gathering form (the default) and with HARC_AMD_S2_GATHER=0 (k_orient in front of stage II, the tiles stream its output back in); both are
held to the CPU oracle through the helpers of the width modules: every stage-I and stage-II file is the oracle's and the streams decode to the input.
temp.dna is fetched AFTER encode, so what is compared with the oracle's file are the words the tiles wrote; one case fetches it before encode as well
(the oriented copy is whole then, and stage II takes it as it is).

bounds   the inputs of tests/test_gpu_consensus_strips.py (6000 reads, 1 % errors, a consensus over some 25 tiles of 2048 columns) at L = 32, 33, 64,
         65, 100, 150, 161, 224, 255: every W = 1 ... 8, 2L a multiple of 64 and not, 64 / W reads a wave with and without idle lanes.  The seeds are chosen
         so that in the oracle's own run a read starts on the last and on the first column of a tile, reads span a tile's edge (both tiles gather them,
         one writes them), one of those is reverse-complemented and each orientation has a tenth of the reads: tests/test_consensus_gather_inputs.py
         asserts it without a GPU.
pile-255 6000 reads on one tile: the loop over pieces of 256 reads turns 24 times.
pile-64k the re-count of an overflowed tile (k_consensus<32>) gathers and writes again.
part     stage II partitioned over two ranks (HARC_AMD_S2_PART=2): the second rank's first tile holds reads of the first rank's shard.
few      fewer reordered reads than one wave gathers in a pass (64 / W = 16 at L = 100).
mod1     a reordered read count of 1 modulo 16: the last pass of the last piece has one read."""
import numpy as np
import pytest

from tests import gen
from tests import oracle_lib as ol
from tests import test_gpu_consensus_strips as cs
from tests import test_gpu_dense_widths as dw
from tests import test_gpu_stage2_widths as sw

pytestmark = pytest.mark.gpu

TILE = 2048
LENGTHS = [32, 33, 64, 65, 100, 150, 161, 224, 255]                   # (224: W = 7, which the other lengths leave out)
assert {(2 * L + 63) // 64 for L in LENGTHS} == set(range(1, 9))
# seed of the bounds input at each length: the first of 9000 + L (the strips module's), 9000 + L + 1000, ... whose oracle run has what the docstring names
BOUNDS_SEED = {32: 9032, 33: 9033, 64: 10064, 65: 11065, 100: 9100, 150: 9150, 161: 9161, 224: 9224, 255: 10255}
FEW = dict(seed=1, n=14, L=100, genome=300)                           # 13 reordered reads
MOD1 = dict(seed=1, n=201, L=100, genome=2000)                        # 193 = 12 x 16 + 1 reordered reads

# name: (reads as text, L, (K, S, E))
CASES = {f"bounds-L{L}": (lambda L=L: gen.reads_text(BOUNDS_SEED[L], cs.N_BOUNDS, L, cs.bounds_genome_len(L), err=0.01), L, sw.schedule(L)) for L in LENGTHS}
CASES.update({name: cs.CASES[name] for name in ("pile-255", "pile-64k", "part")})
CASES.update({
    "few": (lambda: gen.reads_text(FEW["seed"], FEW["n"], FEW["L"], FEW["genome"], err=0.0, n_frac=0.0), FEW["L"], (2, 16, 1)),
    "mod1": (lambda: gen.reads_text(MOD1["seed"], MOD1["n"], MOD1["L"], MOD1["genome"], err=0.0, n_frac=0.0), MOD1["L"], (2, 16, 1)),
})
SWITCH = {"gather": None, "orient": "0"}                               # HARC_AMD_S2_GATHER


def starts(s1, L, E):
    """-> (first consensus column of every reordered read, True where it is reverse-complemented) from the oracle's stage-I files: a read with flag '0'
    and the first read of an encoder shard start a contig L columns on, every other read temppos columns behind its predecessor (encoder.cpp:171-180,
    :219-230)"""
    flag = np.frombuffer(s1["tempflag.txt"], dtype=np.uint8)
    pos = np.frombuffer(s1["temppos.txt"], dtype=np.uint8).astype(np.int64)
    rev = np.frombuffer(s1["read_rev.txt"], dtype=np.uint8) == ord("r")
    M = flag.size
    if M == 0:
        return np.zeros(0, dtype=np.int64), rev
    q = 1 + (M - 1) // E
    head = (flag == ord("0")) | (np.arange(M) % q == 0)
    d = np.where(head, L, pos)
    d[0] = 0
    return np.cumsum(d), rev


def tile_conditions(s1, L, E):
    """what the bounds cases are chosen for, counted in an oracle run"""
    g, rev = starts(s1, L, E)
    spans = g // TILE != (g + L - 1) // TILE
    return dict(reads=int(g.size), last_col=int((g % TILE == TILE - 1).sum()), first_col=int(((g % TILE == 0) & (g > 0)).sum()), spans=int(spans.sum()),
                spans_rev=int((spans & rev).sum()), rev_share=float(rev.mean()) if g.size else 0.0, tiles=int((g.max() + L + TILE - 1) // TILE) if g.size else 0)


@pytest.fixture(scope="module")
def oracle_runs(oracle, tmp_path_factory):
    """the oracle's run of a case: one per case, shared by both settings of the switch"""
    root = tmp_path_factory.mktemp("consensus_gather")
    cache = {}

    def get(name):
        if name not in cache:
            make, L, (K, S, E) = CASES[name]
            d = root / name
            d.mkdir()
            cache[name] = sw.oracle_run(oracle, d, make(), L, K, S, E)
        return cache[name]
    return get


def _set_switch(monkeypatch, switch, env=None):
    sw._set_env(monkeypatch, env or {})
    monkeypatch.delenv("HARC_AMD_S2_GATHER", raising=False)
    if SWITCH[switch] is not None:
        monkeypatch.setenv("HARC_AMD_S2_GATHER", SWITCH[switch])


def _gpu_run_dna_last(h, E, dna_first=False):
    """reorder + encode -> (stage-I files, stage-II files); temp.dna is asked for behind encode -- the oriented reads as stage II left them -- and,
    with dna_first, once before it too (the two must agree)"""
    h.reorder()
    s1 = {f: h.stream(s) for f, s in dw.S1_STREAMS.items() if f != "temp.dna"}
    before = bytes(h.stream("S1_DNA")) if dna_first else None
    h.encode()
    s2 = {f: h.stream(s) for f, s in dw.S2_STREAMS.items()}
    for e in range(E):
        s2.update({fmt % e: h.stream(s, e) for fmt, s in dw.S2_SHARD_STREAMS.items()})
    s1["temp.dna"] = h.stream("S1_DNA")
    if dna_first:
        assert bytes(s1["temp.dna"]) == before
    return s1, s2


def _run_and_check(name, switch, oracle, oracle_runs, tmp_path, monkeypatch, dna_first=False):
    import harc_amd
    _, L, (K, S, E) = CASES[name]
    o = oracle_runs(name)
    _set_switch(monkeypatch, switch)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, o["inputs"], L)
        got = _gpu_run_dna_last(h, E, dna_first)
    c = tile_conditions(o["s1"], L, E)
    what = (f"{name} [{switch}{', temp.dna also before encode' if dna_first else ''}]: L={L} (W={(2 * L + 63) // 64}) K={K} S={S} E={E}, {c['reads']} reordered reads on "
            f"{c['tiles']} tiles, {c['spans']} across a tile's edge: HIP path vs oracle")
    dw._check(oracle, tmp_path, got, (o["s1"], o["s2"]), E, o["txt"], L, what)


@pytest.mark.parametrize("switch", list(SWITCH))
@pytest.mark.parametrize("L", LENGTHS)
def test_tiles_gather_and_write_the_oriented_reads_at_every_width(L, switch, oracle, oracle_runs, tmp_path, monkeypatch):
    """reads that start on the first and the last column of a tile and reads across a tile's edge, both orientations, at every W: temp.dna behind encode
    and every other file are the oracle's"""
    _run_and_check(f"bounds-L{L}", switch, oracle, oracle_runs, tmp_path, monkeypatch)


@pytest.mark.parametrize("switch", list(SWITCH))
def test_oriented_reads_asked_for_before_encode_are_taken_as_they_are(switch, oracle, oracle_runs, tmp_path, monkeypatch):
    """HARC_AMD_S1_DNA before encode makes the oriented copy whole (k_orient): stage II stages from it, and the stream is the same behind encode"""
    _run_and_check("bounds-L100", switch, oracle, oracle_runs, tmp_path, monkeypatch, dna_first=True)


@pytest.mark.parametrize("switch", list(SWITCH))
@pytest.mark.parametrize("name", ["pile-255", "pile-64k"])
def test_piles_gather_piece_by_piece_and_again_in_the_recount(name, switch, oracle, oracle_runs, tmp_path, monkeypatch):
    """6000 reads on one tile go through LDS in 24 pieces; 140 000 on one column overflow the 12 planes and the tile is gathered, counted and written again"""
    _run_and_check(name, switch, oracle, oracle_runs, tmp_path, monkeypatch)


@pytest.mark.parametrize("switch", list(SWITCH))
@pytest.mark.parametrize("name", ["few", "mod1"])
def test_fewer_reads_than_a_pass_and_one_read_in_the_last_pass(name, switch, oracle, oracle_runs, tmp_path, monkeypatch):
    _run_and_check(name, switch, oracle, oracle_runs, tmp_path, monkeypatch)


@pytest.mark.parametrize("switch", list(SWITCH))
def test_rank_partitioned_stage2_gathers_its_neighbours_reads(switch, oracle, oracle_runs, tmp_path, monkeypatch):
    """two ranks, stage II partitioned by encoder shard: rank 1's first tile holds the last reads of rank 0's shard, which it gathers from the reads
    every rank holds; the ranks' pieces put together are the oracle's files"""
    from tests import shard_model
    from tests import test_gpu_replicate as rp
    _, L, (K, S, E) = CASES["part"]
    o = oracle_runs("part")
    col1 = 4 * len(o["s2"]["read_seq.txt.0"]) + len(o["s2"]["read_seq.txt.0.tail"])          # shard 0's columns = the first column of rank 1
    assert col1 > TILE and col1 % TILE != 0, col1
    _set_switch(monkeypatch, switch, {"HARC_AMD_S2_PART": "2", "HARC_AMD_MAILBOX_TIMEOUT": "180"})
    arr = np.frombuffer(o["txt"], dtype=np.uint8).reshape(-1, L + 1)[:, :L].copy()
    mbox = tmp_path / "mbox"
    mbox.mkdir()
    res = rp._ranks(2, shard_model.slices_of(arr, 2), L, E, K, S, str(mbox))
    got = rp._assemble(res, E, L)
    assert all(res[r]["files"]["read_pos.txt.%d" % r] for r in range(2)), "each rank owns one shard"
    errs = dw._diffs(got, o["s2"], sorted(got))
    assert not errs, f"[{switch}] L={L} K={K} S={S} E={E}, stage II partitioned over two ranks from column {col1} (tile {col1 // TILE}) on: vs oracle\n" + "\n".join(errs)
