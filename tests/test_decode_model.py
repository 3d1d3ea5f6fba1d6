"""tests/decode_model.py, the plain model both decoders of the library are held to (tests/test_gpu_decode_streams.py), is itself held here, without a GPU: to
oracle/harc_oracle.c (harc_oracle_decoder, the CPU restatement of decoder.cpp) on every hand-built archive of tests/decode_cases.py, and to what the REAL
reference decoded in the golden fixtures (decoded.txt for -d, reads.txt for the -p chain).  Nothing here needs oracle/_ref."""
import pytest

from tests import decode_cases as dc
from tests import decode_model as dm
from tests import oracle_lib as ol


@pytest.fixture(scope="module")
def oracle():
    return ol.load()


def _oracle_output(oracle, files, E, tmp_path):
    base = ol.stage_dir(tmp_path, files)
    assert oracle.harc_oracle_decoder(base.encode(), E) == 0
    return ol.read_dir(base)["output.dna"]


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_model_equals_oracle_decoder_on_built_archive(case, oracle, tmp_path):
    files, props, E, L = dc.archive(case)
    want = _oracle_output(oracle, files, E, tmp_path)
    got = dm.decode(files, E, L)
    assert got == want
    if "-p" in props:                                                   # the -p chain moves lines, it neither makes nor loses one
        assert sorted(dm.decode_preserve(files, E, L).split(b"\n")) == sorted(want.split(b"\n"))


def _order_from_bit_string(files):
    """the order of a read_order.bin without the reference's loop: a group's numbits words are ONE little-endian string of 32 * numbits bits, entry k is
    its bits [k * numbits, (k + 1) * numbits) (what pack_order.cpp:44-62 writes, read another way than unpack_order.cpp:41-61 and decode_model do)"""
    import numpy as np
    f = files["read_order.bin"]
    numbits, n = int.from_bytes(f[0:4], "little"), int.from_bytes(f[4:8], "little")
    groups = n // 32
    assert len(f) == 8 + 4 * groups * numbits and len(files["read_order.bin.tail"]) == 4 * (n % 32)
    bits = np.unpackbits(np.frombuffer(f[8:], dtype=np.uint8), bitorder="little").reshape(groups * 32, numbits)
    vals = np.zeros(groups * 32, dtype=np.uint32)
    for j in range(numbits):
        vals |= bits[:, j].astype(np.uint32) << np.uint32(j)
    return np.concatenate([vals, np.frombuffer(files["read_order.bin.tail"], dtype="<u4")])


@pytest.mark.parametrize("b", dc.SWEEP)
def test_model_equals_oracle_decoder_on_numbits_archive(b, oracle, tmp_path):
    """the singleton-only archives of the numbits sweep, every one of them: -d against the oracle; for -p, line order[j] of the model's output is line j of
    the oracle's -d output, with the order read off the file as a bit string (not by the model's unpack_order); and where oracle/_ref holds the reference's
    unpack_order.out, decoder_preserve_L3_e1.out and merge_N.out, their output on a copy -- from b = 22 up on a header that names more bits than pack_order
    would"""
    import numpy as np
    files, props, E, L = dc.archive(dc.sweep_case(b))
    want = _oracle_output(oracle, files, E, tmp_path / "o")
    assert dm.decode(files, E, L) == want
    lines = np.frombuffer(want, dtype=np.uint8).reshape(-1, L + 1)
    got_p = dm.decode_preserve(files, E, L)
    order = _order_from_bit_string(files)
    assert (np.sort(order) == np.arange(lines.shape[0])).all()
    assert (np.frombuffer(got_p, dtype=np.uint8).reshape(-1, L + 1)[order] == lines).all()
    ref = dc.reference_chain(files, L, E, tmp_path / "r")
    if ref is not None:
        assert ref == got_p


def test_case_list_holds_every_edge():
    """what the list as a whole must hold (decode_cases.COVERAGE): every tail length of read_seq, read_singleton and read_rev, every shard count ..."""
    seen = set()
    for case in dc.CASES:
        seen.update(dc.archive(case)[1])
    missing = [p for p in dc.COVERAGE if p not in seen]
    assert not missing, missing
    files, props, _, _ = dc.archive(next(c for c in dc.CASES if c.id == dc.BIN_READS_CASE))
    assert "at most 40 lines" in props and "adjacent lines with N" in props


def test_named_twice_follows_the_consensus_base():
    """the two examples: consensus C, codes 1 then 0 -> A (dec_noise['C']['0'], decoder.cpp:296), not T; consensus G, codes 3 then 0 -> T (:300) and the read
    has no N, so it stays among the clean lines"""
    case = next(c for c in dc.CASES if c.id == "named_twice_L100")
    files, props, E, L = dc.archive(case)
    (clean, withN), = dm.decode_shards(files, E, L)[0]
    assert len(clean) == 12 and not withN
    u = dm.unpack(files, E)
    start = -L
    for i, p in enumerate(files["read_pos.txt.0"]):
        start += p
        span = u["seq"][0][start:start + L]
        if i in (3, 8):                                                 # the forward ones
            diff = [(span[k], clean[i][k]) for k in range(L) if span[k] != clean[i][k]]
            assert diff == [(ord("C"), ord("A"))] if i == 3 else diff == [(ord("G"), ord("T"))]
        if i in (4, 9):
            fwd = dm.reverse_complement(clean[i])
            diff = [(span[k], fwd[k]) for k in range(L) if span[k] != fwd[k]]
            assert diff == [(ord("C"), ord("A"))] if i == 4 else diff == [(ord("G"), ord("T"))]


@pytest.mark.parametrize("case", ol.golden_cases())
def test_model_equals_reference_on_golden(case):
    g = ol.load_golden(case)
    files = {k[len("stage2/"):]: v for k, v in g.items() if k.startswith("stage2/")}
    L = int(files["read_meta.txt"].split()[0])
    E = sum(1 for k in files if k.startswith("read_pos.txt."))
    assert dm.decode(files, E, L) == g["decoded.txt"]
    if "packed/read_order.bin" in g:
        files["read_order.bin"], files["read_order.bin.tail"] = g["packed/read_order.bin"], g["packed/read_order.bin.tail"]
        assert dm.decode_preserve(files, E, L) == g["reads.txt"]
