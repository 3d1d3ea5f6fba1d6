"""The decode side (harc_amd/csrc/verify.hip) refuses a damaged archive: the stream files of an archive come from outside the program, and every
one of them is indexed by what the others announce.  One fixture, L100_err_5k (one shard, 4853 aligned reads), no compress run: its stage2/ files are
a -d archive, and with the packed read order written over read_order.bin a -d -p archive.  Five damaged copies, each through both decoders.

Every damage is chosen so that a library WITHOUT the refusal still stays inside its allocations: a patched position stays below 256 (the decode
kernels' buffer), a cut stream is refused on the host or by the span check, an appended newline writes nlpos[n] (allocated), appended bytes are
never read.  The opposite directions (a missing newline, a short read_noisepos) are not cases: without the refusal they would read unwritten device
memory as an index."""
import itertools
import os

import pytest

from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu

CASE, L, E, READS = "L100_err_5k", 100, 1, 4853


@pytest.fixture(scope="module")
def golden():
    g = ol.load_golden(CASE)
    assert g["stage2/read_meta.txt"].split()[0] == b"%d" % L and len(g["stage2/read_pos.txt.0"]) == READS
    return g


def _archive(g, tmp_path, preserve, damage=None):
    files = {k[len("stage2/"):]: v for k, v in g.items() if k.startswith("stage2/")}
    if preserve:
        files["read_order.bin"], files["read_order.bin.tail"] = g["packed/read_order.bin"], g["packed/read_order.bin.tail"]
    if damage:
        name, change = damage(files)
        assert files[name] != change, "the damage changes nothing"
        files[name] = change
    return ol.stage_dir(tmp_path, files)


def _patched_first_delta(files):
    """byte 0 of read_noisepos := L.  It is the first delta of the first read that has noise; every position of that read moves to L or beyond.  All of
    them stay below 256, asserted here from the files: whatever a decode kernel does with such a position, it stays inside its buf[256]"""
    lines = files["read_noise.txt.0"].split(b"\n")
    first = next(i for i, ln in enumerate(lines) if ln)
    deltas = bytearray(files["read_noisepos.txt.0"][:len(lines[first])])
    assert first == 1 and list(deltas) == [46, 27]
    deltas[0] = L
    positions = list(itertools.accumulate(deltas))
    assert positions == [100, 127] and all(L <= p < 256 for p in positions)
    return "read_noisepos.txt.0", bytes([L]) + files["read_noisepos.txt.0"][1:]


def _cut(name, size):
    def damage(files):
        assert len(files[name]) == size
        return name, files[name][:-1]
    return damage


def _append(name, what):
    return lambda files: (name, files[name] + what)


DAMAGED = [
    pytest.param(_patched_first_delta, r"inconsistent", id="noisepos_byte0_is_L"),
    pytest.param(_cut("read_seq.txt.0.tail", 3), r"inconsistent", id="seq_tail_cut"),                 # the last read's span passes the end of the consensus
    pytest.param(_cut("read_rev.txt.0.tail", 5), r"rev stream does not match", id="rev_tail_cut"),
    pytest.param(_append("read_noise.txt.0", b"\n"), r"read_noise holds 4854 lines, read_pos 4853 reads", id="noise_one_more_line"),
    pytest.param(_append("read_noisepos.txt.0", b"\x01"), r"read_noisepos holds 4619 bytes, read_noise announces 4618", id="noisepos_one_more_byte"),
]


@pytest.mark.parametrize("preserve,want", [(False, "decoded.txt"), (True, "reads.txt")], ids=["d", "d_p"])
def test_untouched_archive_decodes(golden, preserve, want, tmp_path):
    """the controls: what the damaged copies are made from decodes to the fixture's output, through either decoder"""
    import harc_amd
    base = _archive(golden, tmp_path, preserve)
    harc_amd.decoder(base, E, preserve_order=preserve)
    assert ol.read_dir(base)["output.dna"] == golden[want]


@pytest.mark.parametrize("preserve", [False, True], ids=["d", "d_p"])
@pytest.mark.parametrize("damage,words", DAMAGED)
def test_damaged_archive_is_refused(golden, damage, words, preserve, tmp_path):
    import harc_amd
    base = _archive(golden, tmp_path, preserve, damage)
    with pytest.raises(harc_amd.HarcAmdError, match=words):
        harc_amd.decoder(base, E, preserve_order=preserve)
