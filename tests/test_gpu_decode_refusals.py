"""The decode side (harc_amd/csrc/verify.hip) refuses a damaged archive: the stream files of an archive come from outside the program, and every
one of them is indexed by what the others announce.  One fixture, L100_err_5k (one shard, 4853 aligned reads), no compress run: its stage2/ files are
a -d archive, and with the packed read order written over read_order.bin a -d -p archive.  Nine damaged copies: six of the stream files, each through both
decoders, and three of the order files, which the -p decoder alone reads.

Every damage is chosen so that a library WITHOUT the refusal still stays inside its allocations: a patched position stays below 256 (the decode
kernels' buffer), a cut stream is refused on the host or by the span check, an appended newline writes nlpos[n] (allocated), appended bytes are
never read.  The opposite directions (a missing newline, a short read_noisepos) are not cases: without the refusal they would read unwritten device
memory as an index.

Four of the nine are values just outside what the other files announce: a noise code of '4' (both decoders), and through the -p decoder an entry of read_order.bin
equal to nC, an entry of read_order_N_pe.bin equal to nN and an entry of read_order_N.bin equal to nC + nN.  They too stay inside the allocations in a
library without the refusal: code 4 shifts a 32-bit constant by 16 and gives base 0; an order of nC (of nN) is at or above the `hi` of every bin of clean
(of N) lines and the line is dropped; flag[] has nC + nN + 1 entries."""
import itertools
import os

import numpy as np
import pytest

from tests import decode_cases as dc
from tests import decode_model as dm
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


NC, NN = 3918, 1082                      # lines without and with N of the fixture; READS of them aligned, the others singletons and input_N.dna


def _noise_code_4(files):
    """the first noise code of the archive := '4'.  Without the refusal: tab >> 16 of a 32-bit constant, base 0 at a position inside the read"""
    noise = files["read_noise.txt.0"]
    assert noise[:3] == b"\n33"
    return "read_noise.txt.0", b"\n43" + noise[3:]


def _order_entry_is_nC(files):
    """entry 0 of read_order.bin := nC, packed again at the file's own numbits (nC < 2^numbits: pack_order.cpp:36).  Without the refusal: nC is at or above
    the hi of every bin, the line is dropped"""
    order = dm.unpack_order(files)
    numbits = int(np.frombuffer(files["read_order.bin"][:4], dtype="<i4")[0])
    assert order.shape[0] == NC and NC < 2 ** numbits and len(files["read_order.bin.tail"]) == 4 * (NC % 32)
    assert dc.pack_order(order, numbits) == (files["read_order.bin"], files["read_order.bin.tail"]), "the packer of the tests does not write the fixture's file"
    order = order.copy(); order[0] = NC
    packed, tail = dc.pack_order(order, numbits)
    assert tail == files["read_order.bin.tail"] and len(packed) == len(files["read_order.bin"])
    return "read_order.bin", packed


def _order_N_pe_entry_is_nN(files):
    """entry 0 of read_order_N_pe.bin := nN.  Without the refusal: nN is at or above the hi of every bin, the line is dropped"""
    pe = np.frombuffer(files["read_order_N_pe.bin"], dtype="<u4").copy()
    assert pe.shape[0] == NN and pe[0] < NN
    pe[0] = NN
    return "read_order_N_pe.bin", pe.tobytes()


def _order_N_entry_is_total(files):
    """the last entry of read_order_N.bin := nC + nN, the file still increases.  Without the refusal: flag[nC + nN] is allocated (total + 1 entries)"""
    lines = np.frombuffer(files["read_order_N.bin"], dtype="<u4").copy()
    assert lines.shape[0] == NN and lines[-1] == NC + NN - 1 and (np.diff(lines.astype(np.int64)) > 0).all()
    lines[-1] = NC + NN
    return "read_order_N.bin", lines.tobytes()


DAMAGED_ORDER = [
    pytest.param(_order_entry_is_nC, r"inconsistent", id="order_entry_is_nC"),
    pytest.param(_order_N_pe_entry_is_nN, r"inconsistent", id="order_N_pe_entry_is_nN"),
    pytest.param(_order_N_entry_is_total, r"inconsistent", id="order_N_entry_is_nC_plus_nN"),
]

DAMAGED = [
    pytest.param(_noise_code_4, r"inconsistent", id="noise_code_4"),
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


@pytest.mark.parametrize("damage,words", DAMAGED_ORDER)
def test_damaged_order_file_is_refused(golden, damage, words, tmp_path):
    """the order files are read by the -p decoder alone"""
    import harc_amd
    base = _archive(golden, tmp_path, True, damage)
    with pytest.raises(harc_amd.HarcAmdError, match=words):
        harc_amd.decoder(base, E, preserve_order=True)
