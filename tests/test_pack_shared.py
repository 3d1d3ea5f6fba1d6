"""What the three packed side files share on the way in and back (harc_amd/csrc/packfile.h: pack_gather_coded, pack_run, pack_device, k_pack_walk,
pack_unpack_host), held for quality (q), ids (id) and streams (s) alike: a device call writes the bytes of the host twin at every alignment and nothing outside
them, knows its size before it writes, refuses a buffer a byte too small with both numbers and without a byte written, and both ways back give the text.

Every call holds whole blocks and a partial last one, and a block is 255 or 257 units (lines; bytes for streams) or, the last, 1 unit: strands without a unit,
strands of one unit, uneven strands.  A stream block of at most 1062 bytes is always stored, so blocks of 255 and 257 bytes are last blocks too, behind three of 4000
bytes in the three modes.  The first test (no GPU) holds the inputs to the mix of stored and coded blocks they are there for, on the host twin."""
import struct

import pytest

from tests import id_cases as ic
from tests import quality_cases as qc
from tests import stream_cases as sc

EINVAL = -1
QL = 24                                                            # the read length of the quality cases
SB = 4000                                                          # the block of the stream cases


def _with_byte(text, at, v):
    b = bytearray(text)
    b[at] = v
    return bytes(b)


class Quality:
    tag = "q"

    @staticmethod
    def cases():
        """{name: (text, reads_per_block, modes)}: a coded block, one stored for a byte outside the alphabet, a line alone (stored: it cannot pay for a head)"""
        c = {}
        for rb in (255, 257):
            mid = _with_byte(qc.eight_bin(rb, QL, seed=rb + 1), (rb // 2) * (QL + 1) + 5, 0x80)
            c["rb%d" % rb] = (qc.eight_bin(rb, QL, seed=rb) + mid + qc.eight_bin(1, QL, seed=7), rb, [1, 0, 0])
        return c

    @staticmethod
    def host(text, rb, header=True):
        import harc_amd
        return harc_amd.qpack_host(text, QL, rb, header=header)

    @staticmethod
    def host_back(blob):
        import harc_amd
        return harc_amd.qunpack_host(blob)

    @staticmethod
    def bound(text, rb):
        import harc_amd
        return harc_amd.qpack_bound(len(text) // (QL + 1), QL, rb)

    @staticmethod
    def pack(h, ptr, text, rb, out_ptr=None, cap=0, header=True):
        return h.qpack_device(ptr, len(text) // (QL + 1), QL, rb, out_ptr, cap, header=header)

    @staticmethod
    def back(h, *a):
        return h.qunpack_device(*a)


class Ids:
    tag = "id"

    @staticmethod
    def cases():
        """{name: (text, lines_per_block, modes)}: a coded block, one stored for a tab, a line alone (stored)"""
        c = {}
        for rb in (255, 257):
            lines = ic.ids(2 * rb + 1)
            k = rb + rb // 2
            lines[k] = lines[k][:20] + b"\t" + lines[k][21:]
            c["rb%d" % rb] = (ic.text(lines), rb, [1, 0, 0])
        return c

    @staticmethod
    def host(text, rb, header=True):
        import harc_amd
        return harc_amd.idpack_host(text, rb, header=header)

    @staticmethod
    def host_back(blob):
        import harc_amd
        return harc_amd.idunpack_host(blob)

    @staticmethod
    def bound(text, rb):
        import harc_amd
        return harc_amd.idpack_bound(len(text), text.count(b"\n"), rb)

    @staticmethod
    def pack(h, ptr, text, rb, out_ptr=None, cap=0, header=True):
        return h.idpack_device(ptr, len(text), rb, out_ptr, cap, header=header)

    @staticmethod
    def back(h, *a):
        return h.idunpack_device(*a)


class Streams:
    tag = "s"

    @staticmethod
    def cases():
        """{name: (text, block_bytes, modes)}: order 1, stored, order 0 and a last block of 1, 255 or 257 bytes (stored)"""
        c = {}
        for last in (1, 255, 257):
            c["last%d" % last] = (sc.cycle(SB) + sc.uniform(SB, seed=2) + sc.two_symbols(SB) + sc.skewed(last, seed=last), SB, [2, 0, 1, 0])
        return c

    @staticmethod
    def host(text, B, header=True):
        import harc_amd
        return harc_amd.spack_host(text, B, header=header)

    @staticmethod
    def host_back(blob):
        import harc_amd
        return harc_amd.sunpack_host(blob)

    @staticmethod
    def bound(text, B):
        import harc_amd
        return harc_amd.spack_bound(len(text), B)

    @staticmethod
    def pack(h, ptr, text, B, out_ptr=None, cap=0, header=True):
        return h.spack_device(ptr, len(text), B, out_ptr, cap, header=header)

    @staticmethod
    def back(h, *a):
        return h.sunpack_device(*a)


FORMATS = {F.tag: F for F in (Quality, Ids, Streams)}
CASES = {(tag, name): case for tag, F in FORMATS.items() for name, case in F.cases().items()}
IDS = sorted(CASES)
_HOST = {}


def _host(key):
    """the host twin's file for a case, computed once"""
    if key not in _HOST:
        text, geom, _ = CASES[key]
        _HOST[key] = FORMATS[key[0]].host(text, geom)
    return _HOST[key]


def _modes(packed):
    """the mode bytes of the blocks of a packed file of any of the three formats, by its payload_bytes prefixes"""
    out, at = [], 32
    while at < len(packed):
        size, mode = struct.unpack_from("<IB", packed, at)
        out.append(mode)
        at += 4 + size
    assert at == len(packed)
    return out


@pytest.mark.parametrize("key", IDS, ids="-".join)
def test_the_inputs_hold_stored_and_coded_blocks_and_a_partial_last_one(key):
    text, geom, want = CASES[key]
    F = FORMATS[key[0]]
    modes = _modes(_host(key))
    assert modes == want
    units = len(text) if key[0] == "s" else text.count(b"\n")
    assert len(modes) >= 3 and units % geom in (1, 255, 257) and 0 in modes and any(modes)
    if key[0] == "s":
        assert set(modes) == {0, 1, 2}
    assert len(text) < 60000
    assert F.host_back(_host(key)) == text
    assert F.host(text, geom, header=False) == _host(key)[32:]


# ------------------------------------------------------------------------------------------------ on the GPU
@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _dev(b, off):
    import torch
    t = torch.zeros(len(b) + off + 32, dtype=torch.uint8, device="cuda")
    t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _guarded(n, off):
    """n bytes at `off` from a 16-byte boundary between guard bytes -> the tensor and where the bytes start in it"""
    import torch
    out = torch.full((n + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    assert out.data_ptr() % 16 == 0
    return out, 16 + off


def _inside(out, at, n):
    """the n bytes at `at`; the guard bytes either side of them must stay 0xEE"""
    host = out.cpu().numpy().tobytes()
    assert host[:at] == b"\xee" * at and host[at + n:] == b"\xee" * (len(host) - at - n), "bytes outside the output were written"
    return host[at:at + n]


@pytest.mark.gpu
@pytest.mark.parametrize("key", IDS, ids="-".join)
def test_device_pack_writes_the_host_bytes_at_every_alignment_and_both_ways_back_give_the_text(ctx, key):
    import torch
    text, geom, _ = CASES[key]
    F = FORMATS[key[0]]
    want = _host(key)
    for in_off in (1, 3):
        tt, pt = _dev(text, in_off)
        for out_off in (1, 2, 3):
            header = (in_off, out_off) != (3, 2)                   # once without the file header
            out, at = _guarded(F.bound(text, geom), out_off)
            torch.cuda.synchronize()                               # the library works on a stream of its own
            got = F.pack(ctx, pt, text, geom, out.data_ptr() + at, F.bound(text, geom), header=header)
            torch.cuda.synchronize()
            blob = _inside(out, at, got)
            assert blob == (want if header else want[32:]), (in_off, out_off)
            # back through the one walk kernel and the format's decode kernel
            tb, pb = _dev(want, in_off)
            back, bat = _guarded(len(text), out_off)
            torch.cuda.synchronize()
            assert F.back(ctx, pb, len(want)) == len(text)
            assert F.back(ctx, pb, len(want), back.data_ptr() + bat, len(text)) == len(text)
            torch.cuda.synchronize()
            assert _inside(back, bat, len(text)) == text, (in_off, out_off)
    assert F.host_back(want) == text


@pytest.mark.gpu
@pytest.mark.parametrize("key", IDS, ids="-".join)
def test_device_pack_knows_its_size_first_and_refuses_a_buffer_one_byte_short_unwritten(ctx, key):
    import harc_amd
    import torch
    text, geom, _ = CASES[key]
    F = FORMATS[key[0]]
    want = _host(key)
    tt, pt = _dev(text, 1)
    torch.cuda.synchronize()
    size = F.pack(ctx, pt, text, geom)                             # no output: the size alone
    assert size == len(want)
    out, at = _guarded(size, 3)
    torch.cuda.synchronize()
    with pytest.raises(harc_amd.HarcAmdError) as e:
        F.pack(ctx, pt, text, geom, out.data_ptr() + at, size - 1)
    assert e.value.code == EINVAL and str(size) in str(e.value) and str(size - 1) in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert _inside(out, at, 0) == b""                              # not a byte written
    assert F.pack(ctx, pt, text, geom, out.data_ptr() + at, size) == size
    torch.cuda.synchronize()
    assert _inside(out, at, size) == want
