"""Checked archives (./harc -c -V; harc_amd/csrc/check_block.h, check.hip), shared by the host tests and the GPU test: the text digest written down a second time
in numpy -- nothing here comes from the library -- and a parser and a writer for the archive member read.check."""
import re

import numpy as np

from tests.bucket_ref import _mix64

MAGIC = "HARCV1"
FIELDS = {"reads": 3, "order": 2, "ids": 3, "quality": 3}          # item -> how many values its line holds
_HEX = re.compile(r"[0-9a-f]{16}\Z")


def text_digest(data, first_offset=0):
    """T = (bytes, newlines, D) of `data`, whose byte i sits at offset first_offset + i of the whole text:
    D = sum of mix64(((o + 1) << 8) | byte_o) mod 2^64"""
    a = np.frombuffer(bytes(data), dtype=np.uint8)
    if a.size == 0:
        return (0, 0, 0)
    with np.errstate(over="ignore"):
        pos = np.uint64(first_offset % (1 << 64)) + np.arange(1, a.size + 1, dtype=np.uint64)
        d = int(_mix64((pos << np.uint64(8)) | a.astype(np.uint64)).sum(dtype=np.uint64))
    return (int(a.size), int((a == 10).sum()), d)


def add(t, u):
    """the digest of a text from the digests of two pieces of it"""
    return (t[0] + u[0], t[1] + u[1], (t[2] + u[2]) % (1 << 64))


def order_digest(reads):
    """the `order` item: (bytes, D) of the text read_0 \\n read_1 \\n ..."""
    t = text_digest(b"".join(r + b"\n" for r in reads))
    return (t[0], t[2])


def write_check(items):
    """{item: tuple of ints} -> the text of read.check, items in the order of FIELDS"""
    out = [MAGIC]
    for k in FIELDS:
        if k in items:
            assert len(items[k]) == FIELDS[k], k
            out.append(k + "".join(" %016x" % v for v in items[k]))
    return ("\n".join(out) + "\n").encode()


def parse_check(data):
    """the text of read.check -> {item: tuple of ints}; ValueError naming the line that is refused"""
    lines = bytes(data).decode("ascii", errors="replace").split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    if not lines or lines[0] != MAGIC:
        raise ValueError("read.check: line 1 is %r, not %s" % (lines[0] if lines else "", MAGIC))
    items = {}
    for k, line in enumerate(lines[1:], 2):
        f = line.split(" ")
        if f[0] not in FIELDS or len(f) != 1 + FIELDS[f[0]] or not all(_HEX.match(x) for x in f[1:]) or f[0] in items:
            raise ValueError("read.check: line %d does not parse: %r" % (k, line))
        items[f[0]] = tuple(int(x, 16) for x in f[1:])
    if "reads" not in items:
        raise ValueError("read.check: no line 'reads'")
    return items
