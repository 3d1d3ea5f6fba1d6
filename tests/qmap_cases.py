"""Lossy quality values (harc_amd/csrc/qm_block.h, qmap.hip), shared by the host test and the GPU test: the four schemes and their statistics written down a
second time in Python -- nothing here comes from the library -- and for every part of the rules and of the two kernels the smallest text at which it can go
wrong.  A case is (text, L): lines of exactly L bytes and a newline."""
import random

import numpy as np

from tests import quality_cases as qc

SCHEMES = ["ill8", "bin:20:40:6", "cap:30", "pblock:1", "pblock:2", "pblock:4", "pblock:46"]
ILL8 = [(0, 1, 0), (2, 9, 6), (10, 19, 15), (20, 24, 22), (25, 29, 27), (30, 34, 33), (35, 39, 37), (40, 93, 40)]      # q from, q to, q'


def table(spec):
    """the 256 bytes of a table scheme"""
    f = spec.split(":")
    t = list(range(256))
    for q in range(94):
        if f[0] == "ill8":
            m = next(to for lo, hi, to in ILL8 if lo <= q <= hi)
        elif f[0] == "bin":
            T, H, L = (int(x) for x in f[1:])
            m = H if q >= T else L
        else:
            assert f[0] == "cap"
            m = min(q, int(f[1]))
        t[33 + q] = 33 + m
    return bytes(t)


def _pblock_line(ln, R):
    out, j, n = bytearray(ln), 0, len(ln)
    while j < n:
        v = ln[j]
        if not 33 <= v <= 126:
            j += 1
            continue
        lo = hi = v
        e = j + 1
        while e < n and 33 <= ln[e] <= 126 and max(hi, ln[e]) - min(lo, ln[e]) <= 2 * R:
            lo, hi = min(lo, ln[e]), max(hi, ln[e])
            e += 1
        out[j:e] = bytes([(lo + hi) // 2]) * (e - j)
        j = e
    return bytes(out)


def stats(text, mapped, L):
    a, b = np.frombuffer(text, dtype=np.uint8).astype(np.int64), np.frombuffer(mapped, dtype=np.uint8).astype(np.int64)
    v = (a >= 33) & (a <= 126)
    d = np.abs(b[v] - a[v])
    return {"values": len(text) // (L + 1) * L, "changed": int((d != 0).sum()), "sum_abs": int(d.sum()), "sum_sq": int((d * d).sum()),
            "max_abs": int(d.max()) if d.size else 0, "distinct_in": len(set(a[v].tolist())), "distinct_out": len(set(b[v].tolist()))}


_MAPPED = {}


def mapped(text, L, spec):
    """-> (the mapped text, its statistics), by the rules of the issue alone; computed once per text and scheme"""
    key = (text, L, spec)
    if key not in _MAPPED:
        if spec.startswith("pblock:"):
            R = int(spec.split(":")[1])
            out = b"".join(_pblock_line(text[i:i + L], R) + text[i + L:i + L + 1] for i in range(0, len(text), L + 1))
        else:
            out = text.translate(table(spec))
        _MAPPED[key] = (out, stats(text, out, L))
    return _MAPPED[key]


def _lines(lines):
    return b"".join(bytes(ln) + b"\n" for ln in lines)


def cases():
    """{name: (text, L)}"""
    rng = random.Random(41)
    c = {"qc_" + k: (t, L) for k, (t, L, _) in qc.small_cases().items()}           # the 0x80 bytes and the empty text among them
    for L in (1, 2, 3, 63, 64, 100, 255):                                          # the row pitches 1, 1, 1, 17, 17, 25 and 65 dwords; L + 1 = 64 and 256 bytes
        c["L%d_300" % L] = (qc.markov(300, L, seed=L), L)
    for n in (1, 255, 256, 257, 513):                                              # the tile edges of k_qm_pblock
        c["tile_%d_L21" % n] = (qc.markov(n, 21, seed=300 + n), 21)
    c["one_block_lines"] = (_lines([[70 + (i + j) % 3 for j in range(50)] for i in range(40)]), 50)          # max - min = 2: one block for every R
    c["alternating_extremes"] = (_lines([[33 if (i + j) % 2 else 126 for j in range(51)] for i in range(40)]), 51)       # every byte a block of its own, also at R = 46
    runs = []
    for R in (1, 2, 4, 46):                                                        # a run whose spread reaches exactly 2R at its last byte / 2R + 1 one byte earlier
        base = 33 if R == 46 else 60
        for d in (2 * R, 2 * R + 1):
            for pad in range(4):
                ln = [base] * (3 + pad) + [base + d] + [base + d] * 3 + [base + 1] * 24
                runs.append((ln + [base] * 40)[:40])
    c["runs_at_2R"] = (_lines(runs), 40)
    bad = []
    for col in (0, 18, 36):                                                        # a byte outside 33..126 at a line's first, middle and last column
        for i in range(6):
            ln = bytearray(qc.markov(1, 37, seed=500 + col + i)[:37])
            ln[col] = 0x80
            bad.append(ln)
    c["byte_0x80_columns"] = (_lines(bad), 37)
    allq = list(range(33, 127))
    c["every_q"] = (_lines([allq, allq[::-1]] + [rng.sample(allq, 94) for _ in range(6)]), 94)
    c["low_bytes"] = (_lines([[rng.choice([9, 32, 33, 126, 127, 255, 0, 70]) for _ in range(13)] for _ in range(70)]), 13)      # the edges of 33..126
    return c
