"""Archives for the decode side that no encoder wrote: the stream files of <basedir>/output/ drawn directly from a seed, so that the decoders
(harc_amd/csrc/verify.hip) meet the edges of the format and not only what stage II happens to produce.  Test infrastructure, numpy only.

build() returns the files and the list of properties it guarantees.  The properties are read back from the BYTES of the files (properties()), not from what
was asked for, and archive() asserts that every property a case names is among them: a case that lost its edge is a failure of the builder, not a pass.

Never built here, the reference is undefined on them: a first position byte other than L, a position byte above L, a noise position at or beyond L, an order
that is no permutation, a read_order_N.bin that does not increase."""
import collections
import os
import subprocess

import numpy as np

from tests import decode_model as dm
from tests import oracle_lib as ol

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------------------------------------ packing, as the encoder side writes the files
def pack_seq(text):
    """ACGT text -> (4 bases per byte with the first base in the low bits, the last len % 4 bases as text): encoder.cpp:527-548"""
    n4 = len(text) // 4 * 4
    code = np.searchsorted(BASES, np.frombuffer(text[:n4], dtype=np.uint8)).astype(np.uint8).reshape(-1, 4)
    return (code[:, 0] | code[:, 1] << 2 | code[:, 2] << 4 | code[:, 3] << 6).astype(np.uint8).tobytes(), text[n4:]


def pack_rev(flags):
    """d / r text -> (8 per byte, first in bit 0; the last len % 8 as text): encoder.cpp:560-578"""
    n8 = len(flags) // 8 * 8
    bits = (np.frombuffer(flags[:n8], dtype=np.uint8) == ord("r")).astype(np.uint8).reshape(-1, 8)
    return np.packbits(bits, axis=1, bitorder="little").tobytes(), flags[n8:]


def pack_order(order, numbits):
    """pack_order.cpp:20-77 at a given numbits (the header names it, unpack_order.cpp:28 reads whatever it says) -> (read_order.bin, read_order.bin.tail)"""
    order = np.asarray(order, dtype=np.uint32)
    n = order.shape[0]
    assert 1 <= numbits <= 32 and (n == 0 or int(order.max()) < 2 ** numbits)
    groups = n // 32
    vals = order[:groups * 32].reshape(groups, 32).astype(np.uint64)
    words = np.zeros((groups, numbits + 1), dtype=np.uint64)
    for k in range(32):
        wi, sh = (k * numbits) >> 5, (k * numbits) & 31
        v = vals[:, k] << np.uint64(sh)
        words[:, wi] |= v & np.uint64(0xFFFFFFFF)
        words[:, wi + 1] |= v >> np.uint64(32)
    assert not words[:, numbits].any()
    head = np.array([numbits], dtype="<i4").tobytes() + np.array([n], dtype="<u4").tobytes()
    return head + words[:, :numbits].astype("<u4").tobytes(), order[groups * 32:].astype("<u4").tobytes()


# ------------------------------------------------------------------------------------------------ noise of one read, from its consensus span
def at(*positions, code="0"):
    return lambda L, span, rng: [(p % L, code) for p in positions]


def every_position(code_of):
    """L entries, one per position; code_of(p) -> '0'..'3'"""
    return lambda L, span, rng: [(p, code_of(p)) for p in range(L)]


def twice(base, first, second):
    """a position whose consensus base is `base` named twice: the second entry has delta 0 (read_noisepos), the codes are `first` then `second`"""
    def noise(L, span, rng):
        where = [p for p in range(L) if span[p] == ord(base)]
        assert where, "no %s in this read's consensus" % base
        p = where[len(where) // 2]
        return [(p, first), (p, second)]
    return noise


def _draw_noise(rng, L, style):
    if style == "clean" or (style in ("random", "noN") and rng.random() < 0.5):
        return []
    k = int(rng.integers(1, min(L, 4) + 1))
    ps = sorted(int(p) for p in rng.choice(L, size=k, replace=False))
    codes = [str(c) for c in rng.choice(4 if style != "noN" else 3, size=k, p=[.3, .3, .3, .1] if style != "noN" else None)]
    if style == "allN":
        codes[int(rng.integers(k))] = "3"
    return list(zip(ps, codes))


# ------------------------------------------------------------------------------------------------ the builder
def build(seed, L, shards, singletons, unaligned_N, order=None, numbits=None):
    """-> ({file name: bytes} ready for oracle_lib.stage_dir, [properties])

    shards: one dict per shard -- n (reads; 0: all seven files empty); style: "random" | "clean" | "noN" | "allN"; styles: [(first, last + 1, style)] over
    ranges of reads; pos_menu: the position bytes half of the reads after the first draw from (the others: uniform in 0..L); pos: {read: byte}; reads:
    {read (negative: from the end): dict(noise=callable(L, span, rng) -> [(position, code)], rev=bool)}.
    singletons / unaligned_N: how many reads of read_singleton.txt / lines of input_N.dna.
    order: None (no -p files) or dict(clean="identity" | "reversed" | "random", N_lines="random" | "edges"): read_order.bin (packed at `numbits`, pack_order's
    own when None), read_order_N_pe.bin, read_order_N.bin"""
    rng = np.random.default_rng(seed)
    files = {"read_meta.txt": b"%d\n" % L}
    E = len(shards)
    n_clean = n_withN = 0
    for e, sh in enumerate(shards):
        n = sh["n"]
        pos = [L] + [int(rng.choice(sh.get("pos_menu", [0, 1, L - 1, L]))) if rng.random() < 0.5 else int(rng.integers(0, L + 1)) for _ in range(n - 1)]
        for i, p in sh.get("pos", {}).items():
            assert 0 < i < n and 0 <= p <= L
            pos[i] = p
        pos = pos[:n]
        consensus = BASES[rng.integers(0, 4, size=sum(pos))].tobytes()
        styles = [sh.get("style", "random")] * n
        for lo, hi, st in sh.get("styles", []):
            styles[lo:hi] = [st] * (hi - lo)
        special = {i % n: r for i, r in sh.get("reads", {}).items()}
        noise_txt, noisepos, rev = bytearray(), bytearray(), bytearray()
        start = -L
        for i in range(n):
            start += pos[i]
            span = consensus[start:start + L]
            sp = special.get(i, {})
            entries = sp["noise"](L, span, rng) if "noise" in sp else _draw_noise(rng, L, styles[i])
            r = sp["rev"] if sp.get("rev") is not None else bool(rng.integers(2))
            prev, final = 0, {}
            for p, code in entries:
                assert prev <= p < L and code in "0123"
                noisepos.append(p - prev); noise_txt += code.encode(); prev = p
                final[p] = code                                         # the last entry for a position stands (decoder.cpp:106 rewrites currentread[noisepos])
            noise_txt += b"\n"
            rev += b"r" if r else b"d"
            if "3" in final.values():
                n_withN += 1
            else:
                n_clean += 1
        files["read_seq.txt.%d" % e], files["read_seq.txt.%d.tail" % e] = pack_seq(consensus)
        files["read_rev.txt.%d" % e], files["read_rev.txt.%d.tail" % e] = pack_rev(bytes(rev))
        files["read_pos.txt.%d" % e], files["read_noise.txt.%d" % e], files["read_noisepos.txt.%d" % e] = bytes(pos), bytes(noise_txt), bytes(noisepos)
        if n == 0:
            assert not any(files[k] for k in files if k.split(".")[-1] == str(e) or k.endswith(".%d.tail" % e))
    sing = BASES[rng.integers(0, 4, size=singletons * L)].tobytes()
    files["read_singleton.txt"], files["read_singleton.txt.tail"] = pack_seq(sing)
    un = BASES[rng.integers(0, 4, size=(unaligned_N, L))]
    for row in un:
        row[rng.choice(L, size=int(rng.integers(1, min(L, 3) + 1)), replace=False)] = ord("N")
    files["input_N.dna"] = b"".join(row.tobytes() + b"\n" for row in un)
    # what was packed unpacks to what was drawn
    u = dm.unpack(files, E)
    assert u["singleton"] == sing and all(len(u["rev"][e]) == shards[e]["n"] for e in range(E))
    nC, nN = n_clean + singletons, n_withN + unaligned_N
    if order is not None:
        total = nC + nN
        assert nC >= 1, "pack_order.cpp:36 is undefined without clean reads"
        kind = order.get("clean", "random")
        perm = {"identity": np.arange(nC), "reversed": np.arange(nC)[::-1], "random": rng.permutation(nC)}[kind].astype(np.uint32)
        files["read_order.bin"], files["read_order.bin.tail"] = pack_order(perm, nC.bit_length() if numbits is None else numbits)
        assert (dm.unpack_order(files) == perm).all()
        files["read_order_N_pe.bin"] = rng.permutation(nN).astype("<u4").tobytes()
        if order.get("N_lines", "random") == "edges":                   # line 0, the last line, and the others in one adjacent run in the middle
            assert nN >= 4 and total >= nN + 2
            mid = (total - (nN - 2)) // 2
            lines = np.array([0] + list(range(mid, mid + nN - 2)) + [total - 1]) if mid > 0 and mid + nN - 2 < total else None
            assert lines is not None
        else:
            lines = np.sort(rng.choice(total, size=nN, replace=False))
        assert lines.shape[0] == nN and (np.diff(lines) > 0).all()
        files["read_order_N.bin"] = lines.astype("<u4").tobytes()
    return files, properties(files, E, L)


# ------------------------------------------------------------------------------------------------ what an archive holds, from its bytes
def properties(files, E, L):
    props = set()
    u = dm.unpack(files, E)
    props.add("E=%d" % E)
    counts = [len(files["read_pos.txt.%d" % e]) for e in range(E)]
    if any(counts[e] == 0 and any(counts[:e]) and any(counts[e + 1:]) for e in range(E)):
        assert all(not files[k % e] for e in range(E) if counts[e] == 0 for k in
                   ("read_seq.txt.%d", "read_seq.txt.%d.tail", "read_pos.txt.%d", "read_noise.txt.%d", "read_noisepos.txt.%d", "read_rev.txt.%d", "read_rev.txt.%d.tail"))
        props.add("a shard of no reads between two shards that have reads")
    pairs = {"d": set(), "r": set()}
    n_clean = n_withN = 0
    for e in range(E):
        n = counts[e]
        if n == 0:
            continue
        pos, seq, rev = files["read_pos.txt.%d" % e], u["seq"][e], u["rev"][e]
        lines = files["read_noise.txt.%d" % e].split(b"\n")
        deltas = files["read_noisepos.txt.%d" % e]
        assert pos[0] == L and len(seq) == sum(pos) and len(rev) == n and len(lines) == n + 1 and lines[n] == b""
        props.add("read_seq tail of %d bases" % len(files["read_seq.txt.%d.tail" % e]))
        props.add("read_rev tail of %d flags" % len(files["read_rev.txt.%d.tail" % e]))
        if len(files["read_rev.txt.%d" % e]) == 0:
            props.add("read_rev is all tail")
        for p, name in ((L, "position byte L after the first read"), (1, "position byte 1"), (L - 1, "position byte L-1")):
            if p in pos[1:]:
                props.add(name)
        zeros = best = 0
        for p in pos[1:]:
            zeros = zeros + 1 if p == 0 else 0
            best = max(best, zeros)
        if best > 256:
            props.add("position byte 0 in a run of more than 256 reads")
        hasN = []
        start, d = -L, 0
        for i in range(n):
            start += pos[i]
            span = seq[start:start + L]
            assert len(span) == L
            final, prev, ps = {}, 0, []
            for k, code in enumerate(lines[i]):
                p = prev + deltas[d]; d += 1
                assert p < L and (k == 0 or p >= prev)
                fwd = "forward" if rev[i] == ord("d") else "reverse"
                if k and p == prev:
                    props.add("position named twice (consensus %s: %s then %s) on a %s read" % (chr(span[p]), chr(lines[i][k - 1]), chr(code), fwd))
                pairs[chr(rev[i])].add((span[p], code))
                final[p] = code; ps.append(p); prev = p
            if ps and ps[0] == 0:
                props.add("noise at position 0 (first delta 0)")
            if ps and ps[-1] == L - 1:
                props.add("noise at position L-1")
            if len(set(ps)) == L:
                props.add("noise at every position of a read")
            if ps == [L - 1]:
                props.add("a single noise entry with delta L-1")
            hasN.append(ord("3") in final.values())
        assert d == len(deltas)
        n_withN += sum(hasN); n_clean += n - sum(hasN)
        if hasN[0]:
            props.add("N read first in its shard")
        if hasN[-1]:
            props.add("N read last in its shard")
        props.add("a shard where every read has N" if all(hasN) else "a shard where no read has N" if not any(hasN) else "a shard with and without N")
        if n > 256 and hasN[255] and hasN[256]:
            props.add("adjacent N reads across a workgroup boundary (reads 255 and 256)")
    for r, name in (("d", "forward"), ("r", "reverse")):
        if len(pairs[r]) == 16:
            props.add("all 16 (consensus base, code) pairs on %s reads" % name)
    ns = len(u["singleton"]) // L
    props.add("no singletons" if ns == 0 else "one singleton" if ns == 1 else "singletons")
    props.add("read_singleton tail of %d bases" % len(files["read_singleton.txt.tail"]))
    props.add("input_N.dna present" if files["input_N.dna"] else "input_N.dna empty")
    if "read_order_N.bin" in files:
        order = dm.unpack_order(files)
        lines = np.frombuffer(files["read_order_N.bin"], dtype="<u4")
        pe = np.frombuffer(files["read_order_N_pe.bin"], dtype="<u4")
        nC, nN = order.shape[0], lines.shape[0]
        total = nC + nN
        assert nC == n_clean + ns and nN == n_withN + len(files["input_N.dna"]) // (L + 1)
        assert (np.sort(order) == np.arange(nC)).all() and (np.sort(pe) == np.arange(nN)).all()
        assert (np.diff(lines.astype(np.int64)) > 0).all() and (nN == 0 or int(lines[-1]) < total)
        props.add("-p")
        props.add("order identity" if (order == np.arange(nC)).all() and nC > 1 else "order reversed" if (order == np.arange(nC)[::-1]).all() and nC > 1 else "order permuted")
        if nN and lines[0] == 0:
            props.add("line 0 has N")
        if nN and lines[-1] == total - 1:
            props.add("the last line has N")
        if (np.diff(lines.astype(np.int64)) == 1).any():
            props.add("adjacent lines with N")
        if nN == 0:
            props.add("nN=0")
        if nC == 1:
            props.add("nC=1")
        props.add("at most 40 lines" if total <= 40 else "more than 40 lines")
        numbits = int(np.frombuffer(files["read_order.bin"][:4], dtype="<i4")[0])
        props.add("numbits=%d" % numbits)
        if numbits > nC.bit_length():
            props.add("numbits above pack_order's")
        if nC >= 32:
            props.add("packed groups of 32")
        if nC % 32:
            props.add("read_order.bin.tail holds entries")
    return sorted(props)


# ------------------------------------------------------------------------------------------------ the case list
Case = collections.namedtuple("Case", "id kw want")

LENGTHS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 254, 255]
COUNTS = [1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 513]
P_RANDOM = dict(clean="random")


def _grid():
    """every L at 257 reads in one shard; every n at L in 1, 100, 255 in two shards of n reads each.  Singletons 0, 1, 2, 3, ... by turns: with the length
    they give every tail of read_singleton"""
    out = []
    for k, L in enumerate(LENGTHS):
        out.append(Case("L%d_n257" % L, dict(seed=1000 + L, L=L, shards=[dict(n=257)], singletons=k % 4, unaligned_N=k % 3, order=P_RANDOM), ["-p", "E=1"]))
    for L in (1, 100, 255):
        for k, n in enumerate(COUNTS):
            want = ["-p", "E=2"] + (["read_rev is all tail"] if n < 8 else []) + ["read_rev tail of %d flags" % (n % 8)]
            out.append(Case("L%d_2x%d" % (L, n), dict(seed=2000 + 1000 * L + n, L=L, shards=[dict(n=n), dict(n=n)], singletons=1 + k % 3, unaligned_N=(k + 1) % 3,
                                                      order=P_RANDOM), want))
    return out


def _edges(L):
    """the stream edges in one archive of five shards, two of them empty"""
    reads = {0: dict(noise=at(0, code="3")), 1: dict(noise=at(0), rev=False), 2: dict(noise=at(L - 1), rev=True), 3: dict(noise=every_position(lambda p: "012"[p % 3])),
             4: dict(noise=at(L - 1, code="2")), 5: dict(noise=every_position(lambda p: "0123"[p % 4]), rev=False), 6: dict(noise=every_position(lambda p: "0123"[(p + 1) % 4]), rev=True),
             -1: dict(noise=at(L - 1, code="3"))}
    shards = [dict(n=300, reads=reads, pos={10: 1, 11: L - 1, 12: L, 13: 0}), dict(n=0),
              dict(n=270, style="allN", pos={i: 0 for i in range(1, 270)}), dict(n=0), dict(n=9, style="noN")]
    want = ["E=5", "a shard of no reads between two shards that have reads", "noise at position 0 (first delta 0)", "noise at position L-1",
            "noise at every position of a read", "a single noise entry with delta L-1", "N read first in its shard", "N read last in its shard",
            "a shard where every read has N", "a shard where no read has N", "adjacent N reads across a workgroup boundary (reads 255 and 256)",
            "position byte 0 in a run of more than 256 reads", "position byte L after the first read", "position byte 1", "position byte L-1",
            "singletons", "input_N.dna present", "-p", "line 0 has N", "the last line has N", "adjacent lines with N"]
    if L >= 4:
        want += ["all 16 (consensus base, code) pairs on forward reads", "all 16 (consensus base, code) pairs on reverse reads"]
    return Case("edges_L%d" % L, dict(seed=77 + L, L=L, shards=shards, singletons=3, unaligned_N=2, order=dict(clean="random", N_lines="edges")), want)


def _twice(L):
    reads = {3: dict(noise=twice("C", "1", "0"), rev=False), 4: dict(noise=twice("C", "1", "0"), rev=True),
             8: dict(noise=twice("G", "3", "0"), rev=False), 9: dict(noise=twice("G", "3", "0"), rev=True)}
    want = ["position named twice (consensus %s: %s then 0) on a %s read" % (b, c, d) for b, c in (("C", "1"), ("G", "3")) for d in ("forward", "reverse")]
    return Case("named_twice_L%d" % L, dict(seed=5 + L, L=L, shards=[dict(n=12, style="noN", reads=reads)], singletons=0, unaligned_N=0, order=P_RANDOM), want + ["-p", "no singletons", "input_N.dna empty"])


def _small_p():
    sh = [dict(n=14, styles=[(0, 3, "allN"), (9, 11, "allN")]), dict(n=11, style="noN")]
    out = [Case("p_" + kind, dict(seed=31, L=9, shards=sh, singletons=5, unaligned_N=2, order=dict(clean=kind, N_lines="edges")),
                ["-p", "order " + name, "line 0 has N", "the last line has N", "adjacent lines with N", "at most 40 lines", "read_order.bin.tail holds entries"])
           for kind, name in (("identity", "identity"), ("reversed", "reversed"), ("random", "permuted"))]
    out.append(Case("p_nN0", dict(seed=32, L=9, shards=[dict(n=40, style="noN")], singletons=2, unaligned_N=0, order=P_RANDOM), ["-p", "nN=0", "input_N.dna empty", "packed groups of 32"]))
    out.append(Case("p_nC1", dict(seed=33, L=9, shards=[dict(n=20, style="allN")], singletons=1, unaligned_N=3, order=P_RANDOM), ["-p", "nC=1", "one singleton", "a shard where every read has N"]))
    out.append(Case("d_only_allN", dict(seed=34, L=6, shards=[dict(n=65, style="allN")], singletons=0, unaligned_N=0), ["no singletons", "input_N.dna empty", "a shard where every read has N"]))
    return out


CASES = _grid() + [_edges(4), _edges(100), _edges(255), _twice(100), _twice(255)] + _small_p()
BIN_READS_CASE = "p_random"          # HARC_AMD_BIN_READS unset, 1 and 5 on it: at most 40 lines

# what the case list as a whole must hold, beyond what each case names for itself
COVERAGE = (["read_seq tail of %d bases" % t for t in range(4)] + ["read_singleton tail of %d bases" % t for t in range(4)] + ["read_rev tail of %d flags" % t for t in (0, 1, 7)]
            + ["E=1", "E=2", "E=5", "no singletons", "one singleton", "singletons", "input_N.dna empty", "input_N.dna present", "read_rev is all tail",
               "order identity", "order reversed", "order permuted", "nN=0", "nC=1"])


def sweep_case(b):
    """numbits sweep: singletons only, E = 1 with empty shard files, L = 3; nC = min(2^b, 2^20) + (0 for even b, 37 for odd b), capped at 2^b; a random
    permutation packed at numbits = b.  From b = 21 up the file uses more bits than pack_order would"""
    nC = min(min(2 ** b, 2 ** 20) + (37 if b % 2 else 0), 2 ** b)
    want = ["-p", "numbits=%d" % b, "packed groups of 32", "order permuted", "nN=0"] + (["numbits above pack_order's"] if b >= 22 else []) + (["read_order.bin.tail holds entries"] if nC % 32 else [])
    return Case("numbits_%d" % b, dict(seed=900 + b, L=3, shards=[dict(n=0)], singletons=nC, unaligned_N=0, order=P_RANDOM, numbits=b), want)


SWEEP = list(range(5, 33))


def archive(case):
    """-> (files, properties, E, L) of a case; the properties the case is there for are asserted"""
    files, props = build(**case.kw)
    missing = [w for w in case.want if w not in props]
    assert not missing, "%s lost what it is there for: %s" % (case.id, missing)
    return files, props, len(case.kw["shards"]), case.kw["L"]


def reference_chain(files, L, E, tmp):
    """output.dna of unpack_order.out, decoder_preserve_L<L>_e<E>.out and merge_N.out on a copy of the archive; None where oracle/_ref does not hold them"""
    exes = [os.path.join(ol.ORACLE_DIR, "_ref", x) for x in ("unpack_order.out", "decoder_preserve_L%d_e%d.out" % (L, E), "merge_N.out")]
    if not all(os.path.exists(x) for x in exes):
        return None
    base = ol.stage_dir(tmp, files)
    for x in exes:
        subprocess.run([x, base], check=True, stdout=subprocess.DEVNULL)
    return ol.read_dir(base)["output.dna"]
