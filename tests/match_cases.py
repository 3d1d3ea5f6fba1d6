"""The rule of a match by sequence (./harc -d -M MOTIFS [-e K]; README: "-M and what it promises") restated in plain Python from its text, not from the C++, and the
cases the host twin and the kernel are held to.

The list is split at newlines, a last line without its newline counts; a line that is empty or begins with '>' is skipped; every other line is a motif of bytes from
ACGTNacgtn folded to upper case (any other byte refuses the list, naming the line and the byte), of 1 to 255 bases, with more than K bases that are not N; equal
motifs count once; at most 1024 distinct motifs and 2^20 bytes.  rc(p) reverses p and exchanges A and T, C and G.  Motif p matches read r when for q = p or rc(p) and
some offset 0 <= o <= L - m at most K of the j with q[j] != 'N' have r[o + j] != q[j]; a read byte that is not one of A C G T equals no motif base."""
import functools
import random

MAX_LEN, MAX_MOTIFS, MAX_LIST, MAX_K = 255, 1024, 2 ** 20, 8
READ_LENGTHS = (1, 31, 32, 33, 63, 64, 65, 100, 127, 128, 129, 191, 192, 193, 255)


class Refused(Exception):
    """the rule refuses the list: .line is the line it names, counted from 1 (0: the list as a whole)"""

    def __init__(self, line, why):
        Exception.__init__(self, why)
        self.line = line


def parse(text, k=0):
    """the distinct motifs of the list in list order"""
    if len(text) > MAX_LIST:
        raise Refused(0, "more than 2^20 bytes")
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    motifs = []
    for no, l in enumerate(lines, 1):
        if l == b"" or l[:1] == b">":
            continue
        for b in l:
            if b not in b"ACGTNacgtn":
                raise Refused(no, "byte 0x%02x" % b)
        p = l.upper()
        if len(p) > MAX_LEN:
            raise Refused(no, "longer than 255")
        if len(p) - p.count(b"N") <= k:
            raise Refused(no, "every window would match")
        if p in motifs:
            continue
        if len(motifs) == MAX_MOTIFS:
            raise Refused(no, "more than 1024 distinct motifs")
        motifs.append(p)
    if not motifs:
        raise Refused(0, "no motif")
    return motifs


def rc(p):
    return p[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def _strand(q, r, k):
    m, n = len(q), len(r)
    if k == 0 and b"N" not in q:
        return q in r                                                 # (a read's N equals no base of q, which has none)
    for o in range(n - m + 1):
        mis = 0
        for j in range(m):
            if q[j] != 78 and r[o + j] != q[j]:
                mis += 1
                if mis > k:
                    break
        if mis <= k:
            return True
    return False


def matches(p, r, k=0):
    return _strand(p, r, k) or _strand(rc(p), r, k)


def flags_hits(motifs, reads, k=0):
    """(a flag byte per read, a hit byte per motif)"""
    hits = [0] * len(motifs)
    flags = bytearray(len(reads))
    for i, r in enumerate(reads):
        for j, p in enumerate(motifs):
            if matches(p, r, k):
                flags[i] = 1
                hits[j] = 1
    return bytes(flags), bytes(hits)


def missing(motifs, hits):
    return [p for p, h in zip(motifs, hits) if not h][:10]


def text_of(reads):
    return b"".join(r + b"\n" for r in reads)


def fastq_reads(fq):
    return fq.split(b"\n")[1:-1:4]


def filter_fastq(fq, flags):
    """the records of the FASTQ text whose flag is set"""
    l = fq.split(b"\n")
    return b"".join(b"".join(x + b"\n" for x in l[4 * i:4 * i + 4]) for i in range(len(flags)) if flags[i])


def gather(reads, flags):
    return b"".join(r + b"\n" for r, f in zip(reads, flags) if f)


# ------------------------------------------------------------------------------------------------ the cases
def _seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def _plant(r, o, q):
    assert o + len(q) <= len(r)
    return r[:o] + q + r[o + len(q):]


def _other(b):
    return b"CGTA"[b"ACGT".index(bytes([b]))]


def _with_mismatches(q, positions):
    q = bytearray(q)
    for j in positions:
        q[j] = _other(q[j])
    return bytes(q)


def _case(motifs, reads, k=0):
    """list text, reads, K, and what the restatement says of them, computed once"""
    ms = parse(motifs, k)
    flags, hits = flags_hits(ms, reads, k)
    return dict(motifs=motifs, reads=reads, k=k, L=len(reads[0]), parsed=ms, flags=flags, hits=hits)


def _length_case(L):
    """every motif length of the issue at one read length: planted at offset 0, at the last offset, in the middle, and reads that carry none of them"""
    rng = random.Random(1000 + L)
    lengths = sorted(set(m for m in (1, 2, 63, 64, 65, 128, L, L + 1) if m <= MAX_LEN))      # (L + 1 = 256 is no motif: the list refuses it)
    motifs = []
    for m in lengths:
        motifs.append(b"A" if m == 1 else b"AT" if m == 2 and L > 1 else b"AG" if m == 2 else _seq(rng, m - 1, "AG") + b"A")
    reads = [_seq(rng, L, "CG") for _ in range(3)]                    # no A, no T: nothing matches on either strand
    for p in motifs:
        m = len(p)
        if m > L:
            continue
        back = _seq(rng, L, "CG")
        reads += [_plant(back, 0, p), _plant(back, L - m, p), _plant(back, (L - m) // 2, rc(p))]
        if m > 2:                                                     # the motif cut short by one base at either end of the read: no match
            reads += [(p[1:] + back)[:L], (back + p[:-1])[-L:]]
    reads.append(_seq(rng, L, "CG"))
    return _case(text_of(motifs), reads)


def _planted(L, m, offsets, strand):
    rng = random.Random(77 + L + m)
    p = b"ACGTTGCAAG"[:m] if m <= 10 else _seq(rng, m)
    assert p != rc(p)
    q = p if strand == "+" else rc(p)
    reads = []
    for o in offsets:
        reads += [_plant(_seq(rng, L, "CT"), o, q), _seq(rng, L, "CT")]
    return p, reads


def _mismatch_cases():
    """a window with exactly K and exactly K + 1 mismatches, K = 0, 1, 2 and 8: the mismatches at the window's first and last base and at the edges of the planes'
    words (bases 31 | 32 and 63 | 64 of the read), the base that makes K + 1 of them at each of those places in turn"""
    L, m, o = 100, 70, 10
    rng = random.Random(5)
    p = _seq(rng, m, "AG")                                            # against reads of C and T: every other window is far from it, on both strands
    places = [0, m - 1, 63 - o, 64 - o, 31 - o, 32 - o, 40, 45, 50]
    out = {}
    for k in (0, 1, 2, 8):
        reads = []
        for turn in range(4):
            order = places[turn:] + places[:turn]
            for strand in (p, rc(p)):
                reads.append(_plant(_seq(rng, L, "CT"), o, _with_mismatches(strand, order[:k])))      # (the places are the window's, on either strand)
                reads.append(_plant(_seq(rng, L, "CT"), o, _with_mismatches(strand, order[:k + 1])))
        c = _case(p + b"\n", reads, k)
        assert c["flags"] == bytes([1, 0] * (len(reads) // 2)), k
        out["mismatch_K%d" % k] = c
    return out


def _random_case():
    """2000 reads of 100, three motifs of 12, 20 and 33 planted in about half of them, a fourth that occurs nowhere"""
    rng = random.Random(20240)
    motifs = [_seq(rng, 12), _seq(rng, 20), _seq(rng, 33), _seq(rng, 25)]
    reads = []
    for i in range(2000):
        r = _seq(rng, 100)
        if rng.random() < 0.5:
            p = motifs[rng.randrange(3)]
            r = _plant(r, rng.randrange(100 - len(p) + 1), p if rng.random() < 0.5 else rc(p))
        reads.append(r)
    return _case(text_of(motifs), reads)


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for L in READ_LENGTHS:
        out["lengths_L%d" % L] = _length_case(L)
    # one motif at every residue of the lane split and the first constant step, at the last offset, and across the 64-bit edges of the planes
    for strand in "+-":
        p, reads = _planted(140, 10, list(range(16)) + [60, 124, 130], strand)
        c = _case(p + b"\n", reads)
        assert c["flags"] == bytes([1, 0] * (len(reads) // 2))
        out["planted_" + ("forward" if strand == "+" else "reverse")] = c
    rng = random.Random(9)
    back = [_seq(rng, 50, "CT") for _ in range(6)]
    c = _case(b"ACGT\n", [_plant(back[0], 0, b"ACGT"), back[1], _plant(back[2], 46, b"ACGT"), back[3], _plant(back[4], 31, b"ACGT")])
    assert c["flags"] == bytes([1, 0, 1, 0, 1])
    out["palindrome"] = c
    out.update(_mismatch_cases())
    # N: a read's N inside the window is a mismatch, a read of N alone is not selected, a motif's N is not compared, not even with a read's N
    w = b"ACGTACGGTA"
    reads = [_plant(back[0], 7, w), _plant(back[0], 7, w[:4] + b"N" + w[5:]), b"N" * 50, _plant(back[1], 30, b"ACNNNNGT"), _plant(back[2], 30, b"ACTCTCGT"),
             _plant(back[3], 30, b"ACTCTCGA"), back[4]]
    for k, want in ((0, [1, 0, 0, 1, 1, 0, 0]), (1, [1, 1, 0, 1, 1, 1, 0])):
        c = _case(w + b"\nACNNNNGT\n", reads, k)
        assert list(c["flags"]) == want, (k, list(c["flags"]))
        out["n_handling_K%d" % k] = c
    out["n_read_K3"] = _case(b"ACGT\n", [b"N" * 50, b"n" * 50, b"acgt" * 12 + b"ac", _plant(b"N" * 50, 9, b"ACGT"), _plant(b"N" * 50, 9, b"ACG")], 3)
    assert list(out["n_read_K3"]["flags"]) == [0, 0, 0, 1, 1]                # (with K = 3 of 4 bases one agreeing base is a match)
    # the list's own forms: a FASTA of adapters, lower case, duplicates, a motif beside its reverse complement, a last line without its newline
    p = b"AGATCGGAAGAGC"
    out["fasta_list"] = _case(b">adapter 1\n" + p.lower() + b"\n\n>the same\n" + p + b"\n>its reverse complement\n" + rc(p) + b"\n>nowhere\nGGGGGGGGGGGGGGGG",
                              [_plant(back[0], 3, p), back[1], _plant(back[2], 20, rc(p))])
    assert out["fasta_list"]["parsed"] == [p, rc(p), b"G" * 16] and out["fasta_list"]["hits"] == b"\1\1\0" and out["fasta_list"]["flags"] == b"\1\0\1"
    r = _random_case()
    assert 0 < sum(r["flags"]) < 2000 and sum(r["hits"]) == 3 and len(r["hits"]) == 4
    out["random_2000"] = r
    rng = random.Random(31)
    motifs = [_seq(rng, 16), _seq(rng, 40)]
    reads = []
    for i in range(300):
        x = _seq(rng, 77)
        if i % 3 == 0:
            p = motifs[i % 2]
            x = _plant(x, rng.randrange(77 - len(p) + 1), _with_mismatches(p if i % 4 else rc(p), rng.sample(range(len(p)), i % 5)))
        reads.append(x)
    c = _case(text_of(motifs), reads, 2)
    assert 0 < sum(c["flags"]) < 100
    out["random_300_K2"] = c
    return out


def refusals():
    """(list text, K, the line the refusal names; 0: the list as a whole)"""
    return [
        (b"ACGT\nAC\rT\n", 0, 2),
        (b"ACGT\r\n", 0, 1),
        (b">x\n\nACGU\n", 0, 3),
        (b"ACGT\nAC GT\n", 0, 2),
        (b"ACGT\n" + b"A" * 256 + b"\n", 0, 2),
        (b"ACGT\nNNNN\n", 0, 2),
        (b"ACGTA\nACNNT\n", 3, 2),
        (b"ACGTACGTA\nACGTACGT", 8, 2),
        (b">only a header\n\n", 0, 0),
        (b"", 0, 0),
        (b"".join(b"%s\n" % _kmer(i) for i in range(1025)), 0, 1025),
        (b">" + b"x" * (2 ** 20) + b"\nACGT\n", 0, 0),
    ]


def _kmer(i):
    return bytes(b"ACGT"[(i >> (2 * j)) & 3] for j in range(6))
