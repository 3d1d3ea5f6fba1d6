"""Texts for the BGZF writer (harc_amd/csrc/deflate_member.h, bgzf_out.hip), shared by the host test and the GPU test: for every part of the encoder the
smallest text at which it can go wrong.  Also the token rule once more in plain Python (run_lengths), to show that a text holds the runs it is meant to."""
import random

from tests import bgzf_util as bu

MEMBER = 65280


def _fib(k):
    a, b, out = 1, 1, []
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return out


def fibonacci_bytes(nsym=22, seed=5):
    """byte frequencies 1, 1, 2, 3, 5, ...: the unlimited Huffman code of 22 such symbols (46 367 bytes) is 21 bits deep"""
    f = _fib(nsym)
    b = bytearray()
    for s, c in enumerate(f):
        b += bytes([65 + s]) * c
    random.Random(seed).shuffle(b)
    return bytes(b)


def records(ids, reads, quals):
    return b"".join(b"%s\n%s\n+\n%s\n" % t for t in zip(ids, reads, quals))


def every_run_length():
    """records of L = 255 in which line k and line k - 4 share, record after record, one run of every length 3 .. 258 and otherwise differ in every column
    (but for newlines, '+' and '@').  Inside the read up to 253; a suffix of the read and the "\\n+\\n" behind it up to 257; 258 is a whole read and "\\n+\\n"
    behind an id that is a byte longer than the one before, so that the distance changes where the read starts."""
    rng = random.Random(258)
    L = 255

    def other(prev, alphabet):
        return bytes(rng.choice([c for c in alphabet if c != p]) for p in prev)
    ids, reads, quals = [b"@a"], [bytes(rng.choice(b"ACGT") for _ in range(L))], [bytes(rng.choice(b"FGHI") for _ in range(L))]
    for r in range(3, 259):
        rd = bytearray(other(reads[-1], b"ACGT"))
        idn = b"@a" if ids[-1][:2] == b"@b" else b"@b"
        if r <= 253:
            rd[1:1 + r] = reads[-1][1:1 + r]
        elif r <= 257:
            rd[L - (r - 3):] = reads[-1][L - (r - 3):]
        else:
            rd[:] = reads[-1]
            idn += b"x"
        ids.append(idn); reads.append(bytes(rd)); quals.append(other(quals[-1], b"FGHI"))
    return records(ids, reads, quals)


def run_lengths(text):
    """the token rule of deflate_member.h for one member: the lengths of the maximal runs of equal bytes with one distance"""
    assert len(text) <= MEMBER
    starts, dist = [0], []
    for j, c in enumerate(text):
        d = starts[-1] - starts[-5] if len(starts) >= 5 else 0
        if d > 32768:
            d = 0
        dist.append(d if d and text[j] == text[j - d] else 0)
        if c == 10:
            starts.append(j + 1)
    runs, j = [], 0
    while j < len(text):
        r = 1
        if dist[j]:
            while j + r < len(text) and dist[j + r] == dist[j]:
                r += 1
            runs.append(r)
        j += r
    return runs


def illumina_text(n=20000, seed=11):
    """n records of 100 bases with ids as a sequencer writes them: @SRR870667.<i> HWI-ST1234:100:C0ABCACXX:3:<tile>:<x>:<y> length=100"""
    rng = random.Random(seed)
    out, tile, x = [], 1101, 1000
    for i in range(1, n + 1):
        x += rng.randrange(1, 40)
        if x > 20000:
            x, tile = 1000 + rng.randrange(50), tile + 1
        rid = b"@SRR870667.%d HWI-ST1234:100:C0ABCACXX:3:%d:%d:%d length=100" % (i, tile, x, rng.randrange(1000, 200000))
        seq = bytes(rng.choice(b"ACGT") if rng.random() > 0.002 else 78 for _ in range(100))
        q = bytes(33 + min(40, max(2, int(rng.gauss(30, 6)))) for _ in range(100))
        out.append(rid + b"\n" + seq + b"\n+\n" + q + b"\n")
    return b"".join(out)


def texts():
    """{name: text}"""
    rng = random.Random(17)
    fq = bu.fastq_text(1300, 100, seed=3)
    assert len(fq) > 2 * MEMBER + 1
    t = {"empty": b"", "one_byte": b"A", "one_newline": b"\n", "newlines_1000": b"\n" * 1000, "one_symbol_member": b"A" * MEMBER}
    for cut in (65279, 65280, 65281, 130560, 130561):
        t["fastq_cut_%d" % cut] = fq[:cut]
    for nrec in (300, 600):                                        # whole records (one and two members), the last newline taken away
        whole = bu.fastq_text(nrec, 100, seed=4)
        assert whole.endswith(b"\n")
        t["fastq_%d_records_no_final_newline" % nrec] = whole[:-1]
    t["random_70000"] = bytes(rng.getrandbits(8) for _ in range(70000))
    t["fibonacci_22_symbols"] = fibonacci_bytes()
    assert len(t["fibonacci_22_symbols"]) == 46367
    t["L1_empty_ids"] = records([b""] * 500, [bytes([rng.choice(b"ACGT")]) for _ in range(500)], [bytes([rng.choice(b"FGH")]) for _ in range(500)])
    one = bytes(rng.choice(b"ACGT") for _ in range(255)), bytes(rng.choice(b"FGHIJ#") for _ in range(255))
    t["identical_300_L255"] = records([b"@same id"] * 300, [one[0]] * 300, [one[1]] * 300)
    t["every_run_length_L255"] = every_run_length()
    idlens = [0, 1, 2, 3, 5, 8, 12, 20, 30, 50, 90, 150, 250, 400, 700, 1000, 1500, 2500, 4000, 6000, 10000, 14000, 20000, 30000]
    rd, ql = bytes(rng.choice(b"ACGT") for _ in range(20)), bytes(rng.choice(b"FGHIJ") for _ in range(20))
    t["id_lengths_many_distance_codes"] = records([b"@" + b"x" * k for k in idlens], [rd] * len(idlens), [ql] * len(idlens))
    ids, reads, quals = [b"@r%d" % i for i in range(40)], [bytes(rng.choice(b"ACGT") for _ in range(50))] * 40, [bytes(rng.choice(b"FGH") for _ in range(50))] * 40
    ids[20] = bytes(rng.choice(b"abcdefghij") for _ in range(40000))
    t["one_id_of_40000"] = records(ids, reads, quals)
    t["one_distance_symbol"] = bu.fastq_text(200, 50, seed=6, id_len=12)
    t["no_match_no_newline"] = bytes(rng.choice(b"ACGT") for _ in range(5000))
    t["no_match_three_lines"] = b"@id\n" + bytes(rng.choice(b"ACGT") for _ in range(3000)) + b"\n+\n" + bytes(rng.choice(b"FGHIJ") for _ in range(3000))
    return t
