"""Seeded synthetic read generator for the tests (numpy RandomState is stable across numpy versions).
Same spirit as the reference's util/gen_fastq_noRC (uniform read starts on an i.i.d. genome; -e: 1 % substitutions of which
a quarter become N, gen_fastq_noRC.cpp:67-71,119-130) plus reverse-complemented odd reads as util/gen_fastq."""
import numpy as np

_COMP = np.zeros(256, dtype=np.uint8)
for a, b in zip(b"ACGTN", b"TGCAN"):
    _COMP[a] = b


def reads_array(seed, n, L, genome_len, err=0.0, rc=True, n_frac=0.25):
    """-> uint8 array [n, L] of ASCII bases"""
    rs = np.random.RandomState(seed)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, size=genome_len)]
    starts = rs.randint(0, genome_len - L, size=n)
    idx = starts[:, None] + np.arange(L)[None, :]
    r = genome[idx].copy()
    if err > 0:
        e = rs.random_sample((n, L)) < err
        isN = e & (rs.random_sample((n, L)) < n_frac)
        sub = e & ~isN
        code = np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), r)
        newcode = (code + rs.randint(1, 4, size=(n, L))) % 4
        r[sub] = np.frombuffer(b"ACGT", dtype=np.uint8)[newcode[sub]]
        r[isN] = ord("N")
    if rc:
        odd = np.arange(n) % 2 == 1
        r[odd] = _COMP[r[odd][:, ::-1]]
    return r


def reads_array_big(seed, n, L, genome_len, err=0.0, n_frac=0.25, chunk=250_000):
    """reads_array's distribution for CONFIG-size inputs (millions of reads), made chunk by chunk so that no (n, L) array of doubles
    ever exists; its own stream of random numbers (not reads_array's).  Odd reads reverse-complemented."""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len, dtype=np.uint8)]
    out = np.empty((n, L), dtype=np.uint8)
    ar = np.arange(L)
    for s in range(0, n, chunk):
        m = min(chunk, n - s)
        starts = rs.randint(0, genome_len - L, size=m)
        r = genome[starts[:, None] + ar[None, :]]
        if err > 0:
            e = rs.random_sample((m, L)) < err
            ne = int(e.sum())
            isn = rs.random_sample(ne) < n_frac
            code = np.searchsorted(acgt, r[e])
            newb = acgt[(code + rs.randint(1, 4, size=ne)) % 4]
            newb[isn] = ord("N")
            r[e] = newb
        odd = (np.arange(s, s + m) % 2) == 1
        r[odd] = _COMP[r[odd][:, ::-1]]
        out[s:s + m] = r
    return out


def lines_of(r):
    """[n, L] uint8 -> bytes, one read per line"""
    n, L = r.shape
    out = np.empty((n, L + 1), dtype=np.uint8)
    out[:, :L] = r
    out[:, L] = 10
    return out.tobytes()


def reads_text(*a, **kw):
    """-> bytes: one read per line"""
    r = reads_array(*a, **kw)
    n, L = r.shape
    out = np.empty((n, L + 1), dtype=np.uint8)
    out[:, :L] = r
    out[:, L] = 10
    return out.tobytes()


def reads_text_lowcomplexity(seed, n, L, genome_len, n_repeat=60, n_polya=12, err=0.0):
    """genome with `n_repeat` copies of one 300-bp element and `n_polya` poly-A runs of 150 bp: dictionary bins with
    hundreds to thousands of reads (the maxsearch window and the wave-cooperative bin scan of k_steps)"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len)].copy()
    rep = acgt[rs.randint(0, 4, size=300)]
    for p in rs.randint(0, genome_len - 400, size=n_repeat):
        genome[p:p + 300] = rep
    for p in rs.randint(0, genome_len - 400, size=n_polya):
        genome[p:p + 150] = ord("A")
    starts = rs.randint(0, genome_len - L, size=n)
    r = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    if err > 0:
        e = rs.random_sample((n, L)) < err
        r[e] = acgt[rs.randint(0, 4, size=int(e.sum()))]
    odd = np.arange(n) % 2 == 1
    r[odd] = _COMP[r[odd][:, ::-1]]
    out = np.empty((n, L + 1), dtype=np.uint8)
    out[:, :L] = r
    out[:, L] = 10
    return out.tobytes()


def reads_text_bigbin_stage2(seed, n_clean=3000, n_dupN=2500, L=100, genome_len=5000):
    """stage-II bins above maxsearch: n_dupN reads with N that all share their first 50 bases (copies of one genome window
    with an N and a substitution in the second half), next to n_clean ordinary reads that build the contig they realign to"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len)]
    starts = rs.randint(0, genome_len - L, size=n_clean)
    clean = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    p = genome_len // 2
    dup = np.tile(genome[p:p + L], (n_dupN, 1)).copy()
    dup[np.arange(n_dupN), rs.randint(50, L, size=n_dupN)] = ord("N")
    sub = rs.randint(50, L, size=n_dupN)
    dup[np.arange(n_dupN), sub] = np.where(dup[np.arange(n_dupN), sub] == ord("N"), ord("N"), acgt[rs.randint(0, 4, size=n_dupN)])
    allr = np.concatenate([clean, dup])
    rs.shuffle(allr)
    out = np.empty((allr.shape[0], L + 1), dtype=np.uint8)
    out[:, :L] = allr
    out[:, L] = 10
    return out.tobytes()


def reads_text_bigbin_stage2_mixed(seed, n_clean=4000, n_dupN=3000, L=100, genome_len=6000, copies=3, fail_frac=0.6, nsub=32):
    """as reads_text_bigbin_stage2, but the shared 100-base window occurs `copies` times in the genome (several probes per bin, in
    tuple order) and a random fail_frac of the N reads carry nsub substitutions in their second half: they sit in the same two bins
    but fail the Hamming test, so they stay unclaimed inside every probe's maxsearch window and push it on unevenly"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len)]
    win = genome[200:200 + L].copy()
    for k in range(1, copies):
        at = 200 + k * (genome_len - 400) // copies
        genome[at:at + L] = win
    starts = rs.randint(0, genome_len - L, size=n_clean)
    clean = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    dup = np.tile(win, (n_dupN, 1)).copy()
    bad = rs.rand(n_dupN) < fail_frac
    for i in np.nonzero(bad)[0]:
        cols = rs.choice(np.arange(50, L), size=nsub, replace=False)
        dup[i, cols] = acgt[(np.searchsorted(acgt, dup[i, cols]) + 1 + rs.randint(0, 3, size=nsub)) % 4]
    dup[np.arange(n_dupN), rs.randint(50, L, size=n_dupN)] = ord("N")
    allr = np.concatenate([clean, dup])
    rs.shuffle(allr)
    out = np.empty((allr.shape[0], L + 1), dtype=np.uint8)
    out[:, :L] = allr
    out[:, L] = 10
    return out.tobytes()


def reads_text_hugebin_stage1(seed, n_core=9000, n_norm=6000, L=100, genome_len=40000):
    """stage-I bins far above maxsearch AND above the 4096 entries k_compact_huge looks at per pass: n_core reads that share bases [15, 55) (the first
    dictionary's whole window) and are random elsewhere -- one bin of n_core reads none of which overlaps another within the Hamming threshold, thinned
    from the top as the chains take their seeds from the descending cursor -- shuffled among ordinary reads of a small genome"""
    rs = np.random.RandomState(seed)
    core = rs.randint(0, 4, 40)
    a = rs.randint(0, 4, (n_core, L))
    a[:, 15:55] = core
    g = rs.randint(0, 4, genome_len)
    st = rs.randint(0, genome_len - L, n_norm)
    b = g[st[:, None] + np.arange(L)[None, :]]
    allr = np.concatenate([a, b])
    allr = allr[rs.permutation(allr.shape[0])]
    return lines_of(np.frombuffer(b"ACGT", dtype=np.uint8)[allr])


def reads_text_hugebin_families(seed, L, n_core=10400, n_norm=6000, genome_len=60000, fam_size=4):
    """stage-I bins above maxsearch and above 4096 at ANY read length, with hits deep inside them: n_core // fam_size random templates of L bases, each
    repeated fam_size times with one substitution at a random column (mates pass the Hamming threshold of 4), then columns [L/2 - w - 3, L/2 + 5) of all of
    them -- the first dictionary's whole window, w as harc:57-58 -- overwritten with one shared string.  Mixed with n_norm reads of an i.i.d. genome, permuted,
    odd reads reverse-complemented: the core reads that stay forward share their first-dictionary k-mer, the reversed ones their second-dictionary k-mer --
    one bin of about n_core / 2 reads in each dictionary, whose scans find mates inside the maxsearch window and miss the ones beyond it"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    nfam = n_core // fam_size
    core = np.repeat(rs.randint(0, 4, (nfam, L)), fam_size, axis=0)
    m = core.shape[0]
    col = rs.randint(0, L, size=m)
    core[np.arange(m), col] = (core[np.arange(m), col] + rs.randint(1, 4, size=m)) % 4
    w = 32 if L >= 100 else 32 * L // 100                              # harc:57-58
    lo, hi = max(0, L // 2 - w - 3), L // 2 + 5
    core[:, lo:hi] = rs.randint(0, 4, hi - lo)
    g = rs.randint(0, 4, genome_len)
    st = rs.randint(0, genome_len - L, n_norm)
    norm = g[st[:, None] + np.arange(L)[None, :]]
    allr = np.concatenate([core, norm])
    r = acgt[allr[rs.permutation(allr.shape[0])]]
    odd = np.arange(r.shape[0]) % 2 == 1
    r[odd] = _COMP[r[odd][:, ::-1]]
    return lines_of(r)


def reads_array_per_start(seed, L, n_start, per=(4, 5, 6, 7, 8, 9, 10), big=(), windows=None, heavy=0.5, nheavy=8, step=9, err=0.01, n_frac=0.25, rc_share=0.3):
    """several reads per start position, for scans that must stop inside a bin: n_start starts `step` bases apart on an i.i.d. genome, the i-th with
    per[rs] reads (big[i] for the first len(big) starts).  A `heavy` share of the reads carries nheavy substitutions in columns outside the dictionary
    windows (`windows`: [(first, last), ...] in read coordinates, and outside their mirror images, so that this also holds for the reads that are
    reverse-complemented): they sit in their start's bin in both dictionaries and fail every Hamming test of a small threshold, so how far a scan
    goes into the bin decides what it finds.  Then substitutions at rate err (a share n_frac of them N), an rc_share of the reads reverse-complemented,
    all of it permuted.  -> [n, L] uint8"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=n_start * step + L)]
    cnt = rs.choice(np.asarray(per), size=n_start)
    cnt[:len(big)] = big
    starts = np.repeat(np.arange(n_start) * step, cnt)
    n = starts.shape[0]
    r = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    if windows is None:
        w = 32 if L > 100 else L * 32 // 100                          # harc:57-60
        windows = [(L // 2 - w, L // 2 - 1), (L // 2, L // 2 - 1 + w)]
    free = np.ones(L, dtype=bool)
    for a, b in windows:
        free[a:b + 1] = False
        free[L - 1 - b:L - a] = False
    free = np.nonzero(free)[0]
    k = min(nheavy, free.size)
    for i in np.nonzero(rs.random_sample(n) < heavy)[0]:
        cols = rs.choice(free, size=k, replace=False)
        r[i, cols] = acgt[(np.searchsorted(acgt, r[i, cols]) + rs.randint(1, 4, size=k)) % 4]
    if err > 0:
        e = rs.random_sample((n, L)) < err
        isN = e & (rs.random_sample((n, L)) < n_frac)
        sub = e & ~isN
        r[sub] = acgt[(np.searchsorted(acgt, r[sub]) + rs.randint(1, 4, size=int(sub.sum()))) % 4]
        r[isN] = ord("N")
    rev = rs.random_sample(n) < rc_share
    r[rev] = _COMP[r[rev][:, ::-1]]
    return r[rs.permutation(n)]


def auto_chains(n_clean, reads_per_chain=2048, clean=None):
    """auto_chains() of harc_amd/csrc/stage1.hip: K when harc_amd_params.num_chains = 0.  clean: the clean reads ([n, L] uint8 array or
    the lines of input_clean.dna) for the low-coverage rule of stage1_run_w -- more than 98 % distinct first-dictionary k-mers: up to
    4096 chains of at least 256 reads"""
    k = n_clean // reads_per_chain
    k = max(k, min(2048, n_clean // 1024))
    k = max(1, min(k, 65536))
    if clean is not None and n_clean > 0:
        if isinstance(clean, (bytes, bytearray)):
            rows = [l for l in bytes(clean).split(b"\n") if l and b"N" not in l]
            clean = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)
        L = clean.shape[1]
        ds = L // 2 - 32 if L > 100 else L // 2 - L * 32 // 100      # harc:57-58, dict1_start .. dict1_end
        de = L // 2 - 1
        nbins = np.unique(np.ascontiguousarray(clean[:, ds:de + 1]), axis=0).shape[0]
        if nbins > 0.98 * n_clean:
            k = max(k, min(4096, n_clean // 256))
    return k


def _clean_array(clean):
    if isinstance(clean, (bytes, bytearray)):
        rows = [l for l in bytes(clean).split(b"\n") if l and b"N" not in l]
        return np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(rows), -1)
    return clean


def auto_steps(clean, K):
    """steps per super-round when harc_amd_params.num_steps = 0 (stage1_run_w): 64 for one chain; 32 with more than 16 384 chains, or from 2048 chains on an input
    that is not a low-coverage one (at most 98 % distinct first-dictionary k-mers) -- in both cases only where the bins of more than 16 reads of the two
    dictionaries hold at most 2 % of N entries; 16 otherwise.  clean: the clean reads ([n, L] uint8 array or the lines of input_clean.dna)"""
    if K == 1:
        return 64
    a = _clean_array(clean)
    n, L = a.shape
    if n == 0:
        return 16
    w = 32 if L >= 100 else L * 32 // 100
    d1 = (L // 2 - w, L // 2 - 1)                                  # harc:57-60
    d2 = (L // 2, L // 2 + w - 1)
    large = 0
    nb1 = 0
    for k, (ds, de) in enumerate((d1, d2)):
        _, cnt = np.unique(np.ascontiguousarray(a[:, ds:de + 1]), axis=0, return_counts=True)
        if k == 0:
            nb1 = cnt.shape[0]
        large += int(cnt[cnt > 16].sum())
    lowcov = nb1 > 0.98 * n
    return 32 if (K > 16384 or (K >= 2048 and not lowcov)) and large * 50 <= n else 16


def edge_columns_3bit(L):
    """the columns of a read of L bases at which the 3-bit store (three bits a base, 64-bit words) has an edge: the first and the last base, bases 31 and
    32 (the word boundary of the 2-bit copies), every base whose field straddles two words (3b mod 64 > 61) and the first and last whole field of a word"""
    cols = {0, L - 1} | {b for b in (31, 32) if b < L}
    cols |= {b for b in range(L) if (3 * b) % 64 > 61}
    cols |= {b for b in range(L) if (3 * b) % 64 == 0 or (3 * b + 3) % 64 == 0}
    return sorted(cols)


def reads_text_edge_N(seed, n, L, genome_len, n_share=0.3, err=0.01):
    """reads of an i.i.d. genome with substitutions only (reads_array with n_frac = 0), of which a random n_share then get one to three N each, all of them
    at columns of edge_columns_3bit(L): every N of the input sits where a kernel that puts a 3-bit field together by hand can drop half of it"""
    r = reads_array(seed, n, L, genome_len, err=err, n_frac=0.0)
    rs = np.random.RandomState(seed + 1)
    cols = np.array(edge_columns_3bit(L))
    for i in np.nonzero(rs.random_sample(n) < n_share)[0]:
        k = min(int(rs.randint(1, 4)), cols.size)
        r[i, rs.choice(cols, size=k, replace=False)] = ord("N")
    return lines_of(r)


def reads_text_bigbin_stage2_at(seed, L, n_clean=4000, n_dupN=3000, genome_len=8000, copies=3, fail_frac=0.5):
    """reads_text_bigbin_stage2_mixed for any read length: the N reads share their first P bases -- through the end of stage II's second window
    (encoder.cpp:132-145: 42 bases above 50 bp, 41 * L / 50 + 1 below) -- and differ in the free columns [P, L) only: the one N of every read and the
    nsub = min(L - P - 1, max(16, L / 3)) substitutions of the failing share go there"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    P = 42 if L > 50 else 41 * L // 50 + 1
    nsub = min(L - P - 1, max(16, L // 3))
    genome = acgt[rs.randint(0, 4, size=genome_len)]
    win = genome[200:200 + L].copy()
    for k in range(1, copies):
        at = 200 + k * (genome_len - 400) // copies
        genome[at:at + L] = win
    starts = rs.randint(0, genome_len - L, size=n_clean)
    clean = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    dup = np.tile(win, (n_dupN, 1)).copy()
    bad = rs.rand(n_dupN) < fail_frac
    for i in np.nonzero(bad)[0]:
        cols = rs.choice(np.arange(P, L), size=nsub, replace=False)
        dup[i, cols] = acgt[(np.searchsorted(acgt, dup[i, cols]) + 1 + rs.randint(0, 3, size=nsub)) % 4]
    dup[np.arange(n_dupN), rs.randint(P, L, size=n_dupN)] = ord("N")
    allr = np.concatenate([clean, dup])
    rs.shuffle(allr)
    return lines_of(allr)


def reads_text_table_end(seed, n=3000, genome_len=30000, n_plant=12, err=0.01, L=100):
    """k-mers that live at the very END of both stage-I dictionaries.  At L = 100 both dictionary windows (bases 18-49 and 50-81) are 32 bases, a full
    64-bit key: n_plant crafted 32-mers -- each the unscrambled value of a scrambled key whose high word is 0xFFFFFFFF, the last bucket of any table,
    spelled in the 2-bit code of the packed reads (A 0, G 1, C 2, T 3, base j at bits 2j) -- are planted at well-separated loci of a random genome.
    n reads as reads_array samples them, plus error-free reads that start at locus - 18 + d and locus - 50 + d for d = -6 .. 6 (those with odd d
    reverse-complemented): each planted k-mer is a bin of both dictionaries and is probed at several shifts and in both orientations.
    -> (text, planted unscrambled keys)"""
    from tests import index_ref as ix
    assert L == 100
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len)].copy()
    h = np.uint64(0xFFFFFFFF00000000) + np.unique(rs.randint(0, 1 << 32, size=4 * n_plant, dtype=np.uint64))[:n_plant]
    keys = ix.unscramble(rs.permutation(h))
    loci = 1000 + np.arange(n_plant) * ((genome_len - 2000) // n_plant)
    agct = np.frombuffer(b"AGCT", dtype=np.uint8)
    for key, at in zip(keys, loci):
        genome[at:at + 32] = agct[((np.uint64(key) >> (np.uint64(2) * np.arange(32, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)]
    starts = rs.randint(0, genome_len - L, size=n)
    r = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    e = rs.random_sample((n, L)) < err
    isN = e & (rs.random_sample((n, L)) < 0.25)
    sub = e & ~isN
    r[sub] = acgt[(np.searchsorted(acgt, r[sub]) + rs.randint(1, 4, size=int(sub.sum()))) % 4]
    r[isN] = ord("N")
    odd = np.arange(n) % 2 == 1
    r[odd] = _COMP[r[odd][:, ::-1]]
    exact = np.array([at - w + d for at in loci for w in (18, 50) for d in range(-6, 7)])
    x = genome[exact[:, None] + np.arange(L)[None, :]].copy()
    rev = np.array([d % 2 != 0 for at in loci for w in (18, 50) for d in range(-6, 7)])      # d = 0 stays forward: the planted k-mer itself is a key
    x[rev] = _COMP[x[rev][:, ::-1]]
    allr = np.concatenate([r, x])
    return lines_of(allr[rs.permutation(allr.shape[0])]), keys


_CODE3 = np.zeros(256, dtype=np.uint64)                               # the 3-bit read store: A 0, N 1, G 2, C 4, T 6, base j at bits 3j
for _ch, _v in zip(b"ANGCT", (0, 1, 2, 4, 6)):
    _CODE3[_ch] = _v


def keys3(reads, start, nbases=21):
    """[n, L] uint8 reads -> the 3-bit-coded key of bases [start, start + nbases) of each (stage II's dictionaries: bases 0-20 and 21-41 above 50 bp)"""
    return (_CODE3[reads[:, start:start + nbases]] << (np.uint64(3) * np.arange(nbases, dtype=np.uint64))).sum(axis=1, dtype=np.uint64)


def reads_text_table_end_stage2(seed, n=3000, genome_len=30000, n_plant=12, err=0.01, L=100, max_buckets=2048):
    """k-mers that live at the very END of both STAGE-II dictionaries (built over the singletons and the reads with N, keyed by the 3-bit-coded bases 0-20
    and 21-41).  A key there is 21 three-bit codes, not any 64-bit value, so the k-mers are drawn by rejection: random 21-mers whose scrambled key has its
    high word in the top 1 / max_buckets of the range -- the last bucket of every table of at most max_buckets buckets.  n_plant 42-mers made of two such
    21-mers are planted in a random genome, the odd ones reverse-complemented; for each, three reads that BEGIN with the 42-mer (the odd ones read from the
    other strand) and carry one N behind it.  Reads with N never enter stage I: all of them are candidates of stage II, where the consensus of the n reads
    sampled around them (reads_array's way) has to find them.  -> (text, the planted 42-mers as [n_plant, 42] uint8)"""
    from tests import index_ref as ix
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rs.randint(0, 4, size=genome_len)].copy()
    found = []
    while sum(len(f) for f in found) < 2 * n_plant:
        c = acgt[rs.randint(0, 4, size=(200000, 21))]
        top = ix.scramble(keys3(c, 0)) >> np.uint64(32)
        found.append(c[top >= np.uint64((1 << 32) - (1 << 32) // max_buckets)])
    mers = np.concatenate(found)[:2 * n_plant].reshape(n_plant, 42)
    loci = 1000 + np.arange(n_plant) * ((genome_len - 2000) // n_plant)
    planted = []
    for i, (p, at) in enumerate(zip(mers, loci)):
        genome[at:at + 42] = p if i % 2 == 0 else _COMP[p[::-1]]
        for k in range(3):
            r = genome[at:at + L].copy() if i % 2 == 0 else _COMP[genome[at + 42 - L:at + 42][::-1]]
            r[42 + 7 * k + i] = ord("N")
            planted.append(r)
    starts = rs.randint(0, genome_len - L, size=n)
    r = genome[starts[:, None] + np.arange(L)[None, :]].copy()
    e = rs.random_sample((n, L)) < err
    isN = e & (rs.random_sample((n, L)) < 0.25)
    sub = e & ~isN
    r[sub] = acgt[(np.searchsorted(acgt, r[sub]) + rs.randint(1, 4, size=int(sub.sum()))) % 4]
    r[isN] = ord("N")
    odd = np.arange(n) % 2 == 1
    r[odd] = _COMP[r[odd][:, ::-1]]
    allr = np.concatenate([r, np.array(planted)])
    return lines_of(allr[rs.permutation(allr.shape[0])]), mers
