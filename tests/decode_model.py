"""A plain model of the decode chain, written from the reference line by line: decoder.cpp for -d, unpack_order.cpp + decoder_preserve.cpp + merge_N.cpp for
-d -p.  Pure Python and numpy, test infrastructure only.  `files` is the content of <basedir>/output/ as {name: bytes} (oracle_lib.read_dir / stage_dir);
nothing is written.  The model follows the reference's files and loops, not the library's kernels: it is what both decoders of the library are held to
(tests/test_gpu_decode_streams.py), and it is itself held to oracle/harc_oracle.c and to the golden fixtures (tests/test_decode_model.py)."""
import numpy as np

# decoder.cpp:290-311 (setglobalarrays): dec_noise[consensus base][code]; the row of 'N' is never reached from a 2-bit consensus
DEC_NOISE = {ord("A"): b"CGTN", ord("C"): b"AGTN", ord("G"): b"TACN", ord("T"): b"GCAN", ord("N"): b"AGCT"}
# decoder.cpp:317-321: chartorevchar
REVCHAR = bytes.maketrans(b"ACGTN", b"TGCAN")

_INT2BASE = np.frombuffer(b"ACGT", dtype=np.uint8)
_INT2REV = np.frombuffer(b"dr", dtype=np.uint8)


def _unpack_bits(packed, tail, bits, table):
    """every byte of `packed` as 8 / bits symbols, low bits first (dnabin % 4, dnabin /= 4 ... decoder.cpp:193-205; % 2 for rev, :214-233), then the
    tail file as it is (:207, :235)"""
    b = np.frombuffer(packed, dtype=np.uint8)
    per = 8 // bits
    sym = (b[:, None] >> (bits * np.arange(per, dtype=np.uint8))[None, :]) & (2 ** bits - 1)
    return table[sym.reshape(-1)].tobytes() + tail


def unpack(files, E):
    """unpackbits (decoder.cpp:174-280) -> {"seq": [E texts of ACGT], "rev": [E texts of d / r], "singleton": text of ACGT}"""
    out = {"seq": [], "rev": []}
    for e in range(E):
        out["seq"].append(_unpack_bits(files["read_seq.txt.%d" % e], files["read_seq.txt.%d.tail" % e], 2, _INT2BASE))      # :193-208
        out["rev"].append(_unpack_bits(files["read_rev.txt.%d" % e], files["read_rev.txt.%d.tail" % e], 1, _INT2REV))       # :210-236
    out["singleton"] = _unpack_bits(files["read_singleton.txt"], files["read_singleton.txt.tail"], 2, _INT2BASE)            # :249-278
    return out


def reverse_complement(s):
    """decoder.cpp:282-287"""
    return s[::-1].translate(REVCHAR)


def decode_shards(files, E, L):
    """the per-shard loop of decoder.cpp:73-139 -> [(lines without N, lines with N)] per shard, each a list of L bytes (no newline), and the singleton
    reads of :149-157"""
    u = unpack(files, E)
    shards = []
    for e in range(E):
        seq, rev = u["seq"][e], u["rev"][e]
        pos_file, noisepos = files["read_pos.txt.%d" % e], files["read_noisepos.txt.%d" % e]
        noise_lines = files["read_noise.txt.%d" % e].split(b"\n")       # std::getline, :101
        f, f_N = [], []
        ref = bytearray(L)
        sp = npp = 0
        for i, pos in enumerate(pos_file):                              # :90-92, one byte per read
            if pos != 0:                                                # :93-98
                ref[0:L - pos] = ref[pos:L]
                ref[L - pos:L] = seq[sp:sp + pos]
                sp += pos
            currentread = bytearray(ref)                                # :99
            prevnoisepos = 0
            for code in noise_lines[i]:                                 # :102-108
                noisepos_ = noisepos[npp] + prevnoisepos
                npp += 1
                currentread[noisepos_] = DEC_NOISE[ref[noisepos_]][code - ord("0")]      # :106, the row of the CONSENSUS base
                prevnoisepos = noisepos_
            c = rev[i]                                                  # :109
            dst = f_N if b"N" in currentread else f                     # :110, on the finished read, before the reverse complement
            dst.append(bytes(currentread) if c == ord("d") else reverse_complement(bytes(currentread)))      # :112-128
        shards.append((f, f_N))
    s = u["singleton"]
    singles = [s[k:k + L] for k in range(0, len(s) - L + 1, L)]         # f_singleton.read(currentread, readlen) until eof, :152-157
    return shards, singles


def _text(lines):
    return b"".join(ln + b"\n" for ln in lines)


def decode(files, E, L):
    """output.dna of decoder.cpp:141-169: every shard's clean lines, the singletons, every shard's N lines, input_N.dna"""
    shards, singles = decode_shards(files, E, L)
    return (b"".join(_text(f) for f, _ in shards) + _text(singles)      # :142-158
            + b"".join(_text(fN) for _, fN in shards)                   # :159-165
            + files.get("input_N.dna", b""))                            # :166-168


def unpack_order(files):
    """unpack_order.cpp:20-72 -> the order as uint32, packed groups then the tail file"""
    f_in = files["read_order.bin"]
    numbits = int(np.frombuffer(f_in[0:4], dtype="<i4")[0])             # :28
    numreads = int(np.frombuffer(f_in[4:8], dtype="<u4")[0])            # :29
    groups = numreads // 32
    input_array = np.frombuffer(f_in[8:8 + 4 * groups * numbits], dtype="<u4").reshape(groups, numbits)      # :35-36
    order_array = np.zeros((groups, 32), dtype=np.uint32)
    mask = np.uint32(0xFFFFFFFF >> (32 - numbits))                      # :40
    pos_in_int = pos_in_array = 0
    for k in range(32):                                                 # :41-61, every group at once
        order_array[:, k] = (input_array[:, pos_in_array] >> np.uint32(pos_in_int)) & mask
        if 32 - pos_in_int > numbits:
            pos_in_int += numbits
        elif 32 - pos_in_int == numbits:
            pos_in_array += 1
            pos_in_int = 0
        else:
            pos_in_array += 1
            order_array[:, k] += (input_array[:, pos_in_array] << np.uint32(32 - pos_in_int)) & mask      # :58
            pos_in_int = numbits - (32 - pos_in_int)
    tail = np.frombuffer(files["read_order.bin.tail"], dtype="<u4")     # :65
    return np.concatenate([order_array.reshape(-1), tail]).astype(np.uint32)


def _as_lines(text, L):
    """lines of L bytes and a newline as an [n, L + 1] array"""
    assert len(text) % (L + 1) == 0
    return np.frombuffer(text, dtype=np.uint8).reshape(-1, L + 1)


def decode_preserve(files, E, L):
    """output.dna of the -p chain (harc:183-185): unpack_order.out, decoder_preserve.out, merge_N.out"""
    order = unpack_order(files)
    shards, singles = decode_shards(files, E, L)                        # decoder_preserve.cpp:88-170 is decoder.cpp's loop; the 2-bit store of the
    #                                                                     clean reads (chartobitset :483, bitsettostring :467) gives the same letters back
    clean = _as_lines(b"".join(_text(f) for f, _ in shards) + _text(singles), L)            # :174-194, numreads of them
    withN = _as_lines(b"".join(_text(fN) for _, fN in shards) + files.get("input_N.dna", b""), L)      # :195-207
    # restore_order_N (:212-244): index_array[order] = j, then line j of the output is reads_N[index_array[j]]
    order_N_pe = np.frombuffer(files["read_order_N_pe.bin"], dtype="<u4")
    assert order_N_pe.shape[0] == withN.shape[0], "read_order_N_pe.bin holds %d entries, the archive %d lines with N" % (order_N_pe.shape[0], withN.shape[0])
    out_N = np.empty_like(withN)
    out_N[order_N_pe] = withN
    # restore_order (:246-290): the same in bins of max_bin_size reads; every read falls into exactly one bin
    assert order.shape[0] == clean.shape[0], "read_order.bin holds %d entries, the archive %d lines without N" % (order.shape[0], clean.shape[0])
    out_clean = np.empty_like(clean)
    out_clean[order] = clean
    # merge_N.cpp:37-57.  (A run of clean lines up to the next line with N is copied at once: the loop of :39-50 without its inner loop firing)
    order_N = np.frombuffer(files["read_order_N.bin"], dtype="<u4")
    nC, nN = out_clean.shape[0], order_N.shape[0]
    parts = []
    i = k = c = 0                                                       # k: entries of read_order_N.bin read so far; `next` is order_N[k] while k < nN (!eof)
    while c < nC:                                                       # :39
        while k < nN and i == int(order_N[k]):                          # :41-47
            parts.append(out_N[k:k + 1]); i += 1; k += 1
        run = int(order_N[k]) - i if k < nN and int(order_N[k]) > i else nC - c
        run = min(run, nC - c)
        parts.append(out_clean[c:c + run]); i += run; c += run          # :48-49
    while k < nN and i == int(order_N[k]):                              # :51-57
        parts.append(out_N[k:k + 1]); i += 1; k += 1
    return np.concatenate(parts).tobytes() if parts else b""
