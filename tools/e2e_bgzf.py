"""FASTQ -> stream files from a BGZF copy against the plain file, one MI355X: python tools/e2e_bgzf.py [--reads N] [--level L]

Writes N x 100 bp reads (seeded, non-constant qualities) as FASTQ into /dev/shm, a BGZF copy by up to 16 worker processes, runs compress_fastq on
both (each a fresh child process under its own time limit), compares every output file, times `gzip -cd` of the BGZF file on one core and a
16-process zlib inflate of it (text discarded), and prints one JSON line.  The kernel table: a separate `rocprofv3 --kernel-trace --stats` run of
the BGZF leg (--leg bgzf --fastq FILE --out DIR)."""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import time
import zlib
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEMBER = 65280
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _write_reads(args):
    path, first, n, seed = args
    import numpy as np
    rs = np.random.RandomState(seed)
    L = 100
    with open(path, "wb") as f:
        for a in range(0, n, 200000):
            m = min(200000, n - a)
            rec = np.empty((m, 18 + 2 * L), dtype=np.uint8)
            idx = np.arange(first + a, first + a + m)
            rec[:, 0] = ord("@")
            for k in range(12):
                rec[:, 1 + k] = 48 + (idx // 10 ** (11 - k)) % 10
            rec[:, 13] = 10
            rec[:, 14:14 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[rs.randint(0, 4, (m, L))]
            rec[:, 14 + L] = 10; rec[:, 15 + L] = ord("+"); rec[:, 16 + L] = 10
            rec[:, 17 + L:17 + 2 * L] = 35 + rs.randint(0, 38, (m, L)).astype(np.uint8)
            rec[:, 17 + 2 * L] = 10
            f.write(rec.tobytes())


def _bgzf_slice(args):
    path, lo, hi, level = args
    out = []
    with open(path, "rb") as f:
        f.seek(lo)
        data = f.read(hi - lo)
    for i in range(0, len(data), MEMBER):
        t = data[i:i + MEMBER]
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        cd = co.compress(t) + co.flush()
        hdr = b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<H", 12 + 6 + len(cd) + 8 - 1)
        out.append(hdr + cd + struct.pack("<II", zlib.crc32(t), len(t)))
    return b"".join(out)


def _inflate_slice(args):
    path, lo, hi = args
    with open(path, "rb") as f:
        f.seek(lo)
        b = f.read(hi - lo)
    at, n = 0, 0
    while at < len(b):
        bsize = struct.unpack_from("<H", b, at + 16)[0]
        n += len(zlib.decompress(b[at + 18:at + bsize + 1 - 8], -15))
        at += bsize + 1
    return n


def _members(path):
    offs, at, size = [], 0, os.path.getsize(path)
    with open(path, "rb") as f:
        while at < size:
            f.seek(at + 16)
            offs.append(at)
            at += struct.unpack("<H", f.read(2))[0] + 1
    return offs + [size]


def leg(fastq, out):
    import harc_amd
    os.makedirs(os.path.join(out, "output"), exist_ok=True)
    t0 = time.perf_counter()
    harc_amd.compress_fastq(fastq, out, 100, num_thr=8, num_chains=0)
    wall = time.perf_counter() - t0
    print(json.dumps({"wall_s": wall, "lib": harc_amd.last_fastq_timing(9)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100_000_000)
    ap.add_argument("--level", type=int, default=1)
    ap.add_argument("--dir", default="/dev/shm/e2e_bgzf")
    ap.add_argument("--leg", choices=["plain", "bgzf"])
    ap.add_argument("--fastq"); ap.add_argument("--out")
    ap.add_argument("--rocprof", help="also run the BGZF leg under rocprofv3 --kernel-trace --stats into this directory")
    a = ap.parse_args()
    if a.leg:
        return leg(a.fastq, a.out)
    os.makedirs(a.dir, exist_ok=True)
    rec = 18 + 2 * 100
    free = shutil.disk_usage(a.dir).free
    n = a.reads
    need = lambda k: k * rec * 1.6 + k * 24 * 4                   # text + BGZF copy + two sets of stream files
    if need(n) > 0.9 * free:
        n = int(0.9 * free / (rec * 1.6 + 96))
        print(f"not enough space in {a.dir} for {a.reads} reads: {n} instead", file=sys.stderr)
    plain, gz = os.path.join(a.dir, "r.fastq"), os.path.join(a.dir, "r.fastq.gz")
    W = 16
    parts = [(plain + f".{k}", k * (n // W), (n // W) + (n % W if k == W - 1 else 0), 11 + k) for k in range(W)]
    with Pool(W) as p:
        p.map(_write_reads, parts)
    with open(plain, "wb") as f:
        for q in parts:
            with open(q[0], "rb") as g:
                shutil.copyfileobj(g, f, 1 << 24)
            os.remove(q[0])
    tsz = os.path.getsize(plain)
    print(f"{n} reads written ({tsz} bytes)", file=sys.stderr, flush=True)
    step = MEMBER * max(1, tsz // MEMBER // (W * 8) + 1)
    with Pool(W) as p, open(gz, "wb") as f:
        for blob in p.imap(_bgzf_slice, [(plain, lo, min(tsz, lo + step), a.level) for lo in range(0, tsz, step)]):
            f.write(blob)
        f.write(EOF_MARKER)
    csz = os.path.getsize(gz)
    print(f"BGZF copy written ({csz} bytes)", file=sys.stderr, flush=True)
    res = {"reads": n, "text_bytes": tsz, "bgzf_bytes": csz, "level": a.level}
    for kind, path in (("plain", plain), ("bgzf", gz)):
        out = os.path.join(a.dir, kind)
        shutil.rmtree(out, ignore_errors=True)
        r = subprocess.run(["timeout", "-k", "10", "900", sys.executable, __file__, "--leg", kind, "--fastq", path, "--out", out],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode:
            print(r.stdout[-2000:], r.stderr[-2000:], file=sys.stderr)
            sys.exit(r.returncode)
        res[kind] = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"{kind} leg: {res[kind]['wall_s']:.2f} s", file=sys.stderr, flush=True)
    if a.rocprof:
        out = os.path.join(a.dir, "prof")
        shutil.rmtree(out, ignore_errors=True)
        subprocess.run(["timeout", "-k", "10", "900", "rocprofv3", "--kernel-trace", "--stats", "-d", a.rocprof, "-o", "bgzf", "--",
                        sys.executable, __file__, "--leg", "bgzf", "--fastq", gz, "--out", out], check=True, stdout=subprocess.DEVNULL)
        shutil.rmtree(out, ignore_errors=True)
    od = [os.path.join(a.dir, k, "output") for k in ("plain", "bgzf")]
    names = sorted(os.listdir(od[0]))
    res["files_equal"] = names == sorted(os.listdir(od[1])) and all(
        subprocess.run(["cmp", "-s", os.path.join(od[0], x), os.path.join(od[1], x)]).returncode == 0 for x in names)
    t0 = time.perf_counter()
    subprocess.run(f"timeout -k 10 900 gzip -cd < {gz} > /dev/null", shell=True, check=True)
    res["gzip_cd_1core_s"] = time.perf_counter() - t0
    print(f"gzip -cd: {res['gzip_cd_1core_s']:.1f} s", file=sys.stderr, flush=True)
    offs = _members(gz)
    cut = [offs[i * (len(offs) - 1) // W] for i in range(W)] + [offs[-1]]
    t0 = time.perf_counter()
    with Pool(W) as p:
        got = sum(p.map(_inflate_slice, [(gz, cut[i], cut[i + 1]) for i in range(W)]))
    res["zlib_16proc_inflate_s"] = time.perf_counter() - t0
    assert got == tsz
    for kind in ("plain", "bgzf"):
        shutil.rmtree(os.path.join(a.dir, kind), ignore_errors=True)
    os.remove(plain); os.remove(gz)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
