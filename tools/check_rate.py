#!/usr/bin/env python3
"""Checked archives (./harc -c -V): what the digest costs.  One MI355X; there is no CPU path, without a GPU it fails.

    python tools/check_rate.py [--bytes 1073741824] [--reps 20] [--dir /dev/shm] [--out FILE]
    python tools/check_rate.py --e2e [--reads 2000000] [--rounds 2] [--other DIR] [--dir /dev/shm] [--out FILE]

Without --e2e: the digest kernel alone on --bytes resident bytes (the library's own seconds between two HIP events around the kernel, from its "[check] device call"
line under HARC_AMD_TRACE=1, and the host's clock around the whole call, which ends in a synchronise; two calls unmeasured, then the median and the best of --reps),
then harc_amd_text_digest_files on a file of the same bytes in --dir (one call unmeasured, then three; the "[check]" line of each gives the seconds in the kernels
and waiting for the readers).  Both must give the same triple.

--e2e: a FASTQ of --reads records of 100 bases (the reads of NOTES.md's other end-to-end lines, ids of 13 bytes, quality lines of tools/qpack_rate.py) in --dir;
./harc -c -p -q -Q -I -t 8 without and with -V and ./harc -d -p -q of both archives, wall time of the whole ./harc by the host's clock, --rounds times, the variants
alternating; --other DIR: the ./harc of another build of the project (a checkout of the parent commit, built) runs the same without -V in the same rounds."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.qmap_rate import Stderr                                  # noqa: E402
from tools.qpack_rate import markov_device                          # noqa: E402


def kernel_and_file(args):
    import torch
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    n = args.bytes
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    t = torch.randint(0, 256, (n + 16,), dtype=torch.uint8, device="cuda", generator=g)
    torch.cuda.synchronize()
    res = {"tool": "check_rate", "bytes": n}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        wall, kern, want = [], [], None
        for k in range(2 + args.reps):
            with Stderr() as err:
                t0 = time.perf_counter()
                got = h.text_digest_device(t.data_ptr(), n)
                dt = time.perf_counter() - t0
            assert want is None or got == want
            want = got
            m = re.search(r"kernel ([0-9.]+) ms", err.text)
            if k >= 2:
                wall.append(dt); kern.append(1e-3 * float(m.group(1)))
        res["kernel"] = {"median_s": statistics.median(kern), "best_s": min(kern), "GBps_median": 1e-9 * n / statistics.median(kern),
                         "call_median_s": statistics.median(wall), "call_GBps_median": 1e-9 * n / statistics.median(wall), "reps": args.reps}
    path = os.path.join(args.dir, "check_rate.%d.bin" % os.getpid())
    try:
        with open(path, "wb") as f:
            for a in range(0, n, 1 << 28):
                f.write(t[a:min(n, a + (1 << 28))].cpu().numpy().tobytes())
        runs = []
        for k in range(4):
            with Stderr() as err:
                t0 = time.perf_counter()
                got = harc_amd.text_digest_file(path)
                dt = time.perf_counter() - t0
            assert got == want, (got, want)
            m = re.search(r"\[check\] \d+ bytes of text in (\d+) pieces, ([0-9.]+) s: ([0-9.]+) s in the kernels, ([0-9.]+) s waiting for the readers", err.text)
            if k >= 1:
                runs.append({"call_s": dt, "pieces": int(m.group(1)), "feed_and_kernels_s": float(m.group(2)), "kernels_s": float(m.group(3)), "waiting_for_readers_s": float(m.group(4))})
        res["file"] = {"runs": runs, "feed_GBps_median": 1e-9 * n / statistics.median(r["feed_and_kernels_s"] for r in runs),
                       "kernels_GBps_median": 1e-9 * n / statistics.median(r["kernels_s"] for r in runs)}
    finally:
        if os.path.exists(path):
            os.remove(path)
    res["digest"] = ["%016x" % v for v in want]
    return res


def write_fastq(path, n, L=100):
    import numpy as np
    from tests import gen
    reads = gen.reads_array_big(7, n, L, 10000000, err=0.01, n_frac=0.02)
    q = markov_device(n, L, seed=5).cpu().numpy()
    with open(path, "wb") as f:
        for a in range(0, n, 200000):
            m = min(200000, n - a)
            rec = np.empty((m, 18 + 2 * L), dtype=np.uint8)
            idx = np.arange(a, a + m)
            rec[:, 0] = ord("@")
            for k in range(12):
                rec[:, 1 + k] = 48 + (idx // 10 ** (11 - k)) % 10
            rec[:, 13] = 10
            rec[:, 14:14 + L] = reads[a:a + m]
            rec[:, 14 + L] = 10; rec[:, 15 + L] = ord("+"); rec[:, 16 + L] = 10
            rec[:, 17 + L:18 + 2 * L] = q[a:a + m]
            f.write(rec.tobytes())


def timed(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stdout[-3000:]))
    return dt, r.stdout


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "check_e2e.%d" % os.getpid())
    os.makedirs(base)
    res = {"tool": "check_rate", "mode": "e2e", "reads": args.reads, "rounds": []}
    try:
        fq = os.path.join(base, "in.fastq")
        write_fastq(fq, args.reads)
        res["fastq_bytes"] = os.path.getsize(fq)
        variants = [("plain", os.path.join(ROOT, "harc"), []), ("checked", os.path.join(ROOT, "harc"), ["-V"])]
        if args.other:
            variants.insert(0, ("other", os.path.join(os.path.abspath(args.other), "harc"), []))
        sizes = {}
        for rnd in range(args.rounds):
            row = {}
            for name, harc, extra in variants:
                d = os.path.join(base, name)
                os.makedirs(d)
                os.link(fq, os.path.join(d, "x.fastq"))
                tc, _ = timed([harc, "-c", os.path.join(d, "x.fastq"), "-p", "-q", "-Q", "-I", "-t", "8"] + extra, env)
                td, out = timed([harc, "-d", os.path.join(d, "x.harc"), "-p", "-q"], env)
                with open(os.path.join(d, "x.d.fastq"), "rb") as a, open(fq, "rb") as b:
                    same = all(x == y for x, y in zip(iter(lambda: a.read(1 << 24), b""), iter(lambda: b.read(1 << 24), b""))) and os.path.getsize(fq) == os.path.getsize(os.path.join(d, "x.d.fastq"))
                assert same, name + ": x.d.fastq is not the input"
                row[name] = {"c_s": round(tc, 3), "d_s": round(td, 3), "check_line": [l for l in out.splitlines() if l.startswith("[check]")]}
                sizes[name] = {f: os.path.getsize(os.path.join(d, f)) for f in ("x.harc", "x.quality.hq", "x.id.hi")}
                shutil.rmtree(d)
            res["rounds"].append(row)
        res["sizes"] = sizes
    finally:
        shutil.rmtree(base, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("check_rate: no GPU: there is nothing to measure here")
    res = e2e(args) if args.e2e else kernel_and_file(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
