#!/usr/bin/env python3
"""Range restore (./harc -d -r FIRST:LAST): what a slice costs.  One MI355X; there is no CPU path, without a GPU it fails.

    python tools/range_rate.py [--bytes 1073741824] [--reps 20] [--out FILE]
    python tools/range_rate.py --e2e [--reads 2000000] [--rounds 3] [--other DIR] [--dir /dev/shm] [--out FILE]

Without --e2e: the line select kernels on --bytes resident bytes, asked for the line in the middle and for the last one, next to the digest kernel of ./harc -V on
the same bytes in the same process (the library's own seconds between two HIP events around the kernels, from its "[linesel] device call" and "[check] device call"
lines under HARC_AMD_TRACE=1; two calls unmeasured, then the median and the best of --reps).  Both are one streaming read of the text.

--e2e: the FASTQ of tools/check_rate.py --e2e (--reads records of 100 bases) in --dir, packed once with ./harc -c -p -q -Q -I -t 8; then, --rounds times and
alternating (the variant that runs first changes from round to round), the wall time of the whole ./harc by the host's clock for ./harc -d -p -q (full) and
./harc -d -p -q -r over the middle hundredth of the records; --other DIR: the ./harc of another build of the project (a checkout of the parent commit, built) restores the full file in the same rounds.  The slice must be
the slice of the input.  The status lines of the range unpackers say how many bytes of X.quality.hq and X.id.hi were read."""
import argparse
import json
import os
import re
import shutil
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.check_rate import timed, write_fastq                     # noqa: E402
from tools.qmap_rate import Stderr                                  # noqa: E402


def kernels(args):
    import torch
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    n = args.bytes
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    # bytes of an id file: printable, a newline about every 64 bytes
    t = torch.randint(33, 127, (n + 16,), dtype=torch.uint8, device="cuda", generator=g)
    t[torch.randint(0, n, (n // 64,), device="cuda", generator=g)] = 10
    torch.cuda.synchronize()
    res = {"tool": "range_rate", "bytes": n}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        lines = h.line_offset_device(t.data_ptr(), n, 0)[0]
        res["lines"] = lines
        for name, k in (("middle_line", lines // 2), ("last_line", lines)):
            kern, want = [], None
            for rep in range(2 + args.reps):
                with Stderr() as err:
                    got = h.line_offset_device(t.data_ptr(), n, k)
                assert want is None or got == want
                want = got
                if rep >= 2:
                    kern.append(1e-3 * float(re.search(r"kernels ([0-9.]+) ms", err.text).group(1)))
            assert want[0] == lines and int(t[want[1] - 1]) == 10
            res[name] = {"k": k, "offset": want[1], "median_ms": 1e3 * statistics.median(kern), "best_ms": 1e3 * min(kern), "GBps_median": 1e-9 * n / statistics.median(kern)}
        kern = []
        for rep in range(2 + args.reps):
            with Stderr() as err:
                h.text_digest_device(t.data_ptr(), n)
            if rep >= 2:
                kern.append(1e-3 * float(re.search(r"kernel ([0-9.]+) ms", err.text).group(1)))
        res["digest_kernel"] = {"median_ms": 1e3 * statistics.median(kern), "best_ms": 1e3 * min(kern), "GBps_median": 1e-9 * n / statistics.median(kern)}
    return res


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "range_e2e.%d" % os.getpid())
    os.makedirs(base)
    n = args.reads
    first, last = n // 2 - n // 200 + 1, n // 2 + n // 200
    res = {"tool": "range_rate", "mode": "e2e", "reads": n, "records": [first, last], "rounds": []}
    harc = os.path.join(ROOT, "harc")
    try:
        fq = os.path.join(base, "x.fastq")
        write_fastq(fq, n)
        rec = 218                                                   # bytes of a record of write_fastq: an id of 13 bytes, 100 bases, +, 100 quality values
        assert os.path.getsize(fq) == n * rec
        res["fastq_bytes"] = n * rec
        tc, _ = timed([harc, "-c", fq, "-p", "-q", "-Q", "-I", "-t", "8"], env)
        res["c_s"] = round(tc, 3)
        arc = os.path.join(base, "x.harc")
        res["sizes"] = {f: os.path.getsize(os.path.join(base, f)) for f in ("x.harc", "x.quality.hq", "x.id.hi")}
        with open(fq, "rb") as f:
            f.seek((first - 1) * rec)
            want = f.read((last - first + 1) * rec)
        variants = [("full", harc, []), ("range", harc, ["-r", "%d:%d" % (first, last)])]
        if args.other:
            variants.insert(0, ("other_full", os.path.join(os.path.abspath(args.other), "harc"), []))
        for rnd in range(args.rounds):
            row = {}
            for name, prog, extra in variants[rnd % len(variants):] + variants[:rnd % len(variants)]:      # (every variant is first in its turn)
                td, out = timed([prog, "-d", arc, "-p", "-q"] + extra, env)
                got = os.path.join(base, "x.%d-%d.d.fastq" % (first, last) if extra else "x.d.fastq")
                if extra:
                    with open(got, "rb") as f:
                        assert f.read() == want, "the slice is not the slice of the input"
                    row["unpack_lines"] = [l for l in out.splitlines() if l.startswith("[qunpack]") or l.startswith("[idunpack]")]
                else:
                    assert os.path.getsize(got) == n * rec
                row[name] = {"d_s": round(td, 3), "bytes_written": os.path.getsize(got)}
                os.remove(got)
            res["rounds"].append(row)
        for name, _, _ in variants:
            t = [r[name]["d_s"] for r in res["rounds"]]
            res[name] = {"median_s": statistics.median(t), "min_s": min(t), "max_s": max(t)}
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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("range_rate: no GPU: there is nothing to measure here")
    res = e2e(args) if args.e2e else kernels(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
