#!/usr/bin/env python3
"""The recovery record (./harc -c -P, -R): what it costs.  One MI355X; there is no CPU path, without a GPU it fails.

    python tools/recovery_rate.py [--block 4194304] [--reps 10] [--out FILE]
    python tools/recovery_rate.py --e2e [--reads 2000000] [--rounds 3] [--dir /dev/shm] [--out FILE]

Without --e2e: k_gf_combine alone on k = 128 resident source blocks of --block random bytes, m = 7 outputs (PCT 5: one pass over the sources) and m = 26 (PCT 20:
four passes), the Cauchy coefficients of the record; the library's own seconds between two HIP events around the kernel, from its "[recovery] device call" line under
HARC_AMD_TRACE=1; two calls unmeasured, then the median and the best of --reps, in GB/s of source bytes.  (A block of 4 MiB gives the one job of this call the 1024
workgroups that the 64 groups of a span of 64-KiB blocks give one launch of the file call.)  Then the block digest kernel on the same bytes, by the host's clock
around the call.

--e2e: the FASTQ of tools/check_rate.py --e2e in --dir; ./harc -c -p -q -Q -I -t 8 without and with -P 5 under HARC_AMD_STAGE3=none, wall time of the whole ./harc
by the host's clock, --rounds times, the variants alternating; then ./harc -R -n on the files of the last round, and the sizes."""
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


def kernel(args):
    import torch
    import harc_amd
    from tests import recovery_cases as rc
    os.environ["HARC_AMD_TRACE"] = "1"
    B, k = args.block, 128
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    src = torch.randint(0, 256, (k * B,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.zeros((26 * B,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "recovery_rate", "block_bytes": B, "sources": k, "source_bytes": k * B, "estimate_GBps_m8_from_instruction_counts": 2000}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        for m in (7, 26):
            coef = [[rc.cauchy(i, j) for j in range(k)] for i in range(m)]
            kern = []
            for rep in range(2 + args.reps):
                with Stderr() as err:
                    h.gf_combine_device(B, [src.data_ptr() + s * B for s in range(k)], [out.data_ptr() + q * B for q in range(m)], coef)
                mt = re.search(r"kernel ([0-9.]+) ms", err.text)
                if rep >= 2:
                    kern.append(1e-3 * float(mt.group(1)))
            # the first 64 bytes of every output against the plain Python reference
            got = out.view(26, B)[:m, :64].cpu().numpy()
            members = [bytes(src[s * B:s * B + 64].cpu().numpy().tobytes()) for s in range(k)]
            assert [bytes(r.tobytes()) for r in got] == rc.combine(members, coef)
            res["m%d" % m] = {"median_s": statistics.median(kern), "best_s": min(kern), "GBps_of_source_bytes_median": 1e-9 * k * B / statistics.median(kern),
                              "passes": (m + 7) // 8, "reps": args.reps}
        wall = []
        for rep in range(2 + args.reps):
            t0 = time.perf_counter()
            h.block_digests_device(src.data_ptr(), k, B)
            if rep >= 2:
                wall.append(time.perf_counter() - t0)
        res["digests"] = {"call_median_s": statistics.median(wall), "call_GBps_median": 1e-9 * k * B / statistics.median(wall)}
    return res


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "recovery_e2e.%d" % os.getpid())
    os.makedirs(base)
    harc = os.path.join(ROOT, "harc")
    res = {"tool": "recovery_rate", "mode": "e2e", "reads": args.reads, "rounds": []}
    try:
        fq = os.path.join(base, "in.fastq")
        write_fastq(fq, args.reads)
        res["fastq_bytes"] = os.path.getsize(fq)
        for rnd in range(args.rounds):
            row = {}
            for name, extra in (("plain", []), ("recovery", ["-P", "5"])):
                d = os.path.join(base, name)
                os.makedirs(d)
                os.link(fq, os.path.join(d, "x.fastq"))
                tc, out = timed([harc, "-c", os.path.join(d, "x.fastq"), "-p", "-q", "-Q", "-I", "-t", "8"] + extra, env)
                row[name] = {"c_s": round(tc, 3)}
                if extra:
                    row[name]["line"] = [l for l in out.splitlines() if l.startswith("[recovery]")]
                    tr, out = timed([harc, "-R", os.path.join(d, "x.harc"), "-n"], env)
                    row[name]["R_n_s"] = round(tr, 3)
                    res["sizes"] = {f: os.path.getsize(os.path.join(d, f)) for f in ("x.harc", "x.quality.hq", "x.id.hi", "x.hr")}
                shutil.rmtree(d)
            res["rounds"].append(row)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--block", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("recovery_rate: no GPU: there is nothing to measure here")
    res = e2e(args) if args.e2e else kernel(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
