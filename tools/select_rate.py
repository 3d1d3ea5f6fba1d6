#!/usr/bin/env python3
"""Selection by name (./harc -d -q -L NAMES): what the probe, the gather and a whole selection cost.  One MI355X; there is no CPU path, without a GPU it fails.

    python tools/select_rate.py [--bytes 1073741824] [--reps 15] [--out FILE]
    python tools/select_rate.py --e2e [--reads 2000000] [--rounds 3] [--other DIR] [--dir /dev/shm] [--out FILE]

Without --e2e: the probe kernel on --bytes resident bytes of id lines in the Illumina style ("@SRR870667.<i> HWI-ST1234:100:C0ABCACXX:3:1101:<x>:<y> length=100",
one width), with a list of 1 000 and a list of 1 000 000 of their names; next to it, on the same bytes in the same process, the two streaming kernels the project
already times on id text: the digest kernel of ./harc -V and the line select's count.  All are the library's own seconds between two HIP events around the
kernels, from its "[select] device call", "[check] device call" and "[linesel] device call" lines under HARC_AMD_TRACE=1; two calls unmeasured, then the median and
the best of --reps.  Then the stride gather on --bytes of quality text (lines of 101 bytes) with 1 % and 50 % of the lines flagged, against a device-to-device copy
of as many bytes as the gather writes (torch, device events).

--e2e: the FASTQ of tools/check_rate.py --e2e (--reads records of 100 bases) in --dir, packed once with ./harc -c -p -q -t 8; then, --rounds times and alternating
(the variant that runs first changes from round to round), the wall time of the whole ./harc by the host's clock for ./harc -d -p -q (full) and ./harc -d -p -q -L
with a list of a hundredth of the names; --other DIR: the ./harc of another build of the project (a checkout of the parent commit, built) restores the full file
in the same rounds.  The selection must be the filter of the input.  The bytes written next to the archive are reported for each."""
import argparse
import json
import os
import re
import shutil
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.check_rate import timed, write_fastq                     # noqa: E402
from tools.qmap_rate import Stderr                                  # noqa: E402

HEAD, TAIL = b"@SRR870667.", b" HWI-ST1234:100:C0ABCACXX:3:1101:12345:123456 length=100\n"


def id_text(n_lines):
    """n_lines id lines of one width in device memory, line i named SRR870667.<i as 8 digits>"""
    import torch
    row = torch.frombuffer(bytearray(HEAD + b"00000000" + TAIL), dtype=torch.uint8).to("cuda")
    t = row.repeat(n_lines, 1)
    idx = torch.arange(n_lines, device="cuda", dtype=torch.int64)
    for k in range(8):
        t[:, len(HEAD) + k] = (48 + (idx // 10 ** (7 - k)) % 10).to(torch.uint8)
    return t.reshape(-1)


def stats(kern, nbytes):
    med = statistics.median(kern)
    return {"median_ms": 1e3 * med, "best_ms": 1e3 * min(kern), "GBps_median": 1e-9 * nbytes / med, "ms_per_GiB_median": 1e3 * med * (1 << 30) / nbytes}


def kernels(args):
    import torch
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    width = len(HEAD) + 8 + len(TAIL)
    n_lines = args.bytes // width
    n = n_lines * width
    t = id_text(n_lines)
    flags = torch.zeros(n_lines + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "select_rate", "bytes": n, "lines": n_lines, "line_bytes": width}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        for k in (1000, 1000000):
            k = min(k, n_lines)
            step = n_lines // k
            names = b"".join(b"SRR870667.%08d\n" % (i * step) for i in range(k))
            tn = torch.frombuffer(bytearray(names), dtype=torch.uint8).to("cuda")
            torch.cuda.synchronize()
            kern = []
            for rep in range(2 + args.reps):
                with Stderr() as err:
                    got = h.select_flags_device(tn.data_ptr(), len(names), t.data_ptr(), n, flags.data_ptr())
                assert got == (n_lines, k, k), got
                if rep >= 2:
                    kern.append(1e-3 * float(re.search(r"probe kernel ([0-9.]+) ms", err.text).group(1)))
            assert int(flags[:n_lines].sum()) == k and int(flags[:n_lines:step][:k].sum()) == k
            res["probe_%d_names" % k] = stats(kern, n)
        kern = []
        for rep in range(2 + args.reps):
            with Stderr() as err:
                h.text_digest_device(t.data_ptr(), n)
            if rep >= 2:
                kern.append(1e-3 * float(re.search(r"kernel ([0-9.]+) ms", err.text).group(1)))
        res["digest_kernel"] = stats(kern, n)
        kern = []
        for rep in range(2 + args.reps):
            with Stderr() as err:
                assert h.line_offset_device(t.data_ptr(), n, n_lines) == (n_lines, n)
            if rep >= 2:
                kern.append(1e-3 * float(re.search(r"kernels ([0-9.]+) ms", err.text).group(1)))
        res["line_select_kernels"] = stats(kern, n)
        del t
        # the stride gather: quality text of 101 bytes a line
        S = 101
        q_lines = args.bytes // S
        qn = q_lines * S
        g = torch.Generator(device="cuda"); g.manual_seed(5)
        q = torch.randint(33, 74, (qn,), dtype=torch.uint8, device="cuda", generator=g)
        q[S - 1::S] = 10
        for pct in (1, 50):
            f = (torch.rand(q_lines, device="cuda", generator=g) < pct / 100).to(torch.uint8)
            m = int(f.sum())
            out = torch.empty(m * S + 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            kern = []
            for rep in range(2 + args.reps):
                with Stderr() as err:
                    assert h.lines_gather_device(q.data_ptr(), qn, S, f.data_ptr(), q_lines, out.data_ptr(), m * S) == m * S
                if rep >= 2:
                    kern.append(1e-3 * float(re.search(r"stride gather kernel ([0-9.]+) ms", err.text).group(1)))
            sel = torch.nonzero(f)[:, 0]
            assert torch.equal(out[:m * S].reshape(m, S)[::max(1, m // 1000)], q.reshape(q_lines, S)[sel[::max(1, m // 1000)]])
            copy = []
            for rep in range(2 + args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); out[:m * S].copy_(q[:m * S]); e1.record(); torch.cuda.synchronize()
                if rep >= 2:
                    copy.append(1e-3 * e0.elapsed_time(e1))
            res["gather_%d_pct" % pct] = dict(stats(kern, m * S), lines=m, bytes_out=m * S, d2d_copy=stats(copy, m * S))
    return res


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "select_e2e.%d" % os.getpid())
    os.makedirs(base)
    n = args.reads
    res = {"tool": "select_rate", "mode": "e2e", "reads": n, "rounds": []}
    harc = os.path.join(ROOT, "harc")
    try:
        fq = os.path.join(base, "x.fastq")
        write_fastq(fq, n)
        rec = 218                                                   # bytes of a record of write_fastq: an id of 13 bytes, 100 bases, +, 100 quality values
        assert os.path.getsize(fq) == n * rec
        res["fastq_bytes"] = n * rec
        picked = list(range(37, n, 100))                            # a hundredth of the records
        with open(os.path.join(base, "names.txt"), "wb") as f:
            f.write(b"".join(b"%012d\n" % i for i in reversed(picked)))
        res["names"] = len(picked)
        want = bytearray()
        with open(fq, "rb") as f:
            for i in picked:
                f.seek(i * rec)
                want += f.read(rec)
        tc, _ = timed([harc, "-c", fq, "-p", "-q", "-t", "8"], env)
        res["c_s"] = round(tc, 3)
        arc = os.path.join(base, "x.harc")
        variants = [("full", harc, []), ("select", harc, ["-L", os.path.join(base, "names.txt")])]
        if args.other:
            variants.insert(0, ("other_full", os.path.join(os.path.abspath(args.other), "harc"), []))
        for rnd in range(args.rounds):
            row = {}
            for name, prog, extra in variants[rnd % len(variants):] + variants[:rnd % len(variants)]:      # (every variant is first in its turn)
                td, out = timed([prog, "-d", arc, "-p", "-q"] + extra, env)
                got = os.path.join(base, "x.sel.d.fastq" if extra else "x.d.fastq")
                if extra:
                    with open(got, "rb") as f:
                        assert f.read() == want, "the selection is not the filter of the input"
                    row["select_line"] = [l for l in out.splitlines() if l.startswith("[select]")]
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
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--other", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("select_rate: no GPU: there is nothing to measure here")
    res = e2e(args) if args.e2e else kernels(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
