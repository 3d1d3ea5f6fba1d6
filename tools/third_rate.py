"""What keeping the third lines costs on one MI355X (NOTES.md, "Third lines").

    python tools/third_rate.py [--bytes 1073741824] [--records 4000000] [--reps 10] [--out FILE]
        (a) the rule kernel (harc_amd_third_rule_device) on --bytes of resident FASTQ text whose third lines repeat the ids, and on the same records with bare ones;
        (b) the assembly kernel (harc_amd_fastq_assemble_third_device) under `same` and in its bare form on the same --records records, alternating, in one process
    python tools/third_rate.py --e2e [--reads 2000000] [--rounds 3] [--warm 1] [--other DIR] [--dir /dev/shm] [--out FILE]
        (c) wall time of `./harc -c X -p -q -t 8` and `./harc -d X.harc -p -q` on --reads reads of 100 bases, HARC_AMD_STAGE3=none: the input with bare third
        lines, then the one with +id third lines; with --other DIR also DIR/harc, a build of another commit, on the bare input, the builds alternating in every
        round, after --warm rounds that are run and not timed.  Every restored file is compared with its input (the other build's only on the bare input, where it promises the bytes).
One JSON line on stdout (and in --out)."""
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
from tools.pair_rate import timed                                   # noqa: E402

ID = b"@SRR1234567.00000000 00000000 length=100"                    # the two numbers are the record's, eight digits each
L = 100


def records_device(n, third):
    """n FASTQ records of one width in device memory: sra-style ids, random bases, third lines that repeat the id (`same`) or a bare '+'"""
    import torch
    w_id = len(ID)
    w3 = w_id if third == "same" else 1
    w = w_id + 1 + L + 1 + w3 + 1 + L + 1
    rec = torch.empty((n, w), dtype=torch.uint8, device="cuda")
    idx = torch.arange(n, device="cuda", dtype=torch.int64)
    ids = torch.frombuffer(bytearray(ID), dtype=torch.uint8).to("cuda").repeat(n, 1)
    for col in (12, 21):
        for k in range(8):
            ids[:, col + k] = (48 + (idx // 10 ** (7 - k)) % 10).to(torch.uint8)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")[torch.randint(0, 4, (n, L), device="cuda", generator=g)]
    at = 0
    rec[:, at:at + w_id] = ids; at += w_id
    rec[:, at] = 10; at += 1
    rec[:, at:at + L] = bases; at += L
    rec[:, at] = 10; at += 1
    if third == "same":
        rec[:, at:at + w_id] = ids
    rec[:, at] = ord("+"); at += w3
    rec[:, at] = 10; at += 1
    rec[:, at:at + L + 1] = markov_device(n, L, seed=5)              # (the lines come with their newline)
    torch.cuda.synchronize()
    return rec, ids, bases


def kernels(args):
    import torch
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    res = {"tool": "third_rate"}
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        # (a) the rule kernel over resident text
        for third in ("same", "bare"):
            n = args.bytes // (2 * len(ID) + 2 * L + 4)                # the same records under both forms
            rec, _, _ = records_device(n, third)
            nb = rec.numel()
            kern = []
            for k in range(2 + args.reps):
                with Stderr() as err:
                    got = h.third_rule_device(rec.data_ptr(), nb)
                assert got == (third, n, 2 if third == "same" else 1), got
                if k >= 2:
                    kern.append(1e-3 * float(re.search(r"rule kernel ([0-9.]+) ms", err.text).group(1)))
            res["rule_" + third] = {"records": n, "text_bytes": nb, "median_s": statistics.median(kern), "best_s": min(kern), "worst_s": max(kern),
                                    "GBps_of_text_median": 1e-9 * nb / statistics.median(kern), "reps": args.reps}
            del rec
            torch.cuda.empty_cache()
        # (b) the assembly kernel, bare and same alternating on the same records
        n = args.records
        rec, ids, bases = records_device(n, "bare")
        nl = torch.full((n, 1), 10, dtype=torch.uint8, device="cuda")
        idtext = torch.cat([ids, nl], dim=1).contiguous()
        dna = torch.cat([bases, nl], dim=1).contiguous()
        qual = rec[:, -(L + 1):].contiguous()
        del rec
        torch.cuda.synchronize()                                  # the library works on a stream of its own: its inputs must be complete
        size = {t: h.fastq_assemble_device(idtext.data_ptr(), idtext.numel(), dna.data_ptr(), qual.data_ptr(), n, L, third=t) for t in ("bare", "same")}
        out = torch.empty(size["same"] + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        kern = {"bare": [], "same": []}
        for k in range(2 + args.reps):
            for t in ("bare", "same"):
                with Stderr() as err:
                    got = h.fastq_assemble_device(idtext.data_ptr(), idtext.numel(), dna.data_ptr(), qual.data_ptr(), n, L, out.data_ptr(), size[t], third=t)
                assert got == size[t]
                if k >= 2:
                    kern[t].append(1e-3 * float(re.search(r"tile kernel ([0-9.]+) ms", err.text).group(1)))
        for t in ("bare", "same"):
            m = statistics.median(kern[t])
            res["assemble_" + t] = {"records": n, "out_bytes": size[t], "median_s": m, "best_s": min(kern[t]), "worst_s": max(kern[t]),
                                    "GBps_of_output_median": 1e-9 * size[t] / m, "reps": args.reps}
        # the text under same is the join of the lines
        k = 1000
        host = out[:k * (2 * (len(ID) + 1) + 2 * L + 2)].cpu().numpy().tobytes()
        ih, dh, qh = idtext[:k].cpu().numpy().tobytes().split(b"\n"), dna[:k].cpu().numpy().tobytes().split(b"\n"), qual[:k].cpu().numpy().tobytes().split(b"\n")
        assert host == b"".join(b"%s\n%s\n+%s\n%s\n" % (ih[i], dh[i], ih[i][1:], qh[i]) for i in range(k)), "the assembled text is not the join of the lines"
    return res


def write_fastq(path, n, third):
    import numpy as np
    from tests import gen
    reads = gen.reads_array_big(7, n, L, 10000000, err=0.01, n_frac=0.02)
    q = markov_device(n, L, seed=5).cpu().numpy()
    w_id = len(ID)
    w3 = w_id if third == "same" else 1
    w = w_id + 1 + L + 1 + w3 + 1 + L + 1
    idt = np.frombuffer(ID, dtype=np.uint8)
    with open(path, "wb") as f:
        for a in range(0, n, 200000):
            m = min(200000, n - a)
            rec = np.empty((m, w), dtype=np.uint8)
            idx = np.arange(a, a + m)
            ids = np.tile(idt, (m, 1))
            for col in (12, 21):
                for k in range(8):
                    ids[:, col + k] = 48 + (idx // 10 ** (7 - k)) % 10
            at = 0
            rec[:, at:at + w_id] = ids; at += w_id
            rec[:, at] = 10; at += 1
            rec[:, at:at + L] = reads[a:a + m]; at += L
            rec[:, at] = 10; at += 1
            if third == "same":
                rec[:, at:at + w_id] = ids
            rec[:, at] = ord("+"); at += w3
            rec[:, at] = 10; at += 1
            rec[:, at:at + L + 1] = q[a:a + m]
            f.write(rec.tobytes())


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "third_e2e.%d" % os.getpid())
    os.makedirs(base)
    res = {"tool": "third_rate", "mode": "e2e", "reads": args.reads, "warm_rounds": args.warm, "rounds": []}
    try:
        src = {}
        for third in ("bare", "same"):
            src[third] = os.path.join(base, third + ".fastq")
            write_fastq(src[third], args.reads, third)
        res["fastq_bytes"] = {t: os.path.getsize(p) for t, p in src.items()}
        builds = [("this", os.path.join(ROOT, "harc"))]
        if args.other:
            builds.append(("other", os.path.join(os.path.abspath(args.other), "harc")))
        for rnd in range(-args.warm, args.rounds):                 # rounds below 0: not timed (the first read of a freshly written file in tmpfs is slower than the later ones)
            row = {}
            order = [(b, "bare") for b in (builds if rnd % 2 == 0 else builds[::-1])] + [(builds[0], "same")]
            for (name, harc), third in order:
                d = os.path.join(base, "run")
                os.makedirs(d)
                os.link(src[third], os.path.join(d, "x.fastq"))
                tc, _ = timed([harc, "-c", os.path.join(d, "x.fastq"), "-p", "-q", "-t", "8"], env)
                sizes = {f: os.path.getsize(os.path.join(d, f)) for f in ("x.harc", "x.id", "x.quality")}
                td, _ = timed([harc, "-d", os.path.join(d, "x.harc"), "-p", "-q"], env)
                assert subprocess.call(["cmp", "-s", src[third], os.path.join(d, "x.d.fastq")]) == 0, "%s build, %s input: x.d.fastq is not the input" % (name, third)
                row["%s_%s" % (name, third)] = {"c_s": round(tc, 3), "d_s": round(td, 3), "sizes": sizes}
                shutil.rmtree(d)
            if rnd >= 0:
                res["rounds"].append(row)
        keys = sorted(res["rounds"][0])
        res["median_s"] = {k: {p: statistics.median(r[k][p] for r in res["rounds"]) for p in ("c_s", "d_s")} for k in keys}
        res["spread_s"] = {k: {p: [min(r[k][p] for r in res["rounds"]), max(r[k][p] for r in res["rounds"])] for p in ("c_s", "d_s")} for k in keys}
        if args.other:
            res["this_bare_median_inside_the_others_spread"] = {p: res["spread_s"]["other_bare"][p][0] <= res["median_s"]["this_bare"][p] <= res["spread_s"]["other_bare"][p][1]
                                                                  for p in ("c_s", "d_s")}
            res["archive_bytes_equal_on_the_bare_input"] = res["rounds"][0]["this_bare"]["sizes"] == res["rounds"][0]["other_bare"]["sizes"]
    finally:
        shutil.rmtree(base, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--records", type=int, default=4000000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reads", type=int, default=2000000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--other", default=None)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = e2e(args) if args.e2e else kernels(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
