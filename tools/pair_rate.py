"""What paired-end input costs on one MI355X (NOTES.md, "Paired-end input").

    python tools/pair_rate.py [--bytes 1073741824] [--reps 10] [--out FILE]
        the rule kernel (harc_amd_idmate_rule_device) and the patch kernel on two resident id texts of --bytes each, Illumina-style lines
    python tools/pair_rate.py --e2e [--reads 1000000] [--rounds 3] [--other DIR] [--dir /dev/shm] [--out FILE]
        wall time of `./harc -c A -2 B -p -q` against `cat A B > C && ./harc -c C -p -q` (the cat included; with --other DIR: DIR/harc, a build of
        another commit), 2 x --reads reads of 100 bases, HARC_AMD_STAGE3=none, the variants alternating; the two archives must hold the same streams
One JSON line on stdout (and in --out)."""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tarfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.qmap_rate import Stderr                                  # noqa: E402
from tools.qpack_rate import markov_device                          # noqa: E402

TEMPLATE = b"@HWI-ST1234:100:C0ABCACXX:3:0000:00000:000000 1:N:0:ATCACG\n"


def id_texts_device(nbytes):
    """two id texts of about nbytes each in device memory: file 1's ids and their mates by the space rule"""
    import torch
    w = len(TEMPLATE)
    m = nbytes // w
    a = torch.frombuffer(bytearray(TEMPLATE), dtype=torch.uint8).to("cuda").repeat(m, 1)
    idx = torch.arange(m, device="cuda", dtype=torch.int64)
    for col, div, digits in ((28, 6000000, 4), (33, 60, 5), (39, 1, 6)):              # tile, x, y: digits that change from line to line
        v = (idx // div) * (7 if digits == 6 else 1)
        for k in range(digits):
            a[:, col + k] = (48 + (v // 10 ** (digits - 1 - k)) % 10).to(torch.uint8)
    b = a.clone()
    b[:, TEMPLATE.index(b" 1:") + 1] = ord("2")
    torch.cuda.synchronize()
    return a, b, m


def kernels(args):
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    a, b, m = id_texts_device(args.bytes)
    n = a.numel()
    res = {"tool": "pair_rate", "bytes_each": n, "pairs": m}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        kern, wall = [], []
        for k in range(2 + args.reps):
            with Stderr() as err:
                t0 = time.perf_counter()
                got = h.idmate_rule_device(a.data_ptr(), n, b.data_ptr(), n)
                dt = time.perf_counter() - t0
            assert got == ("space", m, 4), got
            if k >= 2:
                kern.append(1e-3 * float(re.search(r"rule kernel ([0-9.]+) ms", err.text).group(1))); wall.append(dt)
        res["rule_kernel"] = {"median_s": statistics.median(kern), "best_s": min(kern), "GBps_of_both_texts_median": 1e-9 * 2 * n / statistics.median(kern),
                              "call_median_s": statistics.median(wall), "reps": args.reps}
        # the patch kernel with its line index, on a copy each time: file 2's ids from file 1's
        calls = []
        for k in range(3):
            c = a.clone()
            import torch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            bad = h.idmate_apply_device(c.data_ptr(), n, "space")
            calls.append(time.perf_counter() - t0)
            assert bad == 0 and bool((c == b).all())
        res["apply_call_s"] = [round(x, 4) for x in calls]
    return res


def write_pair(base, n, L=100):
    import numpy as np
    from tests import gen
    reads = gen.reads_array_big(7, 2 * n, L, 10000000, err=0.01, n_frac=0.02)
    q = markov_device(2 * n, L, seed=5).cpu().numpy()
    tail = b" 1:N:0:ATCACG"
    w = 13 + len(tail) + 1
    for side in range(2):
        with open(os.path.join(base, "s_%d.fastq" % (side + 1)), "wb") as f:
            for a in range(0, n, 200000):
                m = min(200000, n - a)
                rec = np.empty((m, w + 2 * L + 4), dtype=np.uint8)
                idx = np.arange(a, a + m)
                rec[:, 0] = ord("@")
                for k in range(12):
                    rec[:, 1 + k] = 48 + (idx // 10 ** (11 - k)) % 10
                rec[:, 13:13 + len(tail)] = np.frombuffer(tail, dtype=np.uint8)
                rec[:, 14] = ord("1") + side
                rec[:, w - 1] = 10
                rec[:, w:w + L] = reads[side * n + a:side * n + a + m]
                rec[:, w + L] = 10; rec[:, w + L + 1] = ord("+"); rec[:, w + L + 2] = 10
                rec[:, w + L + 3:w + 2 * L + 4] = q[side * n + a:side * n + a + m]          # (the lines come with their newline)
                f.write(rec.tobytes())


def timed(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s" % (" ".join(cmd), r.returncode, r.stdout[-3000:]))
    return dt, r.stdout


def members(arc):
    """{name: bytes} of an archive; a stream tar inside it as the files it holds (its headers carry the time of the run)"""
    import io
    out = {}
    with tarfile.open(arc) as t:
        for m in t.getmembers():
            if not m.isfile():
                continue
            data = t.extractfile(m).read()
            if m.name.endswith(".tar"):
                with tarfile.open(fileobj=io.BytesIO(data)) as inner:
                    for x in inner.getmembers():
                        if x.isfile():
                            out[m.name + ":" + x.name] = inner.extractfile(x).read()
            else:
                out[m.name] = data
    return out


def e2e(args):
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "pair_e2e.%d" % os.getpid())
    os.makedirs(base)
    res = {"tool": "pair_rate", "mode": "e2e", "reads_per_file": args.reads, "rounds": []}
    try:
        write_pair(base, args.reads)
        f1, f2 = os.path.join(base, "s_1.fastq"), os.path.join(base, "s_2.fastq")
        res["fastq_bytes_each"] = os.path.getsize(f1)
        cat_harc = os.path.join(os.path.abspath(args.other), "harc") if args.other else os.path.join(ROOT, "harc")
        for rnd in range(args.rounds):
            row = {}
            for name in ("cat", "pair"):
                d = os.path.join(base, name)
                os.makedirs(d)
                if name == "cat":
                    t0 = time.perf_counter()
                    with open(os.path.join(d, "s_1.fastq"), "wb") as o:
                        subprocess.check_call(["cat", f1, f2], stdout=o)
                    t_cat = time.perf_counter() - t0
                    tc, _ = timed([cat_harc, "-c", os.path.join(d, "s_1.fastq"), "-p", "-q", "-t", "8"], env)
                    row[name] = {"cat_s": round(t_cat, 3), "c_s": round(tc, 3), "total_s": round(t_cat + tc, 3)}
                else:
                    os.link(f1, os.path.join(d, "s_1.fastq")); os.link(f2, os.path.join(d, "s_2.fastq"))
                    tc, _ = timed([os.path.join(ROOT, "harc"), "-c", os.path.join(d, "s_1.fastq"), "-2", os.path.join(d, "s_2.fastq"), "-p", "-q", "-t", "8"], env)
                    row[name] = {"total_s": round(tc, 3)}
                if rnd == 0:
                    row[name]["sizes"] = {f: os.path.getsize(os.path.join(d, f)) for f in ("s_1.harc", "s_1.id", "s_1.quality")}
                    res.setdefault("members", {})[name] = members(os.path.join(d, "s_1.harc"))
                    if name == "pair":                                # ... and back: both files byte for byte
                        td, _ = timed([os.path.join(ROOT, "harc"), "-d", os.path.join(d, "s_1.harc"), "-p", "-q"], env)
                        for k, src in ((1, f1), (2, f2)):
                            assert subprocess.call(["cmp", "-s", src, os.path.join(d, "s_1.d.%d.fastq" % k)]) == 0, "s_1.d.%d.fastq is not the input" % k
                        row[name]["d_s"] = round(td, 3)
                shutil.rmtree(d)
            res["rounds"].append(row)
        got = res.pop("members")
        pair_record = got["pair"].pop("./read.pair")
        differ = sorted(k for k in set(got["pair"]) | set(got["cat"]) if got["pair"].get(k) != got["cat"].get(k))
        assert not differ, "the pair archive is not the archive of the cat plus read.pair: %s" % differ
        res["members_equal"] = len(got["cat"])
        res["read_pair"] = pair_record.decode().split("\n")[:-1]
        res["median_total_s"] = {k: statistics.median(r[k]["total_s"] for r in res["rounds"]) for k in ("cat", "pair")}
    finally:
        shutil.rmtree(base, ignore_errors=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--rounds", type=int, default=3)
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
