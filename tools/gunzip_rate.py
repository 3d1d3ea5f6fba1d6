#!/usr/bin/env python3
"""Plain gzip input: the host's gzip against harc_amd_stage gunzip, and ./harc -c on the .gz with and without the GPU inflate (NOTES.md, "Plain gzip input").

    python tools/gunzip_rate.py [--reads 2000000] [--rounds 3] [--dir /dev/shm] [--profile] [--chunks 32768,65536] [--no-e2e] [--out FILE]

The workload is tools/check_rate.py's --e2e FASTQ (--reads records of 100 bases, ids of 13 bytes), written with gzip -6 into --dir.  Every round runs, in this
order, (i) gzip -cd < x.fastq.gz > file, (ii) harc_amd_stage gunzip, and unless --no-e2e (iv) ./harc -c x.fastq.gz -p -q with HARC_AMD_GUNZIP=0 and with
HARC_AMD_GUNZIP=1: the variants alternate, so that drift of the machine lands on all of them.  The text of (ii) is compared with (i)'s once.  One more run of (ii) with
HARC_AMD_TRACE=1 gives the laps of the stages, and --profile one under rocprofv3 --kernel-trace --stats, a run of its own, for (iii) the kernel times.
One JSON line on stdout."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
STAGE = os.path.join(ROOT, "harc_amd", "harc_amd_stage")


def timed(cmd, env, **kw):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, **kw)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise SystemExit("%s failed (%d):\n%s\n%s" % (cmd, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
    return dt, r.stdout, r.stderr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--chunks", type=lambda s: [int(x) for x in s.split(",") if x], default=[], help="more chunk sizes to time (ii) with, e.g. 32768,65536")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    import check_rate
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    for k in ("HARC_AMD_TRACE", "HARC_AMD_GUNZIP", "HARC_AMD_GUNZIP_CHUNK", "HARC_AMD_GUNZIP_PIECE"):
        env.pop(k, None)
    base = os.path.join(args.dir, "gunzip_rate.%d" % os.getpid())
    os.makedirs(base)
    res = {"tool": "gunzip_rate", "reads": args.reads, "rounds": []}
    try:
        fq, gz = os.path.join(base, "x.fastq"), os.path.join(base, "x.fastq.gz")
        check_rate.write_fastq(fq, args.reads)
        with open(fq, "rb") as i, open(gz, "wb") as o:
            subprocess.check_call(["gzip", "-6", "-c"], stdin=i, stdout=o)
        res["text_bytes"], res["gz_bytes"] = os.path.getsize(fq), os.path.getsize(gz)
        os.remove(fq)
        host_out, gpu_out = os.path.join(base, "host.fastq"), os.path.join(base, "gpu.fastq")
        for rnd in range(args.rounds):
            row = {}
            with open(gz, "rb") as i, open(host_out, "wb") as o:
                row["host_gzip_s"] = round(_gzip(i, o), 3)
            dt, out, _ = timed([STAGE, "gunzip", gz, "0", gpu_out], env)
            row["stage_gunzip_s"] = round(dt, 3)
            row["line"] = out.strip()
            if rnd == 0:
                subprocess.check_call(["cmp", host_out, gpu_out])
            for cb in args.chunks:                                  # the same call with other chunk sizes (the default is 256 KiB)
                dt, out, _ = timed([STAGE, "gunzip", gz, "0", gpu_out], dict(env, HARC_AMD_GUNZIP_CHUNK=str(cb)))
                row["stage_gunzip_chunk%d_s" % cb] = round(dt, 3)
                row["line_chunk%d" % cb] = out.strip()
            os.remove(gpu_out); os.remove(host_out)
            if not args.no_e2e:
                for name, extra in (("harc_c_host_s", {"HARC_AMD_GUNZIP": "0"}), ("harc_c_gpu_s", {"HARC_AMD_GUNZIP": "1"})):
                    d = os.path.join(base, name)
                    os.makedirs(d)
                    os.link(gz, os.path.join(d, "x.fastq.gz"))
                    dt, out, _ = timed([os.path.join(ROOT, "harc"), "-c", os.path.join(d, "x.fastq.gz"), "-p", "-q", "-t", "8"], dict(env, **extra))
                    assert ("[gunzip]" in out) == (extra["HARC_AMD_GUNZIP"] == "1"), out[-2000:]
                    row[name] = round(dt, 3)
                    shutil.rmtree(d)
            res["rounds"].append(row)
        for k in [k for k in res["rounds"][0] if k.endswith("_s")]:
            v = sorted(r[k] for r in res["rounds"])
            res[k + "_median"] = v[len(v) // 2]; res[k + "_spread"] = round(v[-1] - v[0], 3)
        res["text_MBps_host"] = round(1e-6 * res["text_bytes"] / res["host_gzip_s_median"], 1)
        res["text_MBps_stage"] = round(1e-6 * res["text_bytes"] / res["stage_gunzip_s_median"], 1)
        _, _, err = timed([STAGE, "gunzip", gz, "0", gpu_out], dict(env, HARC_AMD_TRACE="1"))
        laps = {}
        for line in err.splitlines():
            if line.startswith("[gunzip] ") and line.endswith(" s"):
                what, sec = line[len("[gunzip] "):-2].rsplit(": ", 1)
                laps[what] = round(laps.get(what, 0.0) + float(sec), 4)
        res["laps_s"] = laps
        os.remove(gpu_out)
        if args.profile:
            pd = os.path.join(base, "prof")
            timed(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", pd, "--", STAGE, "gunzip", gz, "0", gpu_out], env)
            kern = {}
            for f in glob.glob(os.path.join(pd, "**", "*kernel_stats.csv"), recursive=True):
                for r in csv.DictReader(open(f)):
                    if r.get("Name", "").startswith("k_gz_"):
                        kern[r["Name"].split("(")[0]] = {"calls": int(r["Calls"]), "total_ms": round(float(r["TotalDurationNs"]) * 1e-6, 3)}
            res["kernels"] = kern
    finally:
        shutil.rmtree(base, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


def _gzip(i, o):
    t0 = time.perf_counter()
    subprocess.check_call(["gzip", "-cd"], stdin=i, stdout=o)
    return time.perf_counter() - t0


if __name__ == "__main__":
    main()
