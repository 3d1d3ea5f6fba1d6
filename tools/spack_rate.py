#!/usr/bin/env python3
"""Rate of the packed stream file's two file calls (harc_amd_spack_files / harc_amd_sunpack_files) and two device calls on the stream files of a run.

    python tools/spack_rate.py [--reads 2000000] [--archive X.harc] [--reps 3] [--dir /dev/shm] [--out FILE]

The stream files are the members of an archive written with HARC_AMD_STAGE3=none that -S would pack: the five stream tars, input_N.dna and
read_singleton.txt (with -p also the packed read order).  --archive names one; without it the tool makes its own: --reads reads of 100 bases
(tests/gen.reads_array_big, 1 % errors, a fiftieth of them N, a genome of five bases per read) through ./harc -c -t 8.  Every call ends in a device synchronise
of its own (sizes and error words are fetched), so the host clock sees all of it; each is run once unmeasured and then --reps times, and the median is
reported per file and over all files (the sum of the bytes over the sum of the medians).  The rate is GB/s of TEXT.  Every unpacked file is compared with
its input.  There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tarfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEMBERS = ["read_seq.tar", "read_pos.tar", "read_noise.tar", "read_noisepos.tar", "read_rev.tar", "input_N.dna", "read_singleton.txt",
           "read_order.bin", "read_order_N.bin", "read_order_N_pe.bin"]


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def make_archive(d, reads):
    from tests import gen
    fq = os.path.join(d, "r.fastq")
    arr = gen.reads_array_big(7, reads, 100, 5 * reads, err=0.01, n_frac=0.02)
    qual = b"I" * 100
    with open(fq, "wb") as f:
        for a in range(0, reads, 100000):
            f.write(b"".join(b"@r%d\n%s\n+\n%s\n" % (a + i, r.tobytes(), qual) for i, r in enumerate(arr[a:a + 100000])))
    subprocess.check_call([os.path.join(ROOT, "harc"), "-c", fq, "-t", "8"], cwd=ROOT, env=dict(os.environ, HARC_AMD_STAGE3="none"), stdout=subprocess.DEVNULL)
    return os.path.join(d, "r.harc")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2_000_000)
    ap.add_argument("--archive", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import harc_amd
    if not torch.cuda.is_available():
        raise SystemExit("spack_rate: no GPU; this is a measurement, there is nothing to fall back to")
    d = os.path.join(a.dir, "spack_rate.%d" % os.getpid())
    os.makedirs(d)
    res = {"tool": "spack_rate", "device": torch.cuda.get_device_name(0), "build_id": harc_amd.build_id(), "reps": a.reps, "files": {}}
    try:
        arc = a.archive or make_archive(d, a.reads)
        with tarfile.open(arc) as tf:
            tf.extractall(os.path.join(d, "s"))
        files = [os.path.join(d, "s", m) for m in MEMBERS if os.path.exists(os.path.join(d, "s", m))]
        if not files:
            raise SystemExit("spack_rate: %s holds no raw stream (was it written with HARC_AMD_STAGE3=none?)" % arc)
        total = {k: [0, 0.0] for k in ("files_pack", "files_unpack", "device_pack", "device_unpack")}
        with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
            for src in files:
                hs, bk, nbytes = src + ".hs", src + ".back", os.path.getsize(src)
                row = {"text_bytes": nbytes}
                for key, fn in (("files_pack", lambda: harc_amd.spack_files(src, hs)), ("files_unpack", lambda: harc_amd.sunpack_files(hs, bk))):
                    row[key + "_s"] = timed(fn, a.reps)
                row["packed_bytes"] = os.path.getsize(hs)
                row["round_trip_equal"] = os.path.getsize(bk) == nbytes and os.system("cmp -s '%s' '%s'" % (src, bk)) == 0
                text = torch.frombuffer(bytearray(open(src, "rb").read() or b"\0"), dtype=torch.uint8).to("cuda")
                cap = harc_amd.spack_bound(nbytes)
                packed = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
                back = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                npk = h.spack_device(text.data_ptr(), nbytes, 0, packed.data_ptr(), cap)
                for key, fn in (("device_pack", lambda: h.spack_device(text.data_ptr(), nbytes, 0, packed.data_ptr(), cap)),
                                ("device_unpack", lambda: h.sunpack_device(packed.data_ptr(), npk, back.data_ptr(), nbytes))):
                    row[key + "_s"] = timed(fn, a.reps)
                torch.cuda.synchronize()
                row["device_round_trip_equal"] = bool(torch.equal(back[:nbytes], text[:nbytes])) and npk == row["packed_bytes"]
                for key in total:
                    med = statistics.median(row[key + "_s"])
                    row[key + "_text_GBps_median"] = nbytes / med / 1e9
                    total[key][0] += nbytes; total[key][1] += med
                res["files"][os.path.basename(src)] = row
                del text, packed, back
                torch.cuda.empty_cache()
        res["text_bytes"] = sum(r["text_bytes"] for r in res["files"].values())
        res["packed_bytes"] = sum(r["packed_bytes"] for r in res["files"].values())
        for key, (nb, s) in total.items():
            res[key + "_text_GBps"] = nb / s / 1e9
        # the library's own split for the largest file, from a fresh process with the trace on
        big = max(files, key=os.path.getsize)
        code = "import harc_amd; harc_amd.spack_files(%r, %r); harc_amd.sunpack_files(%r, %r)" % (big, big + ".hs", big + ".hs", big + ".back")
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, HARC_AMD_TRACE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        res["trace"] = [l for l in r.stderr.splitlines() if l.startswith("[spack]")]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
