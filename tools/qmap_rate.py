#!/usr/bin/env python3
"""Lossy quality values (harc_amd_qmap_device, harc_amd_qpack_files_ex): what they cost and what they save.

    python tools/qmap_rate.py --sizes                                   the size table, host only: no GPU needed
    python tools/qmap_rate.py [--lines 20000000] [--readlen 100] [--reps 5] [--dir /dev/shm] [--no-files] [--out FILE]

--sizes: 20 000 lines of 100 from each generator of tests/quality_cases.py, packed by harc_amd_qpack_host as they are and after each of the four schemes.

Otherwise, on the GPU: the lines are made on the device (tools/qpack_rate.py: markov_device).  The kernel seconds are the library's own, between two HIP events
on its stream around the kernel alone (HARC_AMD_TRACE=1: the "[qmap] device call" line): k_qm_table with and without the statistics, k_qm_pblock, out of place,
against a device-to-device copy of the same bytes in the same process, between two events as well.  Each is run once unmeasured, then the median of --reps.
Then the file calls on files in --dir: harc_amd_qpack_files_ex with ill8 against harc_amd_qpack_files on the file mapped beforehand, the seconds in the kernels
of both from their "[qpack]" lines, and the share that is the map.  There is no CPU path for this part: without a GPU it fails."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCHEMES = ["ill8", "bin:20:40:6", "cap:30", "pblock:2"]


def sizes():
    import harc_amd
    from tests import quality_cases as qc
    n, L = 20000, 100
    res = {"tool": "qmap_rate", "mode": "sizes", "lines": n, "readlen": L, "packed_bytes": {}}
    for name, text in (("markov", qc.markov(n, L)), ("iid", qc.iid(n)), ("eight_bin", qc.eight_bin(n, L))):
        row = {"none": len(harc_amd.qpack_host(text, L))}
        for spec in SCHEMES:
            mapped, st = harc_amd.qmap_host(text, L, spec)
            row[spec] = len(harc_amd.qpack_host(mapped, L))
            row[spec + " mean_abs"] = round(st["sum_abs"] / st["values"], 3)
        res["packed_bytes"][name] = row
    return res


class Stderr:
    """what the library writes to descriptor 2 inside the block -> .text"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.keep = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *a):
        os.dup2(self.keep, 2)
        os.close(self.keep)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", action="store_true")
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.sizes:
        res = sizes()
    else:
        res = rates(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def rates(a):
    import torch
    import harc_amd
    from tools.qpack_rate import markov_device
    if not torch.cuda.is_available():
        raise SystemExit("qmap_rate: no GPU; this is a measurement, there is nothing to fall back to")
    n, L = a.lines, a.readlen
    text = markov_device(n, L).reshape(-1)
    nbytes = n * (L + 1)
    out = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "qmap_rate", "mode": "rates", "device": torch.cuda.get_device_name(0), "build_id": harc_amd.build_id(), "lines": n, "readlen": L, "text_bytes": nbytes,
           "reps": a.reps}
    os.environ["HARC_AMD_TRACE"] = "1"

    def copy_ms():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        out[:nbytes].copy_(text)                                   # hipMemcpyDtoDAsync
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    copy_ms()
    res["copy_ms"] = statistics.median(copy_ms() for _ in range(a.reps))
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        for key, spec, stats in (("table", "ill8", False), ("table_stats", "ill8", True), ("pblock", "pblock:2", False), ("pblock_stats", "pblock:2", True)):
            def call():
                with Stderr() as err:
                    h.qmap_device(text.data_ptr(), n, L, spec, out.data_ptr(), stats=stats)
                return float(re.search(r"\[qmap\] device call: .* kernel ([0-9.]+) ms", err.text).group(1))
            call()
            ms = [call() for _ in range(a.reps)]
            res[key + "_ms"] = statistics.median(ms)
            res[key + "_ms_min_max"] = [min(ms), max(ms)]
            res[key + "_over_copy"] = res[key + "_ms"] / res["copy_ms"]
            res[key + "_text_GBps"] = nbytes / (res[key + "_ms"] * 1e-3) / 1e9
    if not a.no_files:
        import shutil
        d = os.path.join(a.dir, "qmap_rate.%d" % os.getpid())
        os.makedirs(d)
        try:
            q, mq, hq = (os.path.join(d, k) for k in ("r.quality", "r.mapped", "r.hq"))
            with open(q, "wb") as f:
                for a0 in range(0, nbytes, 1 << 28):
                    f.write(text[a0:a0 + (1 << 28)].cpu().numpy().tobytes())
            del text, out
            torch.cuda.empty_cache()
            harc_amd.qmap_files(q, mq, "ill8")

            def kernels(fn):
                with Stderr() as err:
                    fn()
                line = [l for l in err.text.splitlines() if l.startswith("[qpack]")][-1]
                m = re.search(r"([0-9.]+) s in the kernels of the map", line)
                return float(re.search(r"pieces: ([0-9.]+) s in the kernels", line).group(1)), float(m.group(1)) if m else None
            for key, fn in (("files_plain", lambda: harc_amd.qpack_files(mq, hq)), ("files_ill8", lambda: harc_amd.qpack_files(q, hq, spec="ill8"))):
                fn()
                got = [kernels(fn) for _ in range(3)]
                res[key + "_coder_kernel_s"] = statistics.median(g[0] for g in got)
                if got[0][1] is not None:
                    res[key + "_map_kernel_s"] = statistics.median(g[1] for g in got)
            res["files_map_share"] = res["files_ill8_map_kernel_s"] / (res["files_ill8_map_kernel_s"] + res["files_ill8_coder_kernel_s"])
        finally:
            shutil.rmtree(d, ignore_errors=True)
    return res


if __name__ == "__main__":
    main()
