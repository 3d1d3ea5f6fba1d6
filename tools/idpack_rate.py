#!/usr/bin/env python3
"""Rate of the packed id file's two file calls (harc_amd_idpack_files / harc_amd_idunpack_files) and two device calls, next to harc_amd_qpack_files on a text
of the same size.

    python tools/idpack_rate.py [--ids 4000000] [--reps 3] [--dir /dev/shm] [--no-quality] [--out FILE]

The ids are those of tests/bgzf_out_cases.illumina_text, made with numpy: @SRR870667.<i> HWI-ST1234:100:C0ABCACXX:3:<tile>:<x>:<y> length=100, about 72 bytes
each, in order.  Every call ends in a device synchronise of its own (sizes and error words are fetched), so the host clock sees all of it; each is run once
unmeasured and then --reps times, and the median and the range are reported.  HARC_AMD_TRACE=1 on the last repetition gives the library's own split into
kernels / readers / writers ([idpack] lines, kept in the result).  The rate is GB/s of TEXT.  The unpacked file is compared with the input.  There is no CPU
path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_ids(path, n, seed=11):
    import numpy as np
    rng = np.random.default_rng(seed)
    with open(path, "wb") as f:
        x, tile, i = 1000, 1101, 1
        while i <= n:
            m = min(n + 1 - i, 1 << 18)
            xs = x + np.cumsum(rng.integers(1, 40, m))
            ys = rng.integers(1000, 200000, m)
            lines = []
            for k in range(m):
                v = int(xs[k])
                if v > 20000:
                    xs[k:] -= v - 1000
                    v, tile = 1000, tile + 1
                lines.append(b"@SRR870667.%d HWI-ST1234:100:C0ABCACXX:3:%d:%d:%d length=100\n" % (i + k, tile, v, int(ys[k])))
            f.write(b"".join(lines))
            x, i = int(xs[-1]), i + m
    return os.path.getsize(path)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import harc_amd
    if not torch.cuda.is_available():
        raise SystemExit("idpack_rate: no GPU; this is a measurement, there is nothing to fall back to")
    d = os.path.join(a.dir, "idpack_rate.%d" % os.getpid())
    os.makedirs(d)
    res = {"tool": "idpack_rate", "device": torch.cuda.get_device_name(0), "build_id": harc_amd.build_id(), "ids": a.ids, "reps": a.reps}
    try:
        ids, hi, bk = (os.path.join(d, k) for k in ("r.id", "r.id.hi", "r.back"))
        nbytes = write_ids(ids, a.ids)
        res["text_bytes"] = nbytes
        for key, fn in (("files_pack", lambda: harc_amd.idpack_files(ids, hi)), ("files_unpack", lambda: harc_amd.idunpack_files(hi, bk))):
            ts = timed(fn, a.reps)
            res[key + "_s"] = ts
            res[key + "_text_GBps_median"] = nbytes / statistics.median(ts) / 1e9
        res["packed_bytes"] = os.path.getsize(hi)
        res["packed_over_text"] = res["packed_bytes"] / nbytes
        res["round_trip_equal"] = os.path.getsize(bk) == nbytes and os.system("cmp -s '%s' '%s'" % (ids, bk)) == 0
        # the library's own split, from a fresh process with the trace on
        code = "import harc_amd; harc_amd.idpack_files(%r, %r); harc_amd.idunpack_files(%r, %r)" % (ids, hi, hi, bk)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, HARC_AMD_TRACE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        res["trace"] = [l for l in r.stderr.splitlines() if l.startswith("[idpack]")]
        # the device calls on the whole text at once
        text = torch.frombuffer(bytearray(open(ids, "rb").read()), dtype=torch.uint8).to("cuda")
        cap = harc_amd.idpack_bound(nbytes, a.ids)
        packed = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
        back = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
            npk = h.idpack_device(text.data_ptr(), nbytes, 0, packed.data_ptr(), cap)
            for key, fn in (("device_pack", lambda: h.idpack_device(text.data_ptr(), nbytes, 0, packed.data_ptr(), cap)),
                            ("device_unpack", lambda: h.idunpack_device(packed.data_ptr(), npk, back.data_ptr(), nbytes))):
                ts = timed(fn, a.reps)
                res[key + "_s"] = ts
                res[key + "_text_GBps_median"] = nbytes / statistics.median(ts) / 1e9
            torch.cuda.synchronize()
            res["device_round_trip_equal"] = bool(torch.equal(back[:nbytes], text))
        del text, packed, back
        torch.cuda.empty_cache()
        if not a.no_quality:                                       # harc_amd_qpack_files on text of the same size: lines of 100 quality values
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import qpack_rate
            n = nbytes // 101
            q, hq = os.path.join(d, "r.quality"), os.path.join(d, "r.quality.hq")
            flat = qpack_rate.markov_device(n, 100).reshape(-1)
            with open(q, "wb") as f:
                for a0 in range(0, flat.numel(), 1 << 28):
                    f.write(flat[a0:a0 + (1 << 28)].cpu().numpy().tobytes())
            del flat
            torch.cuda.empty_cache()
            ts = timed(lambda: harc_amd.qpack_files(q, hq), a.reps)
            res["qpack_files_text_bytes"] = n * 101
            res["qpack_files_s"] = ts
            res["qpack_files_text_GBps_median"] = n * 101 / statistics.median(ts) / 1e9
    finally:
        import shutil
        shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
