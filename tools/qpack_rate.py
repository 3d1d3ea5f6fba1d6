#!/usr/bin/env python3
"""Rate of the packed quality file's two device calls and two file calls (harc_amd_qpack_device / harc_amd_qunpack_device, harc_amd_qpack_files /
harc_amd_qunpack_files).

    python tools/qpack_rate.py [--lines 20000000] [--readlen 100] [--reps 5] [--warmup 1] [--dir /dev/shm] [--no-files] [--out FILE]

The lines are made on the device from a seed by the Markov generator of tests/quality_cases.py restated in torch (start near 37, drift down along the line, a
tail of quality 2 on 15 % of the lines).  Each device call is timed after warm-up calls between two HIP events and by a host clock; both calls end in a
device synchronise of their own (they fetch sizes and error words), so both clocks see all of them.  The rate is GB/s of TEXT, n * (readlen + 1) bytes.  The
unpacked text is compared with the input before anything is timed.  The file calls run on files in --dir and are timed by the host clock alone, three times
each.  There is no CPU path: without a GPU the tool fails."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def markov_device(n, L, seed=1):
    import torch
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(seed)
    text = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
    for r0 in range(0, n, 1 << 20):
        m = min(n, r0 + (1 << 20)) - r0
        q = torch.clamp((torch.randn(m, device=dev, generator=g) * 3 + 37).trunc(), 2, 41)
        tail = torch.where(torch.rand(m, device=dev, generator=g) < 0.15, torch.randint(L // 2, max(L, L // 2 + 1), (m,), device=dev, generator=g), torch.full((m,), L, device=dev))
        for t in range(L):
            move = torch.rand(m, device=dev, generator=g) < 0.35
            step = (torch.randn(m, device=dev, generator=g) * 3 - 0.3 - t / L).trunc()
            q = torch.where(move, torch.clamp(q + step, 2, 41), q)
            text[r0:r0 + m, t] = (33 + torch.where(tail <= t, torch.full_like(q, 2), q)).to(torch.uint8)
    text[:, L] = 10
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=20_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--no-files", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import harc_amd
    if not torch.cuda.is_available():
        raise SystemExit("qpack_rate: no GPU; this is a measurement, there is nothing to fall back to")
    n, L = a.lines, a.readlen
    text = markov_device(n, L)
    nbytes = n * (L + 1)
    cap = harc_amd.qpack_bound(n, L)
    packed = torch.empty(cap + 16, dtype=torch.uint8, device="cuda")
    back = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "qpack_rate", "device": torch.cuda.get_device_name(0), "build_id": harc_amd.build_id(), "lines": n, "readlen": L, "text_bytes": nbytes,
           "reps": a.reps, "warmup": a.warmup}
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        def pack():
            return h.qpack_device(text.data_ptr(), n, L, 0, packed.data_ptr(), cap)

        npk = pack()

        def unpack():
            return h.qunpack_device(packed.data_ptr(), npk, back.data_ptr(), nbytes)

        assert unpack() == nbytes
        torch.cuda.synchronize()
        if not torch.equal(back[:nbytes], text.reshape(-1)):
            raise SystemExit("qpack_rate: the unpacked text is not the input; nothing timed")

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e-3, time.perf_counter() - t0

        for _ in range(a.warmup):
            timed(pack); timed(unpack)
        tp, tu = [], []
        for _ in range(a.reps):
            tp.append(timed(pack)); tu.append(timed(unpack))
        for key, ts in (("pack", tp), ("unpack", tu)):
            res[key + "_call_s_events_median"] = statistics.median(t[0] for t in ts)
            res[key + "_call_s_host_median"] = statistics.median(t[1] for t in ts)
            res[key + "_call_s_host_min_max"] = [min(t[1] for t in ts), max(t[1] for t in ts)]
            res[key + "_text_GBps"] = nbytes / res[key + "_call_s_host_median"] / 1e9
        res["packed_bytes"] = npk
        res["packed_over_text"] = npk / nbytes
    if not a.no_files:
        d = os.path.join(a.dir, "qpack_rate.%d" % os.getpid())
        os.makedirs(d)
        try:
            q, hq, bk = (os.path.join(d, k) for k in ("r.quality", "r.quality.hq", "r.back"))
            flat = text.reshape(-1)
            with open(q, "wb") as f:
                for a0 in range(0, flat.numel(), 1 << 28):
                    f.write(flat[a0:a0 + (1 << 28)].cpu().numpy().tobytes())
            del text, packed, back, flat
            torch.cuda.empty_cache()
            for key, fn in (("files_pack_s", lambda: harc_amd.qpack_files(q, hq)), ("files_unpack_s", lambda: harc_amd.qunpack_files(hq, bk))):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    fn()
                    ts.append(time.perf_counter() - t0)
                res[key] = ts
            res["file_packed_bytes"] = os.path.getsize(hq)
            res["file_round_trip_equal"] = os.path.getsize(bk) == nbytes and os.system("cmp -s '%s' '%s'" % (q, bk)) == 0
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
