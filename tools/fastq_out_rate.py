#!/usr/bin/env python3
"""Rate of harc_amd_fastq_assemble_device against its yardstick, a device-to-device hipMemcpyAsync of the same number of output bytes (the kernel reads B
bytes and writes B bytes; the copy moves the same bytes once each way).

    python tools/fastq_out_rate.py [--records 20000000] [--readlen 100] [--reps 10] [--warmup 3] [--out FILE]

The records are made on the device from a seed: ids of 30-50 bytes, reads over ACGT, quality values over 40 printable characters.  The call and the copy
alternate inside one timed loop (other work shares the host), each between two HIP events and a host clock; the call ends in a device synchronise of its own
(it fetches its error counter), so both clocks see all of it -- line index of the id text included.  HARC_AMD_TRACE=1 makes the library print the time of the
tile kernel alone for every call.  The first and the last records of the output are compared with the Python join before anything is timed.
There is no CPU path: without a GPU the tool fails.

    python tools/fastq_out_rate.py --bgzf [--dir /dev/shm] ...

also deflates the assembled text on the GPU (harc_amd_bgzf_deflate_device, timed like the call above), writes the three line files to --dir and times
harc_amd.fastq_assemble plain and with bgzf=True on them, and, as the yardstick, has 16 host processes compress the same text member by member with zlib
level 1 (what 16 threads of bgzip -l 1 do), then level 6 for the size.  The result line gains the "bgzf" object."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MEMBER = 65280


def _zlib_slice(job):
    """(path, first byte, last byte, level) -> bytes of BGZF that zlib makes of that slice of the file, members of 65 280 bytes of text (a host process without a GPU)"""
    import zlib
    path, a, b, level = job
    total = 0
    with open(path, "rb") as f:
        f.seek(a)
        data = f.read(b - a)
    for i in range(0, len(data), MEMBER):
        co = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += 26 + len(co.compress(data[i:i + MEMBER])) + len(co.flush())
    return total


def _host_zlib(path, nbytes, level, procs=16):
    """-> (seconds, bytes): the text file compressed by `procs` processes, each a run of whole members; the pool is started before the clock"""
    import multiprocessing as mp
    nm = (nbytes + MEMBER - 1) // MEMBER
    per = (nm + 8 * procs - 1) // (8 * procs)
    jobs = [(path, m * MEMBER, min(nbytes, (m + per) * MEMBER), level) for m in range(0, nm, per)]
    with mp.get_context("spawn").Pool(procs) as pool:
        pool.map(_zlib_slice, [(path, 0, min(nbytes, MEMBER), level)] * procs)      # the workers are up
        t0 = time.perf_counter()
        sizes = pool.map(_zlib_slice, jobs, chunksize=1)
        return time.perf_counter() - t0, sum(sizes) + 28


def _hip_runtime():
    """the HIP runtime torch has loaded (a second copy of it would not know torch's allocations' device)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


def _first_members(gz, ngz):
    """bytes of the first members of the BGZF tensor that lie inside its first 4 MiB whole"""
    b = gz[:min(ngz, 1 << 22)].cpu().numpy().tobytes()
    at = 0
    while at + 18 <= len(b):
        size = int.from_bytes(b[at + 16:at + 18], "little") + 1
        if at + size > len(b):
            break
        at += size
    return at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--readlen", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bgzf", action="store_true", help="also time the BGZF writer, the file calls and 16 host processes of zlib level 1")
    ap.add_argument("--dir", default="/dev/shm", help="where --bgzf puts its files")
    a = ap.parse_args()
    import torch
    import harc_amd
    if not torch.cuda.is_available():
        raise SystemExit("fastq_out_rate: no GPU; this is a measurement, there is nothing to fall back to")
    n, L = a.records, a.readlen
    dev = "cuda"
    g = torch.Generator(device=dev); g.manual_seed(20)
    lens = torch.randint(30, 51, (n,), device=dev, generator=g)
    ends = torch.cumsum(lens + 1, 0)                              # one past every id's newline
    id_bytes = int(ends[-1])
    ids = (torch.randint(0, 26, (id_bytes,), device=dev, generator=g, dtype=torch.int16) + 97).to(torch.uint8)
    ids[ends - 1] = 10
    ids[ends - (lens + 1)] = 64                                   # '@'
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    dna = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
    qual = torch.empty((n, L + 1), dtype=torch.uint8, device=dev)
    for r0 in range(0, n, 1 << 20):                               # a million records at a time: the index tensors are 64-bit
        r1 = min(n, r0 + (1 << 20))
        dna[r0:r1, :L] = acgt[torch.randint(0, 4, (r1 - r0, L), device=dev, generator=g)]
        qual[r0:r1, :L] = (torch.randint(0, 40, (r1 - r0, L), device=dev, generator=g, dtype=torch.int16) + 35).to(torch.uint8)
    dna[:, L] = 10
    qual[:, L] = 10
    total = id_bytes + n * (2 * L + 4)
    out = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    src = torch.empty(total + 16, dtype=torch.uint8, device=dev)
    hip = _hip_runtime()
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    D2D = 3
    torch.cuda.synchronize()
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        def call():
            return h.fastq_assemble_device(ids.data_ptr(), id_bytes, dna.data_ptr(), qual.data_ptr(), n, L, out.data_ptr(), total)

        def copy():
            rc = hip.hipMemcpyAsync(out.data_ptr(), src.data_ptr(), total, D2D, None)
            if rc != 0:
                raise RuntimeError("hipMemcpyAsync failed: %d" % rc)

        assert call() == total
        torch.cuda.synchronize()
        # the first two and the last record against the join
        le = [int(x) for x in lens[:2].cpu()] + [int(lens[-1])]
        head_ids = ids[:le[0] + le[1] + 2].cpu().numpy().tobytes().split(b"\n")[:2]
        last_id = ids[id_bytes - le[2] - 1:id_bytes - 1].cpu().numpy().tobytes()
        want_head = b"".join(b"%s\n%s\n+\n%s\n" % (head_ids[i], dna[i, :L].cpu().numpy().tobytes(), qual[i, :L].cpu().numpy().tobytes()) for i in range(2))
        want_tail = b"%s\n%s\n+\n%s\n" % (last_id, dna[n - 1, :L].cpu().numpy().tobytes(), qual[n - 1, :L].cpu().numpy().tobytes())
        got_head = out[:len(want_head)].cpu().numpy().tobytes()
        got_tail = out[total - len(want_tail):total].cpu().numpy().tobytes()
        if got_head != want_head or got_tail != want_tail:
            raise SystemExit("fastq_out_rate: the output is not the join of the lines; nothing timed")

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
            timed(call); timed(copy)
        tc, tm = [], []
        for _ in range(a.reps):
            tc.append(timed(call)); tm.append(timed(copy))
        bg = None
        if a.bgzf:
            cap = harc_amd.bgzf_bound(total)
            gz = torch.empty(cap + 16, dtype=torch.uint8, device=dev)

            def deflate():
                return h.bgzf_deflate_device(out.data_ptr(), total, gz.data_ptr(), cap)

            assert call() == total
            ngz = deflate()
            torch.cuda.synchronize()
            import gzip
            head = gzip.decompress(gz[:min(ngz, 1 << 22)].cpu().numpy().tobytes()[:_first_members(gz, ngz)])
            if head != out[:len(head)].cpu().numpy().tobytes() or not head:
                raise SystemExit("fastq_out_rate: the BGZF does not inflate to the text; nothing timed")
            for _ in range(a.warmup):
                timed(deflate)
            td = [timed(deflate) for _ in range(a.reps)]
            bg = {"bgzf_bytes": ngz, "deflate_call_s_events_median": statistics.median(t[0] for t in td), "deflate_call_s_host_median": statistics.median(t[1] for t in td),
                  "deflate_call_s_host_min_max": [min(t[1] for t in td), max(t[1] for t in td)]}
            bg["deflate_text_GBps"] = total / bg["deflate_call_s_host_median"] / 1e9
    if a.bgzf:
        # the files, the file calls, and the host's zlib over the same text
        d = os.path.join(a.dir, "fastq_out_rate.%d" % os.getpid())
        os.makedirs(d)
        try:
            paths = {k: os.path.join(d, k) for k in ("r.dna", "r.id", "r.quality", "r.fastq", "r.fastq.gz")}
            for k, t in (("r.dna", dna), ("r.id", ids), ("r.quality", qual)):
                with open(paths[k], "wb") as f:
                    flat = t.reshape(-1)
                    for a0 in range(0, flat.numel(), 1 << 28):
                        f.write(flat[a0:a0 + (1 << 28)].cpu().numpy().tobytes())
            del dna, qual, ids, out, src, gz
            torch.cuda.empty_cache()
            for key, kw in (("files_plain_s", {}), ("files_bgzf_s", {"bgzf": True})):
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    harc_amd.fastq_assemble(paths["r.dna"], paths["r.id"], paths["r.quality"], paths["r.fastq.gz" if kw else "r.fastq"], **kw)
                    ts.append(time.perf_counter() - t0)
                bg[key] = ts
            bg["file_bgzf_bytes"] = os.path.getsize(paths["r.fastq.gz"])
            bg["host_zlib1_16proc_s"], bg["zlib1_bytes"] = _host_zlib(paths["r.fastq"], total, 1)
            bg["host_zlib6_16proc_s"], bg["zlib6_bytes"] = _host_zlib(paths["r.fastq"], total, 6)
            bg["size_over_zlib1"], bg["size_over_zlib6"] = bg["file_bgzf_bytes"] / bg["zlib1_bytes"], bg["file_bgzf_bytes"] / bg["zlib6_bytes"]
        finally:
            import shutil
            shutil.rmtree(d, ignore_errors=True)
    ev_call, ev_copy = statistics.median(t[0] for t in tc), statistics.median(t[0] for t in tm)
    host_call, host_copy = statistics.median(t[1] for t in tc), statistics.median(t[1] for t in tm)
    res = {
        "tool": "fastq_out_rate", "device": torch.cuda.get_device_name(0), "build_id": harc_amd.build_id(), "records": n, "readlen": L, "id_bytes": id_bytes,
        "output_bytes": total, "reps": a.reps, "warmup": a.warmup,
        "assemble_call_s_events_median": ev_call, "assemble_call_s_host_median": host_call,
        "assemble_call_s_host_min_max": [min(t[1] for t in tc), max(t[1] for t in tc)],
        "d2d_copy_s_events_median": ev_copy, "d2d_copy_s_host_median": host_copy,
        "d2d_copy_s_host_min_max": [min(t[1] for t in tm), max(t[1] for t in tm)],
        "assemble_output_GBps": total / host_call / 1e9, "d2d_copy_GBps_one_way": total / host_copy / 1e9,
        "ratio_call_over_copy_host": host_call / host_copy,
        "note": "the call's time holds the line index of the id text (two passes and a scan over id_bytes), the tile kernel and three host synchronisations; "
                "the events sit on another stream than the library's and agree with the host clock only because the call ends in a synchronise",
    }
    if bg:
        res["bgzf"] = bg
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
