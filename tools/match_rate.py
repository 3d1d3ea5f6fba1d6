#!/usr/bin/env python3
"""Match by sequence (./harc -d -M MOTIFS [-e K]): what the match kernel and a whole match cost.  One MI355X; there is no CPU path, without a GPU it fails.

    python tools/match_rate.py [--bytes 1073741824] [--reps 15] [--out FILE]
    python tools/match_rate.py --e2e [--reads 2000000] [--rounds 3] [--other DIR] [--dir /dev/shm] [--out FILE]

Without --e2e: k_motif_match on --bytes resident bytes of random reads of 100 (lines of 101 bytes) with 1, 16 and 256 motifs of 20 bases at K = 0 and K = 2; the
first motif is planted in every hundredth read.  Next to it, on the same number of bytes in the same process, the two streaming kernels the project already times:
the digest kernel of ./harc -V on the reads and k_name_probe on id lines.  All are the library's own seconds between two HIP events around the kernels, from its
"[match] device call", "[check] device call" and "[select] device call" lines under HARC_AMD_TRACE=1; two calls unmeasured, then the median and the best of --reps.

--e2e: the FASTQ of tools/check_rate.py --e2e (--reads records of 100 bases) in --dir with one motif of 25 bases planted in every hundredth read, packed once with
./harc -c -p -q -t 8; then, --rounds times and alternating (the variant that runs first changes from round to round), the wall time by the host's clock of
./harc -d -p -q -M (match), of the full ./harc -d -p -q (full) and of the full restore followed by grep -B1 -A2 of the motif over what it wrote (full_grep); --other
DIR: the ./harc of another build of the project (a checkout of the parent commit, built) does the two full restores.  The match must be what grep finds."""
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
from tools.check_rate import timed, write_fastq                     # noqa: E402
from tools.qmap_rate import Stderr                                  # noqa: E402
from tools.select_rate import id_text, stats, HEAD, TAIL            # noqa: E402

MOTIF = b"GATTACAGATTACACATTAGGACC"


def kernels(args):
    import torch
    import harc_amd
    os.environ["HARC_AMD_TRACE"] = "1"
    L, S = 100, 101
    n_lines = args.bytes // S
    n = n_lines * S
    g = torch.Generator(device="cuda"); g.manual_seed(11)
    codes = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device="cuda")
    t = codes[torch.randint(0, 4, (n_lines, S), device="cuda", generator=g)]
    t[:, L] = 10
    rng = __import__("random").Random(3)
    motifs = ["".join(rng.choice("ACGT") for _ in range(20)).encode() for _ in range(256)]
    planted = torch.frombuffer(bytearray(motifs[0]), dtype=torch.uint8).to("cuda")
    t[37::100, 40:60] = planted
    t = t.reshape(-1)
    flags = torch.zeros(n_lines + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {"tool": "match_rate", "bytes": n, "reads": n_lines, "readlen": L}
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        for count in (1, 16, 256):
            lst = b"".join(m + b"\n" for m in motifs[:count])
            for k in (0, 2):
                kern = []
                for rep in range(2 + args.reps):
                    with Stderr() as err:
                        hits, found = h.motif_flags_device(lst, t.data_ptr(), n_lines, L, flags.data_ptr(), k)
                    if rep >= 2:
                        kern.append(1e-3 * float(re.search(r"match kernel ([0-9.]+) ms", err.text).group(1)))
                assert hits[0] == 1 and int(flags[37:n_lines:100].min()) == 1
                row = stats(kern, n)
                row.update(found=found, selected=int(flags[:n_lines].sum()), ms_per_motif_and_GiB=row["ms_per_GiB_median"] / count)
                res["match_%d_motifs_K%d" % (count, k)] = row
        kern = []
        for rep in range(2 + args.reps):
            with Stderr() as err:
                h.text_digest_device(t.data_ptr(), n)
            if rep >= 2:
                kern.append(1e-3 * float(re.search(r"kernel ([0-9.]+) ms", err.text).group(1)))
        res["digest_kernel"] = stats(kern, n)
        del t
        width = len(HEAD) + 8 + len(TAIL)
        id_lines = args.bytes // width
        ids = id_text(id_lines)
        names = b"".join(b"SRR870667.%08d\n" % (i * (id_lines // 1000)) for i in range(1000))
        tn = torch.frombuffer(bytearray(names), dtype=torch.uint8).to("cuda")
        idf = torch.zeros(id_lines + 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        kern = []
        for rep in range(2 + args.reps):
            with Stderr() as err:
                h.select_flags_device(tn.data_ptr(), len(names), ids.data_ptr(), id_lines * width, idf.data_ptr())
            if rep >= 2:
                kern.append(1e-3 * float(re.search(r"probe kernel ([0-9.]+) ms", err.text).group(1)))
        res["name_probe_1000_names"] = stats(kern, id_lines * width)
    return res


def e2e(args):
    import numpy as np
    env = dict(os.environ, HARC_AMD_STAGE3="none")
    env.pop("HARC_AMD_TRACE", None)
    base = os.path.join(args.dir, "match_e2e.%d" % os.getpid())
    os.makedirs(base)
    n = args.reads
    res = {"tool": "match_rate", "mode": "e2e", "reads": n, "motif": MOTIF.decode(), "rounds": []}
    harc = os.path.join(ROOT, "harc")
    other = os.path.join(os.path.abspath(args.other), "harc") if args.other else harc
    try:
        fq = os.path.join(base, "x.fastq")
        write_fastq(fq, n)
        rec = 218                                                   # bytes of a record of write_fastq: an id of 13 bytes, 100 bases, +, 100 quality values
        a = np.fromfile(fq, dtype=np.uint8).reshape(n, rec)
        a[37::100, 14 + 30:14 + 30 + len(MOTIF)] = np.frombuffer(MOTIF, dtype=np.uint8)
        a.tofile(fq)
        want = a[37::100].tobytes()
        del a
        res["fastq_bytes"] = n * rec
        with open(os.path.join(base, "motifs.txt"), "wb") as f:
            f.write(b">planted\n" + MOTIF + b"\n")
        tc, _ = timed([harc, "-c", fq, "-p", "-q", "-t", "8"], env)
        res["c_s"] = round(tc, 3)
        arc = os.path.join(base, "x.harc")
        variants = ["match", "full", "full_grep"]
        for rnd in range(args.rounds):
            row = {}
            for name in variants[rnd % 3:] + variants[:rnd % 3]:      # (every variant is first in its turn)
                if name == "match":
                    td, out = timed([harc, "-d", arc, "-p", "-q", "-M", os.path.join(base, "motifs.txt")], env)
                    got = os.path.join(base, "x.hit.d.fastq")
                    with open(got, "rb") as f:
                        assert f.read() == want, "the match is not the filter of the input"
                    row["match_line"] = [l for l in out.splitlines() if l.startswith("[match]")]
                    written = os.path.getsize(got)
                else:
                    td, out = timed([other, "-d", arc, "-p", "-q"], env)
                    got = os.path.join(base, "x.d.fastq")
                    written = os.path.getsize(got)
                    assert written == n * rec
                    if name == "full_grep":
                        t0 = time.perf_counter()
                        r = subprocess.run(["grep", "-B1", "-A2", "--no-group-separator", MOTIF.decode(), got], env=dict(env, LC_ALL="C"), stdout=subprocess.PIPE)
                        td += time.perf_counter() - t0
                        assert r.stdout == want, "grep over the full restore does not find what was planted"
                row[name] = {"d_s": round(td, 3), "bytes_written": written}
                os.remove(got)
            res["rounds"].append(row)
        for name in variants:
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
        raise SystemExit("match_rate: no GPU: there is nothing to measure here")
    res = e2e(args) if args.e2e else kernels(args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
