#!/usr/bin/env python3
"""Static report on the compiled k_steps kernels, from the device-only assembly of stage1.hip (`make -C harc_amd/csrc isa`).

    python tools/isa_report.py [harc_amd/csrc/stage1.s] [--kernel 4,0,0,4,1,1 ...]

For every instantiation of k_steps<W, QUAD, COOP, NWV, SEQ, SPEC>: the registers of the kernel descriptor (.sgpr_count, .sgpr_spill_count,
.vgpr_count, .vgpr_spill_count, scratch bytes).  For every named one (default: the dense wave-uniform kernels of 100-bp and 150-bp reads)
also
  * instruction counts by loop depth (depth 1 = the step loop, 2 = the batch loop, 3-4 = slot search and candidate loops): reloads and
    stores of spilled scalars (v_readlane / v_writelane on the registers the kernel keeps its spilled SGPRs in), s_nop, vector, scalar,
    global loads, LDS, s_waitcnt vmcnt;
  * for every loop whose own blocks hold global loads: the "serial memory waits", i.e. how often a global load follows an
    `s_waitcnt vmcnt` inside the loop body (every one of them is a dependent trip to memory), and whether it is the slot search (two
    global_load_dwordx4) or the candidate loop (v_bcnt + the four row_shr adds).
Nothing here runs on a GPU; the counts are exact for the compiler that made the assembly.  tests/test_ksteps_isa.py asserts on analyse().
"""
import argparse
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_ASM = os.path.join(ROOT, "harc_amd", "csrc", "stage1.s")
DEFAULT_KERNELS = ["4,0,0,4,1,1", "5,0,0,4,1,1"]

_SYM = re.compile(r"^_Z7k_stepsILi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])ELb([01])EEv6S1Args$")
_BLOCK = re.compile(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)")
_HDR = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
_INLOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")


def kernel_key(sym):
    m = _SYM.match(sym)
    return ",".join(m.groups()) if m else None


def kernel_title(key):
    w, quad, coop, nwv, seq, spec = key.split(",")
    b = lambda x: "true" if x == "1" else "false"
    return "k_steps<%s,%s,%s,%s,%s,%s>" % (w, b(quad), b(coop), nwv, b(seq), b(spec))


def read_metadata(lines):
    """symbol -> dict of the .amdhsa kernel metadata fields we report"""
    out, cur = {}, None
    want = ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")
    for ln in lines:
        s = ln.strip()
        if s.startswith("- .agpr_count:") or s.startswith("- .args:"):
            cur = {}
        if cur is None:
            continue
        for k in want:
            if s.lstrip("- ").startswith("." + k + ":"):
                cur[k] = int(s.split(":")[1])
        if s.startswith(".name:"):
            out[s.split(":", 1)[1].strip()] = cur
        if s.startswith(".wavefront_size:"):
            cur = None
    return out


def function_bodies(lines):
    """symbol -> list of lines of every k_steps kernel"""
    out, cur = {}, None
    for ln in lines:
        if cur is None:
            if ln.startswith("_Z7k_stepsI"):
                sym = ln.split(":")[0]
                if kernel_key(sym):
                    cur = out.setdefault(sym, [])
        elif ln.startswith(".Lfunc_end"):
            cur = None
        else:
            cur.append(ln.rstrip("\n"))
    return out


class Block:
    def __init__(self, label):
        self.label, self.loop, self.depth, self.ins = label, None, 0, []


def split_blocks(body):
    """basic blocks in text order, each with its innermost loop (the header's label) and that loop's depth; parents: loop -> enclosing loop"""
    blocks, parents = [Block(None)], {}
    hdr_open = False
    for ln in body:
        m = _BLOCK.match(ln)
        if m:
            blocks.append(Block(m.group(1)))
            hdr_open = True
        cur = blocks[-1]
        s = ln.strip()
        if hdr_open and (m or s.startswith(";")):
            chain = _PARENT.findall(ln)
            if chain:
                cur.__dict__.setdefault("pchain", []).extend(chain)
            h = _HDR.search(ln)
            if h:
                cur.loop, cur.depth = cur.label, int(h.group(1))
                pc = cur.__dict__.get("pchain", [])
                if pc:
                    parents[cur.label] = pc[-1][0]
            i = _INLOOP.search(ln)
            if i:
                cur.loop, cur.depth = i.group(1), int(i.group(2))
            continue
        hdr_open = False
        if not s or s.startswith(";") or s.startswith("."):
            continue
        cur.ins.append(s.split(";")[0].strip())
    return blocks, parents


def spill_vgprs(body):
    """the vector registers the kernel keeps spilled scalars in: targets of `v_writelane_b32 vN, sX, lane` with a literal lane, read back by
    `v_readlane_b32 sX, vN, lane` (the compiler's spill code; the kernel's own cross-lane traffic uses a scalar lane index or other forms)"""
    wr, rd = set(), set()
    for ln in body:
        s = ln.strip()
        m = re.match(r"v_writelane_b32 (v\d+), s\d+, \d+$", s.split(";")[0].strip())
        if m:
            wr.add(m.group(1))
        m = re.match(r"v_readlane_b32 s\d+, (v\d+), \d+$", s.split(";")[0].strip())
        if m:
            rd.add(m.group(1))
    return wr & rd


COLS = ("spill_rd", "spill_wr", "s_nop", "valu", "salu", "gload", "ds", "vmcnt_waits")


def classify(ins, spillregs):
    op = ins.split()[0]
    out = []
    if op == "v_readlane_b32" and re.match(r"v_readlane_b32 s\d+, (v\d+), \d+$", ins) and ins.split()[2].rstrip(",") in spillregs:
        out.append("spill_rd")
    if op == "v_writelane_b32" and re.match(r"v_writelane_b32 (v\d+), s\d+, \d+$", ins) and ins.split()[1].rstrip(",") in spillregs:
        out.append("spill_wr")
    if op == "s_nop":
        out.append("s_nop")
    if op.startswith("v_"):
        out.append("valu")
    if op.startswith("s_"):
        out.append("salu")
    if op.startswith("global_load"):
        out.append("gload")
    if op.startswith("ds_"):
        out.append("ds")
    if op == "s_waitcnt" and "vmcnt" in ins:
        out.append("vmcnt_waits")
    return out


def loop_stream(blocks, loop):
    """the instructions of the loop's own blocks (child loops left out) in text order, starting at its header"""
    idx = [i for i, b in enumerate(blocks) if b.loop == loop]
    start = next((k for k, i in enumerate(idx) if blocks[i].label == loop), 0)
    out = []
    for i in idx[start:] + idx[:start]:
        out.extend(blocks[i].ins)
    return out


def analyse_kernel(body, meta):
    blocks, parents = split_blocks(body)
    spillregs = spill_vgprs(body)
    depth = {}
    for b in blocks:
        row = depth.setdefault(b.depth, dict.fromkeys(COLS, 0))
        for ins in b.ins:
            for k in classify(ins, spillregs):
                row[k] += 1
    loops = []
    for lp in sorted({b.loop for b in blocks if b.loop}, key=lambda x: [int(t) for t in re.findall(r"\d+", x)]):
        st = loop_stream(blocks, lp)
        loads = [k for k, i in enumerate(st) if i.startswith("global_load")]
        if not loads:
            continue
        serial, waited = 0, False
        for i in st:
            if i.startswith("s_waitcnt") and "vmcnt" in i:
                waited = True
            elif i.startswith("global_load"):
                serial += 1 if waited else 0
                waited = False
        x4 = sum(1 for i in st if i.startswith("global_load_dwordx4"))
        bc = next((k for k, i in enumerate(st) if i.startswith("v_bcnt_u32_b32")), None)
        cand = bc is not None and sum(1 for i in st[bc:] if "_dpp" in i and "row_shr" in i) >= 4
        info = {"loop": lp, "depth": next(b.depth for b in blocks if b.loop == lp), "gloads": len(loads), "gload_x4": x4,
                "vmcnt_waits": sum(1 for i in st if i.startswith("s_waitcnt") and "vmcnt" in i), "serial_waits": serial,
                "kind": "candidate" if cand else ("slot-search" if x4 >= 2 else "")}
        if cand:
            # the last two loads in front of the Hamming test are the claim word and the read's dword: waits between them
            before = [k for k in loads if k < bc]
            info["waits_claim_to_read"] = (sum(1 for i in st[before[-2]:before[-1]] if i.startswith("s_waitcnt") and "vmcnt" in i)
                                           if len(before) >= 2 else None)
            info["loads_before_test"] = len(before)
        loops.append(info)
    inloop = {k: sum(r[k] for d, r in depth.items() if d > 0) for k in COLS}
    return {"meta": meta, "spill_vgprs": sorted(spillregs), "depth": depth, "loops": loops, "inloop": inloop}


def analyse(path, kernels=None):
    """{key: {"meta": ..., "depth": ..., "loops": ..., "inloop": ...}} for the named kernels, {"all": {key: meta}} for every k_steps"""
    with open(path) as f:
        lines = f.readlines()
    meta = read_metadata(lines)
    bodies = function_bodies(lines)
    res = {"all": {}}
    for sym in bodies:
        res["all"][kernel_key(sym)] = meta.get(sym, {})
    for key in kernels or DEFAULT_KERNELS:
        sym = next((s for s in bodies if kernel_key(s) == key), None)
        if sym is None:
            raise SystemExit("no k_steps instantiation %s in %s" % (key, path))
        res[key] = analyse_kernel(bodies[sym], meta.get(sym, {}))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="?", default=DEFAULT_ASM)
    ap.add_argument("--kernel", action="append", help="W,QUAD,COOP,NWV,SEQ,SPEC with 0/1 for the flags (repeatable)")
    a = ap.parse_args()
    keys = a.kernel or DEFAULT_KERNELS
    res = analyse(a.asm, keys)
    print("k_steps instantiations: registers of the kernel descriptor")
    print("%-44s %6s %11s %6s %11s %8s" % ("kernel", "sgpr", "sgpr_spill", "vgpr", "vgpr_spill", "scratch"))
    for key in sorted(res["all"], key=lambda k: [int(x) for x in k.split(",")]):
        m = res["all"][key]
        print("%-44s %6s %11s %6s %11s %8s" % (kernel_title(key), m.get("sgpr_count"), m.get("sgpr_spill_count"), m.get("vgpr_count"),
                                              m.get("vgpr_spill_count"), m.get("private_segment_fixed_size")))
    for key in keys:
        r = res[key]
        print()
        print("%s   spilled scalars live in %s" % (kernel_title(key), ", ".join(r["spill_vgprs"]) or "-"))
        print("%-6s" % "depth" + "".join("%12s" % c for c in COLS))
        for d in sorted(r["depth"]):
            print("%-6d" % d + "".join("%12d" % r["depth"][d][c] for c in COLS))
        print("%-6s" % "loops" + "".join("%12d" % r["inloop"][c] for c in COLS))
        print("loops with global loads (own blocks):")
        print("  %-12s %5s %7s %9s %12s %13s  %s" % ("header", "depth", "gloads", "gload_x4", "vmcnt_waits", "serial_waits", "kind"))
        for lp in r["loops"]:
            extra = ""
            if lp["kind"] == "candidate":
                extra = "  (%s loads in front of the test, %s waits between claim word and read)" % (lp["loads_before_test"], lp["waits_claim_to_read"])
            print("  %-12s %5d %7d %9d %12d %13d  %s%s" % (lp["loop"], lp["depth"], lp["gloads"], lp["gload_x4"], lp["vmcnt_waits"], lp["serial_waits"], lp["kind"], extra))
    return 0


if __name__ == "__main__":
    sys.exit(main())
