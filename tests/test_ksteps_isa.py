"""What the compiler made of the dense chain kernels, checked on the assembly (no GPU): `make -C harc_amd/csrc isa` emits the
device-only assembly of stage1.hip (one compile, about a minute; make reuses it while it is newer than the sources) and
tools/isa_report.py counts.  The loops are found by what they contain -- the candidate loop by the v_bcnt and the four
row_shr adds of the Hamming sum, the slot search by its pair of global_load_dwordx4 -- not by block numbers.

Numbers of the parent of this change, same compiler (profiles/r07/ksteps_isa_parent.txt), next to what is asserted:
  candidate loop, `s_waitcnt vmcnt` between the claim-word load and the read's load:   parent 1   now 0
  slot search, global loads that follow a wait inside the loop body:                    parent 3   now 1  (the second half bucket)
  k_steps<4,false,false,4,true,true>: reloads + stores of spilled scalars inside loops: parent 80 (64 + 16)   now 67 (57 + 10)
"""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "harc_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DENSE = ["4,0,0,4,1,1", "5,0,0,4,1,1"]          # k_steps<W, QUAD, COOP, NWV, SEQ, SPEC>: the dense wave-uniform kernels of 100-bp and 150-bp reads

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")

# (.vgpr_spill_count, scratch bytes) of every k_steps instantiation on the parent, ROCm 7.2 (AMD clang 22.0.0git): none may get worse
PARENT_VGPR_SPILL = {
    "1,0,0,4,0,0": (0, 0), "1,0,0,4,1,0": (0, 0), "1,0,0,4,1,1": (0, 0), "1,1,0,4,0,0": (0, 0), "1,1,1,1,0,0": (0, 0), "1,1,1,2,0,0": (0, 0), "1,1,1,4,0,0": (0, 0),
    "2,0,0,4,0,0": (0, 0), "2,0,0,4,1,0": (0, 0), "2,0,0,4,1,1": (0, 0), "2,1,0,4,0,0": (0, 0), "2,1,1,1,0,0": (0, 0), "2,1,1,2,0,0": (0, 0), "2,1,1,4,0,0": (0, 0),
    "3,0,0,4,0,0": (2, 12), "3,0,0,4,1,0": (1, 8), "3,0,0,4,1,1": (0, 0), "3,1,0,4,0,0": (0, 0), "3,1,1,1,0,0": (20, 36), "3,1,1,2,0,0": (0, 0), "3,1,1,4,0,0": (0, 0),
    "4,0,0,4,0,0": (6, 28), "4,0,0,4,1,0": (1, 8), "4,0,0,4,1,1": (0, 0), "4,1,0,4,0,0": (0, 0), "4,1,1,1,0,0": (43, 64), "4,1,1,2,0,0": (6, 20), "4,1,1,4,0,0": (6, 20),
    "5,0,0,4,0,0": (6, 28), "5,0,0,4,1,0": (0, 0), "5,0,0,4,1,1": (0, 0), "5,1,0,4,0,0": (0, 0), "5,1,1,1,0,0": (106, 140), "5,1,1,2,0,0": (64, 84), "5,1,1,4,0,0": (64, 84),
    "6,0,0,4,0,0": (12, 52), "6,0,0,4,1,0": (0, 0), "6,0,0,4,1,1": (0, 0), "6,1,0,4,0,0": (0, 0), "6,1,1,1,0,0": (119, 176), "6,1,1,2,0,0": (73, 104), "6,1,1,4,0,0": (73, 104),
    "7,0,0,4,0,0": (52, 92), "7,0,0,4,1,0": (24, 48), "7,0,0,4,1,1": (24, 48), "7,1,0,4,0,0": (0, 0), "7,1,1,1,0,0": (148, 248), "7,1,1,2,0,0": (110, 172), "7,1,1,4,0,0": (110, 172),
    "8,0,0,4,0,0": (53, 96), "8,0,0,4,1,0": (25, 52), "8,0,0,4,1,1": (25, 52), "8,1,0,4,0,0": (0, 0), "8,1,1,1,0,0": (151, 260), "8,1,1,2,0,0": (147, 248), "8,1,1,4,0,0": (147, 248),
}
PARENT_INLOOP_SPILL_TRAFFIC_W4 = 80        # 64 v_readlane + 16 v_writelane of spilled scalars inside the loops of the dense W = 4 kernel
INLOOP_SPILL_TRAFFIC_W4 = 67               # what this tree reaches (57 + 10); the bound the test pins


@pytest.fixture(scope="module")
def report():
    hipcc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    subprocess.check_call(["make", "-C", CSRC, "isa", "HIPCC=" + hipcc], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import isa_report
    finally:
        sys.path.pop(0)
    return isa_report.analyse(os.path.join(CSRC, "stage1.s"), DENSE)


def _only(loops, kind):
    got = [lp for lp in loops if lp["kind"] == kind]
    assert len(got) == 1, "expected one %s loop, found %r" % (kind, got)
    return got[0]


@pytest.mark.parametrize("key", DENSE)
def test_candidate_test_is_one_trip(report, key):
    """(a) claim word and read are asked for together: no wait for memory between the two loads, and nothing else is loaded per candidate"""
    lp = _only(report[key]["loops"], "candidate")
    print(key, lp)
    assert lp["loads_before_test"] == 2          # the ids of a multi-read bin are fetched once per bin, outside this loop
    assert lp["waits_claim_to_read"] == 0


@pytest.mark.parametrize("key", DENSE)
def test_slot_search_one_wait_per_half_bucket(report, key):
    """(b) each half bucket is two whole 16-byte loads behind which nothing is loaded again: the only load that follows a wait is the
    second half bucket's"""
    lp = _only(report[key]["loops"], "slot-search")
    print(key, lp)
    assert lp["gloads"] == 4 and lp["gload_x4"] == 4
    assert lp["serial_waits"] <= 1


@pytest.mark.parametrize("key", DENSE)
def test_registers(report, key):
    """(c) nothing spilled to scratch; the W = 4 kernel keeps the registers of eight waves per SIMD"""
    m = report[key]["meta"]
    print(key, m)
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0
    if key.startswith("4,"):
        assert m["sgpr_count"] <= 80 and m["vgpr_count"] <= 64


def test_scalar_spill_traffic_in_loops(report):
    """(d) reloads and stores of spilled scalars inside the loops of the dense W = 4 kernel"""
    r = report["4,0,0,4,1,1"]["inloop"]
    print(r)
    assert INLOOP_SPILL_TRAFFIC_W4 < PARENT_INLOOP_SPILL_TRAFFIC_W4
    assert r["spill_rd"] + r["spill_wr"] <= INLOOP_SPILL_TRAFFIC_W4
    # none of it in the slot search or the candidate loop
    assert all(report["4,0,0,4,1,1"]["depth"][d]["spill_rd"] + report["4,0,0,4,1,1"]["depth"][d]["spill_wr"] == 0 for d in report["4,0,0,4,1,1"]["depth"] if d >= 3)


def test_no_instantiation_spills_more_than_the_parent(report):
    worse = {}
    for key, m in report["all"].items():
        if key not in PARENT_VGPR_SPILL:
            continue
        ps, pb = PARENT_VGPR_SPILL[key]
        if m["vgpr_spill_count"] > ps or m["private_segment_fixed_size"] > pb:
            worse[key] = (m["vgpr_spill_count"], m["private_segment_fixed_size"], "parent", ps, pb)
    assert len(report["all"]) >= len(PARENT_VGPR_SPILL)
    assert not worse, worse
