"""The stash of the dense SPEC kernel's probe carry, written in the next step's numbering, against the CPU oracle (run with -m gpu).

A step of k_steps<W, false, false, 4, true, true> that accepts a read with Hamming distance 0 at shift fj leaves what its lanes found at the entry of the
probe that looks at the same k-mer in the next step: old probe `po` (shift j) goes to `po - 4 fj` while j lies in the regular prefix of the probe table
(nreg = 18 shifts at L = 100 and 101, 43 at L = 150: tests/test_probe_prefix.py), through the (dir, dictionary, shift) -> probe map behind it, and
nowhere when that index is negative or 64 and more.  The next step reads its own entry, and when the carried part leaves no candidate its first batch
starts behind the known lanes in the same turn of the batch loop (same probes, same counts as in a turn of its own).  A wrong entry still decodes losslessly, so every case is
compared with the oracle's schedule byte for byte, with the helpers of test_gpu_dense_widths.py and in the style of test_gpu_probe_carry.py: the SPEC
kernel and, as the control, the general wave-uniform kernel, each with HARC_AMD_CARRY unset and =0 -- four runs on one context against one run of the
oracle.

Inputs, a few thousand reads each, the smallest at which each path can go wrong:
  spaced   error-free reads tiled along 40 loci, starts 1, 9, 15, 16, 17, 18, 19 bases apart in a row: fj on both sides of nreg = 18 at L = 100 (j and
           j - fj in and behind the prefix: the subtraction and the map), entries that fall in front of the stash (pn < 0) and behind it (pn >= 64: a
           hit in the second batch at fj >= 16), and at the end of every locus a step with no hit at all behind a carried pass (look-ahead seeds)
  alt      starts 1 and 14 bases apart in turn: a hit inside the carried part, then a hit behind the first lane that is not known, and so on; a quarter
           of the loci with every second read reverse-complemented (hits in both directions)
  dups     error-free, a 1500-bp genome: the chain's own reads in the shift-0 bins of both dictionaries, bins of 2 to 16 reads as winners
  rich     repeat copies and poly-A runs: large bins among the carried and the looked-up probes (`mb`, defer), the cooperative kernel, walks that resume
  sub1     1 % substitutions: steps with distance > 0 drop the carry in the middle of a walk
with 1, 4, 61 and 2048 chains (S = 64, 16, 32, 32) at L = 100, 101 (W = 4) and 150 (W = 5)."""
import re

import numpy as np
import pytest

from tests import gen
from tests import test_gpu_dense_widths as dw
from tests import test_gpu_probe_carry as pc

pytestmark = pytest.mark.gpu

LENGTHS = [100, 101, 150]
SCHEDULES = [(1, 64), (4, 16), (61, 32), (2048, 32)]
SPACED = (1, 9, 15, 16, 17, 18, 19)
ALT = (1, 14)


def tiled(seed, L, spacings, n_loci, per_locus, rc_loci=0):
    """error-free reads tiled along n_loci random loci, read i + 1 of a locus starting spacings[i mod len] bases behind read i; in the first rc_loci
    loci every second read is reverse-complemented; the reads are shuffled"""
    rs = np.random.RandomState(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows = []
    for k in range(n_loci):
        steps = np.array([spacings[i % len(spacings)] for i in range(per_locus - 1)])
        starts = np.concatenate([[0], np.cumsum(steps)])
        genome = acgt[rs.randint(0, 4, size=int(starts[-1]) + L)]
        r = genome[starts[:, None] + np.arange(L)[None, :]].copy()
        if k < rc_loci:
            odd = np.arange(per_locus) % 2 == 1
            r[odd] = gen._COMP[r[odd][:, ::-1]]
        rows.append(r)
    r = np.concatenate(rows)
    return gen.lines_of(r[rs.permutation(len(r))])


N_READS = 6000
INPUTS = {
    "spaced": lambda L: tiled(500 + L, L, SPACED, 40, N_READS // 40),
    "alt": lambda L: tiled(600 + L, L, ALT, 40, N_READS // 40, rc_loci=10),
    "dups": lambda L: gen.reads_text(13, N_READS, L, 1500, err=0.0),
    "rich": lambda L: gen.reads_text_lowcomplexity(700 + L, N_READS, L, 15000, n_repeat=18, n_polya=4, err=0.004),
    "sub1": lambda L: gen.reads_text(14, N_READS, L, N_READS * L // 20, err=0.01, n_frac=0.0),
}
ERROR_FREE = ("spaced", "alt", "dups")
CASES = [pytest.param(L, K, S, 1 + 2 * ((i + k) % 2), name, id=f"L{L}-K{K}-S{S}-{name}")
         for L in LENGTHS for k, (K, S) in enumerate(SCHEDULES) for i, name in enumerate(INPUTS)]


@pytest.fixture(scope="module")
def texts():
    """the reads of an (L, input): made once, shared by the schedules, never changed"""
    cache = {}

    def get(L, name):
        if (L, name) not in cache:
            cache[(L, name)] = INPUTS[name](L)
        return cache[(L, name)]
    return get


def test_spacings_reach_both_sides_of_the_prefix():
    """what the `spaced` input is for, said on the parameters (no GPU work): with nreg = 18 at L = 100 its shifts lie in front of, at and behind the prefix,
    a stash written at fj >= 16 has entries behind lane 63 of the old batch only, and one written at fj = 1 drops four entries in front"""
    import harc_amd
    from harc_amd import api
    _, nreg = api.probe_prefix(harc_amd.default_params(100))
    assert min(SPACED) < nreg - 1 and nreg - 1 in SPACED and nreg in SPACED and nreg + 1 in SPACED
    assert any(4 * fj >= 64 for fj in SPACED) and any(0 < 4 * fj < 64 for fj in SPACED)
    assert all(api.probe_prefix(harc_amd.default_params(L))[1] > max(SPACED) for L in (150,))       # W = 5: the same spacings stay inside the prefix


@pytest.mark.parametrize("L,K,S,E,name", CASES)
def test_stash_in_next_numbering_matches_oracle(L, K, S, E, name, oracle, texts, tmp_path, monkeypatch):
    import harc_amd
    txt = texts(L, name)
    inputs, s1, s2 = dw._oracle_run(oracle, tmp_path, txt, L, K, S, E)
    share = dw._matched_share(s1)
    print(f"L={L} K={K} S={S} E={E} {name}: the oracle matched {share:.3f} of the reads")
    assert share > (0.5 if K < 2048 else 0.2)                          # (2048 chains on 6000 reads: a third of the reads are seeds)
    cnt = {}
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, inputs, L)
        for form, fenv in pc.FORMS.items():
            for carry, cenv in (("on", {}), ("off", {"HARC_AMD_CARRY": "0"})):
                pc._set_env(monkeypatch, dict(fenv, **cenv))
                got = dw._gpu_run(h, E)
                c = h.counters()
                cnt[(form, carry)] = (int(c.probes), int(c.useful_probes), int(c.dense_steps))
                d = tmp_path / f"{form}_{carry}"
                d.mkdir()
                dw._check(oracle, d, got, (s1, s2), E, txt, L,
                          f"L={L} (W={(2 * L + 63) // 64}) {name} K={K} S={S} E={E} under {dict(fenv, **cenv)!r}: HIP path vs oracle")
                assert cnt[(form, carry)][2] > 0
    on, off = cnt[("spec", "on")], cnt[("spec", "off")]
    print(f"slots looked at, carry on / off: {on[0]} / {off[0]} = {on[0] / max(1, off[0]):.3f}; useful probes "
          + " / ".join(f"{f} {c}: {cnt[(f, c)][1]}" for f in pc.FORMS for c in ("on", "off")))
    assert cnt[("nospec", "on")] == cnt[("nospec", "off")]             # the general kernel has no carry: the switch changes nothing at all
    assert len({v[1] for v in cnt.values()}) == 1                      # the winners' priority indices, in the new step's numbering, in all four runs
    if name in ERROR_FREE:
        assert on[0] < off[0]                                          # the carried pass ran


# batches per step of the parent of this change on the input below (dbg[5] / dbg[4] as the trace prints them), same session, same machine
PARENT_BATCHES_PER_STEP = 0.50


def test_batches_per_step_not_above_parent(oracle, tmp_path, monkeypatch, capfd):
    """error-free reads at 26x, 61 chains: the trace's batches per step (HARC_AMD_TRACE=1: `[k_steps] ... per step batches`, dbg[5] / dbg[4]; the
    carried pass is no batch) must not be above what the parent of this change needs on the same input.  Measured on one MI355X, parent and this tree in one session: parent 0.50,
    this tree 0.50 (12 352 steps walked on both: a carried pass without a candidate and the batch behind it are one turn now and count as the one
    batch they were).  The issue's own form of that turn -- the lanes [P*, 64) looked up with base 0 -- gave 0.53 and was not kept."""
    import harc_amd
    L, K, S, E = 100, 61, 32, 1
    txt = gen.reads_text(21, 8000, L, 8000 * L // 26, err=0.0)
    inputs, s1, s2 = dw._oracle_run(oracle, tmp_path, txt, L, K, S, E)
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, inputs, L)
        pc._set_env(monkeypatch, pc.SPEC_FORM)
        monkeypatch.setenv("HARC_AMD_TRACE", "1")
        capfd.readouterr()
        got = dw._gpu_run(h, E)
        err = capfd.readouterr().err
        monkeypatch.delenv("HARC_AMD_TRACE")
        d = tmp_path / "trace"
        d.mkdir()
        dw._check(oracle, d, got, (s1, s2), E, txt, L, "L=100 26x K=61 S=32 with the trace on: HIP path vs oracle")
    m = re.findall(r"\[k_steps\] steps walked (\d+) .*?per step batches ([0-9.]+)", err)
    assert m, err[-2000:]
    steps, bps = int(m[-1][0]), float(m[-1][1])
    print(f"steps walked {steps}, batches per step {bps:.2f} (parent {PARENT_BATCHES_PER_STEP})")
    assert steps > 4000
    assert PARENT_BATCHES_PER_STEP is not None and bps <= PARENT_BATCHES_PER_STEP
