"""The probe carry of the dense SPEC kernel against the CPU oracle (run with -m gpu).

A step of k_steps<W, false, false, 4, true, true> that accepts a read with Hamming distance 0 leaves what the lanes of its batch found behind the hit in
LDS, and the next step takes the probes it can map onto them from there instead of computing key, scramble, minimizer, bitmap word and slot search again
(stage1.hip, CARRY).  A carry that hands a step a wrong bin, skips a probe in front of a carried candidate or survives a step it must not survive still
decodes losslessly, so only the comparison with the oracle's schedule can tell: every stage-I and stage-II file byte for byte, then the decoder's
multiset, with the helpers of test_gpu_dense_widths.py.

Every case forces the SPEC kernel (and, as the control, the general wave-uniform kernel under SPEC's conditions, which has no carry) with HARC_AMD_CARRY
unset and with HARC_AMD_CARRY=0 -- four runs on one context against one run of the oracle.  Read lengths 100, 101, 150 are W = 4, 4, 5; the schedules
(K, S) are (24, 16), (61, 32), (300, 32), (61, 64); the encoder's thread count E is 1 and 3; all of them crossed with the five inputs (a case is a
quarter of a second).

The inputs, 20 000 reads each, one per way the carry can go wrong (matched share of the oracle at L = 100 in brackets):
  clean12   error-free at 12x: the plain case, hits in both directions, winners in a second batch                                    (0.972)
  clean40   error-free at 40x: four or five steps in a row served by one batch                                                      (0.989)
  dups      error-free, a 2000-bp genome: hits at shift 0 (the winner's own lane is carried), multi-read bins, the own-read weeding  (0.993)
  err15     0.5 % errors and reads with N at 15x: steps with distance > 0 and look-ahead seeds between carried steps drop the carry  (0.939)
  rich      repeat copies and poly-A runs: large bins among the carried lanes, defer, the cooperative kernel, roll-backs
On the three error-free inputs the switch must leave counters().useful_probes (the winners' priority indices, in the new step's numbering) what it is and
must lower counters().probes (slots looked at) -- the second is what shows that the carried pass ran at all."""
import pytest

from tests import gen
from tests import oracle_lib as ol
from tests import test_gpu_dense_widths as dw

pytestmark = pytest.mark.gpu

N_READS = 20000
LENGTHS = [100, 101, 150]
SCHEDULES = [(24, 16), (61, 32), (300, 32), (61, 64)]
INPUTS = {
    "clean12": lambda L: gen.reads_text(11, N_READS, L, N_READS * L // 12, err=0.0),
    "clean40": lambda L: gen.reads_text(11, N_READS, L, N_READS * L // 40, err=0.0),
    "dups": lambda L: gen.reads_text(13, N_READS, L, 2000, err=0.0),
    "err15": lambda L: gen.reads_text(14, N_READS, L, N_READS * L // 15, err=0.005),
    "rich": lambda L: gen.reads_text_lowcomplexity(3000 + L, N_READS, L, 50000, err=0.004),
}
ERROR_FREE = ("clean12", "clean40", "dups")
SPEC_FORM = {"HARC_AMD_QUAD": "0", "HARC_AMD_SEQ": "1", "HARC_AMD_S1BLOOM_MZMB": "0"}       # SPEC at L >= 100
FORMS = {"spec": SPEC_FORM, "nospec": dict(SPEC_FORM, HARC_AMD_SPEC="0")}
_VARS = dw._DENSE_VARS + ("HARC_AMD_CARRY",)


def _set_env(monkeypatch, env):
    for v in _VARS:                                                    # nothing inherited: the case alone says which kernel runs
        monkeypatch.delenv(v, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


CASES = [pytest.param(L, K, S, E, name, id=f"L{L}-K{K}-S{S}-E{E}-{name}") for L in LENGTHS for (K, S) in SCHEDULES for E in (1, 3) for name in INPUTS]


@pytest.fixture(scope="module")
def texts():
    """the reads of an (L, input): made once, shared by the schedules and thread counts, never changed"""
    cache = {}

    def get(L, name):
        if (L, name) not in cache:
            cache[(L, name)] = INPUTS[name](L)
        return cache[(L, name)]
    return get


@pytest.mark.parametrize("L,K,S,E,name", CASES)
def test_carry_on_and_off_match_oracle(L, K, S, E, name, oracle, texts, tmp_path, monkeypatch):
    import harc_amd
    txt = texts(L, name)
    inputs, s1, s2 = dw._oracle_run(oracle, tmp_path, txt, L, K, S, E)
    share = dw._matched_share(s1)
    print(f"L={L} K={K} S={S} E={E} {name}: the oracle matched {share:.3f} of the reads")
    assert share > 0.80
    cnt = {}
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=S)) as h:
        dw._load(h, inputs, L)
        for form, fenv in FORMS.items():
            for carry, cenv in (("on", {}), ("off", {"HARC_AMD_CARRY": "0"})):
                _set_env(monkeypatch, dict(fenv, **cenv))
                got = dw._gpu_run(h, E)
                c = h.counters()
                cnt[(form, carry)] = (int(c.probes), int(c.useful_probes), int(c.dense_steps))
                d = tmp_path / f"{form}_{carry}"
                d.mkdir()
                dw._check(oracle, d, got, (s1, s2), E, txt, L,
                          f"L={L} (W={(2 * L + 63) // 64}) {name} K={K} S={S} E={E} under {dict(fenv, **cenv)!r}: HIP path vs oracle")
                assert cnt[(form, carry)][2] > 0
    on, off = cnt[("spec", "on")], cnt[("spec", "off")]
    print(f"slots looked at, carry on / off: {on[0]} / {off[0]} = {on[0] / max(1, off[0]):.3f}; useful probes {on[1]} / {off[1]}")
    assert cnt[("nospec", "on")] == cnt[("nospec", "off")]             # the general kernel has no carry: the switch changes nothing at all
    if name in ERROR_FREE:
        assert on[1] == off[1]
        assert on[0] < off[0]


def test_carry_20000_chains_own_choices(oracle, tmp_path, monkeypatch):
    """300 000 reads of 101 bases, K = 20 000, num_steps = 0: S, the dense launch and the back-off by the library's own rules (lines by minimizer asked
    for, as in test_gpu_dense_widths.py's clean-mzmb0: a bitmap of 300 000 reads is too small for them otherwise, and without them there is no SPEC kernel
    and no carry), once with the switch unset and once off: the oracle's bytes both times, and the same useful_probes"""
    import harc_amd
    L, N, K, E = 101, 300000, 20000, 4
    txt = gen.lines_of(gen.reads_array_big(60 + L, N, L, N * L // 12, err=0.003))
    base = ol.stage_dir(tmp_path, {})
    assert oracle.harc_oracle_preprocess(txt, len(txt), L, base.encode()) == 0
    inputs = {k: v for k, v in ol.read_dir(base).items() if k in ("input_clean.dna", "numreads.bin", "input_N.dna")}
    for f in (tmp_path / "output").iterdir():
        f.unlink()
    S = gen.auto_steps(inputs["input_clean.dna"], K)
    _, s1, s2 = dw._oracle_run(oracle, tmp_path, txt, L, K, S, E)
    assert dw._matched_share(s1) > 0.80
    probes = {}
    with harc_amd.HarcAmd(harc_amd.default_params(L, num_thr=E, num_chains=K, num_steps=0)) as h:
        dw._load(h, inputs, L)
        for carry, cenv in (("on", {}), ("off", {"HARC_AMD_CARRY": "0"})):
            _set_env(monkeypatch, dict({"HARC_AMD_S1BLOOM_MZMB": "0"}, **cenv))
            got = dw._gpu_run(h, E)
            c = h.counters()
            assert int(c.chains) == K and int(c.dense_steps) > 0
            probes[carry] = (int(c.probes), int(c.useful_probes))
            d = tmp_path / carry
            d.mkdir()
            dw._check(oracle, d, got, (s1, s2), E, txt, L, f"L={L} K={K} S=0 (oracle: {S}) E={E}, carry {carry}: HIP path vs oracle")
    print(f"slots looked at, carry on / off: {probes['on'][0]} / {probes['off'][0]} = {probes['on'][0] / max(1, probes['off'][0]):.3f}; "
          f"useful probes {probes['on'][1]} / {probes['off'][1]}")
    assert probes['on'][1] == probes['off'][1]                         # the winners' priority indices are in the new step's numbering on the library's own path too
