"""The mate rule on the GPU: harc_amd_idmate_rule_device and harc_amd_idmate_apply_device against the Python restatement of tests/idmate_cases.py on every
case, with the texts at device addresses misaligned by 0, 1 and 15 bytes; and the file call in pieces of a few lines, where the lines of the two files fall
differently into the pieces and both texts are carried, with the pair that breaks the rule first, last and at a piece boundary."""
import functools

import pytest

from tests import idmate_cases as mc

pytestmark = pytest.mark.gpu
CASES = mc.cases()
LEADS = (0, 1, 15)
N_FILES = 3001


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _on_device(b, lead, fill=0x31):
    """b at `lead` bytes behind the start of an allocation -> (tensor, device address of b); the bytes around it are '1': a patch outside the text shows"""
    import torch
    t = torch.full((lead + len(b) + 64,), fill, dtype=torch.uint8, device="cuda")
    if b:
        t[lead:lead + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    torch.cuda.synchronize()                                          # the library works on a stream of its own
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + lead


@pytest.mark.parametrize("lead_a, lead_b", [(0, 0), (1, 15), (15, 0), (1, 1)])
def test_rule_device_equals_the_restatement_at_every_alignment(ctx, lead_a, lead_b):
    for name in sorted(CASES):
        a, b = CASES[name]
        ta, pa = _on_device(a, lead_a)
        tb, pb = _on_device(b, lead_b, fill=0x32)
        got = ctx.idmate_rule_device(pa if a else 0, len(a), pb if b else 0, len(b))
        assert got == (mc.rule(a, b), len(mc.lines(a)), mc.flags_and(a, b)), (name, lead_a, lead_b)


@pytest.mark.parametrize("lead", LEADS)
@pytest.mark.parametrize("r", ["slash", "space", "same", "none"])
def test_apply_device_equals_the_restatement_and_touches_nothing_else(ctx, lead, r):
    for name, text in sorted(mc.apply_cases().items()):
        if not text:
            assert ctx.idmate_apply_device(0, 0, r) == 0
            continue
        t, p = _on_device(text, lead)
        bad = ctx.idmate_apply_device(p, len(text), r)
        got = bytes(t.cpu().numpy().tobytes())
        want, want_bad = mc.apply(text, r)
        assert bad == want_bad, (name, r, lead)
        assert got == b"1" * lead + want + b"1" * 64, (name, r, lead)


def test_apply_device_makes_file_2_from_file_1(ctx):
    for name in sorted(CASES):
        a, b = CASES[name]
        r = mc.rule(a, b)
        if r == "none" or not a:
            continue
        t, p = _on_device(a, 3)
        assert ctx.idmate_apply_device(p, len(a), r) == 0, name
        assert bytes(t.cpu().numpy().tobytes())[3:3 + len(a)] == b, name


def test_apply_device_leaves_an_open_last_line_alone(ctx):
    text = b"@a/1\n@b/1"
    t, p = _on_device(text, 1)
    assert ctx.idmate_apply_device(p, len(text), "slash") == 0
    assert bytes(t.cpu().numpy().tobytes())[1:1 + len(text)] == b"@a/2\n@b/1"


def test_unequal_line_counts_and_an_open_last_line_are_refused(ctx):
    import harc_amd
    for a, b, words in ((b"@a\n@b\n@c\n", b"@a\n@b\n", "3 lines"), (b"@a\n@b", b"@a\n@b\n", "no newline"), (b"@a\n", b"", "1 lines")):
        ta, pa = _on_device(a, 0)
        tb, pb = _on_device(b, 0)
        with pytest.raises(harc_amd.HarcAmdError) as e:
            ctx.idmate_rule_device(pa, len(a), pb if b else 0, len(b))
        assert e.value.code == -1 and words in str(e.value), str(e.value)


@functools.lru_cache(maxsize=None)
def _file_ids():
    a, b = mc.illumina_pairs(N_FILES)
    return list(a), list(b)


def _boundary_line(ids, piece):
    """the line of the text that holds byte 10 * piece: a line that a piece boundary cuts or ends"""
    at = 0
    for k, x in enumerate(ids):
        at += len(x) + 1
        if at > 10 * piece:
            return k
    raise AssertionError


@pytest.mark.parametrize("piece", [64, 100, 4096])
@pytest.mark.parametrize("where", ["nowhere", "first", "last", "boundary"])
def test_rule_files_gives_one_answer_whatever_the_piece(tmp_path, monkeypatch, piece, where):
    import harc_amd
    a, b = _file_ids()
    b = list(b)
    # a piece is a byte range: it ends inside a line, and what is behind its last paired line is carried in both files
    k = {"nowhere": None, "first": 0, "last": N_FILES - 1, "boundary": _boundary_line(a, piece)}[where]
    if k is not None:
        b[k] = b[k][:-1] + b"C"                                      # a second difference: no rule holds for this pair
    fa, fb = tmp_path / "a.id", tmp_path / "b.id"
    fa.write_bytes(mc.text_of(a))
    fb.write_bytes(mc.text_of(b))
    want = (mc.rule(mc.text_of(a), mc.text_of(b)), N_FILES)
    assert want[0] == ("space" if k is None else "none")
    monkeypatch.setenv("HARC_AMD_IDMATE_PIECE", str(piece))
    assert harc_amd.idmate_rule_files(str(fa), str(fb)) == want


def test_rule_files_with_lines_of_different_lengths_in_the_two_files(tmp_path, monkeypatch):
    """file 2's lines are much shorter than file 1's: a piece of B holds many more lines than a piece of A, B's text is carried over many turns"""
    import harc_amd
    a, _ = _file_ids()
    b = [b"@%d" % i for i in range(N_FILES)]
    (tmp_path / "a.id").write_bytes(mc.text_of(a))
    (tmp_path / "b.id").write_bytes(mc.text_of(b))
    for piece in ("100", "5000"):
        monkeypatch.setenv("HARC_AMD_IDMATE_PIECE", piece)
        assert harc_amd.idmate_rule_files(str(tmp_path / "a.id"), str(tmp_path / "b.id")) == ("none", N_FILES)
        assert harc_amd.idmate_rule_files(str(tmp_path / "b.id"), str(tmp_path / "a.id")) == ("none", N_FILES)
        assert harc_amd.idmate_rule_files(str(tmp_path / "b.id"), str(tmp_path / "b.id")) == ("same", N_FILES)


def test_rule_files_refuses_different_line_counts_and_an_open_last_line(tmp_path, monkeypatch):
    import harc_amd
    a, b = _file_ids()
    (tmp_path / "a.id").write_bytes(mc.text_of(a[:500]))
    (tmp_path / "short.id").write_bytes(mc.text_of(b[:499]))
    (tmp_path / "open.id").write_bytes(mc.text_of(b[:500])[:-1])
    (tmp_path / "empty.id").write_bytes(b"")
    for piece in ("100", "1000000"):
        monkeypatch.setenv("HARC_AMD_IDMATE_PIECE", piece)
        for x, y in (("a.id", "short.id"), ("short.id", "a.id"), ("a.id", "empty.id")):
            with pytest.raises(harc_amd.HarcAmdError) as e:
                harc_amd.idmate_rule_files(str(tmp_path / x), str(tmp_path / y))
            assert e.value.code == -1 and " 500" in str(e.value) and "mates are paired by their place" in str(e.value), str(e.value)
        for x, y in (("a.id", "open.id"), ("open.id", "a.id")):
            with pytest.raises(harc_amd.HarcAmdError) as e:
                harc_amd.idmate_rule_files(str(tmp_path / x), str(tmp_path / y))
            assert e.value.code == -1 and "no newline" in str(e.value) and "open.id" in str(e.value), str(e.value)
    assert harc_amd.idmate_rule_files(str(tmp_path / "empty.id"), str(tmp_path / "empty.id")) == ("same", 0)
