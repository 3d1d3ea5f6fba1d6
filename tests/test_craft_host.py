"""The three rANS unpackers against hand-built blocks, without a GPU: the crafted files of tests/{quality,id,stream}_craft_cases.py -- valid blocks that the
library's encoders never write, and blocks with one or two violations -- through the sanitizer builds of qv_block.h, id_block.h and sv_block.h (the stand-alone
drivers of tests/test_{qpack,idpack,spack}_host.py, every output a heap block of exactly its declared size) and through the library's host twins.  The expected
text or (block, code) is the case author's; the byte offset and the reason text in the message are worked out here from the file and the sources."""
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import id_craft_cases, quality_craft_cases, rans_craft, stream_craft_cases
from tests import test_idpack_host, test_qpack_host, test_spack_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "harc_amd", "csrc")
EINVAL = -1
# format -> (case module, module with the DRIVER, header, source with the reason texts, prefix of the enum, tag of the messages, name of the host twin)
FORMATS = {
    "quality": (quality_craft_cases, test_qpack_host, "qv_block.h", "qpack.hip", "QV_E_", "q", "qunpack_host"),
    "id": (id_craft_cases, test_idpack_host, "id_block.h", "idpack.hip", "ID_E_", "id", "idunpack_host"),
    "stream": (stream_craft_cases, test_spack_host, "sv_block.h", "spack.hip", "SV_E_", "s", "sunpack_host"),
}
_CASES = {}


def cases(fmt):
    """{name: (file, text or (block, code))} of a format, valid ones and refusals, built once"""
    if fmt not in _CASES:
        mod = FORMATS[fmt][0]
        v, r = mod.valid(), mod.refusals()
        assert not set(v) & set(r)
        _CASES[fmt] = dict(v, **r)
    return _CASES[fmt]


def enum_codes(fmt):
    """{name: value} of the format's error enum, from its header"""
    text = open(os.path.join(CSRC, FORMATS[fmt][2])).read()
    return {k: int(v) for k, v in re.findall(r"^\s+(%s[A-Z]+) = (\d+),?\s" % FORMATS[fmt][4], text, re.M)}


def reasons(fmt):
    """{code: the reason text of the library's message}, from the switch in the format's source"""
    names = enum_codes(fmt)
    text = open(os.path.join(CSRC, FORMATS[fmt][3])).read()
    return {names[k]: v for k, v in re.findall(r'case (%s[A-Z]+): return "([^"]*)";' % FORMATS[fmt][4], text)}


def message(fmt, f, want):
    """the library's message for block want[0] of the crafted file f refused with code want[1]"""
    block, code = want
    return "%sunpack: block %d at byte %d is damaged: %s" % (FORMATS[fmt][5], block, rans_craft.block_offsets(f)[block], reasons(fmt)[code])


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the host forms of the block headers")
    d = tmp_path_factory.mktemp("craft")
    built = {}

    def run(fmt, blob):
        if fmt not in built:
            src, built[fmt] = d / (fmt + ".cpp"), d / fmt
            src.write_text(FORMATS[fmt][1].DRIVER)
            subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                                   "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(built[fmt])])
        cin, cout = d / (fmt + ".in"), d / (fmt + ".out")
        cin.write_bytes(blob)
        r = subprocess.run([str(built[fmt]), "dec", str(cin), str(cout)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]                  # the sanitizers are silent
        return cout.read_bytes()
    return run


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_the_expected_codes_are_the_enum(fmt):
    mod = FORMATS[fmt][0]
    assert set(enum_codes(fmt).values()) == mod.CODES and set(reasons(fmt)) == mod.CODES
    want = [w for _, w in mod.refusals().values()]
    assert {code for _, code in want} == mod.CODES
    assert {block for block, _ in want} == {0, 1, 2}
    for name, (f, _) in cases(fmt).items():                       # a file's blocks are walked by their prefixes: what a case damages lies behind them
        off = rans_craft.block_offsets(f)
        assert len(off) in (1, 3) and off[-1] + 4 + struct.unpack_from("<I", f, off[-1])[0] == len(f), name


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_the_readme_decoder_reads_every_valid_case_and_meets_the_coder_edges(fmt):
    seen = FORMATS[fmt][0].check_edges()
    print("craft %s: the README decoder saw %s" % (fmt, seen))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_the_sanitizer_build_answers_every_crafted_file_as_expected(drivers, fmt):
    """no case is left out: every crafted file goes through the sanitizer build silently, with the expected text or the expected block and code"""
    c = cases(fmt)
    names = sorted(c)
    out = drivers(fmt, b"".join(struct.pack("<I", len(c[k][0])) + c[k][0] for k in names))
    at, wrong = 0, []
    for k in names:
        code, block, tb = struct.unpack_from("<III", out, at)
        got, at = out[at + 12:at + 12 + tb], at + 12 + tb
        want = c[k][1]
        if (code, got) != (0, want) if isinstance(want, bytes) else (block, code) != want:
            wrong.append((k, "block %d code %d" % (block, code), want if isinstance(want, tuple) else "its text"))
    assert at == len(out)
    assert not wrong, wrong


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_the_host_twin_gives_the_text_or_names_block_byte_and_reason(fmt):
    import harc_amd
    unpack = getattr(harc_amd, FORMATS[fmt][6])
    wrong = []
    for k, (f, want) in sorted(cases(fmt).items()):
        try:
            got = unpack(f)
        except harc_amd.HarcAmdError as e:
            got = (e.code, str(e))
        if isinstance(want, bytes):
            ok = got == want
        else:
            ok = isinstance(got, tuple) and got[0] == EINVAL and got[1].endswith(message(fmt, f, want))
        if not ok:
            wrong.append((k, got if isinstance(got, tuple) else "a text", want))
    assert not wrong, wrong
