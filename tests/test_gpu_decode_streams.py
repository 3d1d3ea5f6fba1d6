"""Both decoders of the library (harc_amd/csrc/verify.hip: decode_read, k_unpack_seq, k_split_lines, k_unpack_order, k_permute_lines, k_mark_N, k_merge_lines)
on archives that no encoder wrote (tests/decode_cases.py), against the plain model of the reference's decode chain (tests/decode_model.py, itself held to the
oracle and the goldens in tests/test_decode_model.py): output.dna byte for byte, for -d and, where the archive has order files, for -d -p.  Where oracle/_ref
holds the reference's own -p binaries for the archive's (L, E) they decode a copy as well."""
import pytest

from tests import decode_cases as dc
from tests import decode_model as dm
from tests import oracle_lib as ol

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def small_ring(monkeypatch):
    """output.dna of -d leaves through a ring of pinned slices sized for files of many GB: one small slice and one writer per call here"""
    monkeypatch.setenv("HARC_AMD_FEED_SLICE", "65536"); monkeypatch.setenv("HARC_AMD_FEED_THREADS", "1")
    monkeypatch.delenv("HARC_AMD_BIN_READS", raising=False)


def _first_difference(got, want, L):
    a, b = got.split(b"\n"), want.split(b"\n")
    k = next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))
    return "%d bytes, the model %d; first differing line %d:\n  decoder %r\n  model   %r" % (len(got), len(want), k, a[k] if k < len(a) else None, b[k] if k < len(b) else None)


def _decode(files, E, preserve, tmp):
    import harc_amd
    base = ol.stage_dir(tmp, files)
    harc_amd.decoder(base, E, preserve_order=preserve)
    return ol.read_dir(base)["output.dna"]


@pytest.mark.parametrize("case", dc.CASES, ids=[c.id for c in dc.CASES])
def test_decoders_equal_model_on_built_archive(case, tmp_path):
    files, props, E, L = dc.archive(case)
    want = dm.decode(files, E, L)
    got = _decode(files, E, False, tmp_path / "d")
    assert got == want, "-d: " + _first_difference(got, want, L)
    if "-p" not in props:
        return
    want_p = dm.decode_preserve(files, E, L)
    got_p = _decode(files, E, True, tmp_path / "p")
    assert got_p == want_p, "-d -p: " + _first_difference(got_p, want_p, L)
    ref = dc.reference_chain(files, L, E, tmp_path / "r")
    if ref is not None:
        assert ref == want_p, "reference chain: " + _first_difference(ref, want_p, L)


@pytest.mark.parametrize("bin_reads", [None, 1, 5])
def test_preserve_decoder_in_small_bins(bin_reads, tmp_path, monkeypatch):
    """restore_order in bins (decoder_preserve.cpp:246-290): bins of one and of five output lines, and the default, on an archive of at most 40 lines
    whose lines with N sit at line 0, at the last line and in an adjacent run"""
    if bin_reads:
        monkeypatch.setenv("HARC_AMD_BIN_READS", str(bin_reads))
    files, props, E, L = dc.archive(next(c for c in dc.CASES if c.id == dc.BIN_READS_CASE))
    assert "at most 40 lines" in props
    want = dm.decode_preserve(files, E, L)
    got = _decode(files, E, True, tmp_path / "p")
    assert got == want, _first_difference(got, want, L)


@pytest.mark.parametrize("b", dc.SWEEP)
def test_preserve_decoder_at_numbits(b, tmp_path):
    """read_order.bin packed at numbits = b, 5 .. 32: the groups of 32 entries cross the 32-bit words at every offset (unpack_order.cpp:41-61)"""
    files, props, E, L = dc.archive(dc.sweep_case(b))
    want = dm.decode_preserve(files, E, L)
    got = _decode(files, E, True, tmp_path / "p")
    assert got == want, _first_difference(got, want, L)
    ref = dc.reference_chain(files, L, E, tmp_path / "r")                # (unpack_order.out on a header that names more bits than pack_order would)
    if ref is not None:
        assert ref == want, "reference chain: " + _first_difference(ref, want, L)
