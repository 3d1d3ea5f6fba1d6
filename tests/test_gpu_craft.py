"""The three rANS unpack kernels (k_qp_decode, k_ip_decode, the decode kernel of spack.hip) against hand-built blocks: the crafted files of
tests/{quality,id,stream}_craft_cases.py, whole -- tests/test_craft_host.py holds every one of them to the sanitizer build of the same functions first.  A valid
file must come back as its text, a damaged one must be refused with the message of the host twin, string for string; either way nothing outside the declared text
is written, and the context goes on."""
import struct

import pytest

from tests.test_craft_host import FORMATS, cases, message

pytestmark = pytest.mark.gpu
EINVAL = -1
DEVICE = {"quality": "qunpack_device", "id": "idunpack_device", "stream": "sunpack_device"}
ALL = [(fmt, name) for fmt in sorted(FORMATS) for name in sorted(cases(fmt))]
IN_OFF = {case: (1, 5, 9)[k % 3] for k, case in enumerate(ALL)}


@pytest.fixture(scope="module")
def ctx():
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(100)) as h:
        yield h


def _text_bytes(fmt, f):
    """the bytes of text that the file's header announces"""
    if fmt == "quality":
        L, _, n = struct.unpack_from("<IIQ", f, 8)
        return n * (L + 1)
    return struct.unpack_from("<Q", f, 24 if fmt == "id" else 16)[0]


def _dev(b, off):
    import torch
    t = torch.zeros(len(b) + off + 32, dtype=torch.uint8, device="cuda")
    t[off:off + len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + off


def _unpack(h, fmt, blob, in_off, out_off=7):
    """one device call -> (the text or the error, the bytes in front of the text's place, the bytes behind it)"""
    import harc_amd
    import torch
    size = _text_bytes(fmt, blob)
    tb, pb = _dev(blob, in_off)
    out = torch.full((size + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    at = 16 + out_off
    torch.cuda.synchronize()                                      # the library works on a stream of its own
    try:
        got = getattr(h, DEVICE[fmt])(pb, len(blob), out.data_ptr() + at, size)
        assert got == size
    except harc_amd.HarcAmdError as e:
        got = e
    torch.cuda.synchronize()
    host = out.cpu().numpy().tobytes()
    return (got if isinstance(got, Exception) else host[at:at + size]), host[:at], host[at + size:]


@pytest.mark.parametrize("fmt,name", ALL)
def test_device_unpack_of_a_crafted_file(ctx, fmt, name):
    import harc_amd
    blob, want = cases(fmt)[name]
    got, front, behind = _unpack(ctx, fmt, blob, IN_OFF[fmt, name])
    assert front == b"\xee" * len(front) and behind == b"\xee" * len(behind), "bytes outside the text were written"
    if isinstance(want, bytes):
        assert not isinstance(got, Exception), str(got)
        assert got == want
        return
    with pytest.raises(harc_amd.HarcAmdError) as host:
        getattr(harc_amd, FORMATS[fmt][6])(blob)
    assert isinstance(got, harc_amd.HarcAmdError), "block %d code %d was expected, the kernel returned a text" % want
    assert got.code == EINVAL and str(got) == str(host.value)
    assert str(got).endswith(message(fmt, blob, want))           # the block, its byte and the reason of the code that the case's author expects
    # the next call on the same context
    good_name = sorted(k for k, (_, w) in cases(fmt).items() if isinstance(w, bytes))[0]
    good, text = cases(fmt)[good_name]
    again, front, behind = _unpack(ctx, fmt, good, 5)
    assert not isinstance(again, Exception) and again == text and front + behind == b"\xee" * len(front + behind)
