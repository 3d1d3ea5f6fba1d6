"""The read-multiset signature kernels of harc_amd/csrc/verify.hip against tests/bucket_ref.reads_signature: k_sig_ascii through reads_signature_device,
k_sig_packed2 and k_sig_packed3 through input_signature after set_reads_ascii / set_nreads_ascii.  Read counts around a wavefront and a workgroup; read
lengths that put the last base on either side of a 3-bit code at bit 62 or 63 of a word (bases 21, 42, 85, 106 of the 3-bit store: k_sig_packed3 joins two
words there, and only when a next word exists) and on either side of a 2-bit word (64 bases)."""
import numpy as np
import pytest

from tests.bucket_ref import reads_signature

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257]
LENGTHS = [21, 22, 42, 43, 64, 85, 86, 106, 107, 255]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _reads(seed, n, L, with_N):
    """[n, L + 1] lines; with_N: every read holds N, every other one as its last base too"""
    rng = np.random.default_rng(seed)
    a = np.full((n, L + 1), 10, dtype=np.uint8)
    a[:, :L] = BASES[rng.integers(0, 4, size=(n, L))]
    if with_N:
        for i in range(n):
            a[i, rng.choice(L, size=int(rng.integers(1, 4)), replace=False)] = ord("N")
        a[1::2, L - 1] = ord("N")
    return a


def _lines(a):
    return [row[:-1].tobytes() for row in a]


@pytest.mark.parametrize("L", LENGTHS)
def test_reads_signature_device_equals_model(L):
    import torch
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        for n in COUNTS:
            a = np.concatenate([_reads(10 * L + n, n - n // 2, L, False), _reads(11 * L + n, n // 2, L, True)])
            t = torch.from_numpy(a.copy()).cuda()
            torch.cuda.synchronize()
            got = h.reads_signature_device(t.data_ptr() if n else 0, n, L + 1)
            assert got == reads_signature(_lines(a)), f"L={L} n={n}"
            if n == 0:
                assert got == (0, 0, 0)


@pytest.mark.parametrize("L", LENGTHS)
def test_input_signature_equals_model(L):
    """n reads without N in the 2-bit store and n reads with N in the 3-bit store (W3 = ceil(3 L / 64) words a read)"""
    import harc_amd
    with harc_amd.HarcAmd(harc_amd.default_params(L)) as h:
        for n in COUNTS:
            clean, withN = _reads(20 * L + n, n, L, False), _reads(21 * L + n, n, L, True)
            h.set_reads_ascii(clean.tobytes(), n, L + 1)
            h.set_nreads_ascii(withN.tobytes(), n, L + 1)
            got = h.input_signature()
            assert got == reads_signature(_lines(clean) + _lines(withN)), f"L={L} n={n}"
            if n == 0:
                assert got == (0, 0, 0)
            # each store alone
            h.set_nreads_ascii(b"", 0, L + 1)
            assert h.input_signature() == reads_signature(_lines(clean)), f"L={L} n={n}, 2-bit store alone"
            h.set_reads_ascii(b"", 0, L + 1)
            h.set_nreads_ascii(withN.tobytes(), n, L + 1)
            assert h.input_signature() == reads_signature(_lines(withN)), f"L={L} n={n}, 3-bit store alone"
