"""The regular prefix of the probe table (host code, no GPU): harc_amd_selftest_probe_prefix runs the library's make_probe_table and
probe_prefix, the very functions stage I hands `nreg` to the dense chain kernel from.  Below nreg probe 4 j + 2 dir + dict of a step is
(shift j, dir, dict); the kernel's carry writes its stash by `p - 4 fj` there and asks the probe map only behind it, so a prefix that is
too long by one shift would hand a step another probe's bin.

Checked against a restatement of the table (reorder.cpp:517-649: shift by shift, forward dictionaries 0, 1 while the k-mer ends inside
the read, reverse dictionaries 0, 1 while it starts behind the shift) and a prefix counted on that list."""
import pytest


def _table(p):
    t = []
    for j in range(p.maxmatch):
        t += [(j, 0, l) for l in (0, 1) if p.dict_end[l] + j < p.readlen]
        t += [(j, 1, l) for l in (0, 1) if p.dict_start[l] > j]
    return t


def _prefix(t):
    n = 0
    while t[4 * n:4 * n + 4] == [(n, 0, 0), (n, 0, 1), (n, 1, 0), (n, 1, 1)]:
        n += 1
    return n


# the library's default parameters: the first probe to go is the reverse one of dictionary 0 (dict_start[0] > j fails at j = dict_start[0])
@pytest.mark.parametrize("L,want", [(50, None), (63, 11), (100, 18), (101, 18), (150, 43), (255, 95)])
def test_default_parameters(L, want):
    import harc_amd
    from harc_amd import api
    p = harc_amd.default_params(L)
    t = _table(p)
    nprobe, nreg = api.probe_prefix(p)
    print(f"L={L}: dictionaries {tuple(p.dict_start)} .. {tuple(p.dict_end)}, maxmatch {p.maxmatch}: {nprobe} probes, nreg {nreg}")
    assert nprobe == len(t)
    assert nreg == _prefix(t) == p.dict_start[0]
    assert want is None or nreg == want
    assert 0 < nreg < p.maxmatch
    # what the kernel relies on, said on the table itself: below nreg the probe one step later is 4 fj entries in front
    for j in range(nreg):
        for k in range(4):
            assert t[4 * j + k] == (j, k >> 1, k & 1)
    assert len([e for e in t if e[0] == nreg]) < 4


def test_irregular_from_shift_0():
    """dictionary 0 at the very start of the read: shift 0 has no reverse probe of it"""
    import harc_amd
    from harc_amd import api
    p = harc_amd.default_params(100)
    width = p.dict_end[0] - p.dict_start[0]
    p.dict_start[0], p.dict_end[0] = 0, width
    t = _table(p)
    assert t[:3] == [(0, 0, 0), (0, 0, 1), (0, 1, 1)]
    assert api.probe_prefix(p) == (len(t), 0) and _prefix(t) == 0


def test_regular_for_all_shifts():
    """fewer shifts than the first dictionary's start: every shift holds all four probes, the prefix is the whole table"""
    import harc_amd
    from harc_amd import api
    p = harc_amd.default_params(100)
    p.maxmatch = 10
    t = _table(p)
    assert len(t) == 40 and _prefix(t) == 10
    assert api.probe_prefix(p) == (40, 10)


def test_empty_table_and_bad_arguments():
    import harc_amd
    from harc_amd import api
    p = harc_amd.default_params(100)
    p.maxmatch = 0
    assert api.probe_prefix(p) == (0, 0)
    p.maxmatch = 256                                                   # the table's shifts are bytes
    with pytest.raises(harc_amd.HarcAmdError):
        api.probe_prefix(p)
