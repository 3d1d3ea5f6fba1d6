"""ctypes loader for the CPU oracle (oracle/harc_oracle.c).  Test infrastructure only."""
import ctypes as C
import io
import os
import subprocess
import tarfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")

_lib = None


class OracleParams(C.Structure):
    """harc_oracle_params of oracle/harc_oracle.c: the macros of the reference's config.h (harc:52-63) as arguments of the _ex entry points"""
    _fields_ = [("L", C.c_int32), ("maxmatch", C.c_int32), ("thresh", C.c_int32), ("thresh_s", C.c_int32), ("maxsearch", C.c_int32),
                ("ds", C.c_int32 * 2), ("de", C.c_int32 * 2)]


PARAM_FIELDS = ("maxmatch", "thresh", "thresh_s", "maxsearch", "dict_start", "dict_end")


def params_dict(L, overrides=None):
    """the six parameter fields as harc:52-60 derives them from the read length, then `overrides` ({field: value}; dict_start / dict_end: a pair)"""
    h = L // 2
    w = 32 if L > 100 else L * 32 // 100
    d = dict(maxmatch=L // 2, thresh=4, thresh_s=24, maxsearch=1000, dict_start=[h - w, h], dict_end=[h - 1, h - 1 + w])
    for k, v in (overrides or {}).items():
        if k not in PARAM_FIELDS:
            raise KeyError(f"{k} is not a parameter field ({PARAM_FIELDS})")
        d[k] = [int(x) for x in v] if k.startswith("dict_") else int(v)
    return d


def oracle_params(L, overrides=None):
    d = params_dict(L, overrides)
    return OracleParams(L, d["maxmatch"], d["thresh"], d["thresh_s"], d["maxsearch"], (C.c_int32 * 2)(*d["dict_start"]), (C.c_int32 * 2)(*d["dict_end"]))


def both_params(L, overrides=None, **kw):
    """-> (OracleParams, harc_amd.Params) from ONE dict of overrides: the two sides of a comparison cannot disagree about the case.
    kw: the schedule fields of harc_amd.default_params (num_thr, num_chains, num_steps, ...)"""
    import harc_amd
    d = params_dict(L, overrides)
    p = harc_amd.default_params(L, **kw)
    for k in PARAM_FIELDS:
        if k.startswith("dict_"):
            getattr(p, k)[0], getattr(p, k)[1] = d[k]
        else:
            setattr(p, k, d[k])
    return oracle_params(L, overrides), p


def load():
    global _lib
    if _lib is not None:
        return _lib
    so = os.environ.get("HARC_ORACLE_LIB") or os.path.join(ORACLE_DIR, "liboracle.so")      # override: e.g. the ASan/UBSan build (make -C oracle asan)
    src = os.path.join(ORACLE_DIR, "harc_oracle.c")
    if "HARC_ORACLE_LIB" not in os.environ and (not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src)):
        subprocess.check_call(["make", "-C", ORACLE_DIR, "liboracle.so"], stdout=subprocess.DEVNULL)
    lib = C.CDLL(so)
    u32p, u64p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
    lib.harc_oracle_reorder.argtypes = [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, u32p, u64p]
    lib.harc_oracle_encoder.argtypes = [C.c_char_p, C.c_int, C.c_uint32, u32p, u32p]
    lib.harc_oracle_pack_order.argtypes = [C.c_char_p]
    lib.harc_oracle_decoder.argtypes = [C.c_char_p, C.c_uint32]
    lib.harc_oracle_preprocess.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_char_p]
    lib.harc_oracle_quality.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_char_p]
    lib.harc_oracle_stage1_mem.argtypes = [C.c_char_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, u32p, u8p, u8p, u8p, u32p, u32p, u32p, u32p, u64p]
    pp = C.POINTER(OracleParams)
    lib.harc_oracle_reorder_ex.argtypes = [C.c_char_p, pp, C.c_uint32, C.c_uint32, u32p, u64p]
    lib.harc_oracle_encoder_ex.argtypes = [C.c_char_p, pp, C.c_uint32, u32p, u32p]
    lib.harc_oracle_stage1_mem_ex.argtypes = [C.c_char_p, C.c_uint32, pp, C.c_uint32, C.c_uint32, u32p, u8p, u8p, u8p, u32p, u32p, u32p, u32p, u64p]
    _lib = lib
    return lib


def golden_cases():
    return sorted(f[:-7] for f in os.listdir(GOLDEN_DIR) if f.endswith(".tar.xz") and not f.startswith(("q_", "p_")))


def param_cases():
    """fixtures of the reference built with another config.h than the driver writes (oracle/make_goldens.py PCASES): meta.json carries `params`"""
    return sorted(f[:-7] for f in os.listdir(GOLDEN_DIR) if f.endswith(".tar.xz") and f.startswith("p_"))


def quality_cases():
    """-q fixtures (ids + quality values), oracle/make_goldens.py QCASES"""
    return sorted(f[:-7] for f in os.listdir(GOLDEN_DIR) if f.endswith(".tar.xz") and f.startswith("q_"))


def load_golden(name):
    """-> dict arcname -> bytes"""
    out = {}
    with tarfile.open(os.path.join(GOLDEN_DIR, name + ".tar.xz"), "r:xz") as tf:
        for m in tf.getmembers():
            out[m.name] = tf.extractfile(m).read()
    return out


def stage_dir(tmpdir, files):
    """write {name: bytes} into <tmpdir>/output/ and return tmpdir as the reference's <basedir>"""
    od = os.path.join(str(tmpdir), "output")
    os.makedirs(od, exist_ok=True)
    for k, v in files.items():
        with open(os.path.join(od, k), "wb") as f:
            f.write(v)
    return str(tmpdir)


def read_dir(basedir):
    od = os.path.join(basedir, "output")
    out = {}
    for f in sorted(os.listdir(od)):
        p = os.path.join(od, f)
        if os.path.isfile(p):
            with open(p, "rb") as fh:
                out[f] = fh.read()
    return out


STAGE1_FILES = ["temp.dna", "temp.dna.singleton", "read_rev.txt", "tempflag.txt", "temppos.txt", "read_order.bin",
                "read_order.bin.singleton"]


def stage2_files(E=1):
    fs = ["read_order.bin", "read_order_N_pe.bin", "input_N.dna", "read_meta.txt", "read_singleton.txt", "read_singleton.txt.tail"]
    for e in range(E):
        for stem in ["read_seq.txt", "read_pos.txt", "read_noise.txt", "read_noisepos.txt", "read_rev.txt"]:
            fs.append(f"{stem}.{e}")
        fs += [f"read_seq.txt.{e}.tail", f"read_rev.txt.{e}.tail"]
    return fs


def md5_cases():
    """exact mode at CONFIG size (oracle/make_goldens.py MD5CASES): generator call + md5 of every file of the reference at -t 1"""
    return sorted(f[4:-5] for f in os.listdir(GOLDEN_DIR) if f.startswith("md5_") and f.endswith(".json"))


def load_md5_case(name):
    """-> (meta dict, reads as [n, L] uint8) -- the reads are regenerated and checked against the recorded md5"""
    import hashlib
    import json
    from tests import gen
    with open(os.path.join(GOLDEN_DIR, "md5_" + name + ".json")) as f:
        meta = json.load(f)
    kw = {k: v for k, v in meta["gen"].items() if k != "function"}
    arr = gen.reads_array_big(**kw)
    got = hashlib.md5(arr.tobytes()).hexdigest()
    assert got == meta["reads_md5"], f"{name}: the generator gives other reads here ({got}) than where the fixture was made ({meta['reads_md5']})"
    return meta, arr


def md5_mismatches(files, want, names):
    """names whose bytes in `files` do not have the md5 (and size) recorded in want = {name: [md5, size]}"""
    import hashlib
    return [f for f in names if f not in files or [hashlib.md5(files[f]).hexdigest(), len(files[f])] != want[f]]
