"""ctypes binding of include/harc_amd.h."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))


class HarcAmdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"harc_amd error {code}: {msg}")
        self.code = code


class Params(C.Structure):
    """harc_amd_params == src/config.h macros (harc:52-63)"""
    _fields_ = [("readlen", C.c_int32), ("num_thr", C.c_int32), ("num_chains", C.c_int32), ("maxmatch", C.c_int32),
                ("thresh", C.c_int32), ("thresh_s", C.c_int32), ("maxsearch", C.c_int32), ("dict_start", C.c_int32 * 2),
                ("dict_end", C.c_int32 * 2), ("device", C.c_int32), ("profile", C.c_int32), ("num_steps", C.c_int32), ("reads_per_chain", C.c_int32), ("decode_memory_gb", C.c_int32), ("stream_digest", C.c_int32), ("table_slots_per_read", C.c_int32)]


class Counters(C.Structure):
    _fields_ = [("n_clean", C.c_uint64), ("n_N", C.c_uint64), ("n_main", C.c_uint64), ("n_singleton", C.c_uint64),
                ("unmatched", C.c_uint64), ("aligned_singletons", C.c_uint64), ("aligned_N", C.c_uint64),
                ("chains", C.c_uint64), ("rounds", C.c_uint64), ("probes", C.c_uint64), ("candidates", C.c_uint64),
                ("conflicts", C.c_uint64), ("propose_launches", C.c_uint64), ("propose_ms", C.c_double),
                ("index_ms", C.c_double), ("chain_ms", C.c_double), ("encode_ms", C.c_double), ("total_ms", C.c_double),
                ("contigs", C.c_uint64), ("seq_bases", C.c_uint64), ("bins_over_maxsearch", C.c_uint64),
                ("device_bytes_peak", C.c_uint64), ("useful_probes", C.c_uint64), ("candidates_seq", C.c_uint64),
                ("coop_launches", C.c_uint64), ("coop_ms", C.c_double), ("coop_useful_probes", C.c_uint64), ("coop_candidates_seq", C.c_uint64),
                ("coop_candidates", C.c_uint64), ("coop_steps", C.c_uint64), ("dense_steps", C.c_uint64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


STREAMS = dict(S1_ORDER=0, S1_FLAG=1, S1_POS=2, S1_RC=3, S1_ORDER_SINGLETON=4, S1_DNA=5, S1_DNA_SINGLETON=6,
               S2_SEQ=10, S2_SEQ_TAIL=11, S2_POS=12, S2_NOISE=13, S2_NOISEPOS=14, S2_REV=15, S2_REV_TAIL=16,
               S2_ORDER=20, S2_ORDER_N_PE=21, S2_SINGLETON=22, S2_SINGLETON_TAIL=23, S2_INPUT_N=24, S2_META=25,
               P_ORDER=30, P_ORDER_TAIL=31, IN_ORDER_N=40)

_lib = None


class QMap(C.Structure):
    """harc_amd_qmap: kind 1 a table over the byte values, kind 2 run smoothing with `radius`"""
    _fields_ = [("kind", C.c_int32), ("radius", C.c_int32), ("table", C.c_uint8 * 256)]


class QMapStats(C.Structure):
    _fields_ = [("values", C.c_uint64), ("changed", C.c_uint64), ("sum_abs", C.c_uint64), ("sum_sq", C.c_uint64), ("max_abs", C.c_uint32),
                ("distinct_in", C.c_uint32), ("distinct_out", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class GunzipStats(C.Structure):
    """harc_amd_gunzip_stats: what the parallel inflate of a gzip stream did"""
    _fields_ = [("members", C.c_uint64), ("chunks", C.c_uint64), ("starts_found", C.c_uint64), ("starts_dropped", C.c_uint64), ("repair_walks", C.c_uint64),
                ("text_bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


def lib_path():
    return os.environ.get("HARC_AMD_LIB") or os.path.join(HERE, "libharc_amd.so")      # override: experiment builds of the same sources


def lib():
    """Load libharc_amd.so; fails loudly when the HIP extension has not been built (no fallback of any kind)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise HarcAmdError(-2, f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                               "or `make -C harc_amd/csrc`; harc_amd has no CPU path")
    l = C.CDLL(p)
    PP = C.POINTER(Params)
    ctx = C.c_void_p
    l.harc_amd_default_params.argtypes = [C.c_int32, PP]
    l.harc_amd_create.argtypes = [PP, C.POINTER(ctx)]
    l.harc_amd_destroy.argtypes = [ctx]
    l.harc_amd_destroy.restype = None
    l.harc_amd_last_error.restype = C.c_char_p
    l.harc_amd_set_reads_ascii.argtypes = [ctx, C.c_char_p, C.c_uint32, C.c_uint32]
    l.harc_amd_set_reads_ascii_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32]
    l.harc_amd_set_reads_packed_device.argtypes = [ctx, C.c_void_p, C.c_uint32]
    l.harc_amd_set_nreads_ascii.argtypes = [ctx, C.c_char_p, C.c_uint32, C.c_uint32]
    l.harc_amd_set_nreads_ascii_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32]
    l.harc_amd_set_stage1_streams.argtypes = [ctx, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32,
                                              C.c_char_p, C.c_char_p, C.c_uint32]
    l.harc_amd_pack_reads_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    l.harc_amd_bucket_reads_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    l.harc_amd_partition_reads_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    for f in ("harc_amd_reorder", "harc_amd_encode", "harc_amd_pack_order"):
        getattr(l, f).argtypes = [ctx]
    l.harc_amd_get_stream.argtypes = [ctx, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]
    l.harc_amd_get_counters.argtypes = [ctx, C.POINTER(Counters)]
    for f in ("harc_amd_reorder_files", "harc_amd_encoder_files", "harc_amd_compress_files", "harc_amd_pack_order_files"):
        getattr(l, f).argtypes = [PP, C.c_char_p]
    l.harc_amd_preprocess_files.argtypes = [C.c_char_p, C.c_char_p, C.c_int32]
    l.harc_amd_decoder_files.argtypes = [PP, C.c_char_p, C.c_int32]
    l.harc_amd_compress_fastq_files_ex.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]
    l.harc_amd_build_has.argtypes = [C.c_char_p]
    l.harc_amd_last_fastq_timing.argtypes = [C.POINTER(C.c_double), C.c_int32]
    l.harc_amd_decoder_preserve_files.argtypes = [PP, C.c_char_p, C.c_int32]
    l.harc_amd_compress_fastq_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_set_fastq_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_bgzf_inflate_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_set_fastq_bgzf_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_fastq_assemble_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64,
                                                 C.POINTER(C.c_uint64)]
    l.harc_amd_fastq_assemble_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    l.harc_amd_fastq_assemble_files_ex.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32]
    GS = C.POINTER(GunzipStats)
    l.harc_amd_gunzip_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), GS]
    l.harc_amd_gunzip_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), GS]
    l.harc_amd_gunzip_files.argtypes = [PP, C.c_char_p, C.c_char_p, GS]
    l.harc_amd_bgzf_bound.argtypes = [C.c_uint64]
    l.harc_amd_bgzf_bound.restype = C.c_uint64
    l.harc_amd_bgzf_deflate_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_bgzf_deflate_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_qpack_bound.argtypes = [C.c_uint64, C.c_int32, C.c_uint32]
    l.harc_amd_qpack_bound.restype = C.c_uint64
    l.harc_amd_qpack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_qunpack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_qpack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_qunpack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_qpack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_qunpack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    QM, QS = C.POINTER(QMap), C.POINTER(QMapStats)
    l.harc_amd_qmap_parse.argtypes = [C.c_char_p, QM]
    l.harc_amd_qmap_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, QM, C.c_char_p, QS]
    l.harc_amd_qmap_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_int32, QM, C.c_void_p, QS]
    l.harc_amd_qmap_files.argtypes = [PP, C.c_char_p, C.c_char_p, QM, QS]
    l.harc_amd_qpack_files_ex.argtypes = [PP, C.c_char_p, C.c_char_p, QM, QS]
    l.harc_amd_idpack_bound.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
    l.harc_amd_idpack_bound.restype = C.c_uint64
    l.harc_amd_idpack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_idunpack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_idpack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_idunpack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_idpack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_idunpack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_spack_bound.argtypes = [C.c_uint64, C.c_uint32]
    l.harc_amd_spack_bound.restype = C.c_uint64
    l.harc_amd_spack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_sunpack_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_spack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_sunpack_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]
    l.harc_amd_spack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_sunpack_files.argtypes = [PP, C.c_char_p, C.c_char_p]
    l.harc_amd_spack_file_list.argtypes = [PP, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    l.harc_amd_sunpack_file_list.argtypes = [PP, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p)]
    l.harc_amd_decode_signature.argtypes = [ctx, C.POINTER(C.c_uint64)]
    l.harc_amd_input_signature.argtypes = [ctx, C.POINTER(C.c_uint64)]
    l.harc_amd_reads_signature_device.argtypes = [ctx, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    l.harc_amd_comm_get_id.argtypes = [C.c_char_p, C.c_size_t]
    l.harc_amd_comm_init.argtypes = [ctx, C.c_char_p, C.c_size_t, C.c_int32, C.c_int32]
    l.harc_amd_comm_init_mailbox.argtypes = [ctx, C.c_char_p, C.c_int32, C.c_int32]
    l.harc_amd_comm_barrier.argtypes = [ctx]
    l.harc_amd_comm_destroy.argtypes = [ctx]
    l.harc_amd_shard_exchange.argtypes = [ctx, C.POINTER(C.c_uint64)]
    l.harc_amd_shard_reset.argtypes = [ctx]
    l.harc_amd_replicate_exchange.argtypes = [ctx, C.POINTER(C.c_uint64)]
    l.harc_amd_compress_fastq_shard_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_char_p]
    l.harc_amd_merge_shard_files.argtypes = [C.c_char_p, C.c_int32]
    l.harc_amd_stream_digest.argtypes = [ctx, C.POINTER(C.c_uint64)]
    l.harc_amd_selftest_launch.argtypes = [ctx, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    l.harc_amd_selftest_index.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    if hasattr(l, "harc_amd_selftest_contigs"):          # (HARC_AMD_LIB may name a build from before it)
        l.harc_amd_selftest_contigs.argtypes = [ctx, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    if hasattr(l, "harc_amd_selftest_probe_prefix"):     # (as above)
        l.harc_amd_selftest_probe_prefix.argtypes = [PP, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    U3 = C.POINTER(C.c_uint64)
    l.harc_amd_text_digest_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint64, U3]
    l.harc_amd_text_digest_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, U3]
    l.harc_amd_text_digest_files.argtypes = [PP, C.c_char_p, U3]
    l.harc_amd_input_order_digest.argtypes = [ctx, U3]
    l.harc_amd_reads_check_files.argtypes = [PP, C.c_char_p, U3, U3]
    l.harc_amd_compress_fastq_files_checked.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int32]
    U64P, U32P = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    if hasattr(l, "harc_amd_idmate_rule_device"):        # (HARC_AMD_LIB may name a build from before paired-end input)
        l.harc_amd_idmate_rule_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, U64P, U32P]
        l.harc_amd_idmate_rule_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U64P, U32P]
        l.harc_amd_idmate_rule_of.argtypes = [C.c_uint32, C.c_uint64]
        l.harc_amd_idmate_rule_of.restype = C.c_int32
        l.harc_amd_idmate_rule_name.argtypes = [C.c_int32]
        l.harc_amd_idmate_rule_name.restype = C.c_char_p
        l.harc_amd_idmate_rule_parse.argtypes = [C.c_char_p]
        l.harc_amd_idmate_rule_parse.restype = C.c_int32
        l.harc_amd_idmate_rule_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.POINTER(C.c_int32), U64P]
        l.harc_amd_idmate_apply_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_int32, U64P]
        l.harc_amd_idmate_apply_host.argtypes = [C.c_char_p, C.c_uint64, C.c_int32, U64P]
        l.harc_amd_compress_fastq_pair_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, U64P]
        l.harc_amd_fastq_assemble_pair_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int32, C.c_int32]
    if hasattr(l, "harc_amd_third_rule_device"):         # (HARC_AMD_LIB may name a build from before the third lines were kept)
        l.harc_amd_third_rule_device.argtypes = [ctx, C.c_void_p, C.c_uint64, U64P, U32P]
        l.harc_amd_third_rule_host.argtypes = [C.c_char_p, C.c_uint64, U64P, U32P]
        l.harc_amd_third_rule_of.argtypes = [C.c_uint32, C.c_uint64]
        l.harc_amd_third_rule_of.restype = C.c_int32
        l.harc_amd_third_rule_name.argtypes = [C.c_int32]
        l.harc_amd_third_rule_name.restype = C.c_char_p
        l.harc_amd_third_rule_parse.argtypes = [C.c_char_p]
        l.harc_amd_third_rule_parse.restype = C.c_int32
        l.harc_amd_fastq_assemble_third_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32, C.c_void_p, C.c_uint64, U64P, C.c_int32]
        l.harc_amd_fastq_assemble_third_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32]
        l.harc_amd_fastq_assemble_third_pair_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32]
    if hasattr(l, "harc_amd_line_offset_device"):        # (HARC_AMD_LIB may name a build from before range restore)
        l.harc_amd_line_offset_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint64, U64P]
        l.harc_amd_line_offset_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, U64P]
        l.harc_amd_line_range_files.argtypes = [PP, C.c_char_p, C.c_uint64, C.c_uint64, U64P]
        l.harc_amd_qunpack_range_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64]
        l.harc_amd_idunpack_range_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64]
        l.harc_amd_decoder_range_files.argtypes = [PP, C.c_char_p, C.c_int32, C.c_int32, U64P, U64P]
        l.harc_amd_decoder_preserve_range_files.argtypes = [PP, C.c_char_p, C.c_int32, C.c_int32, U64P, U64P]
    if hasattr(l, "harc_amd_select_files"):              # (HARC_AMD_LIB may name a build from before selection by name)
        U8P = C.POINTER(C.c_uint8)
        l.harc_amd_name_key_host.argtypes = [C.c_char_p, C.c_uint64, U64P]
        l.harc_amd_select_flags_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, U64P, U64P, U64P]
        l.harc_amd_select_flags_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U8P, U64P, U64P, U64P]
        l.harc_amd_lines_gather_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, U64P]
        l.harc_amd_lines_gather_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, U64P]
        l.harc_amd_select_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int32, U64P, C.c_char_p, C.c_uint64]
    if hasattr(l, "harc_amd_match_files"):               # (HARC_AMD_LIB may name a build from before the match by sequence)
        U8P = C.POINTER(C.c_uint8)
        l.harc_amd_motifs_check_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, U64P]
        l.harc_amd_motif_flags_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_char_p, C.c_uint64, C.c_uint32, U8P, U8P, U64P, U64P]
        l.harc_amd_motif_flags_device.argtypes = [ctx, C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, U8P, U64P, U64P]
        l.harc_amd_match_files.argtypes = [PP, C.c_char_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int32, U64P, C.c_char_p, C.c_uint64]
    if hasattr(l, "harc_amd_recovery_make_files"):       # (HARC_AMD_LIB may name a build from before the recovery record)
        CPP, VPP, I32P = C.POINTER(C.c_char_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int32)
        l.harc_amd_block_digests_device.argtypes = [ctx, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, U64P]
        l.harc_amd_block_digests_host.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, U64P]
        l.harc_amd_gf_combine_device.argtypes = [ctx, C.c_uint32, C.c_int32, VPP, C.c_int32, VPP, C.c_char_p]
        l.harc_amd_gf_combine_host.argtypes = [C.c_uint32, C.c_int32, VPP, C.c_int32, VPP, C.c_char_p]
        l.harc_amd_recovery_make_files.argtypes = [PP, C.c_int32, CPP, C.c_uint32, C.c_char_p, U64P]
        l.harc_amd_recovery_check_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_uint64, I32P]
        l.harc_amd_recovery_repair_files.argtypes = [PP, C.c_char_p, C.c_char_p, C.c_uint64, I32P]
        l.harc_amd_recovery_make_host.argtypes = [C.c_int32, CPP, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, U64P]
        l.harc_amd_recovery_repair_host.argtypes = [C.c_char_p, C.c_int32, C.c_char_p, C.c_uint64, I32P]
    l.harc_amd_build_id.restype = C.c_char_p
    _lib = l
    return l


def _check(rc):
    if rc != 0:
        raise HarcAmdError(rc, lib().harc_amd_last_error().decode(errors="replace"))


def default_params(readlen, num_thr=8, num_chains=0, device=0, profile=0, num_steps=0, reads_per_chain=0, stream_digest=0, table_slots_per_read=0):
    p = Params()
    _check(lib().harc_amd_default_params(readlen, C.byref(p)))
    p.num_thr, p.num_chains, p.device, p.profile, p.num_steps = num_thr, num_chains, device, profile, num_steps
    p.reads_per_chain = reads_per_chain
    p.stream_digest = stream_digest
    p.table_slots_per_read = table_slots_per_read      # 0: the library chooses (4, 3 or 2 by free memory); include/harc_amd.h
    return p


def probe_prefix(params):
    """(nprobe, nreg) of the probe table these parameters make: the probes of one chain step, and how many leading shifts hold all four of
    them in the canonical order (host code: harc_amd_selftest_probe_prefix)"""
    n, r = C.c_int32(0), C.c_int32(0)
    _check(lib().harc_amd_selftest_probe_prefix(C.byref(params), C.byref(n), C.byref(r)))
    return n.value, r.value


def build_id():
    """sha256 of the kernel sources the loaded library was built from"""
    return lib().harc_amd_build_id().decode()


# ---- the reference's stage programs (file contract)
def reorder(basedir, readlen, num_chains=1, **kw):
    """== `reorder.out <basedir>` (src/reorder.cpp:100-131)"""
    p = default_params(readlen, num_chains=num_chains, **kw)
    _check(lib().harc_amd_reorder_files(C.byref(p), os.fsencode(basedir)))


def encoder(basedir, readlen, num_thr=1, **kw):
    """== `encoder.out <basedir>` (src/encoder.cpp:108-152)"""
    p = default_params(readlen, num_thr=num_thr, **kw)
    _check(lib().harc_amd_encoder_files(C.byref(p), os.fsencode(basedir)))


def compress(basedir, readlen, num_thr=1, num_chains=1, **kw):
    """harc:65-69 fused: stage I -> stage II in HBM"""
    p = default_params(readlen, num_thr=num_thr, num_chains=num_chains, **kw)
    _check(lib().harc_amd_compress_files(C.byref(p), os.fsencode(basedir)))


def preprocess(fastq, basedir, readlen):
    """== `preprocess.out <fastq> <basedir> False False <readlen>` (src/preprocess.cpp:22-137): the N split"""
    _check(lib().harc_amd_preprocess_files(os.fsencode(fastq), os.fsencode(basedir), readlen))


def compress_fastq(fastq, basedir, readlen, num_thr=1, num_chains=1, preserve_order=False, preserve_quality=False, check=False, **kw):
    """harc:50-69 in one call, FASTQ parsed on the GPU; preserve_quality (-q) also writes output.quality / output.id
    (preprocess.cpp:61-118, reorder_quality.cpp); check (-V): the streams are decoded once before they are written and output/read.check is written"""
    p = default_params(readlen, num_thr=num_thr, num_chains=num_chains, **kw)
    _check(lib().harc_amd_compress_fastq_files_checked(C.byref(p), os.fsencode(fastq), os.fsencode(basedir), int(preserve_order), int(preserve_quality), int(check)))


def compress_fastq_pair(fastq1, fastq2, basedir, readlen, num_thr=1, num_chains=1, preserve_quality=False, check=False, **kw):
    """compress_fastq over two files as one job, the order kept (./harc -c R1 -2 R2 -p): the records of fastq1, then those of fastq2 -- the archive of their
    `cat` without the copy, plus output/read.pair; with preserve_quality output.id holds the ids of fastq1 and output.id2 those of fastq2
    (include/harc_amd.h: harc_amd_compress_fastq_pair_files) -> the records in each file"""
    p = default_params(readlen, num_thr=num_thr, num_chains=num_chains, **kw)
    n = C.c_uint64(0)
    _check(lib().harc_amd_compress_fastq_pair_files(C.byref(p), os.fsencode(fastq1), os.fsencode(fastq2), os.fsencode(basedir), int(preserve_quality), int(check), C.byref(n)))
    return n.value


IDMATE_RULES = ("none", "same", "slash", "space")      # HARC_AMD_IDMATE_NONE .. HARC_AMD_IDMATE_SPACE


def _rule_number(rule):
    return IDMATE_RULES.index(rule) if isinstance(rule, str) else int(rule)


def _rule_from_flags(flags, pairs):
    return IDMATE_RULES[lib().harc_amd_idmate_rule_of(flags, pairs)]


def idmate_rule_host(a, b):
    """the mate rule of the id texts a and b (bytes: id lines, a newline behind each) on the host (include/harc_amd.h: harc_amd_idmate_rule_host)
    -> (rule name, pairs, the AND of the pairs' flags: bit 0 same, 1 slash, 2 space); no device"""
    n, f = C.c_uint64(0), C.c_uint32(0)
    _check(lib().harc_amd_idmate_rule_host(a, len(a), b, len(b), C.byref(n), C.byref(f)))
    return _rule_from_flags(f.value, n.value), n.value, f.value


def idmate_apply_host(ids, rule):
    """file 2's ids from file 1's on the host: the whole lines of `ids` patched by `rule` (a name or a number) -> (the patched text, lines that did not carry
    the '1' to replace); no device"""
    buf = C.create_string_buffer(bytes(ids), len(ids) + 1)
    bad = C.c_uint64(0)
    _check(lib().harc_amd_idmate_apply_host(buf, len(ids), _rule_number(rule), C.byref(bad)))
    return buf.raw[:len(ids)], bad.value


def idmate_rule_files(path_a, path_b, device=0):
    """the mate rule of two id files, walked in lockstep on the GPU (include/harc_amd.h: harc_amd_idmate_rule_files) -> (rule name, pairs)"""
    p = default_params(100, device=device)
    r, n = C.c_int32(0), C.c_uint64(0)
    _check(lib().harc_amd_idmate_rule_files(C.byref(p), os.fsencode(path_a), os.fsencode(path_b), C.byref(r), C.byref(n)))
    return IDMATE_RULES[r.value], n.value


THIRD_RULES = ("dropped", "bare", "same")              # HARC_AMD_THIRD_DROPPED .. HARC_AMD_THIRD_SAME


def _third_number(third):
    return THIRD_RULES.index(third) if isinstance(third, str) else int(third)


def third_rule_of(flags, records):
    """the rule of the third lines that a flag word over `records` records stands for (include/harc_amd.h: harc_amd_third_rule_of) -> its name"""
    return THIRD_RULES[lib().harc_amd_third_rule_of(flags, records)]


def third_rule_name(rule):
    return lib().harc_amd_third_rule_name(int(rule)).decode()


def third_rule_parse(name):
    return lib().harc_amd_third_rule_parse(name.encode() if isinstance(name, str) else name)


def third_rule_host(fastq):
    """the rule of the third lines of the FASTQ text `fastq` (bytes) on the host (include/harc_amd.h: harc_amd_third_rule_host)
    -> (rule name, records that took part, the AND of their flags: bit 0 bare, 1 same); no device"""
    n, f = C.c_uint64(0), C.c_uint32(0)
    _check(lib().harc_amd_third_rule_host(fastq, len(fastq), C.byref(n), C.byref(f)))
    return third_rule_of(f.value, n.value), n.value, f.value


def fastq_assemble_pair(dna, ids, quality, out1, out2, records, rule, device=0, bgzf=False, third=None):
    """fastq_assemble for a paired archive: records [0, records) -> out1, [records, 2 records) -> out2; rule none: `ids` holds the lines of both files, any other
    rule: the first file's, and the second file's are made from them on the GPU (include/harc_amd.h: harc_amd_fastq_assemble_pair_files).  third: the rule of
    the third lines, a name or a number (harc_amd_fastq_assemble_third_pair_files)"""
    p = default_params(100, device=device)
    if third is not None:
        _check(lib().harc_amd_fastq_assemble_third_pair_files(C.byref(p), os.fsencode(dna), os.fsencode(ids), os.fsencode(quality), os.fsencode(out1), os.fsencode(out2),
                                                              records, _rule_number(rule), 1 if bgzf else 0, _third_number(third)))
        return
    _check(lib().harc_amd_fastq_assemble_pair_files(C.byref(p), os.fsencode(dna), os.fsencode(ids), os.fsencode(quality), os.fsencode(out1), os.fsencode(out2),
                                                    records, _rule_number(rule), 1 if bgzf else 0))


def build_has(feature):
    """True when the loaded library was built with the optional part `feature` ("test_transport", "experiments")"""
    return bool(lib().harc_amd_build_has(feature.encode()))


def last_fastq_timing(n=8):
    """seconds of the last compress_fastq of this process, by phase (include/harc_amd.h: harc_amd_last_fastq_timing); n=9 adds the
    BGZF member scan and inflate"""
    t = (C.c_double * n)()
    _check(lib().harc_amd_last_fastq_timing(t, n))
    names = ("context_and_pool", "ingest", "ingest_waiting_for_file_readers", "ingest_device_passes", "reorder", "encode", "stream_files", "total",
             "ingest_bgzf_inflate")
    return {k: float(v) for k, v in zip(names, t)}


COMM_ID_BYTES = 128


def comm_get_id():
    """rank 0 of a multi-GPU run: the bytes every rank hands to HarcAmd.comm_init (== ncclGetUniqueId)"""
    b = C.create_string_buffer(COMM_ID_BYTES)
    _check(lib().harc_amd_comm_get_id(b, COMM_ID_BYTES))
    return b.raw


def compress_fastq_shard(fastq, basedir, readlen, world, rank, comm_spec, num_thr=1, num_chains=0, preserve_order=False,
                         preserve_quality=False, **kw):
    """one rank of `./harc -c -g <world>`: slice of the FASTQ -> exchange -> this GPU's shard files"""
    kw.setdefault("reads_per_chain", 1024)
    p = default_params(readlen, num_thr=num_thr, num_chains=num_chains, **kw)
    _check(lib().harc_amd_compress_fastq_shard_files(C.byref(p), os.fsencode(fastq), os.fsencode(basedir), int(preserve_order),
                                                     int(preserve_quality), world, rank, os.fsencode(comm_spec)))


def merge_shards(basedir, world):
    """after every rank has finished: the whole-job files of the archive (host code)"""
    _check(lib().harc_amd_merge_shard_files(os.fsencode(basedir), world))


def decoder(basedir, num_thr_e, device=0, preserve_order=False, memory_gb=0, ranges=None):
    """== `decoder.out <basedir> <num_thr> <num_thr_e>` (src/decoder.cpp:44-172): output/output.dna;
    preserve_order: the -p chain unpack_order + decoder_preserve + merge_N (harc:183-185).  ranges: one or two (first, count) of output lines, first counted
    from 0 -- output.dna then holds those lines alone, one range after the other (include/harc_amd.h: harc_amd_decoder_range_files)"""
    p = default_params(100, device=device)
    p.decode_memory_gb = memory_gb
    if ranges is None:
        f = lib().harc_amd_decoder_preserve_files if preserve_order else lib().harc_amd_decoder_files
        _check(f(C.byref(p), os.fsencode(basedir), num_thr_e))
        return
    first, count = (C.c_uint64 * len(ranges))(*[a for a, _ in ranges]), (C.c_uint64 * len(ranges))(*[b for _, b in ranges])
    f = lib().harc_amd_decoder_preserve_range_files if preserve_order else lib().harc_amd_decoder_range_files
    _check(f(C.byref(p), os.fsencode(basedir), num_thr_e, len(ranges), first, count))


LINE_NONE = 2 ** 64 - 1      # line_offset_*: the text holds fewer than k newlines


def line_offset_host(text, k):
    """(newlines of `text`, the byte offset at which line k starts: 0 for k = 0, else one past the k-th newline, LINE_NONE when there are fewer) on the host:
    what HarcAmd.line_offset_device is held to (include/harc_amd.h: harc_amd_line_offset_host); no device"""
    out = (C.c_uint64 * 2)()
    _check(lib().harc_amd_line_offset_host(bytes(text), len(text), k, out))
    return int(out[0]), int(out[1])


def line_range_file(path, first_line, n_lines, device=0):
    """the byte range (begin, end) of lines first_line .. first_line + n_lines - 1 (counted from 0) of the text file at `path`, the newlines counted on the GPU
    piece by piece (include/harc_amd.h: harc_amd_line_range_files)"""
    p = default_params(100, device=device)
    out = (C.c_uint64 * 2)()
    _check(lib().harc_amd_line_range_files(C.byref(p), os.fsencode(path), first_line, n_lines, out))
    return int(out[0]), int(out[1])


def qunpack_range_files(packed, out, first_line, n_lines, device=0):
    """qunpack_files for lines first_line .. first_line + n_lines - 1 (counted from 0) alone: only the blocks that hold them are read, decoded and checked"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_qunpack_range_files(C.byref(p), os.fsencode(packed), os.fsencode(out), first_line, n_lines))


def idunpack_range_files(packed, out, first_line, n_lines, device=0):
    """idunpack_files for lines first_line .. first_line + n_lines - 1 (counted from 0) alone: only the blocks that hold them are read, decoded and checked"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_idunpack_range_files(C.byref(p), os.fsencode(packed), os.fsencode(out), first_line, n_lines))


def name_key(line):
    """(offset, length) of the name of `line` (bytes, without its newline): a leading '@' skipped, up to the first space or tab, one trailing "/1" or "/2" of a name
    of at least 3 bytes dropped (include/harc_amd.h: harc_amd_name_key_host); no device"""
    out = (C.c_uint64 * 2)()
    line = bytes(line)
    _check(lib().harc_amd_name_key_host(line, len(line), out))
    return int(out[0]), int(out[1])


def select_flags_host(names, ids):
    """(flags, distinct names, names found): flags[i] = 1 when the name of line i of the id text `ids` is the name of a line of the list `names` (both bytes), on
    the host: what HarcAmd.select_flags_device is held to (include/harc_amd.h: harc_amd_select_flags_host); no device"""
    names, ids = bytes(names), bytes(ids)
    room = ids.count(b"\n") + 1
    flags = (C.c_uint8 * room)()
    n, k, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(lib().harc_amd_select_flags_host(names, len(names), ids, len(ids), flags, C.byref(n), C.byref(k), C.byref(f)))
    return bytes(flags[:n.value]), k.value, f.value


def lines_gather_host(text, flags, stride=0):
    """the lines of `text` whose flag byte is not zero, one behind the other: lines of `stride` bytes each, or (stride 0) lines of any length with their newlines
    (include/harc_amd.h: harc_amd_lines_gather_host); no device"""
    text, flags = bytes(text), bytes(flags)
    out = C.create_string_buffer(len(text) + 1)
    n = C.c_uint64(0)
    _check(lib().harc_amd_lines_gather_host(text, len(text), stride, flags, len(flags), out, len(text), C.byref(n)))
    return out.raw[:n.value]


def motifs_check_host(motifs, k=0):
    """the distinct motifs of the list `motifs` (bytes) under `k` mismatches; HarcAmdError with the reason, which names the line, when the rule refuses the list
    (include/harc_amd.h: harc_amd_motifs_check_host); no device"""
    motifs = bytes(motifs)
    n = C.c_uint64(0)
    _check(lib().harc_amd_motifs_check_host(motifs, len(motifs), k, C.byref(n)))
    return n.value


def motif_flags_host(motifs, dna, readlen, k=0):
    """(flags, hits, found): flags[i] = 1 when a motif of the list matches line i of `dna` (lines of readlen + 1 bytes), hits[j] = 1 when distinct motif j matches a
    line, on the host with byte comparisons: what HarcAmd.motif_flags_device is held to (include/harc_amd.h: harc_amd_motif_flags_host); no device"""
    motifs, dna = bytes(motifs), bytes(dna)
    n_lines = len(dna) // (readlen + 1)
    flags, hit = (C.c_uint8 * (n_lines + 1))(), (C.c_uint8 * 1024)()
    n, f = C.c_uint64(0), C.c_uint64(0)
    _check(lib().harc_amd_motif_flags_host(motifs, len(motifs), k, dna, n_lines, readlen, flags, hit, C.byref(n), C.byref(f)))
    return bytes(flags[:n_lines]), bytes(hit[:n.value]), f.value


def match_files(motifs, dna, out_dna, ids=None, quality=None, out_ids=None, out_quality=None, k=0, pair_records=0, pair_rule="none", device=0):
    """the lines of `dna` whose read matches a motif of the list file `motifs` -> out_dna, with ids and quality the same records of those texts -> out_ids and
    out_quality, matched and gathered on the GPU in one call (include/harc_amd.h: harc_amd_match_files) -> (distinct motifs, motifs found, records selected,
    records, [up to ten motifs not found])"""
    p = default_params(100, device=device)
    st = (C.c_uint64 * 4)()
    missing = C.create_string_buffer(1 << 12)
    enc = lambda x: os.fsencode(x) if x is not None else None
    _check(lib().harc_amd_match_files(C.byref(p), enc(motifs), k, enc(dna), enc(ids), enc(quality), enc(out_dna), enc(out_ids), enc(out_quality), pair_records,
                                      _rule_number(pair_rule) if pair_records else 0, st, missing, len(missing)))
    return int(st[0]), int(st[1]), int(st[2]), int(st[3]), [m for m in missing.value.split(b"\n") if m]


def select_files(names, ids, dna, quality, out_ids, out_dna, out_quality, pair_records=0, pair_rule="none", device=0):
    """the records of the three texts of an archive whose id line carries a name of the list file `names` -> the three out files, selected and gathered on the GPU
    in one call (include/harc_amd.h: harc_amd_select_files) -> (distinct names, names found, records selected, records, [up to ten names not found])"""
    p = default_params(100, device=device)
    st = (C.c_uint64 * 4)()
    missing = C.create_string_buffer(1 << 16)
    _check(lib().harc_amd_select_files(C.byref(p), os.fsencode(names), os.fsencode(ids), os.fsencode(dna), os.fsencode(quality), os.fsencode(out_ids), os.fsencode(out_dna),
                                       os.fsencode(out_quality), pair_records, _rule_number(pair_rule) if pair_records else 0, st, missing, len(missing)))
    return int(st[0]), int(st[1]), int(st[2]), int(st[3]), [m for m in missing.value.split(b"\n") if m]


def fastq_assemble(dna, ids, quality, out, device=0, bgzf=False, third=None):
    """line i of the files `dna` (fixed-length reads), `ids` and `quality` -> record i of the FASTQ file `out` (id, read, the third line, quality), assembled on
    the GPU; the read length is that of the first read (include/harc_amd.h: harc_amd_fastq_assemble_files).  bgzf: `out` is that text as BGZF (a .fastq.gz),
    deflated on the GPU as well (harc_amd_fastq_assemble_files_ex).  third: the rule of the third lines, a name or a number; "same" writes '+' and the id
    without its first byte (harc_amd_fastq_assemble_third_files)"""
    p = default_params(100, device=device)
    if third is not None:
        _check(lib().harc_amd_fastq_assemble_third_files(C.byref(p), os.fsencode(dna), os.fsencode(ids), os.fsencode(quality), os.fsencode(out), 1 if bgzf else 0,
                                                         _third_number(third)))
    elif bgzf:
        _check(lib().harc_amd_fastq_assemble_files_ex(C.byref(p), os.fsencode(dna), os.fsencode(ids), os.fsencode(quality), os.fsencode(out), 1))
    else:
        _check(lib().harc_amd_fastq_assemble_files(C.byref(p), os.fsencode(dna), os.fsencode(ids), os.fsencode(quality), os.fsencode(out)))


def bgzf_bound(n):
    """bytes of BGZF that n bytes of text take at most (every member stored, and the end-of-file marker); host only"""
    return int(lib().harc_amd_bgzf_bound(n))


def bgzf_deflate_host(text, eof=True):
    """the encoder of HarcAmd.bgzf_deflate_device run in a row on the host: the bytes the kernels must write (tests; no device)"""
    cap = bgzf_bound(len(text))
    out = C.create_string_buffer(cap)
    n = C.c_uint64(0)
    _check(lib().harc_amd_bgzf_deflate_host(text, len(text), 1 if eof else 0, out, cap, C.byref(n)))
    return out.raw[:n.value]


def gunzip_host(blob, chunk_bytes=0):
    """any gzip byte string -> (its text, the statistics as a dict): the chunked inflate of HarcAmd.gunzip_device run in a row on the host (tests; no device).
    chunk_bytes: compressed bytes per chunk, 0 = the default (include/harc_amd.h: harc_amd_gunzip_host)"""
    n, st = C.c_uint64(0), GunzipStats()
    _check(lib().harc_amd_gunzip_host(blob, len(blob), chunk_bytes, None, 0, C.byref(n), None))
    out = C.create_string_buffer(n.value + 1)
    _check(lib().harc_amd_gunzip_host(blob, len(blob), chunk_bytes, out, n.value, C.byref(n), C.byref(st)))
    return out.raw[:n.value], st.as_dict()


def gunzip_files(gz, out, device=0):
    """the gzip file `gz` (any gzip, not only BGZF) -> the file `out` holding its text, inflated on the GPU -> the statistics as a dict"""
    p, st = default_params(100, device=device), GunzipStats()
    _check(lib().harc_amd_gunzip_files(C.byref(p), os.fsencode(gz), os.fsencode(out), C.byref(st)))
    return st.as_dict()


def qpack_bound(n_reads, readlen, reads_per_block=0):
    """bytes that n_reads quality lines of readlen take at most as a packed quality file: 32 + blocks * 5 + n_reads * readlen; host only"""
    return int(lib().harc_amd_qpack_bound(n_reads, readlen, reads_per_block))


def qpack_host(text, readlen, reads_per_block=0, header=True):
    """the encoder of HarcAmd.qpack_device run in a row on the host: the bytes the kernels must write (tests; no device).  text: lines of readlen quality
    values and a newline each"""
    n, rem = divmod(len(text), readlen + 1)
    if rem:
        raise HarcAmdError(-1, f"{len(text)} bytes are no multiple of the {readlen + 1} bytes of a line")
    cap = qpack_bound(n, readlen, reads_per_block)
    out = C.create_string_buffer(cap)
    got = C.c_uint64(0)
    _check(lib().harc_amd_qpack_host(text, n, readlen, reads_per_block, 1 if header else 0, out, cap, C.byref(got)))
    return out.raw[:got.value]


def qunpack_host(packed):
    """a packed quality file (with its header) -> its lines, decoded on the host by the functions the kernels compile; HarcAmdError(-1) for damaged input"""
    size = C.c_uint64(0)
    _check(lib().harc_amd_qunpack_host(packed, len(packed), None, 0, C.byref(size)))
    out = C.create_string_buffer(size.value + 1)
    _check(lib().harc_amd_qunpack_host(packed, len(packed), out, size.value, C.byref(size)))
    return out.raw[:size.value]


def qpack_files(quality, out, device=0, spec=None):
    """the quality file `quality` (fixed-length lines) -> the packed quality file `out`, coded on the GPU (include/harc_amd.h: harc_amd_qpack_files).
    spec (a spec string or a QMap): the values are mapped in device memory in front of the coder (harc_amd_qpack_files_ex) -> the statistics as a dict"""
    p = default_params(100, device=device)
    if spec is None:
        _check(lib().harc_amd_qpack_files(C.byref(p), os.fsencode(quality), os.fsencode(out)))
        return None
    m, st = _qmap(spec), QMapStats()
    _check(lib().harc_amd_qpack_files_ex(C.byref(p), os.fsencode(quality), os.fsencode(out), C.byref(m), C.byref(st)))
    return st.as_dict()


def qmap_parse(spec):
    """a spec string ("ill8", "bin:T:H:L", "cap:M", "pblock:R") -> its QMap; HarcAmdError(-1) naming the spec and the field for anything else; host only"""
    m = QMap()
    _check(lib().harc_amd_qmap_parse(spec.encode() if isinstance(spec, str) else spec, C.byref(m)))
    return m


def _qmap(spec):
    return spec if isinstance(spec, QMap) else qmap_parse(spec)


def qmap_host(text, readlen, spec, stats=True):
    """the serial mapper of harc_amd/csrc/qm_block.h over lines of readlen quality values and a newline each: what the kernels are held to (no device).
    -> (the mapped text, the statistics as a dict or None)"""
    n, rem = divmod(len(text), readlen + 1)
    if rem:
        raise HarcAmdError(-1, f"{len(text)} bytes are no multiple of the {readlen + 1} bytes of a line")
    m, st = _qmap(spec), QMapStats()
    out = C.create_string_buffer(len(text) + 1)
    _check(lib().harc_amd_qmap_host(text, n, readlen, C.byref(m), out, C.byref(st) if stats else None))
    return out.raw[:len(text)], (st.as_dict() if stats else None)


def qmap_files(quality, out, spec, device=0):
    """the quality file `quality` -> the file `out` with its values mapped on the GPU (include/harc_amd.h: harc_amd_qmap_files) -> the statistics as a dict"""
    p = default_params(100, device=device)
    m, st = _qmap(spec), QMapStats()
    _check(lib().harc_amd_qmap_files(C.byref(p), os.fsencode(quality), os.fsencode(out), C.byref(m), C.byref(st)))
    return st.as_dict()


def qunpack_files(packed, out, device=0):
    """the packed quality file `packed` -> the quality file `out`, decoded on the GPU"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_qunpack_files(C.byref(p), os.fsencode(packed), os.fsencode(out)))


def idpack_bound(text_bytes, n_lines, lines_per_block=0):
    """bytes that n_lines id lines in text_bytes bytes take at most as a packed id file: 32 + blocks * 9 + text_bytes; host only"""
    return int(lib().harc_amd_idpack_bound(text_bytes, n_lines, lines_per_block))


def idpack_host(text, lines_per_block=0, header=True):
    """the encoder of HarcAmd.idpack_device run in a row on the host: the bytes the kernels must write (tests; no device).  text: id lines, a newline behind each"""
    cap = idpack_bound(len(text), text.count(b"\n"), lines_per_block)
    out = C.create_string_buffer(cap + 1)
    got = C.c_uint64(0)
    _check(lib().harc_amd_idpack_host(text, len(text), lines_per_block, 0 if header else 1, out, cap, C.byref(got)))
    return out.raw[:got.value]


def idunpack_host(packed):
    """a packed id file (with its header) -> its text, decoded on the host by the functions the kernels compile; HarcAmdError(-1) for damaged input"""
    size = C.c_uint64(0)
    _check(lib().harc_amd_idunpack_host(packed, len(packed), None, 0, C.byref(size)))
    out = C.create_string_buffer(size.value + 1)
    _check(lib().harc_amd_idunpack_host(packed, len(packed), out, size.value, C.byref(size)))
    return out.raw[:size.value]


def idpack_files(ids, out, device=0):
    """the id file `ids` -> the packed id file `out`, coded on the GPU (include/harc_amd.h: harc_amd_idpack_files)"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_idpack_files(C.byref(p), os.fsencode(ids), os.fsencode(out)))


def idunpack_files(packed, out, device=0):
    """the packed id file `packed` -> the id file `out`, decoded on the GPU"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_idunpack_files(C.byref(p), os.fsencode(packed), os.fsencode(out)))


def spack_bound(text_bytes, block_bytes=0):
    """bytes that text_bytes bytes take at most as a packed stream file: 32 + text_bytes + 13 * blocks; host only"""
    return int(lib().harc_amd_spack_bound(text_bytes, block_bytes))


def spack_host(text, block_bytes=0, header=True):
    """the encoder of HarcAmd.spack_device run in a row on the host: the bytes the kernels must write (tests; no device).  text: any bytes"""
    cap = spack_bound(len(text), block_bytes)
    out = C.create_string_buffer(cap + 1)
    got = C.c_uint64(0)
    _check(lib().harc_amd_spack_host(text, len(text), block_bytes, 1 if header else 0, out, cap, C.byref(got)))
    return out.raw[:got.value]


def sunpack_host(packed):
    """a packed stream file (with its header) -> its text, decoded on the host by the functions the kernels compile; HarcAmdError(-1) for damaged input"""
    size = C.c_uint64(0)
    _check(lib().harc_amd_sunpack_host(packed, len(packed), None, 0, C.byref(size)))
    out = C.create_string_buffer(size.value + 1)
    _check(lib().harc_amd_sunpack_host(packed, len(packed), out, size.value, C.byref(size)))
    return out.raw[:size.value]


def spack_files(path, out, device=0):
    """the file `path` -> the packed stream file `out`, coded on the GPU (include/harc_amd.h: harc_amd_spack_files)"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_spack_files(C.byref(p), os.fsencode(path), os.fsencode(out)))


def sunpack_files(packed, out, device=0):
    """the packed stream file `packed` -> the file `out`, decoded on the GPU"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_sunpack_files(C.byref(p), os.fsencode(packed), os.fsencode(out)))


def _path_list(paths):
    return (C.c_char_p * len(paths))(*[os.fsencode(x) for x in paths])


def spack_file_list(pairs, device=0):
    """spack_files over (path, out) pairs, one after the other on one side context"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_spack_file_list(C.byref(p), len(pairs), _path_list([a for a, _ in pairs]), _path_list([b for _, b in pairs])))


def sunpack_file_list(pairs, device=0):
    """sunpack_files over (packed, out) pairs, one after the other on one side context"""
    p = default_params(100, device=device)
    _check(lib().harc_amd_sunpack_file_list(C.byref(p), len(pairs), _path_list([a for a, _ in pairs]), _path_list([b for _, b in pairs])))


def text_digest_host(text, first_offset=0, acc=(0, 0, 0)):
    """T = (bytes, newlines, D) of `text` at offset `first_offset` of a whole text, added to `acc`, on the host (include/harc_amd.h: harc_amd_text_digest_host)"""
    a = (C.c_uint64 * 3)(*acc)
    _check(lib().harc_amd_text_digest_host(bytes(text), len(text), first_offset, a))
    return tuple(a)


def text_digest_file(path, device=0):
    """T = (bytes, newlines, D) of the file at `path`, digested on the GPU (include/harc_amd.h: harc_amd_text_digest_files)"""
    p = default_params(100, device=device)
    a = (C.c_uint64 * 3)()
    _check(lib().harc_amd_text_digest_files(C.byref(p), os.fsencode(path), a))
    return tuple(a)


def reads_check_file(dna, device=0):
    """the decoders' output read once on the GPU -> (multiset signature of its reads, T of its text) (include/harc_amd.h: harc_amd_reads_check_files)"""
    p = default_params(100, device=device)
    s, t = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    _check(lib().harc_amd_reads_check_files(C.byref(p), os.fsencode(dna), s, t))
    return tuple(s), tuple(t)


_RECOVERY_STATS = ("files", "bytes", "record_bytes", "blocks", "groups")


def recovery_make_host(files, pct, block_bytes=0, span_blocks=0, group_blocks=0, out=None):
    """the recovery record over the files at `files` -> `out` (default: the first file's name with .hr for its last suffix), in plain C++ on the host; 0: the
    environment's or the default geometry.  -> the stats as a dict (include/harc_amd.h: harc_amd_recovery_make_host)"""
    out = out or os.path.splitext(files[0])[0] + ".hr"
    st = (C.c_uint64 * 5)()
    _check(lib().harc_amd_recovery_make_host(len(files), _path_list(files), pct, block_bytes, span_blocks, group_blocks, os.fsencode(out), st))
    return dict(zip(_RECOVERY_STATS, st), out=out)


def recovery_make_files(files, pct, out=None, device=0):
    """the same record made on the GPU, every file through the pinned ring a span at a time (include/harc_amd.h: harc_amd_recovery_make_files)"""
    out = out or os.path.splitext(files[0])[0] + ".hr"
    p = default_params(100, device=device)
    st = (C.c_uint64 * 5)()
    _check(lib().harc_amd_recovery_make_files(C.byref(p), len(files), _path_list(files), pct, os.fsencode(out), st))
    return dict(zip(_RECOVERY_STATS, st), out=out)


def _recovery_run(call):
    rep, status = C.create_string_buffer(1 << 16), C.c_int32(1)
    rc = call(rep, len(rep), C.byref(status))
    if rc != 0:
        raise HarcAmdError(rc, lib().harc_amd_last_error().decode(errors="replace"))
    return status.value, rep.value.decode(errors="replace").splitlines()


def recovery_repair_host(record, files=None, write=True):
    """the files the record names, next to it, held against it and (write) repaired in place, on the host -> (status, report lines); status 0: every file verifies
    in the end (write=False: nothing at all is damaged).  `files` is not needed: the record names them (include/harc_amd.h: harc_amd_recovery_repair_host)"""
    return _recovery_run(lambda rep, cap, st: lib().harc_amd_recovery_repair_host(os.fsencode(record), 1 if write else 0, rep, cap, st))


def recovery_check_files(record, device=0):
    """-> (status, report lines), every digest taken on the GPU, nothing written (include/harc_amd.h: harc_amd_recovery_check_files)"""
    p = default_params(100, device=device)
    return _recovery_run(lambda rep, cap, st: lib().harc_amd_recovery_check_files(C.byref(p), os.fsencode(record), rep, cap, st))


def recovery_repair_files(record, device=0):
    """-> (status, report lines), the lost blocks rebuilt on the GPU and written in place (include/harc_amd.h: harc_amd_recovery_repair_files)"""
    p = default_params(100, device=device)
    return _recovery_run(lambda rep, cap, st: lib().harc_amd_recovery_repair_files(C.byref(p), os.fsencode(record), rep, cap, st))


def block_digests_host(data, block_bytes):
    """the digests of the blocks of `data`, the last one as short as it is (include/harc_amd.h: harc_amd_block_digests_host)"""
    nb = (len(data) + block_bytes - 1) // block_bytes
    out = (C.c_uint64 * max(nb, 1))()
    if nb:
        _check(lib().harc_amd_block_digests_host(bytes(data), nb, block_bytes, len(data) - (nb - 1) * block_bytes, out))
    return list(out)[:nb]


def gf_combine_host(sources, coef):
    """out[q] = XOR_s coef[q][s] * sources[s] over GF(2^8), on the host's packed words -> list of bytes (include/harc_amd.h: harc_amd_gf_combine_host)"""
    B, ns, e = len(sources[0]), len(sources), len(coef)
    src = [C.create_string_buffer(bytes(s), B) for s in sources]
    out = [C.create_string_buffer(B) for _ in range(e)]
    sp = (C.c_void_p * ns)(*[C.addressof(b) for b in src])
    op = (C.c_void_p * e)(*[C.addressof(b) for b in out])
    _check(lib().harc_amd_gf_combine_host(B, ns, sp, e, op, bytes(bytearray(v for row in coef for v in row))))
    return [b.raw for b in out]


def pack_order(basedir, readlen=100, **kw):
    """== `pack_order.out <basedir>` (src/pack_order.cpp:11-77)"""
    p = default_params(readlen, **kw)
    _check(lib().harc_amd_pack_order_files(C.byref(p), os.fsencode(basedir)))


class HarcAmd:
    """In-memory API: one context = one HIP device + stream."""

    def __init__(self, params):
        self.params = params
        self._ctx = C.c_void_p()
        _check(lib().harc_amd_create(C.byref(params), C.byref(self._ctx)))

    def close(self):
        if self._ctx:
            lib().harc_amd_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_reads_ascii(self, buf, n, stride):
        _check(lib().harc_amd_set_reads_ascii(self._ctx, buf, n, stride))

    def set_reads_ascii_device(self, dptr, n, stride):
        _check(lib().harc_amd_set_reads_ascii_device(self._ctx, C.c_void_p(dptr), n, stride))

    def set_fastq_device(self, dptr, nbytes):
        nrec = C.c_uint64(0)
        _check(lib().harc_amd_set_fastq_device(self._ctx, C.c_void_p(dptr), nbytes, C.byref(nrec)))
        return nrec.value

    def bgzf_inflate_device(self, dptr, nbytes, out_ptr=None, out_capacity=0):
        """BGZF bytes in device memory -> their text at out_ptr (device memory); without out_ptr only the text size. -> text bytes"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_bgzf_inflate_device(self._ctx, C.c_void_p(dptr), nbytes, C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def gunzip_device(self, dptr, nbytes, out_ptr=None, out_capacity=0, chunk_bytes=0):
        """any gzip bytes in device memory -> their text at out_ptr (device memory); without out_ptr only the text size. -> (text bytes, statistics as a dict)"""
        n, st = C.c_uint64(0), GunzipStats()
        _check(lib().harc_amd_gunzip_device(self._ctx, C.c_void_p(dptr), nbytes, chunk_bytes, C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n),
                                            C.byref(st)))
        return n.value, st.as_dict()

    def bgzf_deflate_device(self, d_text, nbytes, out_ptr=None, out_capacity=0, eof=True):
        """text in device memory -> BGZF at out_ptr (device memory), members of 65 280 bytes of text deflated on the GPU, the end-of-file marker behind them
        when eof; without out_ptr only the size. -> bytes of BGZF.  bgzf_bound(nbytes) is always enough capacity"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_bgzf_deflate_device(self._ctx, C.c_void_p(d_text) if d_text else None, nbytes, 1 if eof else 0,
                                                  C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def third_rule_device(self, d_fastq, nbytes):
        """the rule of the third lines of a FASTQ text in device memory (include/harc_amd.h: harc_amd_third_rule_device)
        -> (rule name, records that took part, the AND of their flags: bit 0 bare, 1 same)"""
        n, f = C.c_uint64(0), C.c_uint32(0)
        _check(lib().harc_amd_third_rule_device(self._ctx, C.c_void_p(d_fastq) if d_fastq else None, nbytes, C.byref(n), C.byref(f)))
        return third_rule_of(f.value, n.value), n.value, f.value

    def fastq_assemble_device(self, d_ids, id_bytes, d_dna, d_quality, n, readlen, out_ptr=None, out_capacity=0, third=None):
        """n ids (id_bytes of text, a line each), reads and quality values (n lines of readlen + 1 bytes each) in device memory -> the n FASTQ records at
        out_ptr (device memory); without out_ptr the inputs are only validated.  third: the rule of the third lines, a name or a number. -> bytes of the records"""
        n_out = C.c_uint64(0)
        if third is not None:
            _check(lib().harc_amd_fastq_assemble_third_device(self._ctx, C.c_void_p(d_ids) if d_ids else None, id_bytes, C.c_void_p(d_dna) if d_dna else None,
                                                              C.c_void_p(d_quality) if d_quality else None, n, readlen, C.c_void_p(out_ptr) if out_ptr else None,
                                                              out_capacity, C.byref(n_out), _third_number(third)))
            return n_out.value
        _check(lib().harc_amd_fastq_assemble_device(self._ctx, C.c_void_p(d_ids) if d_ids else None, id_bytes, C.c_void_p(d_dna) if d_dna else None,
                                                    C.c_void_p(d_quality) if d_quality else None, n, readlen, C.c_void_p(out_ptr) if out_ptr else None,
                                                    out_capacity, C.byref(n_out)))
        return n_out.value

    def qpack_device(self, d_text, n_reads, readlen, reads_per_block=0, out_ptr=None, out_capacity=0, header=True):
        """n_reads quality lines of readlen (+ newline) in device memory -> the packed form at out_ptr (device memory), with the 32-byte file header when
        header; without out_ptr only the size. -> bytes.  qpack_bound(n_reads, readlen, reads_per_block) is always enough capacity"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_qpack_device(self._ctx, C.c_void_p(d_text) if d_text else None, n_reads, readlen, reads_per_block, 1 if header else 0,
                                           C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def qmap_device(self, d_text, n_reads, readlen, spec, out_ptr, stats=True):
        """n_reads quality lines of readlen (and a newline each) at device address d_text -> the same text with its values mapped at device address out_ptr
        (d_text itself: in place; else disjoint from it; any alignment).  spec: a spec string or a QMap.  -> the statistics as a dict, or None without them"""
        m, st = _qmap(spec), QMapStats()
        _check(lib().harc_amd_qmap_device(self._ctx, C.c_void_p(d_text) if d_text else None, n_reads, readlen, C.byref(m), C.c_void_p(out_ptr) if out_ptr else None,
                                          C.byref(st) if stats else None))
        return st.as_dict() if stats else None

    def qunpack_device(self, d_packed, nbytes, out_ptr=None, out_capacity=0):
        """a packed quality file in device memory -> its lines at out_ptr (device memory); without out_ptr only their size. -> bytes of text"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_qunpack_device(self._ctx, C.c_void_p(d_packed), nbytes, C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def idpack_device(self, d_text, text_bytes, lines_per_block=0, out_ptr=None, out_capacity=0, header=True):
        """an id text in device memory -> the packed form at out_ptr (device memory), with the 32-byte file header when header; without out_ptr only the
        size. -> bytes.  idpack_bound(text_bytes, lines, lines_per_block) is always enough capacity"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_idpack_device(self._ctx, C.c_void_p(d_text) if d_text else None, text_bytes, lines_per_block, 0 if header else 1,
                                            C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def idunpack_device(self, d_packed, nbytes, out_ptr=None, out_capacity=0):
        """a packed id file in device memory -> its text at out_ptr (device memory); without out_ptr only its size. -> bytes of text"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_idunpack_device(self._ctx, C.c_void_p(d_packed), nbytes, C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def spack_device(self, d_text, text_bytes, block_bytes=0, out_ptr=None, out_capacity=0, header=True):
        """text_bytes bytes in device memory -> the packed stream form at out_ptr (device memory), with the 32-byte file header when header; without out_ptr
        only the size. -> bytes.  spack_bound(text_bytes, block_bytes) is always enough capacity"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_spack_device(self._ctx, C.c_void_p(d_text) if d_text else None, text_bytes, block_bytes, 1 if header else 0,
                                           C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def sunpack_device(self, d_packed, nbytes, out_ptr=None, out_capacity=0):
        """a packed stream file in device memory -> its text at out_ptr (device memory); without out_ptr only its size. -> bytes of text"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_sunpack_device(self._ctx, C.c_void_p(d_packed), nbytes, C.c_void_p(out_ptr) if out_ptr else None, out_capacity, C.byref(n)))
        return n.value

    def set_fastq_bgzf_device(self, dptr, nbytes):
        """set_fastq_device for a BGZF-compressed FASTQ in device memory (inflated on the GPU) -> complete records"""
        nrec = C.c_uint64(0)
        _check(lib().harc_amd_set_fastq_bgzf_device(self._ctx, C.c_void_p(dptr), nbytes, C.byref(nrec)))
        return nrec.value

    def set_reads_packed_device(self, dptr, n):
        _check(lib().harc_amd_set_reads_packed_device(self._ctx, C.c_void_p(dptr), n))

    def set_nreads_ascii(self, buf, n, stride):
        _check(lib().harc_amd_set_nreads_ascii(self._ctx, buf, n, stride))

    def set_nreads_ascii_device(self, dptr, n, stride):
        _check(lib().harc_amd_set_nreads_ascii_device(self._ctx, C.c_void_p(dptr), n, stride))

    def pack_reads_device(self, d_ascii, n, stride, d_out):
        _check(lib().harc_amd_pack_reads_device(self._ctx, C.c_void_p(d_ascii), n, stride, C.c_void_p(d_out)))

    def partition_reads_device(self, d_packed, n, n_buckets, d_out, d_counts):
        _check(lib().harc_amd_partition_reads_device(self._ctx, C.c_void_p(d_packed), n, n_buckets, C.c_void_p(d_out), C.c_void_p(d_counts)))

    def bucket_reads_device(self, d_packed, n, n_buckets, d_out):
        _check(lib().harc_amd_bucket_reads_device(self._ctx, C.c_void_p(d_packed), n, n_buckets, C.c_void_p(d_out)))

    def comm_init(self, comm_id, world, rank):
        """join the RCCL communicator of the run (comm_id from comm_get_id() on rank 0)"""
        _check(lib().harc_amd_comm_init(self._ctx, comm_id, len(comm_id), world, rank))

    def comm_init_mailbox(self, directory, world, rank):
        _check(lib().harc_amd_comm_init_mailbox(self._ctx, os.fsencode(directory), world, rank))

    def comm_barrier(self):
        _check(lib().harc_amd_comm_barrier(self._ctx))

    def comm_destroy(self):
        _check(lib().harc_amd_comm_destroy(self._ctx))

    def shard_exchange(self):
        """bucket the context's own reads, ONE all-to-all(v); -> info tuple (see include/harc_amd.h)"""
        info = (C.c_uint64 * 8)()
        _check(lib().harc_amd_shard_exchange(self._ctx, info))
        return tuple(int(x) for x in info)

    def replicate_exchange(self):
        """design (R): all-gather every rank's slice; reorder() then partitions the chains over the ranks and every rank ends with the
        single-GPU result of the whole job; -> info tuple (see include/harc_amd.h)"""
        info = (C.c_uint64 * 8)()
        _check(lib().harc_amd_replicate_exchange(self._ctx, info))
        return tuple(int(x) for x in info)

    def shard_reset(self):
        """the stages read this context's own slice again (no exchange); results of the last run go"""
        _check(lib().harc_amd_shard_reset(self._ctx))

    def reorder(self):
        _check(lib().harc_amd_reorder(self._ctx))

    def set_stage1_streams(self, temp_dna, flag, pos, order, rc, temp_dna_singleton, order_singleton):
        """a stage-I result from outside (the seven files of reorder.cpp:722-830 as bytes): encode() then runs on it"""
        n_main, n_sing = len(order) // 4, len(order_singleton) // 4
        _check(lib().harc_amd_set_stage1_streams(self._ctx, temp_dna, flag, pos, order, rc, n_main, temp_dna_singleton, order_singleton, n_sing))

    def encode(self):
        _check(lib().harc_amd_encode(self._ctx))

    def pack_order(self):
        _check(lib().harc_amd_pack_order(self._ctx))

    def decode_signature(self):
        """(count, sum, xor) of the reads decoded on the GPU from this context's stage-II streams"""
        sig = (C.c_uint64 * 3)()
        _check(lib().harc_amd_decode_signature(self._ctx, sig))
        return tuple(int(x) for x in sig)

    def input_signature(self):
        sig = (C.c_uint64 * 3)()
        _check(lib().harc_amd_input_signature(self._ctx, sig))
        return tuple(int(x) for x in sig)

    def text_digest_device(self, ptr, nbytes, first_offset=0, acc=(0, 0, 0)):
        """T = (bytes, newlines, D) of the nbytes bytes at `ptr` (device memory, any alignment), byte i at offset first_offset + i of the whole text, added to `acc`"""
        a = (C.c_uint64 * 3)(*acc)
        _check(lib().harc_amd_text_digest_device(self._ctx, C.c_void_p(ptr) if ptr else None, nbytes, first_offset, a))
        return tuple(a)

    def block_digests_device(self, ptr, n_blocks, block_bytes, last_bytes=None):
        """the digests of n_blocks blocks of block_bytes bytes at `ptr` (16-byte aligned), the last of last_bytes (include/harc_amd.h: harc_amd_block_digests_device)"""
        out = (C.c_uint64 * max(n_blocks, 1))()
        _check(lib().harc_amd_block_digests_device(self._ctx, C.c_void_p(ptr) if ptr else None, n_blocks, block_bytes, block_bytes if last_bytes is None else last_bytes, out))
        return list(out)[:n_blocks]

    def gf_combine_device(self, block_bytes, src_ptrs, out_ptrs, coef):
        """out[q] = XOR_s coef[q][s] * src[s] over block_bytes bytes, blocks given as device pointers, coef as rows (include/harc_amd.h: harc_amd_gf_combine_device)"""
        ns, e = len(src_ptrs), len(out_ptrs)
        sp, op = (C.c_void_p * ns)(*src_ptrs), (C.c_void_p * e)(*out_ptrs)
        _check(lib().harc_amd_gf_combine_device(self._ctx, block_bytes, ns, sp, e, op, bytes(bytearray(v for row in coef for v in row))))

    def line_offset_device(self, ptr, nbytes, k):
        """(newlines of the nbytes bytes at `ptr` (device memory, any alignment), the byte offset at which line k starts or LINE_NONE): line_offset_host on the GPU"""
        out = (C.c_uint64 * 2)()
        _check(lib().harc_amd_line_offset_device(self._ctx, C.c_void_p(ptr) if ptr else None, nbytes, k, out))
        return int(out[0]), int(out[1])

    def select_flags_device(self, d_names, names_bytes, d_ids, id_bytes, d_flags):
        """select_flags_host on the GPU: both texts in device memory at any alignment, one flag byte per id line written to d_flags -> (id lines, distinct names,
        names found)"""
        n, k, f = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().harc_amd_select_flags_device(self._ctx, C.c_void_p(d_names) if d_names else None, names_bytes, C.c_void_p(d_ids) if d_ids else None, id_bytes,
                                                  C.c_void_p(d_flags) if d_flags else None, C.byref(n), C.byref(k), C.byref(f)))
        return n.value, k.value, f.value

    def motif_flags_device(self, motifs, d_dna, n_lines, readlen, d_flags, k=0):
        """motif_flags_host on the GPU: n_lines lines of readlen + 1 bytes in device memory at any alignment, one flag byte per line written to d_flags; the list
        `motifs` is host bytes -> (hits, found)"""
        motifs = bytes(motifs)
        hit = (C.c_uint8 * 1024)()
        n, f = C.c_uint64(0), C.c_uint64(0)
        _check(lib().harc_amd_motif_flags_device(self._ctx, motifs, len(motifs), k, C.c_void_p(d_dna) if d_dna else None, n_lines, readlen,
                                                 C.c_void_p(d_flags) if d_flags else None, hit, C.byref(n), C.byref(f)))
        return bytes(hit[:n.value]), f.value

    def lines_gather_device(self, d_text, nbytes, stride, d_flags, n_lines, d_out, capacity):
        """lines_gather_host on the GPU: the flagged lines of the text at d_text -> d_out (device memory, any alignment) -> the bytes written"""
        n = C.c_uint64(0)
        _check(lib().harc_amd_lines_gather_device(self._ctx, C.c_void_p(d_text) if d_text else None, nbytes, stride, C.c_void_p(d_flags) if d_flags else None, n_lines,
                                                  C.c_void_p(d_out) if d_out else None, capacity, C.byref(n)))
        return n.value

    def idmate_rule_device(self, d_a, a_bytes, d_b, b_bytes):
        """the mate rule of two id texts in device memory (any alignment) -> (rule name, pairs, the AND of the pairs' flags)"""
        n, f = C.c_uint64(0), C.c_uint32(0)
        _check(lib().harc_amd_idmate_rule_device(self._ctx, C.c_void_p(d_a) if d_a else None, a_bytes, C.c_void_p(d_b) if d_b else None, b_bytes, C.byref(n), C.byref(f)))
        return _rule_from_flags(f.value, n.value), n.value, f.value

    def idmate_apply_device(self, d_ids, id_bytes, rule):
        """the whole lines of the id text at d_ids (device memory, any alignment) patched in place by `rule` -> lines that did not carry the '1' to replace"""
        bad = C.c_uint64(0)
        _check(lib().harc_amd_idmate_apply_device(self._ctx, C.c_void_p(d_ids) if d_ids else None, id_bytes, _rule_number(rule), C.byref(bad)))
        return bad.value

    def input_order_digest(self):
        """T of the text "read_0\\nread_1\\n..." of the reads the context holds, in input record order"""
        a = (C.c_uint64 * 3)()
        _check(lib().harc_amd_input_order_digest(self._ctx, a))
        return tuple(a)

    def reads_signature_device(self, d_ascii, n, stride):
        sig = (C.c_uint64 * 3)()
        _check(lib().harc_amd_reads_signature_device(self._ctx, C.c_void_p(d_ascii), n, stride, sig))
        return tuple(int(x) for x in sig)

    def stream(self, name, shard=0):
        ptr, ln = C.c_void_p(), C.c_size_t()
        _check(lib().harc_amd_get_stream(self._ctx, STREAMS[name], shard, C.byref(ptr), C.byref(ln)))
        return C.string_at(ptr, ln.value) if ln.value else b""

    def selftest_launch(self, n):
        """(visited, sum of indices mod 2^64) of a thread-per-item launch over n items through the library's launch geometry"""
        v, x = C.c_uint64(0), C.c_uint64(0)
        _check(lib().harc_amd_selftest_launch(self._ctx, n, C.byref(v), C.byref(x)))
        return int(v.value), int(x.value)

    def selftest_index(self, keys, slots_per_read=0, bigthresh=0, want_large=False):
        """the index build of the stages over `keys` (unscrambled u64, ids 0 .. n-1): (cap, nbins, slots, ids, large).  slots is a structured array of
        cap (key u64, start u32, count u32), large the list of (slot << 1) | 1 of the bins of more than 16 keys, or None when not asked for"""
        import numpy as np
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = int(keys.size)
        cap, nbins, nl = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        _check(lib().harc_amd_selftest_index(self._ctx, keys.ctypes.data, n, slots_per_read, bigthresh, 0, C.byref(cap), None, None, None, None, 0, None))
        slots = np.zeros(cap.value, dtype=np.dtype([("key", "<u8"), ("start", "<u4"), ("count", "<u4")]))
        ids = np.zeros(n, dtype=np.uint32)
        large = np.zeros(n // 16 + 16, dtype=np.uint64)
        _check(lib().harc_amd_selftest_index(self._ctx, keys.ctypes.data, n, slots_per_read, bigthresh, 1 if want_large else 0, C.byref(cap), C.byref(nbins),
                                             slots.ctypes.data, ids.ctypes.data, large.ctypes.data, large.size, C.byref(nl)))
        if want_large and nl.value > large.size:
            raise HarcAmdError(-1, "harc_amd_selftest_index lists %d large bins among %d keys" % (nl.value, n))
        return int(cap.value), int(nbins.value), slots, ids, (large[:nl.value].copy() if want_large else None)

    def selftest_contigs(self, flag, pos, L, q, cut=10000000):
        """stage II's contig structure over flag[] (bytes, ord('0') = the read starts a contig) and pos[]: (head, cid, gstart, chead, ncontigs, total,
        fellback) -- fellback says whether a read lay more than `cut` reads behind a contig start and the passes that cut contigs ran"""
        import numpy as np
        flag = np.ascontiguousarray(flag, dtype=np.uint8)
        pos = np.ascontiguousarray(pos, dtype=np.uint8)
        n = int(flag.size)
        if int(pos.size) != n:
            raise HarcAmdError(-1, "selftest_contigs: %d flags, %d positions" % (n, int(pos.size)))
        head = np.zeros(n, dtype=np.uint8)
        cid, chead = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        gstart = np.zeros(n, dtype=np.uint64)
        nc, total, fb = C.c_uint32(0), C.c_uint64(0), C.c_int32(0)
        _check(lib().harc_amd_selftest_contigs(self._ctx, flag.ctypes.data, pos.ctypes.data, n, L, q, cut, head.ctypes.data, cid.ctypes.data, gstart.ctypes.data,
                                               chead.ctypes.data, C.byref(nc), C.byref(total), C.byref(fb)))
        return head, cid, gstart, chead[:nc.value].copy(), int(nc.value), int(total.value), bool(fb.value)

    def stream_digest(self):
        """four 64-bit words over the stage-II streams of the last encode(), folded on the device (params.stream_digest = 1)"""
        d = (C.c_uint64 * 4)()
        _check(lib().harc_amd_stream_digest(self._ctx, d))
        return tuple(int(x) for x in d)

    def counters(self):
        c = Counters()
        _check(lib().harc_amd_get_counters(self._ctx, C.byref(c)))
        return c
