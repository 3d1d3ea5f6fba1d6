"""harc_amd -- MI355X (gfx950) implementation of HARC's reorder + encode hot path.

The product is the C-ABI shared library ``libharc_amd.so`` (include/harc_amd.h, sources in harc_amd/csrc).
This package is the thin ctypes binding used by the tests and bench.py; it mirrors the reference's stage
programs (``reorder.out`` / ``encoder.out`` / ``pack_order.out`` <basedir>, harc:65-69,112) and exposes the in-memory API.
There is no CPU fallback: importing works anywhere, every compute call needs a gfx950 device.
"""
from .api import (HarcAmd, HarcAmdError, Params, Counters, default_params, lib, lib_path, reorder, encoder, compress,
                  pack_order, preprocess, decoder, compress_fastq, STREAMS, comm_get_id, compress_fastq_shard, merge_shards, build_id, last_fastq_timing, build_has,
                  fastq_assemble, bgzf_bound, bgzf_deflate_host, GunzipStats, gunzip_host, gunzip_files, qpack_bound, qpack_host, qunpack_host, qpack_files, qunpack_files,
                  QMap, QMapStats, qmap_parse, qmap_host, qmap_files,
                  idpack_bound, idpack_host, idunpack_host, idpack_files, idunpack_files,
                  spack_bound, spack_host, sunpack_host, spack_files, sunpack_files, spack_file_list, sunpack_file_list,
                  text_digest_host, text_digest_file, reads_check_file,
                  compress_fastq_pair, IDMATE_RULES, idmate_rule_host, THIRD_RULES, third_rule_host, third_rule_of, third_rule_name, third_rule_parse, idmate_apply_host, idmate_rule_files, fastq_assemble_pair,
                  LINE_NONE, line_offset_host, line_range_file, qunpack_range_files, idunpack_range_files,
                  name_key, select_flags_host, lines_gather_host, select_files, motifs_check_host, motif_flags_host, match_files,
                  recovery_make_host, recovery_repair_host, recovery_make_files, recovery_check_files, recovery_repair_files, block_digests_host, gf_combine_host)
from ._build import build

__all__ = ["HarcAmd", "HarcAmdError", "Params", "Counters", "default_params", "lib", "lib_path", "reorder", "encoder",
           "compress", "pack_order", "preprocess", "decoder", "compress_fastq", "build", "STREAMS", "comm_get_id", "compress_fastq_shard",
           "merge_shards", "build_id", "last_fastq_timing", "build_has", "fastq_assemble", "bgzf_bound", "bgzf_deflate_host",
           "GunzipStats", "gunzip_host", "gunzip_files",
           "qpack_bound", "qpack_host", "qunpack_host", "qpack_files", "qunpack_files",
           "QMap", "QMapStats", "qmap_parse", "qmap_host", "qmap_files",
           "idpack_bound", "idpack_host", "idunpack_host", "idpack_files", "idunpack_files",
           "spack_bound", "spack_host", "sunpack_host", "spack_files", "sunpack_files", "spack_file_list", "sunpack_file_list",
           "text_digest_host", "text_digest_file", "reads_check_file",
           "compress_fastq_pair", "IDMATE_RULES", "idmate_rule_host", "THIRD_RULES", "third_rule_host", "third_rule_of", "third_rule_name", "third_rule_parse", "idmate_apply_host", "idmate_rule_files", "fastq_assemble_pair",
           "LINE_NONE", "line_offset_host", "line_range_file", "qunpack_range_files", "idunpack_range_files",
           "name_key", "select_flags_host", "lines_gather_host", "select_files", "motifs_check_host", "motif_flags_host", "match_files",
           "recovery_make_host", "recovery_repair_host", "recovery_make_files", "recovery_check_files", "recovery_repair_files", "block_digests_host", "gf_combine_host"]
