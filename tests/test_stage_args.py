"""harc_amd_stage's own argument handling, without a GPU: every row below is refused before a file or a device is touched.  One row per command for a call that
is one word short, and one for every word the program reads strictly (the decimal numbers, the mate rules, the shard mode, the word `check`, a mapping of
quality values).  Status 2 and the one line on stderr, byte for byte; nothing on stdout."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = os.path.join(ROOT, "harc_amd", "harc_amd_stage")

USAGE = "usage: " + STAGE + " reorder|encoder|compress|pack_order <basedir> <readlen> [num_thr] [num_chains]"
FILE = "needs <file> [<device>]"
RECORD = "needs <record> [<device>]"
IN_OUT = "needs <in> <device> <out>"
STREAMS = "needs <device> <in> <out> [<in> <out> ...]"
LINE_RANGE = "line_range needs <file> <first> <count> [<device>], lines counted from 0"
UNPACK_RANGE = "needs <packed> <device> <out> <first> <count>, lines counted from 0"
DECODER_RANGE = "decoder_range needs <basedir> <ignored> <num_thr_e> <first> <count> [<first> <count>], lines counted from 0"
DECODER_PRESERVE_RANGE = "decoder_preserve_range needs <basedir> <ignored> <num_thr_e> <memory_gb> <first> <count> [<first> <count>], lines counted from 0"
RECOVERY_MAKE = "recovery_make needs <pct 1..100> <device> <out> <file> [<file> ...]"
FASTQ_OUT = "fastq_out needs <dna> <ignored> <id> <quality> <out> [bgzf] [third]"
FASTQ_OUT_PAIR = "fastq_out_pair needs <dna> <ignored> <id> <quality> <out1> <out2> <records> <rule> [bgzf] [third]"
SELECT = "records_select needs <names> <device> <ids> <dna> <quality> <out_ids> <out_dna> <out_quality> [pair <records> <none|same|slash|space>]"
PAIR = "compressfq_pair needs <fastq1> <fastq2> <num_thr> <num_chains> <num_steps> <preserve_quality> [check]"
SHARD = "compressfq_shard needs <fastq> <num_thr> <num_chains> <num_steps> <p> <q> <world> <rank> <comm_spec> [device]"
NO_SPEC = "qmap_parse: 'nonsense': the name 'nonsense' is none of ill8, bin, cap and pblock"

SEL = "records_select no.names 0 no.id no.dna no.quality o.id o.dna o.quality"
OUT_PAIR = "fastq_out_pair no.dna 0 no.id no.quality o.1 o.2"
SHARD_WORDS = "compressfq_shard no.dir 100 no.fastq 8 0 0 True True 2 0 rccl:no.id"

ROWS = [
    # ---- one word too few, a row per command
    ("quality_spec", "quality_spec needs <spec>"),
    ("text_digest", "text_digest " + FILE),
    ("reads_check", "reads_check " + FILE),
    ("id_mates no.a", "id_mates needs <a> <b> [<device>]"),
    ("recovery_make 10 0 o.hr", RECOVERY_MAKE),
    ("recovery_check", "recovery_check " + RECORD),
    ("recovery_repair", "recovery_repair " + RECORD),
    ("merge_shards no.dir", USAGE),
    ("fastq_out no.dna 0 no.id no.quality", FASTQ_OUT),
    (OUT_PAIR + " 2", FASTQ_OUT_PAIR),
    ("quality_pack no.quality 0", "quality_pack " + IN_OUT),
    ("quality_unpack no.hq 0", "quality_unpack " + IN_OUT),
    ("quality_map no.quality 0 o.quality", "quality_map needs <quality> <device> <out> <spec>"),
    ("gunzip no.gz 0", "gunzip needs <gz> <device> <out>"),
    ("streams_pack 0 no.in", "streams_pack " + STREAMS),
    ("streams_unpack 0 no.in", "streams_unpack " + STREAMS),
    ("id_pack no.id 0", "id_pack " + IN_OUT),
    ("id_unpack no.hi 0", "id_unpack " + IN_OUT),
    ("line_range no.id 0", LINE_RANGE),
    (SEL.rsplit(" ", 1)[0], SELECT),
    ("quality_unpack_range no.hq 0 o.quality 0", "quality_unpack_range " + UNPACK_RANGE),
    ("id_unpack_range no.hi 0 o.id 0", "id_unpack_range " + UNPACK_RANGE),
    ("decoder_range no.dir 0 1 0", DECODER_RANGE),
    ("decoder_preserve_range no.dir 0 1 7 0", DECODER_PRESERVE_RANGE),
    ("preprocess no.dir 100", "preprocess needs <fastq>"),
    ("compressfq no.dir 100", "compressfq needs <fastq>"),
    ("compressfq_pair no.dir 100 no.1 no.2 8 0 0", PAIR),
    (SHARD_WORDS.rsplit(" ", 1)[0], SHARD),
    ("decoder no.dir", USAGE),
    ("decoder_preserve no.dir", USAGE),
    ("reorder no.dir", USAGE),
    ("encoder no.dir", USAGE),
    ("compress no.dir", USAGE),
    ("pack_order no.dir", USAGE),
    # ---- a list of pairs that is half a pair long
    ("streams_pack 0 no.in o.hs no.in2", "streams_pack " + STREAMS),
    ("streams_unpack 0 no.hs o.out no.hs2", "streams_unpack " + STREAMS),
    # ---- a number that is none
    ("line_range no.id x 1", LINE_RANGE),
    ("line_range no.id 0 -1", LINE_RANGE),
    ("line_range no.id 0 1x", LINE_RANGE),
    ("quality_unpack_range no.hq 0 o.quality 1x 2", "quality_unpack_range " + UNPACK_RANGE),
    ("quality_unpack_range no.hq 0 o.quality 1 +2", "quality_unpack_range " + UNPACK_RANGE),
    ("id_unpack_range no.hi 0 o.id -1 2", "id_unpack_range " + UNPACK_RANGE),
    ("id_unpack_range no.hi 0 o.id 1 two", "id_unpack_range " + UNPACK_RANGE),
    ("decoder_range no.dir 0 1 0 x", DECODER_RANGE),
    ("decoder_range no.dir 0 1 0 1 2", DECODER_RANGE),
    ("decoder_range no.dir 0 1 0 1 2 -3", DECODER_RANGE),
    ("decoder_preserve_range no.dir 0 1 7 0x 1", DECODER_PRESERVE_RANGE),
    ("decoder_preserve_range no.dir 0 1 7 0 1 2", DECODER_PRESERVE_RANGE),
    ("decoder_preserve_range no.dir 0 1 7 0 1 2 3x", DECODER_PRESERVE_RANGE),
    (SEL + " pair x same", SELECT),
    (SEL + " pair 0 same", SELECT),
    (SEL + " pair -2 same", SELECT),
    (SEL + " pair 2", SELECT),
    ("recovery_make 0 0 o.hr no.file", RECOVERY_MAKE),
    ("recovery_make 101 0 o.hr no.file", RECOVERY_MAKE),
    ("recovery_make 10x 0 o.hr no.file", RECOVERY_MAKE),
    ("recovery_make x 0 o.hr no.file", RECOVERY_MAKE),
    (OUT_PAIR + " 2x space", "fastq_out_pair: <records> must be a decimal number (got '2x')"),
    (OUT_PAIR + " two space bgzf third", "fastq_out_pair: <records> must be a decimal number (got 'two')"),
    # ---- a rule word that names no rule
    (OUT_PAIR + " 2 mate", "fastq_out_pair: <rule> must be none, same, slash or space (got 'mate')"),
    (OUT_PAIR + " 2 Same bgzf", "fastq_out_pair: <rule> must be none, same, slash or space (got 'Same')"),
    (SEL + " pair 2 mate", SELECT),
    (SEL + " pairs 2 same", SELECT),
    # ---- the trailing words of fastq_out (tests/test_harc_third.py has the rest)
    ("fastq_out no.dna 0 no.id no.quality o.fastq gz", "fastq_out: behind <out> only 'bgzf', 'third' or 'bgzf third' can follow (got 'gz')"),
    (OUT_PAIR + " 2 same third bgzf", "fastq_out_pair: behind <rule> only 'bgzf', 'third' or 'bgzf third' can follow (got 'bgzf')"),
    # ---- a shard mode that is none
    (SHARD_WORDS + " 0 bukket", "compressfq_shard: mode 'bukket' is neither 'bucket' nor 'replicate'"),
    (SHARD_WORDS + " 0 Replicate", "compressfq_shard: mode 'Replicate' is neither 'bucket' nor 'replicate'"),
    # ---- a word other than check
    ("compressfq no.dir 100 no.fastq 8 0 0 True True chek", "compressfq: the argument behind <preserve_quality> can only be 'check' (got 'chek')"),
    ("compressfq_pair no.dir 100 no.1 no.2 8 0 0 True Check", "compressfq_pair: the argument behind <preserve_quality> can only be 'check' (got 'Check')"),
    # ---- a spec that names no mapping of quality values
    ("quality_spec nonsense", NO_SPEC),
    ("quality_spec ill8 more", "quality_spec needs <spec>"),
    ("quality_map no.quality 0 o.quality nonsense", NO_SPEC),
    ("quality_pack no.quality 0 o.hq nonsense", NO_SPEC),
    # ---- fewer than four words, and a command there is none of
    ("", USAGE),
    ("reorder", USAGE),
    ("bogus no.dir", USAGE),
    ("bogus no.dir 100", "unknown stage bogus"),
    ("bogus no.dir 100 8 0", "unknown stage bogus"),
]


@pytest.mark.parametrize("words, line", ROWS, ids=[(w or "no command").replace(" ", "_") for w, _ in ROWS])
def test_the_call_is_refused_with_status_2_and_its_line(tmp_path, words, line):
    r = subprocess.run([STAGE] + words.split(), cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", line + "\n")
    assert os.listdir(tmp_path) == []


def test_every_row_is_one_of_a_kind():
    assert len({w for w, _ in ROWS}) == len(ROWS)
