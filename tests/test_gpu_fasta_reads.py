"""FASTA reads on the MI355X (lib.FastqReader(fasta=True)): the cases of the emulator suite on real wavefronts (the in-wave and cross-tile
state scans, the ballot search, the LDS compaction of the copy by text position), the copy at every source and destination alignment, a
16 MB file of one-line and wrapped reads through more than ten windows of many line tiles each, and one record carried over more than ten
windows."""
import os
import zlib

import numpy as np
import pytest

import bam_input_cases as K
import fasta_reads_cases as A
import fastq_input_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


def test_gpu_reader_equals_fastx_on_the_emulator_cases(ctx, tmp_path, monkeypatch):
    import test_fasta_reads_emu as E
    recs = A.shape_records(1)
    E.test_rule_in_python_equals_fastx(ctx, tmp_path, recs)
    for eol in ('lf', 'crlf', 'mixed'):
        E.test_shapes(ctx, tmp_path, recs, eol)
    E.test_rule_texts(ctx, tmp_path)
    for args in ((False, False, True), (False, True, False), (True, False, False), (True, True, True)):
        E.test_file_ends(ctx, tmp_path, *args)
    E.test_file_ends_on_a_header_line_and_short_texts(ctx, tmp_path)
    E.test_mixed_files(ctx, tmp_path)
    E.test_truncated_fastq_still_raises(ctx, tmp_path)
    E.test_bad_headers(ctx, tmp_path)
    E.test_flags(ctx, tmp_path)
    for eol in ('lf', 'mixed'):
        E.test_fastq_through_the_general_parser(ctx, tmp_path, eol)


def test_gpu_windows(ctx, tmp_path, monkeypatch):
    import test_fasta_reads_emu as E
    recs = A.shape_records(1)
    for eof in (True, False):
        E.test_last_member_alone_behind_a_carried_record(ctx, tmp_path, monkeypatch, eof)
    for block in (65280, 5000, 333):
        E.test_windows(ctx, tmp_path, monkeypatch, recs, block)
    for kind in ('start', 'crlf', 'header'):
        E.test_window_boundaries(ctx, tmp_path, monkeypatch, kind)
    for wrapped in (True, False):
        E.test_one_record_longer_than_ten_windows(ctx, tmp_path, monkeypatch, wrapped)
    E.test_plain_gzip_with_the_device_inflate(ctx, tmp_path, monkeypatch)


def test_gpu_driver_input(ctx, tmp_path, capsys):
    import test_fasta_reads_emu as E
    E.test_driver_input_reads_fasta_on_the_device(ctx, tmp_path, capsys)


def test_gpu_copy_alignment(ctx, tmp_path):
    """64 x 17 records of one body line, 0 ... 63 bases: every source residue mod 16 of a body line meets every destination residue, and a
    4 096-byte chunk holds many short pieces. Byte for byte against Fastx."""
    from vacmap_amd.lib import FastqReader, Fastx
    recs, pairs = A.alignment_records()
    assert len(pairs) == 256                                                                    # every source residue with every destination residue
    p = str(tmp_path / 'w.fa.gz')
    open(p, 'wb').write(K.bgzf(A.text_of(recs, between_blank=False)))
    a, b = FastqReader(ctx, p, fasta=True), Fastx(p, lib=ctx.lib)
    try:
        K.same_chunks(K.read_all(a, 4096), K.read_all(b, 4096))
    finally:
        a.close(); b.close()


def test_gpu_many_windows_and_tiles(ctx, tmp_path, monkeypatch):
    """about 16 MB of 15 kb reads, every second one wrapped at 60, in windows of 1 MB: at least 10 windows, tens of 256-line tiles in each;
    per-read checksums equal the generator's"""
    from vacmap_amd.lib import FastqReader
    monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(1 << 20))
    pieces, want = A.scale_text(16 << 20)
    total = sum(len(x) for x in pieces)
    p = str(tmp_path / 's.fa.gz')
    K.write_bgzf_zlib(p, pieces, level=1)
    rd = FastqReader(ctx, p, fasta=True)
    try:
        got = K.read_checksums(rd)
        st = rd.stats()
    finally:
        rd.close()
    os.remove(p)
    assert len(got) == len(want) and got == want
    assert st['windows'] >= 10 and st['inflated_bytes'] == total and st['records'] == len(want)
    assert total // 2 // 61 // st['windows'] >= 20 * 256                                        # lines per window: tens of tiles


@pytest.mark.parametrize('wrapped', [True, False])
def test_gpu_one_long_record(ctx, tmp_path, monkeypatch, wrapped):
    """one record of 3 Mb in windows of 256 KB: carried over more than ten windows, equal to the generator"""
    from vacmap_amd.lib import FastqReader
    monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(256 << 10))
    text, bases = A.long_record_text(3 << 20, wrapped)
    p = str(tmp_path / 'l.fa.gz')
    open(p, 'wb').write(K.bgzf(text, 1))
    rd = FastqReader(ctx, p, fasta=True)
    try:
        got = F.chunk_records(K.read_all(rd, 4096))
        st = rd.stats()
    finally:
        rd.close()
    assert st['windows'] > 10 and st['inflated_bytes'] == len(text)
    assert [r[:2] for r in got] == [(b'first', b''), (b'big', b'one'), (b'last', b'')] and got[1][3] == b''
    assert zlib.crc32(got[1][2]) == zlib.crc32(bases) and got[0][2] == b'ACGT' and got[2][2] == b'GG'
