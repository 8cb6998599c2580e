"""Bgzipped FASTQ input on the MI355X: the cases of the emulator suite on real wavefronts (the in-wave and cross-tile scans, the ballot
search, the wide copy), the wide copy at every source and destination alignment, a 100 MB file read through more than ten windows of
many scan tiles each, and the two rejections that return cleanly."""
import os
import zlib

import numpy as np
import pytest

import bam_input_cases as K
import fastq_input_cases as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


def test_gpu_reader_equals_fastx_on_the_emulator_cases(ctx, tmp_path, monkeypatch):
    import test_fastq_input_emu as E
    recs = F.shape_records(1)
    for eol in ('lf', 'crlf', 'mixed'):
        st = E._check_text(ctx, tmp_path, F.text_of(recs, eol, start_blank=True, end_blank=True))
        assert st['records'] == len(recs)
    for args in ((False, False, True), (False, True, False), (True, False, False), (True, True, True)):
        E.test_file_ends(ctx, tmp_path, *args)
    E.test_tiny_files(ctx, tmp_path)
    E.test_max_bases_stops_like_fastx(ctx, tmp_path)
    E.test_truncated_records(ctx, tmp_path)
    E.test_bad_header_and_fasta_record(ctx, tmp_path)
    E.test_open_errors(ctx, tmp_path)
    E.test_header_is_judged_without_the_records_other_lines(ctx, tmp_path)
    E.test_long_fasta_line_is_refused_in_the_first_window(ctx, tmp_path, monkeypatch)
    for block in (65280, 5000, 333):
        E.test_straddling(ctx, tmp_path, monkeypatch, recs, block, True)
    for split in (False, True):
        E.test_window_boundary_behind_a_quality_line_and_inside_crlf(ctx, tmp_path, monkeypatch, split)


def test_gpu_seeded_edits(ctx, tmp_path):
    import test_fastq_input_emu as E
    E.test_seeded_edits(ctx, tmp_path)


def test_gpu_wide_copy_alignment(ctx, tmp_path):
    """64 x 17 short records, base counts 0 ... 63; the name length of each record walks the source start of its bases through every residue
    mod 16 while the destination start (the sum of the counts before) walks through them at another pace. Byte for byte against Fastx."""
    from vacmap_amd.lib import FastqReader, Fastx
    rng = np.random.default_rng(31)
    recs, pairs, src, dst = [], set(), 0, 0
    for i in range(64 * 17):
        n = i % 64
        name = 'w' * (1 + (dst + i // 64 - (src + 3)) % 16)                                     # bases start at (destination residue + round) mod 16
        recs.append((name, F._seq(rng, n, 'ACGTacgtNn'), '+', F._qual(rng, n)))
        src += 1 + len(name) + 1                                                                # '@', the name, '\n'
        pairs.add((src % 16, dst % 16))
        src += n + 1 + 2 + n + 1; dst += n
    assert len(pairs) == 256                                                                    # every source residue with every destination residue
    text = F.text_of(recs, between_blank=False)
    p = str(tmp_path / 'w.fastq.gz')
    open(p, 'wb').write(K.bgzf(text))
    a, b = FastqReader(ctx, p), Fastx(p, lib=ctx.lib)
    try:
        K.same_chunks(K.read_all(a, 4096), K.read_all(b, 4096))
    finally:
        a.close(); b.close()


def test_gpu_many_windows_and_tiles(ctx, tmp_path, monkeypatch):
    """about 100 MB of 15 kb reads in windows of 8 MB: at least 10 windows, 2 000 newline tiles each; per-read checksums equal the generator's"""
    from vacmap_amd.lib import FastqReader
    monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(8 << 20))
    pieces, want = F.scale_text(100 << 20)
    total = sum(len(x) for x in pieces)
    p = str(tmp_path / 's.fastq.gz')
    K.write_bgzf_zlib(p, pieces, level=1)
    rd = FastqReader(ctx, p)
    try:
        got = K.read_checksums(rd)
        st = rd.stats()
    finally:
        rd.close()
    os.remove(p)
    assert len(got) == len(want) and got == want
    assert st['windows'] >= 10 and st['inflated_bytes'] == total and st['records'] == len(want)


def test_gpu_rejects_wrong_crc_and_truncated_file(ctx, tmp_path):
    import test_fastq_input_emu as E
    E.test_bad_members(ctx, tmp_path)                                       # (each reader is closed before the context: _raises)
