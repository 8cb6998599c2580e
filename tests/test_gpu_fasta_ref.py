"""The reference FASTA parsed on the MI355X: the cases of the emulator suite on real wavefronts (the ballots over a step's lanes, the in-wave
and cross-tile composition of the chunk maps, the LDS compaction and the wide stores), kept runs at every source and destination
alignment, and 64 MB of 60-column text through windows of 8 MB with many tiles of chunk maps each."""
import os

import pytest

import bam_input_cases as K
import fasta_ref_cases as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def VL():
    import vacmap_amd.lib as lib
    return lib


def test_gpu_rule_edges(VL, ctx, tmp_path):
    import test_fasta_ref_emu as E
    E.test_reader_keyword_and_gzip_are_new(VL, ctx, tmp_path)
    for group in (R.eol_texts(), R.header_texts(), R.letter_texts()):
        for name in sorted(group):
            R.check_text(VL, ctx, tmp_path, group[name])
    for eof in (True, False):
        E.test_bgzf_eof_member_present_and_absent(VL, ctx, tmp_path, eof)


def test_gpu_widths_windows_and_members(VL, ctx, tmp_path, monkeypatch):
    import test_fasta_ref_emu as E
    for width in (1, 15, 16, 17, 60, 4095, 4096, 4097):
        E.test_line_widths(VL, ctx, tmp_path, monkeypatch, width)
    E.test_unwrapped_line_through_small_windows(VL, ctx, tmp_path, monkeypatch)
    for at in (4096, 65536):
        E.test_contig_boundary_at_a_chunk_and_a_window_edge(VL, ctx, tmp_path, monkeypatch, at)
    E.test_window_ends_inside_crlf_and_inside_a_header(VL, ctx, tmp_path, monkeypatch)
    for block in (65280, 5000, 333):
        E.test_bgzf_member_sizes(VL, ctx, tmp_path, monkeypatch, block)
    E.test_header_longer_than_a_window_is_unsupported(VL, ctx, tmp_path, monkeypatch)


def test_gpu_bad_input_and_seeded_edits(VL, ctx, tmp_path):
    import test_fasta_ref_emu as E
    E.test_bad_compressed_input(VL, ctx, tmp_path)
    E.test_seeded_edits(VL, ctx, tmp_path)


def test_gpu_kept_runs_at_every_alignment(VL, ctx, tmp_path):
    text, pairs = R.alignment_text()
    assert len(pairs) == 256                                                # every source residue with every destination residue
    R.check_text(VL, ctx, tmp_path, text)


def test_gpu_many_windows_and_tiles(VL, ctx, tmp_path, monkeypatch):
    """about 64 MB of 60-column FASTA, 5 contigs (one of 333 bases), in windows of 8 MB: 2 048 chunk maps = 8 tiles per window; the plain and
    the bgzipped file give the host parser's .vmx file"""
    monkeypatch.setenv('VMX_REF_IN_WINDOW', str(8 << 20)); monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(8 << 20))
    pieces = R.scale_text(64 << 20)
    total = sum(len(x) for x in pieces)
    plain, bg = str(tmp_path / 's.fa'), str(tmp_path / 's.fa.gz')
    with open(plain, 'wb') as f:
        for x in pieces:
            f.write(x)
    K.write_bgzf_zlib(bg, pieces, level=1)
    del pieces
    kw = dict(k=15, w=10)
    host = VL.Index.from_fasta(ctx, plain, **kw)
    want = R.vmx_bytes(host, str(tmp_path / 'host.vmx'))
    assert host.nseq == 5 and 333 in host.lens
    host.close()
    for p in (plain, bg):
        idx = VL.Index.from_fasta(ctx, p, reader='native', **kw)
        st = idx.build_stats
        try:
            assert R.vmx_bytes(idx, str(tmp_path / 'got.vmx')) == want, p
        finally:
            idx.close()
        assert st['windows'] >= 8 and st['text_bytes'] == total and st['contigs'] == 5, st
    for p in (plain, bg, str(tmp_path / 'host.vmx'), str(tmp_path / 'got.vmx')):
        os.remove(p)
