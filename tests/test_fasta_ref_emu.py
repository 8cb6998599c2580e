"""The reference FASTA parsed on the device (vm_index_build_fasta_device, lib.Index.from_fasta(reader='native'), driver --ref-reader native) and
gzip / BGZF input of the host parser, on the CPU emulator build of the kernels (tests/emu). The comparator is the host parser on the plain
text: both indexes, saved, are the same .vmx file; fasta_ref_cases.parse states the rule a second time in Python. The emulator runs a
wave's lanes one after the other: test_gpu_fasta_ref.py runs the same cases on real wavefronts."""
import gzip
import os
import zlib

import numpy as np
import pytest

import bam_input_cases as K
import fasta_ref_cases as R


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def VL():
    import vacmap_amd.lib as lib
    return lib


def _small_windows(monkeypatch, window=1 << 16):
    monkeypatch.setenv('VMX_REF_IN_WINDOW', str(window)); monkeypatch.setenv('VMX_BAM_IN_CHUNK', str(1 << 17)); monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(window))


# ---------------------------------------------------------------- 1. the rule's edges in one window

def test_reader_keyword_and_gzip_are_new(VL, ctx, tmp_path):
    """the smallest statement of the feature: reader='native' builds the host's index, and the host reads a gzipped reference"""
    text = R.fasta([(b'c1 d', R.seq(np.random.default_rng(1), 400)), (b'c2', b'acgtnACGTN' * 9)])
    st = R.check_text(VL, ctx, tmp_path, text)
    assert set(st) == {'plain', 'bgzf', 'gzip'} and all(s['windows'] >= 1 for s in st.values())
    with pytest.raises(ValueError):
        VL.Index.from_fasta(ctx, str(tmp_path / 'ref_plain.fa'), reader='gpu', **R.KW)


@pytest.mark.parametrize('name', sorted(R.eol_texts()))
def test_line_ends(VL, ctx, tmp_path, name):
    R.check_text(VL, ctx, tmp_path, R.eol_texts()[name])


@pytest.mark.parametrize('name', sorted(R.header_texts()))
def test_headers(VL, ctx, tmp_path, name):
    text = R.header_texts()[name]
    R.check_text(VL, ctx, tmp_path, text)
    if name in ('no_header', 'empty', 'only_blank'):                       # 0 contigs: the same outcome as the host's, an index without contigs
        p = str(tmp_path / 'ref_plain.fa')
        a, ea = R.build(VL, ctx, p, 'host'); b, eb = R.build(VL, ctx, p, 'native')
        assert ea is None and eb is None and a.nseq == 0 and b.nseq == 0
        a.close(); b.close()


@pytest.mark.parametrize('name', sorted(R.letter_texts()))
def test_letters(VL, ctx, tmp_path, name):
    text = R.letter_texts()[name]
    R.check_text(VL, ctx, tmp_path, text)
    if name == 'blank_inside':                                             # the whitespace-only lines are kept, as the host keeps them
        assert b'   ' in R.parse(text)[0][1] and b' \t ' in R.parse(text)[0][1]


@pytest.mark.parametrize('eof', [True, False])
def test_bgzf_eof_member_present_and_absent(VL, ctx, tmp_path, eof):
    for text in (R.eol_texts()['no_final_nl'], R.eol_texts()['lf']):
        R.check_text(VL, ctx, tmp_path, text, eof=eof, which=('bgzf',))


# ---------------------------------------------------------------- 2. widths, chunks, windows, members

@pytest.mark.parametrize('width', [1, 15, 16, 17, 60, 4095, 4096, 4097])
def test_line_widths(VL, ctx, tmp_path, monkeypatch, width):
    _small_windows(monkeypatch)
    R.check_text(VL, ctx, tmp_path, R.width_text(width))


def test_unwrapped_line_through_small_windows(VL, ctx, tmp_path, monkeypatch):
    """a 200 kb line is never carried: it crosses four windows of 64 KB"""
    _small_windows(monkeypatch)
    text = R.long_line_text()
    st = R.check_text(VL, ctx, tmp_path, text, block=5000)
    assert all(s['windows'] >= len(text) // 65536 for s in st.values())


@pytest.mark.parametrize('at', [4096, 65536])
def test_contig_boundary_at_a_chunk_and_a_window_edge(VL, ctx, tmp_path, monkeypatch, at):
    _small_windows(monkeypatch)
    text = R.boundary_text(at)
    assert text[at:at + 1] == b'>' and text[at - 1:at] == b'\n'
    R.check_text(VL, ctx, tmp_path, text, block=4096)


def test_window_ends_inside_crlf_and_inside_a_header(VL, ctx, tmp_path, monkeypatch):
    _small_windows(monkeypatch)
    st = R.check_text(VL, ctx, tmp_path, R.crlf_split_text(65536), block=4096)
    assert st['plain']['windows'] >= 2 and st['bgzf']['windows'] >= 2
    text = R.header_split_text(65536)
    assert text[65536 - 100:65536 - 96] == b'>c2 '
    R.check_text(VL, ctx, tmp_path, text, block=4096)


@pytest.mark.parametrize('block', [65280, 5000, 333])
def test_bgzf_member_sizes(VL, ctx, tmp_path, monkeypatch, block):
    _small_windows(monkeypatch)
    rng = np.random.default_rng(20)
    text = R.fasta([(b'm%d' % i, R.seq(rng, n, 'ACGTacgtN')) for i, n in enumerate((30000, 7, 0, 41234, 61))]) + b'\r\n'
    if block == 333:
        text = text[:40000]
    st = R.check_text(VL, ctx, tmp_path, text, block=block, level=1 if block == 333 else 6, which=('bgzf',))
    assert st['bgzf']['text_bytes'] == len(text)


def test_header_longer_than_a_window_is_unsupported(VL, ctx, tmp_path, monkeypatch):
    _small_windows(monkeypatch)
    text = R.long_header_text()
    for name, data in R.forms(text).items():
        p = str(tmp_path / ('long_%s.fa' % name))
        open(p, 'wb').write(data)
        idx, e = R.build(VL, ctx, p, 'native')
        assert idx is None and e.code == R.UNSUPPORTED and 'window' in str(e), (name, e)
        host = VL.Index.from_fasta(ctx, p, **R.KW)                       # the host parser takes it
        assert host.names == ['c1', 'c2']
        host.close()


# ---------------------------------------------------------------- 3. bad input: a clean error, never a partial index

def test_bad_compressed_input(VL, ctx, tmp_path):
    rng = np.random.default_rng(21)
    text = R.fasta([(b'c1', R.seq(rng, 9000)), (b'c2', R.seq(rng, 3000))])
    first, rest = text[:3000], text[3000:]
    m0 = K.member(K.deflate(first), first)
    z = K.bgzf(text, 6, block=2000)
    g = gzip.compress(text)
    cases = {'crc.fa.gz': m0 + K.member(K.deflate(rest), rest, crc=zlib.crc32(rest) ^ 4) + K.BGZF_EOF, 'cut_member.fa.gz': z[:len(z) * 2 // 3],
             'cut_gzip.fa.gz': g[:len(g) * 2 // 3]}
    for name, data in cases.items():
        p = str(tmp_path / name)
        open(p, 'wb').write(data)
        for reader in ('native', 'host'):
            idx, e = R.build(VL, ctx, p, reader)
            assert idx is None and e is not None and e.code == -5, (name, reader, e)
    with pytest.raises(VL.VmxError):
        VL.Index.from_fasta(ctx, str(tmp_path / 'missing.fa'), reader='native', **R.KW)


def test_seeded_edits(VL, ctx, tmp_path):
    """120 single edits of a small valid file, plain and bgzipped in turn: both parsers raise, or the two .vmx files are equal"""
    rng = np.random.default_rng(22)
    text = b'\n>e0 c\r\n' + R.wrap(R.seq(rng, 400, 'ACGTacgtN'), 60, b'\r\n') + b'>e1\n>e2\td\n' + R.wrap(R.seq(rng, 150), 17) + b'\n>e3\n' + R.seq(rng, 90)
    outcomes = {'raise': 0, 'same': 0}
    for k, (kind, t) in enumerate(R.edits(text, 120, 5)):
        plain = str(tmp_path / 'e.fa')
        open(plain, 'wb').write(t)
        p = plain
        if k % 2:
            p = str(tmp_path / 'e.fa.gz')
            open(p, 'wb').write(K.bgzf(t, 1, block=400))
        a, ea = R.build(VL, ctx, plain, 'host'); b, eb = R.build(VL, ctx, p, 'native')
        assert (ea is None) == (eb is None), (kind, ea, eb)
        if ea is None:
            assert R.vmx_bytes(a, str(tmp_path / 'a.vmx')) == R.vmx_bytes(b, str(tmp_path / 'b.vmx')), kind
            assert a.names == [n.decode() for n, _ in R.parse(t)]
            a.close(); b.close()
        outcomes['raise' if ea is not None else 'same'] += 1
    print(outcomes)
    assert outcomes['same'] >= 100


# ---------------------------------------------------------------- 4. the driver

def _body(path):
    return [x for x in open(path).read().split('\n') if x and not x.startswith('@PG')]


def test_driver_ref_reader_native_equals_the_default(VL, ctx, tmp_path, monkeypatch, capsys):
    from vacmap_amd import driver
    from test_bam_input_emu import _inputs
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bam, _ = _inputs(tmp_path)
    text = fa.read_bytes()
    refs = {'plain': fa}
    for name, data in (('bgzf', K.bgzf(text, 6, block=4000)), ('gzip', gzip.compress(text))):
        d = tmp_path / name
        d.mkdir()
        refs[name] = d / 'ref.fa.gz'
        refs[name].write_bytes(data)
    common = ['-read', str(bam), '-mode', 'H', '--eqx', '--MD', '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2',
              '-workdir', str(tmp_path / 'wd')]
    real = VL.Index.from_fasta.__func__
    calls = []

    def counted(cls, ctx_, path, k=15, w=10, reader='host'):
        calls.append(reader)
        return real(cls, ctx_, path, k=k, w=w, reader=reader)
    monkeypatch.setattr(VL.Index, 'from_fasta', classmethod(counted))
    out = {}
    for name, ref in refs.items():
        assert driver.main(common + ['-ref', str(ref), '-o', str(tmp_path / (name + '.sam')), '--ref-reader', 'native']) == 0
        out[name] = _body(tmp_path / (name + '.sam'))
    assert calls == ['native'] * 3 and '--ref-reader' not in capsys.readouterr().err

    def boom(*a, **k):
        raise AssertionError('vm_index_build_fasta_device called without --ref-reader native')
    monkeypatch.setattr(ctx.lib.L, 'vm_index_build_fasta_device', boom)
    assert driver.main(common + ['-ref', str(fa), '-o', str(tmp_path / 'host.sam')]) == 0
    want = _body(tmp_path / 'host.sam')
    assert sum(1 for x in want if not x.startswith('@')) >= 6
    for name in refs:
        assert out[name] == want, name


def test_driver_falls_back_on_a_long_header_with_one_line(VL, ctx, tmp_path, monkeypatch, capsys):
    from vacmap_amd import driver
    from test_bam_input_emu import _inputs
    monkeypatch.setattr(VL, '_default', ctx.lib)
    _small_windows(monkeypatch)
    fa, bam, _ = _inputs(tmp_path)
    text = fa.read_bytes().replace(b'>cB\n', b'>cB ' + b'x' * 70000 + b'\n')
    long_fa = tmp_path / 'long.fa'
    long_fa.write_bytes(text)
    common = ['-read', str(bam), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd')]
    capsys.readouterr()
    assert driver.main(common + ['-ref', str(long_fa), '-o', str(tmp_path / 'fb.sam'), '--ref-reader', 'native']) == 0
    err = capsys.readouterr().err
    assert sum(1 for ln in err.split('\n') if '--ref-reader native' in ln) == 1 and str(long_fa) in err and 'window' in err
    assert driver.main(common + ['-ref', str(long_fa), '-o', str(tmp_path / 'host.sam')]) == 0
    assert _body(tmp_path / 'fb.sam') == _body(tmp_path / 'host.sam')
