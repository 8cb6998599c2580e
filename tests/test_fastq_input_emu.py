"""Bgzipped FASTQ input (vm_fastq_reader_*, lib.FastqReader, driver --fastx-reader native) on the CPU emulator build of the kernels (tests/emu).
The reference is lib.Fastx (zlib + vm_fastx_read) on the same BGZF file, chunk by chunk; fastq_input_cases.parse states the rule a second
time in Python. The emulator runs a wave's lanes one after the other: test_gpu_fastq_input.py runs the same cases on real wavefronts."""
import gzip
import os
import zlib

import numpy as np
import pytest

import bam_input_cases as K
import fastq_input_cases as F

SIZES = (1, 3, 64, 4096)


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def shape_recs():
    return F.shape_records(1)


def _small_windows(monkeypatch, chunk=1 << 17, maxinf=1 << 16):
    monkeypatch.setenv('VMX_BAM_IN_CHUNK', str(chunk)); monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(maxinf))


def _check_file(ctx, path, sizes=SIZES):
    """FastqReader and Fastx give equal chunks at every max_reads; returns the reader's last statistics"""
    from vacmap_amd.lib import FastqReader, Fastx
    st = None
    for n in sizes:
        ref = Fastx(path, lib=ctx.lib)
        want = K.read_all(ref, n); ref.close()
        rd = FastqReader(ctx, path)
        try:
            K.same_chunks(K.read_all(rd, n), want)
            st = rd.stats()
        finally:
            rd.close()
    return st


def _check_text(ctx, tmp_path, text, block=65280, eof=True, sizes=SIZES, level=6):
    p = str(tmp_path / 'x.fastq.gz')
    with open(p, 'wb') as f:
        f.write(K.bgzf(text, level, block=block, eof=eof))
    return _check_file(ctx, p, sizes)


# ---------------------------------------------------------------- 1. shapes

def test_rule_in_python_equals_fastx(ctx, tmp_path, shape_recs):
    """the second statement of the rule agrees with the reference reader on the shapes text (so `parse` may judge prefixes below)"""
    from vacmap_amd.lib import Fastx
    text = F.text_of(shape_recs, 'mixed', start_blank=True, end_blank=True)
    p = str(tmp_path / 'p.fastq.gz')
    open(p, 'wb').write(K.bgzf(text))
    rd = Fastx(p, lib=ctx.lib)
    got = F.chunk_records(K.read_all(rd, 1000)); rd.close()
    want, err = F.parse(text)
    assert err is None and got == want and len(got) == len(shape_recs)
    assert (b'', b'x') in [(r[0], r[1]) for r in got] and any(len(r[2]) == 200000 for r in got) and any(r[3][:1] == b'@' for r in got)


@pytest.mark.parametrize('eol', ['lf', 'crlf', 'mixed'])
def test_shapes(ctx, tmp_path, shape_recs, eol):
    st = _check_text(ctx, tmp_path, F.text_of(shape_recs, eol, start_blank=True, end_blank=True))
    assert st['records'] == len(shape_recs)


@pytest.mark.parametrize('final_nl,end_blank,eof', [(False, False, True), (False, True, False), (True, False, False), (True, True, True)])
def test_file_ends(ctx, tmp_path, final_nl, end_blank, eof):
    """the last line with and without its newline, blank lines at the end, the BGZF EOF member present and absent"""
    recs = F.shape_records(2, long_read=0)
    for eol in ('lf', 'crlf'):
        _check_text(ctx, tmp_path, F.text_of(recs, eol, end_blank=end_blank, final_nl=final_nl), eof=eof, sizes=(3, 4096))


def test_tiny_files(ctx, tmp_path):
    from vacmap_amd.lib import FastqReader
    for text in (b'@a\nA\n+\nI', b'@a\nA\n+\nI\n', b'@a\n\n+\n\n', b'\n\n \n', b'', b'@ x\r\nacgt\r\n+\r\n@@@@\r\n'):
        _check_text(ctx, tmp_path, text, sizes=(1, 4096))
    p = str(tmp_path / 'one.fastq.gz')
    open(p, 'wb').write(K.bgzf(b'@ x\r\nacgtn\r\n+\r\n@@@@@\r\n'))
    rd = FastqReader(ctx, p)
    ch = rd.read(10); assert rd.read(10) is None; rd.close()
    assert bytes(ch['names']) == b'' and bytes(ch['comments']) == b'x' and bytes(ch['seqs']) == b'ACGTN' and bytes(ch['quals']) == b'@@@@@'


# ---------------------------------------------------------------- 2. straddling members, chunks and windows

@pytest.mark.parametrize('block,windows', [(65280, False), (5000, False), (333, False), (65280, True), (5000, True), (333, True)])
def test_straddling(ctx, tmp_path, monkeypatch, shape_recs, block, windows):
    """the same stream in members of 65 280, 5 000 and 333 bytes, then through windows of 64 KB: records and each of their four lines cross
    members and windows, and the 200 kb read is larger than a window"""
    if windows:
        _small_windows(monkeypatch)
    text = F.text_of(shape_recs, 'mixed', start_blank=True, end_blank=True)
    st = _check_text(ctx, tmp_path, text, block=block, level=1 if block == 333 else 6)
    assert st['inflated_bytes'] == len(text) and st['records'] == len(shape_recs)
    if windows:
        assert st['windows'] >= len(text) // 65536


@pytest.mark.parametrize('crlf_split', [False, True])
def test_window_boundary_behind_a_quality_line_and_inside_crlf(ctx, tmp_path, monkeypatch, crlf_split):
    """members of 4 096 bytes and windows of 65 536: the first window ends at byte 65 536 exactly, which is the byte behind a quality line's
    newline, or the newline of its '\\r\\n'"""
    _small_windows(monkeypatch)
    text = F.boundary_text(65536, crlf_split)
    st = _check_text(ctx, tmp_path, text, block=4096)
    assert st['windows'] >= 2


# ---------------------------------------------------------------- 3. max_bases

def test_max_bases_stops_like_fastx(ctx, tmp_path):
    from vacmap_amd.lib import FastqReader, Fastx
    rng = np.random.default_rng(6)
    recs = [('m%d' % i, F._seq(rng, n), '+', F._qual(rng, n)) for i, n in enumerate(rng.integers(50, 2000, 50))]
    p = str(tmp_path / 'm.fastq.gz')
    open(p, 'wb').write(K.bgzf(F.text_of(recs), 6, block=20000))
    for mr, mb in ((1000, 5000), (7, 3000), (1000, 1)):
        a, b = FastqReader(ctx, p), Fastx(p, lib=ctx.lib)
        K.same_chunks(K.read_all(a, mr, mb), K.read_all(b, mr, mb))
        a.close(); b.close()


# ---------------------------------------------------------------- 4. errors

def _raises(ctx, path, n=3):
    """(records handed out before the error, the VmxError) of FastqReader on path"""
    from vacmap_amd.lib import FastqReader, VmxError
    got, rd = [], None
    try:
        rd = FastqReader(ctx, path)
        while True:
            ch = rd.read(n)
            if ch is None:
                return F.chunk_records(got), None
            got.append(ch)
    except VmxError as e:
        return F.chunk_records(got), e
    finally:
        if rd is not None:
            rd.close()


def _good(k=12, seed=3):
    rng = np.random.default_rng(seed)
    return [('g%d c%d' % (i, i), F._seq(rng, 100 + i), '+', F._qual(rng, 100 + i)) for i in range(k)]


def test_truncated_records(ctx, tmp_path):
    base = F.text_of(_good(), between_blank=False)
    for tail in (b'@last\n', b'@last\nACGT\n', b'@last\nACGT\n+\n', b'@last', b'@last\nACGT\n+'):
        p = str(tmp_path / 't.fastq.gz')
        open(p, 'wb').write(K.bgzf(base + tail, 6, block=700))
        got, e = _raises(ctx, p)
        assert e is not None and e.code == -5 and 'truncated' in str(e), (tail, e)
        assert got == F.parse(base)[0][:len(got)]
        from vacmap_amd.lib import Fastx, VmxError
        with pytest.raises(VmxError):
            K.read_all(Fastx(p, lib=ctx.lib), 100)


def test_bad_header_and_fasta_record(ctx, tmp_path):
    from vacmap_amd.lib import Fastx, VmxError
    a, b = F.text_of(_good(7, 1), between_blank=False), F.text_of(_good(5, 2), between_blank=False)
    p = str(tmp_path / 'h.fastq.gz')
    long_line = b'xyz ' + b'Q' * 100
    open(p, 'wb').write(K.bgzf(a + long_line + b'\r\nACGT\n+\nIIII\n' + b, 6, block=500))
    got, e = _raises(ctx, p, 1)                                         # (a call that meets the error returns only the error, as vm_fastx_read)
    ref = Fastx(p, lib=ctx.lib)
    with pytest.raises(VmxError) as he:
        K.read_all(ref, 100)
    ref.close()
    assert e is not None and e.code == -5 and 'not FASTA/FASTQ: ' + long_line[:40].decode() in str(e) and str(e).endswith(long_line[:40].decode())
    assert 'not FASTA/FASTQ: ' + long_line[:40].decode() in str(he.value)
    assert got == F.parse(a)[0]
    open(p, 'wb').write(K.bgzf(a + b'xy\r\nACGT\n+\nIIII\n' + b))
    got, e = _raises(ctx, p, 1)                                         # (a call that meets the error returns only the error, as vm_fastx_read)
    assert e.code == -5 and str(e).endswith('not FASTA/FASTQ: xy')
    open(p, 'wb').write(K.bgzf(a + b'>fa\nACGT\n' + b, 6, block=500))
    got, e = _raises(ctx, p, 1)                                         # (a call that meets the error returns only the error, as vm_fastx_read)
    assert e is not None and e.code == -7 and 'record 8' in str(e) and 'host reader' in str(e)
    assert got == F.parse(a)[0]


SHORT_FASTA = (b'>c1 d\nACGTACGT\n', b'>c1\nACGT\nACGT\n', b'>c1', b'>c1 d\n', b'\n \n>c1\nacgt', b'>c1\nAC\n>c2\nGT\n')


def test_header_is_judged_without_the_records_other_lines(ctx, tmp_path):
    """a FASTA of one, two or three lines is refused at open as FASTA (not as a truncated FASTQ record); a '>' or 'x' header inside the file's
    last three lines gives the same error as one in the middle"""
    from vacmap_amd.lib import FastqReader, Fastx, VmxError
    p = str(tmp_path / 's.fa.gz')
    for text in SHORT_FASTA[:5]:
        open(p, 'wb').write(K.bgzf(text))
        with pytest.raises(VmxError) as e:
            FastqReader(ctx, p)
        assert e.value.code == -7 and "'>'" in str(e.value), (text, e.value)
        ref = Fastx(p, lib=ctx.lib)
        assert len(F.chunk_records(K.read_all(ref, 10))) == 1                                  # (the host reads one FASTA record there)
        ref.close()
    a = F.text_of(_good(7, 1), between_blank=False)
    for tail in (b'>c\nACGT\n', b'>c\n', b'>c', b'>c\nACGT\n+\n'):
        open(p, 'wb').write(K.bgzf(a + tail, 6, block=500))
        got, e = _raises(ctx, p, 1)
        assert e is not None and e.code == -7 and 'record 8' in str(e), (tail, e)
        assert got == F.parse(a)[0]
    for tail in (b'xyz\n', b'xyz\nAC\n', b'xyz\r\nAC\n+\n', b'xyz'):
        open(p, 'wb').write(K.bgzf(a + tail, 6, block=500))
        got, e = _raises(ctx, p, 1)
        assert e is not None and e.code == -5 and str(e).endswith('not FASTA/FASTQ: xyz'), (tail, e)
        assert got == F.parse(a)[0]
        ref = Fastx(p, lib=ctx.lib)
        with pytest.raises(VmxError) as he:
            K.read_all(ref, 100)
        ref.close()
        assert 'not FASTA/FASTQ: xyz' in str(he.value)
    open(p, 'wb').write(K.bgzf(b'xyz\n'))
    with pytest.raises(VmxError) as e:
        FastqReader(ctx, p)
    assert e.value.code == -5 and str(e.value).endswith('not FASTA/FASTQ: xyz')


def test_long_fasta_line_is_refused_in_the_first_window(ctx, tmp_path, monkeypatch):
    """a FASTA whose first record has unwrapped lines longer than a window: refused once the header line is complete, nothing is carried"""
    from vacmap_amd.lib import FastqReader, VmxError
    _small_windows(monkeypatch)
    p = str(tmp_path / 'l.fa.gz')
    open(p, 'wb').write(K.bgzf(b'>chr1 long\n' + b'ACGT' * 100000 + b'\n>chr2\n' + b'GGCC' * 100000 + b'\n', 6, block=4096))
    with pytest.raises(VmxError) as e:
        FastqReader(ctx, p)
    assert e.value.code == -7


def test_driver_input_falls_back_on_short_fasta_and_plain_gzip(ctx, tmp_path, capsys):
    """the driver's input generator: a bgzipped FASTA of one to three lines and a plain-gzip FASTQ go to the host reader with one stderr line
    that names the file and the reason, and give the host reader's chunks"""
    from vacmap_amd import driver
    from vacmap_amd.lib import Fastx
    cases = [(t, K.bgzf(t), 'is FASTA') for t in SHORT_FASTA] + [(b'@a x\nAC\n+\nII\n', gzip.compress(b'@a x\nAC\n+\nII\n'), 'not BGZF')]
    for k, (text, data, why) in enumerate(cases):
        p = str(tmp_path / ('in%d.gz' % k))
        open(p, 'wb').write(data)
        capsys.readouterr()
        got = list(driver._input_chunks(p, 64, ctx.lib, fastx_reader='native'))
        err = capsys.readouterr().err
        assert err.count('\n') == 1 and p in err and why in err, err
        ref = Fastx(p, lib=ctx.lib)
        K.same_chunks(got, K.read_all(ref, 64)); ref.close()
        assert len(got) == 1


def test_open_errors(ctx, tmp_path):
    from vacmap_amd.lib import FastqReader, VmxError
    text = F.text_of(_good())
    cases = {'plain.fastq.gz': (gzip.compress(text), -7), 'fasta.fa.gz': (K.bgzf(b'\n>c1 d\nACGT\nACGT\n>c2\nAC\n'), -7), 'text.fastq': (text, -7), 'empty.fastq.gz': (b'', -5)}
    for name, (data, code) in cases.items():
        p = str(tmp_path / name)
        open(p, 'wb').write(data)
        with pytest.raises(VmxError) as e:
            FastqReader(ctx, p)
        assert e.value.code == code, (name, e.value)
    with pytest.raises(VmxError):
        FastqReader(ctx, str(tmp_path / 'missing.fastq.gz'))


def test_bad_members(ctx, tmp_path):
    """a wrong CRC names the member's file offset; a file cut inside a member is 'truncated'; a member that is not BGZF later in the file fails"""
    text = F.text_of(_good(40))
    first, rest = text[:3000], text[3000:]
    m0 = K.member(K.deflate(first), first)
    p = str(tmp_path / 'c.fastq.gz')
    open(p, 'wb').write(m0 + K.member(K.deflate(rest), rest, crc=zlib.crc32(rest) ^ 4) + K.BGZF_EOF)
    got, e = _raises(ctx, p)
    assert e is not None and e.code == -5 and 'CRC32' in str(e) and 'offset %d' % len(m0) in str(e)
    z = K.bgzf(text, 6, block=2000)
    open(p, 'wb').write(z[:len(z) * 2 // 3])
    got, e = _raises(ctx, p)
    assert e is not None and 'truncated' in str(e) and got == F.parse(text)[0][:len(got)]
    open(p, 'wb').write(m0 + gzip.compress(rest))
    got, e = _raises(ctx, p)
    assert e is not None and 'offset %d' % len(m0) in str(e)


# ---------------------------------------------------------------- 5. seeded edits

def test_seeded_edits(ctx, tmp_path):
    """200 single edits of a small valid file: both readers raise, or their chunks are equal; what the device handed out before it raised is
    a prefix of the records the rule gives for the edited text"""
    from vacmap_amd.lib import Fastx, VmxError
    rng = np.random.default_rng(77)
    recs = [('e%d%s' % (i, ['', ' c', '\tc d'][i % 3]), F._seq(rng, n, 'ACGTacgtN'), '+', F._qual(rng, n)) for i, n in enumerate(rng.integers(0, 120, 14))]
    text = F.text_of(recs, 'mixed')
    outcomes = {'raise': 0, 'same': 0}
    p = str(tmp_path / 'e.fastq.gz')
    for kind, t in F.edits(text, 200, 5):
        open(p, 'wb').write(K.bgzf(t, 1, block=400))
        ref = Fastx(p, lib=ctx.lib)
        try:
            want = K.read_all(ref, 3)
        except VmxError:
            want = None
        finally:
            ref.close()
        got, e = _raises(ctx, p)
        assert (e is None) == (want is not None), (kind, e, want is None)
        if e is None:
            assert got == F.chunk_records(want), kind
            outcomes['same'] += 1
        else:
            assert got == F.parse(t)[0][:len(got)], kind
            outcomes['raise'] += 1
    print(outcomes)


# ---------------------------------------------------------------- 6. the driver

def _fastq_inputs(tmp_path):
    from vacmap_amd import driver
    from test_bam_input_emu import _inputs
    fa, bam, _ = _inputs(tmp_path)
    text = ''.join('@%s\n%s\n+\n%s\n' % (name, seq, qual) for name, seq, qual, _ in driver.read_bam(str(bam))).encode()
    bg, plain = tmp_path / 'reads.fastq.gz', tmp_path / 'plain.fastq.gz'
    bg.write_bytes(K.bgzf(text, 6, block=4000)); plain.write_bytes(gzip.compress(text))
    return fa, bg, plain


@pytest.mark.parametrize('extra', [['-mode', 'H', '--eqx', '--MD'], ['-mode', 'asm']])
def test_driver_native_reader_equals_host_reader(ctx, tmp_path, monkeypatch, capsys, extra):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bg, plain = _fastq_inputs(tmp_path)
    common = ['-ref', str(fa), '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd')] + extra

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@PG')]
    assert driver.main(common + ['-read', str(bg), '-o', str(tmp_path / 'nat.sam'), '--fastx-reader', 'native']) == 0
    capsys.readouterr()
    assert driver.main(common + ['-read', str(plain), '-o', str(tmp_path / 'fb.sam'), '--fastx-reader', 'native']) == 0
    err = capsys.readouterr().err
    assert sum(1 for ln in err.split('\n') if '--fastx-reader native' in ln) == 1 and str(plain) in err and 'not BGZF' in err

    def boom(*a, **k):
        raise AssertionError('FastqReader constructed without --fastx-reader native')
    monkeypatch.setattr(VL, 'FastqReader', boom)
    assert driver.main(common + ['-read', str(bg), '-o', str(tmp_path / 'host.sam')]) == 0
    a = body(tmp_path / 'host.sam')
    assert a == body(tmp_path / 'nat.sam') and sum(1 for x in a if not x.startswith('@')) >= 6
    assert body(tmp_path / 'fb.sam') == a
