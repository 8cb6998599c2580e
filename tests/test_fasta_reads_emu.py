"""FASTA reads and contigs on the device (vm_fastq_reader_open_opts with VM_READER_FASTA, lib.FastqReader(fasta=True), driver --fasta-reads
device) on the CPU emulator build of the kernels (tests/emu). The reference is lib.Fastx (zlib + vm_fastx_read) on the same file, chunk by
chunk at max_reads 1, 3, 64 and 4096; fasta_reads_cases.parse states the rule a second time in Python. The emulator runs a wave's lanes one
after the other: test_gpu_fasta_reads.py runs the same cases on real wavefronts."""
import ctypes
import gzip

import numpy as np
import pytest

import bam_input_cases as K
import fasta_reads_cases as A
import fastq_input_cases as F

SIZES = (1, 3, 64, 4096)


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def shape_recs():
    return A.shape_records(1)


def _small_windows(monkeypatch, chunk=1 << 17, maxinf=1 << 16):
    monkeypatch.setenv('VMX_BAM_IN_CHUNK', str(chunk)); monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(maxinf))


def _check_file(ctx, path, sizes=SIZES, gz='host'):
    """FastqReader(fasta=True) and Fastx give equal chunks at every max_reads; returns the reader's last statistics"""
    from vacmap_amd.lib import FastqReader, Fastx
    st = None
    for n in sizes:
        ref = Fastx(path, lib=ctx.lib)
        want = K.read_all(ref, n); ref.close()
        rd = FastqReader(ctx, path, gzip=gz, fasta=True)
        try:
            K.same_chunks(K.read_all(rd, n), want)
            st = rd.stats()
        finally:
            rd.close()
    return st


def _check_text(ctx, tmp_path, text, block=65280, eof=True, sizes=SIZES, level=6):
    p = str(tmp_path / 'x.fa.gz')
    with open(p, 'wb') as f:
        f.write(K.bgzf(text, level, block=block, eof=eof))
    return _check_file(ctx, p, sizes)


def _raises(ctx, path, n=3):
    """(records handed out before the error, the VmxError) of FastqReader(fasta=True) on path"""
    from vacmap_amd.lib import FastqReader, VmxError
    got, rd = [], None
    try:
        rd = FastqReader(ctx, path, fasta=True)
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


# ---------------------------------------------------------------- 1. shapes

def test_rule_in_python_equals_fastx(ctx, tmp_path, shape_recs):
    """the second statement of the rule agrees with the reference reader on the shapes text and on the rule's own examples"""
    from vacmap_amd.lib import Fastx
    p = str(tmp_path / 'p.fa.gz')
    text = A.text_of(shape_recs, 'mixed', start_blank=True, end_blank=True)
    fq = F.text_of(F.shape_records(2, long_read=0), 'mixed')
    for t in (text, fq + text, text + fq) + tuple(t for t, _ in A.RULE_TEXTS):
        open(p, 'wb').write(K.bgzf(t))
        rd = Fastx(p, lib=ctx.lib)
        got = F.chunk_records(K.read_all(rd, 1000)); rd.close()
        want, err, _ = A.parse(t)
        assert err is None and got == want
    assert len(A.parse(text)[0]) == len(shape_recs)
    for t, want in A.RULE_TEXTS:
        assert A.parse(t)[0] == want
    got = A.parse(text)[0]
    assert (b'', b'x') in [(r[0], r[1]) for r in got] and sum(len(r[2]) == 200000 for r in got) == 2 and any(b'>X' in r[2] for r in got)


@pytest.mark.parametrize('eol', ['lf', 'crlf', 'mixed'])
def test_shapes(ctx, tmp_path, shape_recs, eol):
    text = A.text_of(shape_recs, eol, start_blank=True, end_blank=True)
    st = _check_text(ctx, tmp_path, text)
    assert st['records'] == len(shape_recs) and st['inflated_bytes'] == len(text)


def test_rule_texts(ctx, tmp_path):
    """the consequences the rule names, byte for byte"""
    from vacmap_amd.lib import FastqReader
    p = str(tmp_path / 'r.fa.gz')
    for text, want in A.RULE_TEXTS:
        open(p, 'wb').write(K.bgzf(text))
        rd = FastqReader(ctx, p, fasta=True)
        try:
            assert F.chunk_records(K.read_all(rd, 4096)) == want, text
        finally:
            rd.close()
        _check_file(ctx, p, (1, 3))


# ---------------------------------------------------------------- 2. file ends

@pytest.mark.parametrize('final_nl,end_blank,eof', [(False, False, True), (False, True, False), (True, False, False), (True, True, True)])
def test_file_ends(ctx, tmp_path, final_nl, end_blank, eof):
    """the last line with and without its newline, blank lines at the end, the BGZF EOF member present and absent"""
    recs = A.shape_records(2, long_line=0)
    for eol in ('lf', 'crlf'):
        _check_text(ctx, tmp_path, A.text_of(recs, eol, end_blank=end_blank, final_nl=final_nl), eof=eof, sizes=(3, 4096))


def test_file_ends_on_a_header_line_and_short_texts(ctx, tmp_path):
    """the texts the FASTQ-only reader refuses at open now open and give the host's records; a record without body lines ends the file"""
    for text in A.SHORT_FASTA + (b'>c1 d', b'>a\nAC\n>c1', b'>a\nAC\n>c1 d\n', b'>', b'>\n', b'\n\n \n', b'', b'>c\r\nac\r\n\r\n'):
        for eof in (True, False):
            if text or eof:
                _check_text(ctx, tmp_path, text, eof=eof, sizes=(1, 4096))


@pytest.mark.parametrize('eof', [True, False])
def test_last_member_alone_behind_a_carried_record(ctx, tmp_path, monkeypatch, eof):
    """stored members of 65 280 bytes, two to a chunk of 131 072: the text is exactly four members, so the file's end (the EOF member alone in
    the third chunk, or nothing at all) arrives behind a window that carried its last FASTA record"""
    _small_windows(monkeypatch, maxinf=1 << 20)
    rng = np.random.default_rng(4)
    text = bytes(A.filler(rng, 4 * 65280 - 3000) + b'>tail rec\n' + b'\n'.join(A.wrap(A._seq(rng, 2900))))
    text += b'\n' * (4 * 65280 - len(text))
    assert len(text) == 4 * 65280
    st = _check_text(ctx, tmp_path, text, eof=eof, level=0)
    assert st['records'] == len(A.parse(text)[0]) and st['inflated_bytes'] == len(text)


# ---------------------------------------------------------------- 3. mixed files

def test_mixed_files(ctx, tmp_path):
    fq = F.text_of(F.shape_records(2, long_read=0), 'mixed')
    fa = A.text_of(A.shape_records(3, long_line=0), 'mixed')
    _check_text(ctx, tmp_path, fq + fa, block=5000)                         # FASTQ, then FASTA
    _check_text(ctx, tmp_path, fa + fq, block=5000)                         # FASTA swallows every FASTQ-looking line behind it
    want = A.parse(fa + fq)[0]
    assert len(want) == len(A.parse(fa)[0]) and want[-1][2].endswith(A.parse(fq)[0][-1][3].upper())
    # a FASTQ record that lacks lines behind FASTA is body of the last FASTA record: no error
    _check_text(ctx, tmp_path, fa + b'@last\nACGT\n', sizes=(3, 4096))
    _check_text(ctx, tmp_path, fq + b'>f\nAC\n@last\nACGT\n+\n', sizes=(3, 4096))


def test_truncated_fastq_still_raises(ctx, tmp_path):
    from vacmap_amd.lib import Fastx, VmxError
    base = F.text_of(F.shape_records(2, long_read=0)[:12], between_blank=False)
    p = str(tmp_path / 't.fastq.gz')
    for tail in (b'@last\n', b'@last\nACGT\n', b'@last\nACGT\n+\n', b'@last', b'@last\nACGT\n+'):
        open(p, 'wb').write(K.bgzf(base + tail, 6, block=700))
        got, e = _raises(ctx, p)
        assert e is not None and e.code == -5 and 'truncated' in str(e), (tail, e)
        assert got == A.parse(base)[0][:len(got)]
        ref = Fastx(p, lib=ctx.lib)
        with pytest.raises(VmxError):
            K.read_all(ref, 100)
        ref.close()


# ---------------------------------------------------------------- 4. errors

def test_bad_headers(ctx, tmp_path):
    """'xyz' and ' >x' where a record must start: -5, the message ends with the host's 40 bytes, the records in front come through earlier calls"""
    from vacmap_amd.lib import FastqReader, Fastx, VmxError
    p = str(tmp_path / 'h.fa.gz')
    good = F.text_of(F.shape_records(2, long_read=0)[:9], between_blank=False)           # (ends in state 0: the next line must start a record)
    long_line = b'xyz ' + b'Q' * 100
    for bad in (b'xyz', b' >x', long_line, b' >' + b'y' * 60):
        for tail in (b'\n', b'\nAC\n', b'\r\nAC\n+\nII\n>f\nAC\n', b''):
            open(p, 'wb').write(K.bgzf(bad + tail))
            with pytest.raises(VmxError) as e:
                FastqReader(ctx, p, fasta=True)
            assert e.value.code == -5 and str(e.value).endswith('not FASTA/FASTQ: ' + bad[:40].decode()), (bad, tail, e.value)
            open(p, 'wb').write(K.bgzf(good + bad + tail, 6, block=500))
            got, e = _raises(ctx, p, 1)
            assert e is not None and e.code == -5 and str(e).endswith('not FASTA/FASTQ: ' + bad[:40].decode()), (bad, tail, e)
            assert got == A.parse(good)[0]
            ref = Fastx(p, lib=ctx.lib)
            with pytest.raises(VmxError) as he:
                K.read_all(ref, 100)
            ref.close()
            assert str(he.value).endswith('not FASTA/FASTQ: ' + bad[:40].decode())
    # inside a FASTA record the same lines are body
    _check_text(ctx, tmp_path, b'>f\nAC\n' + b'xyz\n >x\n', sizes=(1, 64))


# ---------------------------------------------------------------- 5. FASTQ through the new path

@pytest.mark.parametrize('eol', ['lf', 'mixed'])
def test_fastq_through_the_general_parser(ctx, tmp_path, eol):
    recs = F.shape_records(1)
    st = _check_text(ctx, tmp_path, F.text_of(recs, eol, start_blank=True, end_blank=True))
    assert st['records'] == len(recs)


# ---------------------------------------------------------------- 6. windows

@pytest.mark.parametrize('block', [65280, 5000, 333])
def test_windows(ctx, tmp_path, monkeypatch, shape_recs, block):
    """the shapes text in members of 65 280, 5 000 and 333 bytes through windows of 64 KB: records, header lines and body lines cross members
    and windows, and both 200 kb records are larger than a window"""
    _small_windows(monkeypatch)
    text = A.text_of(shape_recs, 'mixed', start_blank=True, end_blank=True)
    st = _check_text(ctx, tmp_path, text, block=block, level=1 if block == 333 else 6)
    assert st['inflated_bytes'] == len(text) and st['records'] == len(shape_recs) and st['windows'] >= len(text) // 65536


@pytest.mark.parametrize('kind', ['start', 'crlf', 'header'])
def test_window_boundaries(ctx, tmp_path, monkeypatch, kind):
    """members of 4 096 bytes and windows of 65 536: the first window ends at byte 65 536 exactly, where a record starts, between the '\\r' and
    the '\\n' of a body line, or right behind a header's newline"""
    _small_windows(monkeypatch)
    st = _check_text(ctx, tmp_path, A.boundary_text(65536, kind), block=4096)
    assert st['windows'] >= 2


@pytest.mark.parametrize('wrapped', [True, False])
def test_one_record_longer_than_ten_windows(ctx, tmp_path, monkeypatch, wrapped):
    """700 000 bases in windows of 64 KB: the record is carried until the next record's header arrives; the windows in between hold no
    complete record"""
    from vacmap_amd.lib import FastqReader
    _small_windows(monkeypatch)
    text, bases = A.long_record_text(700000, wrapped)
    p = str(tmp_path / 'l.fa.gz')
    open(p, 'wb').write(K.bgzf(text, 1))
    st = _check_file(ctx, p, (3,))
    assert st['windows'] > 10 and st['records'] == 3
    rd = FastqReader(ctx, p, fasta=True)
    try:
        got = F.chunk_records(K.read_all(rd, 4096))
    finally:
        rd.close()
    assert got == [(b'first', b'', b'ACGT', b''), (b'big', b'one', bases, b''), (b'last', b'', b'GG', b'')]


# ---------------------------------------------------------------- 7. plain gzip, flags

def test_plain_gzip_with_the_device_inflate(ctx, tmp_path, monkeypatch):
    _small_windows(monkeypatch)
    text = A.text_of(A.shape_records(5, long_line=300000), 'mixed', start_blank=True)
    p = str(tmp_path / 'g.fa.gz')
    open(p, 'wb').write(gzip.compress(text))
    st = _check_file(ctx, p, (3, 4096), gz='device')
    assert st['inflated_bytes'] == len(text) and st['windows'] >= 2


def test_flags(ctx, tmp_path):
    """flag 0 still refuses FASTA with -7; a flag bit the header does not name is VM_ERR_ARG (-1), as the header states"""
    from vacmap_amd.lib import FastqReader, VmxError
    p = str(tmp_path / 'f.fa.gz')
    open(p, 'wb').write(K.bgzf(b'>c1 d\nACGT\n'))
    with pytest.raises(VmxError) as e:
        FastqReader(ctx, p)
    assert e.value.code == -7
    L = ctx.lib.L
    for flags, ok in ((2, True), (3, True), (4, False), (2 | 8, False)):
        h = ctypes.c_void_p()
        rc = L.vm_fastq_reader_open_opts(ctx.h, p.encode(), flags, ctypes.byref(h))
        if ok:
            assert rc == 0 and h.value
            L.vm_fastq_reader_close(h)
        else:
            assert rc == -1 and not h.value
            with pytest.raises(VmxError) as e:
                ctx.lib.check(rc)
            assert 'flag' in str(e.value)


# ---------------------------------------------------------------- 8. the driver

def test_driver_input_reads_fasta_on_the_device(ctx, tmp_path, capsys):
    from vacmap_amd import driver
    from vacmap_amd.lib import Fastx
    text = A.text_of(A.shape_records(2, long_line=0), 'mixed')
    for k, data in enumerate((K.bgzf(text, 6, block=5000), K.bgzf(A.SHORT_FASTA[1]))):
        p = str(tmp_path / ('in%d.fa.gz' % k))
        open(p, 'wb').write(data)
        ref = Fastx(p, lib=ctx.lib)
        want = K.read_all(ref, 64); ref.close()
        capsys.readouterr()
        got = list(driver._input_chunks(p, 64, ctx.lib, fastx_reader='native', fasta_reads='device'))
        assert capsys.readouterr().err == ''
        K.same_chunks(got, want)
        got = list(driver._input_chunks(p, 64, ctx.lib, fastx_reader='native', fasta_reads='host'))
        err = capsys.readouterr().err
        assert err.count('\n') == 1 and p in err and 'is FASTA' in err
        K.same_chunks(got, want)
    # what is still refused at open falls back with the one line: plain gzip without the device inflate
    p = str(tmp_path / 'plain.fa.gz')
    open(p, 'wb').write(gzip.compress(text))
    got = list(driver._input_chunks(p, 64, ctx.lib, fastx_reader='native', fasta_reads='device'))
    err = capsys.readouterr().err
    assert err.count('\n') == 1 and p in err and 'not BGZF' in err
    ref = Fastx(p, lib=ctx.lib)
    K.same_chunks(got, K.read_all(ref, 64)); ref.close()
    got = list(driver._input_chunks(p, 64, ctx.lib, fastx_reader='native', gzip_inflate='device', fasta_reads='device'))
    assert capsys.readouterr().err == ''
    ref = Fastx(p, lib=ctx.lib)
    K.same_chunks(got, K.read_all(ref, 64)); ref.close()


def test_driver_arguments():
    from vacmap_amd import driver
    parser = driver.build_parser()
    base = ['-ref', 'r.fa', '-read', 'x.fa.gz', '-o', 'o.sam', '-mode', 'asm']
    assert parser.parse_args(base).fasta_reads == 'host'
    assert parser.parse_args(base + ['--fastx-reader', 'native', '--fasta-reads', 'device']).fasta_reads == 'device'
    with pytest.raises(SystemExit):
        parser.parse_args(base + ['--fasta-reads', 'gpu'])
