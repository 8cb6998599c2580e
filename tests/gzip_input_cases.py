"""TEST-ONLY: plain-gzip inputs for lib.gzip_decompress (vm_gzip_decompress, kernels k_gzip_in.hip) and the checks that the emulator and the
GPU suite share. The comparator is Python's zlib / gzip. Every text is at most 1.5 MB (the 8 MB of zeros aside: 8 KB compressed)."""
import gzip
import struct
import zlib

import numpy as np

_cache = {}


def fastq_text(n_bytes, seed=1, read_len=(200, 9000)):
    """FASTQ-shaped text of about n_bytes: names, uniform ACGT, qualities of a narrow distribution"""
    key = (n_bytes, seed, read_len)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        parts, n, i = [], 0, 0
        acgt = np.frombuffer(b'ACGT', np.uint8)
        while n < n_bytes:
            L = int(rng.integers(read_len[0], read_len[1]))
            s = acgt[rng.integers(0, 4, L)].tobytes()
            q = (33 + np.clip(rng.normal(28, 7, L), 2, 40).astype(np.uint8)).tobytes()
            r = b'@read_%d_%d ch=%d\n' % (seed, i, i % 512) + s + b'\n+\n' + q + b'\n'
            parts.append(r); n += len(r); i += 1
        _cache[key] = b''.join(parts)
    return _cache[key]


def deflate_gz(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_every=0):
    """one gzip member by zlib (wbits 31); flush_every: Z_SYNC_FLUSH and Z_FULL_FLUSH in turn after every that many bytes"""
    co = zlib.compressobj(level, zlib.DEFLATED, 31, 9, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    out = []
    for k, at in enumerate(range(0, len(data), flush_every)):
        out.append(co.compress(data[at:at + flush_every]))
        out.append(co.flush(zlib.Z_FULL_FLUSH if k % 2 else zlib.Z_SYNC_FLUSH))
    out.append(co.flush())
    return b''.join(out)


def member(payload, level=6, extra=None, name=None, comment=None, hcrc=False, trailer=None):
    """a gzip member written by hand: any header field, any trailer"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = b'\x1f\x8b\x08' + bytes([flg]) + b'\0\0\0\0\x00\x03'
    if extra is not None:
        h += struct.pack('<H', len(extra)) + extra
    if name is not None:
        h += name + b'\0'
    if comment is not None:
        h += comment + b'\0'
    if hcrc:
        h += struct.pack('<H', zlib.crc32(h) & 0xffff)
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = co.compress(payload) + co.flush()
    if trailer is None:
        trailer = struct.pack('<II', zlib.crc32(payload), len(payload) & 0xffffffff)
    return h + body + trailer


def byte_cases():
    """name -> (gzip bytes, text): the streams whose bytes must equal zlib's"""
    t = fastq_text(1_100_000)
    c = {}
    for lvl in (1, 6, 9):
        c['level%d' % lvl] = (gzip.compress(t, lvl), t)
    small = t[:300_000]
    c['fixed'] = (deflate_gz(small, 6, zlib.Z_FIXED), small)                       # no candidate anywhere: one chain
    c['stored'] = (deflate_gz(small, 0), small)                                    # stored blocks only
    c['huffman_only'] = (deflate_gz(small, 6, zlib.Z_HUFFMAN_ONLY), small)
    rle = (np.repeat(np.random.default_rng(3).integers(0, 256, 30_000, dtype=np.uint8), np.random.default_rng(4).integers(1, 40, 30_000))).tobytes()
    c['rle'] = (deflate_gz(rle, 6, zlib.Z_RLE), rle)                               # distance 1, length > distance
    c['flushes'] = (deflate_gz(small, 6, flush_every=10_000), small)               # empty stored blocks, byte-aligned boundaries
    c['empty'] = (gzip.compress(b''), b'')
    c['one_byte'] = (gzip.compress(b'x'), b'x')
    z = b'\0' * (8 << 20)
    c['zeros'] = (gzip.compress(z, 6), z)
    return c


def marker_cases():
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    u = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    return {'twice_32768': a + a,                   # distance 32 768 exactly, across chunk boundaries
            'unit_20000_x50': u * 50}               # almost every symbol of every chunk is a marker, copied from copies


def false_candidate_case():
    """gzip -0 of (gzip -6 of a 1 MB text): the inner stream's dynamic headers lie verbatim inside the outer stored blocks"""
    inner = gzip.compress(fastq_text(1_000_000, seed=2), 6)
    return gzip.compress(inner, 0), inner


def three_members():
    t = fastq_text(120_000, seed=3)
    parts = [t[:50_000], b'', t[50_000:]]
    z = gzip.compress(parts[0], 6) + gzip.compress(b'') + member(parts[2], 9, extra=b'AB\x03\x00xyz', name=b'reads.fastq', comment=b'a comment', hcrc=True)
    return z, b''.join(parts)


def offset_members():
    """the 64 concatenations whose second member starts at byte 4096 k + d, k = 1 ... 16, d in (-1, 0, 1, 9): the first member is padded to
    its length with a comment"""
    t = fastq_text(200_000, seed=4)
    second_text = fastq_text(30_000, seed=5)
    second = gzip.compress(second_text, 6)
    for k in range(1, 17):
        first_text = t[:7000 * k]
        base = member(first_text, 6, comment=b'')
        for d in (-1, 0, 1, 9):
            pad = 4096 * k + d - len(base)
            assert pad >= 0, (k, d, len(base))
            first = member(first_text, 6, comment=b'p' * pad)
            assert len(first) == 4096 * k + d
            yield (k, d), first + second, first_text + second_text


def edits(data, n, seed):
    """n seeded single-byte edits of data"""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        at = int(rng.integers(0, len(data)))
        b = bytearray(data)
        b[at] = int((b[at] + rng.integers(1, 256)) % 256)
        yield at, bytes(b)


def python_gunzip(z):
    """(bytes, None) or (None, the exception) of Python's gzip module"""
    try:
        return gzip.decompress(z), None
    except (OSError, EOFError, zlib.error) as e:
        return None, e


def device_gunzip(ctx, z, stats=None):
    from vacmap_amd.lib import gzip_decompress, VmxError
    try:
        return gzip_decompress(ctx, z, stats), None
    except VmxError as e:
        return None, e


def same_outcome(ctx, z, what=''):
    """both sides raise, or both give equal bytes; returns the device's error (None: bytes)"""
    want, ew = python_gunzip(z)
    got, eg = device_gunzip(ctx, z)
    assert (ew is None) == (eg is None), (what, ew, eg)
    if ew is None:
        assert got == want, what
    return eg


# ---------------------------------------------------------------- the checks both suites run (ctx: the emulator's or the device's)

def check_bytes(ctx, monkeypatch, chunk):
    from vacmap_amd.lib import gzip_decompress
    monkeypatch.setenv('VMX_GZ_CHUNK', str(chunk))
    for name, (z, text) in byte_cases().items():
        st = {}
        got = gzip_decompress(ctx, z, st)
        assert got == text and text == zlib.decompress(z, 31), name
        if name == 'level6':
            assert st['chunks_started'] - st['candidates_rejected'] >= 4, st      # (the prototype found one block per 18 KB of compressed data)
        if name in ('fixed', 'stored', 'empty', 'one_byte'):
            assert st['chunks_started'] - st['candidates_rejected'] == 1, (name, st)
            assert st['first_chain_bytes'] == len(text), (name, st)


def check_markers(ctx, monkeypatch):
    from vacmap_amd.lib import gzip_decompress
    monkeypatch.setenv('VMX_GZ_CHUNK', '1024')
    for name, text in marker_cases().items():
        for lvl in (6, 9):
            assert gzip_decompress(ctx, gzip.compress(text, lvl), None) == text, (name, lvl)
    # zlib closes a block after 16 383 symbols and a 258-byte match is one symbol, so the streams above have few blocks. One byte in 24 changed
    # makes the matches short: several dynamic blocks, each a wave of its own whose text is nearly all markers
    u = np.frombuffer(marker_cases()['unit_20000_x50'], np.uint8).copy()
    u[np.arange(7, len(u), 24)] ^= np.random.default_rng(12).integers(1, 256, len(np.arange(7, len(u), 24)), dtype=np.uint8)
    st = {}
    assert gzip_decompress(ctx, gzip.compress(u.tobytes(), 6), st) == u.tobytes()
    assert st['chunks_started'] - st['candidates_rejected'] >= 4, st


def check_false_candidates(ctx, monkeypatch):
    from vacmap_amd.lib import gzip_decompress
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096')
    z, inner = false_candidate_case()
    st = {}
    assert gzip_decompress(ctx, z, st) == inner
    assert st['candidates_rejected'] >= 1 and st['chunks_redone'] >= 1, st


def check_members(ctx, monkeypatch):
    from vacmap_amd.lib import gzip_decompress
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096')
    z, text = three_members()
    assert gzip.decompress(z) == text and gzip_decompress(ctx, z) == text
    for key, z, text in offset_members():
        assert gzip_decompress(ctx, z) == text, key
    z = gzip.compress(b'') * 2000
    assert gzip_decompress(ctx, z) == b''
    z = gzip.compress(b'') * 10 + gzip.compress(b'tail') + gzip.compress(b'') * 10 + b'\0' * 7       # (zero padding behind the last member: gzip(1) and Python skip it)
    assert gzip.decompress(z) == b'tail' and gzip_decompress(ctx, z) == b'tail'


def check_errors(ctx, monkeypatch):
    monkeypatch.setenv('VMX_GZ_CHUNK', '1024')
    t = fastq_text(60_000, seed=6)
    z = gzip.compress(t, 6)
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]
    for what, bad, word in (('crc', flip(z, len(z) - 7), 'CRC32'), ('isize', flip(z, len(z) - 2), 'ISIZE'), ('cut 2/3', z[:2 * len(z) // 3], 'truncated'),
                            ('cut in trailer', z[:-3], 'truncated'), ('bad magic', z + b'\x1f\x8c' + z[2:], 'magic')):
        e = same_outcome(ctx, bad, what)
        assert e is not None and word in str(e), (what, e)
    # a bad member after a good one names its offset
    second = gzip.compress(t[:20_000], 6)
    e = same_outcome(ctx, z + flip(second, len(second) - 7), 'second crc')
    assert e is not None and 'file offset %d' % len(z) in str(e) and 'CRC32' in str(e), e
    e = same_outcome(ctx, z + second[:len(second) // 2], 'second cut')
    assert e is not None and 'truncated' in str(e), e


def check_seeded_edits(ctx, monkeypatch, n=150):
    """n single-byte edits of a 60 KB file: both sides raise, or both give equal bytes"""
    monkeypatch.setenv('VMX_GZ_CHUNK', '1024')
    t = fastq_text(150_000, seed=7)
    # a whole file of 60 KB: the text whose compressed form is nearest below
    lo, hi = 100_000, 150_000
    while hi - lo > 64:
        mid = (lo + hi) // 2
        if len(gzip.compress(t[:mid], 6)) <= 60_000:
            lo = mid
        else:
            hi = mid
    z = gzip.compress(t[:lo], 6)
    assert 59_000 <= len(z) <= 60_000
    outcomes = {'raise': 0, 'same': 0}
    for at, bad in edits(z, n, 9):
        outcomes['raise' if same_outcome(ctx, bad, at) is not None else 'same'] += 1
    print(outcomes)
    assert outcomes['raise'] >= n // 2          # (nearly every edit of deflate data breaks a code or the CRC)


# ---------------------------------------------------------------- FastqReader(gzip='device'): the comparator is lib.Fastx on the same file

def reader_chunks(ctx, path, n, stats=None):
    import bam_input_cases as K
    from vacmap_amd.lib import FastqReader
    rd = FastqReader(ctx, path, gzip='device')
    try:
        out = K.read_all(rd, n)
        if stats is not None:
            stats.update(rd.stats())
        return out
    finally:
        rd.close()


def check_reader_file(ctx, path, sizes=(1, 3, 64, 4096)):
    """FastqReader(gzip='device') equals Fastx chunk for chunk at every max_reads; returns the last statistics"""
    import bam_input_cases as K
    from vacmap_amd.lib import Fastx
    st = {}
    for n in sizes:
        ref = Fastx(path, lib=ctx.lib)
        want = K.read_all(ref, n); ref.close()
        K.same_chunks(reader_chunks(ctx, path, n, st), want)
    return st


def check_reader_shapes(ctx, monkeypatch, tmp_path):
    """the shapes text of fastq_input_cases (LF, CRLF, mixed; the 200 kb read) as plain gzip"""
    import fastq_input_cases as F
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096')
    recs = F.shape_records(1)
    for eol in ('lf', 'crlf', 'mixed'):
        p = str(tmp_path / ('s_%s.fastq.gz' % eol))
        open(p, 'wb').write(gzip.compress(F.text_of(recs, eol), 6))
        st = check_reader_file(ctx, p)
        assert st['chunks_started'] >= 2, st


def check_reader_windows(ctx, monkeypatch, tmp_path):
    """window, CRC and size carried across at least 5 windows; one window's text many times max_inf"""
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096'); monkeypatch.setenv('VMX_BAM_IN_CHUNK', '131072'); monkeypatch.setenv('VMX_BAM_IN_MAXINF', '65536')
    t = fastq_text(1_400_000, seed=8)
    for lvl in (1, 6):
        p = str(tmp_path / ('w%d.fastq.gz' % lvl))
        open(p, 'wb').write(gzip.compress(t, lvl))
        st = check_reader_file(ctx, p, sizes=(64,))
        assert st['windows'] >= 5 and st['inflated_bytes'] == len(t), st
    # several members, so that members end and begin inside windows and at their edges
    p = str(tmp_path / 'wm.fastq.gz')
    cut = t.index(b'\n@read', 500_000) + 1
    open(p, 'wb').write(gzip.compress(t[:cut], 6) + gzip.compress(b'') + gzip.compress(t[cut:], 1) + b'\0' * 5)
    st = check_reader_file(ctx, p, sizes=(64,))
    assert st['windows'] >= 5 and st['inflated_bytes'] == len(t), st
    # 8 MB of text in 8 KB of gzip: one compressed window, text many times max_inf. As FASTQ (one read of 4 M bases), and as the zeros file,
    # which is not FASTQ: both readers refuse it, the device reader after having inflated it
    big = b'@big\n' + b'A' * (4 << 20) + b'\n+\n' + b'I' * (4 << 20) + b'\n'
    p = str(tmp_path / 'big.fastq.gz')
    open(p, 'wb').write(gzip.compress(big, 6))
    st = check_reader_file(ctx, p, sizes=(3,))
    assert st['inflated_bytes'] == len(big), st
    from vacmap_amd.lib import Fastx, VmxError
    p = str(tmp_path / 'zeros.gz')
    open(p, 'wb').write(gzip.compress(b'\0' * (8 << 20), 6))
    for make in (lambda: reader_chunks(ctx, p, 3), lambda: Fastx(p, lib=ctx.lib).read(3)):
        try:
            make()
            raise AssertionError('8 MB of zeros read as FASTQ')
        except VmxError:
            pass


def check_reader_errors(ctx, monkeypatch, tmp_path):
    """a corrupt file: the reader raises, and what it handed out before is a prefix of the text's records"""
    import fastq_input_cases as F
    from vacmap_amd.lib import FastqReader, VmxError
    monkeypatch.setenv('VMX_GZ_CHUNK', '1024'); monkeypatch.setenv('VMX_BAM_IN_CHUNK', '131072'); monkeypatch.setenv('VMX_BAM_IN_MAXINF', '65536')
    t = fastq_text(600_000, seed=10, read_len=(200, 3000))
    want = F.parse(t)[0]
    z = gzip.compress(t, 6)
    flip = lambda b, at: b[:at] + bytes([b[at] ^ 0x10]) + b[at + 1:]
    p = str(tmp_path / 'bad.fastq.gz')
    for what, bad, word in (('crc', flip(z, len(z) - 7), 'CRC32'), ('isize', flip(z, len(z) - 2), 'ISIZE'), ('cut 2/3', z[:2 * len(z) // 3], 'truncated'),
                            ('cut in trailer', z[:-3], 'truncated'), ('bad magic', z + b'\x1f\x8c' + z[2:], 'magic')):
        open(p, 'wb').write(bad)
        got, err, rd = [], None, None
        try:
            rd = FastqReader(ctx, p, gzip='device')
            while True:
                ch = rd.read(64)
                if ch is None:
                    break
                got.append(ch)
        except VmxError as e:
            err = e
        finally:
            if rd is not None:
                rd.close()
        assert err is not None and word in str(err), (what, err)
        got = F.chunk_records(got)
        assert got == want[:len(got)], what
        if what in ('crc', 'isize', 'cut in trailer', 'bad magic'):
            assert len(got) >= len(want) // 2, (what, len(got), len(want))      # (the windows in front of the bad one were handed out)
    # without the option a plain-gzip file is refused as before
    open(p, 'wb').write(z)
    try:
        FastqReader(ctx, p).close()
        raise AssertionError('plain gzip accepted without gzip=device')
    except VmxError as e:
        assert e.args[0] == -7 or '-7' in str(e) or 'BGZF' in str(e), e


# ---------------------------------------------------------------- Index.from_fasta(reader='native', gzip='device'): the comparator is the host parser's .vmx

def ref_texts():
    """name -> text: the texts of fasta_ref_cases (line ends, headers, letters, an unwrapped line, contig and CRLF / header splits at 65 536, a 600 KB scale text)"""
    import fasta_ref_cases as R
    t = {}
    for fam, d in (('eol', R.eol_texts()), ('hdr', R.header_texts()), ('let', R.letter_texts())):
        for k, v in d.items():
            t['%s_%s' % (fam, k)] = v
    t['width_61'] = R.width_text(61)
    t['long_line'] = R.long_line_text()
    t['boundary'] = R.boundary_text(65536)
    t['crlf_split'] = R.crlf_split_text(65536)
    t['header_split'] = R.header_split_text(65536)
    t['scale'] = b''.join(R.scale_text(600_000))
    return t


def check_ref_vmx(VL, ctx, monkeypatch, tmp_path):
    """reader='native', gzip='device' on the plain-gzip form writes the host parser's .vmx byte for byte: in one window, and through windows of
    64 KB of text (VMX_BAM_IN_MAXINF) with 128 KB of compressed data each"""
    import os
    import fasta_ref_cases as R
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096')
    d = str(tmp_path)
    for small in (False, True):
        if small:
            monkeypatch.setenv('VMX_BAM_IN_CHUNK', '131072'); monkeypatch.setenv('VMX_BAM_IN_MAXINF', '65536')
        for name, text in ref_texts().items():
            plain, gz = os.path.join(d, 'r.fa'), os.path.join(d, 'r.fa.gz')
            open(plain, 'wb').write(text); open(gz, 'wb').write(gzip.compress(text, 6))
            host = VL.Index.from_fasta(ctx, plain, **R.KW)
            want = R.vmx_bytes(host, os.path.join(d, 'host.vmx')); host.close()
            idx = VL.Index.from_fasta(ctx, gz, reader='native', gzip='device', **R.KW)
            try:
                assert R.vmx_bytes(idx, os.path.join(d, 'got.vmx')) == want, (name, small)
                assert idx.build_stats['text_bytes'] == len(text) and idx.build_stats['contigs'] == len(R.parse(text)), (name, idx.build_stats)
                if small and len(text) > 300_000:
                    assert idx.build_stats['windows'] >= 4, (name, idx.build_stats)
            finally:
                idx.close()
    # a corrupt reference raises (CRC32), and a bgzipped one takes the BGZF path as before
    z = gzip.compress(ref_texts()['scale'], 6)
    open(gz, 'wb').write(z[:len(z) - 7] + bytes([z[-7] ^ 1]) + z[len(z) - 6:])
    try:
        VL.Index.from_fasta(ctx, gz, reader='native', gzip='device', **R.KW).close()
        raise AssertionError('a reference with a wrong CRC32 was accepted')
    except VL.VmxError as e:
        assert 'CRC32' in str(e), e
