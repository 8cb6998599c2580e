"""Native BAM input (vm_bgzf_decompress, vm_bam_reader_*, lib.BamReader, driver --bam-reader native) on the CPU emulator build of the kernels
(tests/emu). References: Python's zlib / gzip for the inflate, driver.read_bam / driver._bam_chunks and tests/bam_codec.py for the records.
The emulator runs a wave's lanes one after the other, so it cannot show a missing store -> load ordering between lanes of the match copy:
that is test_gpu_bam_input.py's wave-ordering test."""
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import bam_codec as B
import bam_input_cases as K

HDR = '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:5000\n'


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def codec(ctx):
    from vacmap_amd.lib import BamCodec
    c = BamCodec(ctx, HDR)
    yield c
    c.close()


@pytest.fixture(scope='module')
def bam_bytes(codec):
    from test_bam_emu import synth_sam
    return codec.encode('\n'.join(synth_sam(120, 5)) + '\n')


@pytest.fixture(scope='module')
def cases(bam_bytes):
    return K.inflate_cases(bam_bytes)


# ---------------------------------------------------------------- 1. bgzf_decompress against zlib

def test_case_set_covers_every_block_type(cases):
    """the builders really make what they are named after: BTYPE 0, 1 and 2 as first block, and a member of several blocks"""
    seen, multi = set(), False
    for z in cases.values():
        for _, m in K.split_members(z):
            bt, bfinal = K.block_types(m)
            seen.add(bt); multi |= bfinal == 0
    assert seen == {0, 1, 2} and multi
    assert {K.block_types(m)[0] for _, m in K.split_members(cases['fixed'])} == {1}
    assert all(K.block_types(m)[1] == 0 for _, m in K.split_members(cases['full_flush'])[:-1])
    assert len(K.split_members(cases['size0'])[0][1]) > 0 and struct.unpack('<I', K.split_members(cases['size65280'])[0][1][-4:])[0] == 65280


def test_bgzf_decompress_equals_zlib(ctx, cases):
    from vacmap_amd.lib import bgzf_decompress
    for name, z in cases.items():
        assert bgzf_decompress(ctx, z) == gzip.decompress(z), name
    assert bgzf_decompress(ctx, b'') == b''


def test_bgzf_roundtrip_with_device_deflate(ctx, bam_bytes):
    from vacmap_amd.lib import bgzf_compress, bgzf_decompress
    for d in (b'', b'x', bam_bytes, b'\0' * 100000, K.periodic(3, 70000), np.random.default_rng(2).integers(0, 256, 66000).astype(np.uint8).tobytes()):
        assert bgzf_decompress(ctx, bgzf_compress(ctx, d)) == d


# ---------------------------------------------------------------- 2. BamReader against _bam_chunks

def _small_windows(monkeypatch, chunk=1 << 17, maxinf=1 << 16):
    monkeypatch.setenv('VMX_BAM_IN_CHUNK', str(chunk)); monkeypatch.setenv('VMX_BAM_IN_MAXINF', str(maxinf))


def _check_file(ctx, path, sizes=(1, 3, 64, 4096)):
    from vacmap_amd import driver
    from vacmap_amd.lib import BamReader
    for n in sizes:
        rd = BamReader(ctx, path)
        K.same_chunks(K.read_all(rd, n), list(driver._bam_chunks(path, n)))
        rd.close()


def _ubam_stream():
    recs = K.random_reads(40, 1, 1, 900) + [('long', 'ACGT' * 50000, 'I' * 200000, 16), ('one', 'G', '#', 0), ('empty', '', None, 4)] + K.random_reads(25, 2, 100, 6000)
    return K.bam_header('@HD\tVN:1.6\tSO:unsorted\n'), b''.join(K.bam_record(*r) for r in recs)


@pytest.mark.parametrize('block,windows', [(65280, False), (5000, True), (333, True)])
def test_reader_unaligned_bam(ctx, tmp_path, monkeypatch, block, windows):
    """1 base to 200 kb, both strands, no qualities, no bases; small members make records straddle two and three members, small windows
    make them straddle windows (the carried tail)"""
    if windows:
        _small_windows(monkeypatch)
    head, body = _ubam_stream()
    p = str(tmp_path / 'u.bam')
    open(p, 'wb').write(K.bgzf(head + body, 6, block=block))
    _check_file(ctx, p)


def test_reader_header_straddles_members_and_windows(ctx, tmp_path, monkeypatch):
    _small_windows(monkeypatch)
    refs = [('contig_%05d' % i, 1000 + i) for i in range(6000)]
    head = K.bam_header('@HD\tVN:1.6\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % r for r in refs), refs)
    assert len(head) > 3 * 65536
    p = str(tmp_path / 'h.bam')
    open(p, 'wb').write(K.bgzf(head + b''.join(K.bam_record(*r) for r in K.random_reads(10, 4)), 1, block=40000))
    _check_file(ctx, p)


def test_reader_aligned_bam_from_the_product_codec(ctx, codec, tmp_path):
    """aligned records of the product's own encoder: both strands, more than 65 535 CIGAR operations (CG tag), '*' qualities, no bases"""
    from test_bam_emu import synth_sam
    from vacmap_amd.lib import bgzf_decompress
    big = '%s\t16\tchr1\t7\t60\t%s\t*\t0\t0\t%s\t%s\tNM:i:0' % ('bigcigar', '1M1I' * 33000 + '5M', 'AC' * 33000 + 'GGGGG', 'F' * 66005)
    lines = synth_sam(30, 9) + [big, 'noq\t0\tchr2\t5\t9\t4M\t*\t0\t0\tACGT\t*', 'noseq\t16\tchr1\t9\t0\t3M\t*\t0\t0\t*\t*\tXX:i:1'] + synth_sam(5, 10)
    raw = gzip.decompress(codec.header()) + codec.encode('\n'.join(lines) + '\n')
    text, refs, recs = B.read_bam(K.bgzf(raw))
    assert len(recs) == len(lines) and any(int(f[1]) & 16 for f, _ in recs) and any(int(f[1]) & 16 == 0 for f, _ in recs)
    assert any(f[5].count('M') > 33000 for f, _ in recs) and any(f[9] == '*' for f, _ in recs) and any(f[10] == '*' and f[9] != '*' for f, _ in recs)
    p = str(tmp_path / 'a.bam')
    open(p, 'wb').write(K.bgzf(raw, 6))
    _check_file(ctx, p)
    assert bgzf_decompress(ctx, K.bgzf(raw, 9)) == raw


def test_reader_max_bases_stops_like_fastx(ctx, tmp_path):
    from vacmap_amd import driver
    from vacmap_amd.lib import BamReader, Fastx
    recs = [r for r in K.random_reads(60, 6, 50, 2000) if r[2] is not None and r[1]]
    p = str(tmp_path / 'm.bam')
    open(p, 'wb').write(K.bgzf(K.bam_header() + b''.join(K.bam_record(*r) for r in recs), 6, block=20000))
    fq = str(tmp_path / 'm.fq')
    with open(fq, 'w') as f:
        for name, seq, qual, _ in driver.read_bam(p):
            f.write('@%s\n%s\n+\n%s\n' % (name, seq, qual))
    for mr, mb in ((1000, 5000), (7, 3000), (1000, 1)):
        a, b = BamReader(ctx, p), Fastx(fq, lib=ctx.lib)
        K.same_chunks(K.read_all(a, mr, mb), K.read_all(b, mr, mb))
        a.close(); b.close()


def test_reader_five_records_of_the_host_logic_test(ctx, tmp_path):
    from vacmap_amd.lib import BamReader
    recs = [('r1', 'ACGTNACGTA', 'IIIIIHHHHH', 0), ('r2', 'AACCGGTTA', 'ABCDEFGHI', 16), ('r3', 'GATTACA', None, 4), ('r4', '', None, 4), ('r5', 'ACGRYK', '!!!!!!', 0)]
    p = str(tmp_path / 'x.bam')
    open(p, 'wb').write(K.bgzf(K.bam_header() + b''.join(K.bam_record(*r) for r in recs), 6, block=50))
    rd = BamReader(ctx, p)
    chunks = K.read_all(rd, 3)
    assert [len(c['seqs_off']) - 1 for c in chunks] == [3, 1]
    c0, c1 = chunks
    assert c0['seqs'].tobytes() == b'ACGTNACGTATAACCGGTTGATTACA' and c0['quals_off'].tolist() == [0, 10, 19, 19] and c0['names'].tobytes() == b'r1r2r3'
    assert c0['quals'].tobytes() == b'IIIIIHHHHHIHGFEDCBA' and c1['seqs'].tobytes() == b'ACGRYK' and c1['quals'].tobytes() == b'!!!!!!' and c1['names'].tobytes() == b'r5'
    assert rd.stats()['dropped'] == 1
    rd.close()


def test_open_errors(ctx, tmp_path):
    from vacmap_amd.lib import BamReader, VmxError
    from test_host_logic import _write_bam
    p = str(tmp_path / 'plain_gzip.bam')
    _write_bam(p, [('r1', 'ACGT', 'IIII', 0)])
    with pytest.raises(VmxError) as e:
        BamReader(ctx, p)
    assert e.value.code == -7
    q = str(tmp_path / 'notbam.bam')
    open(q, 'wb').write(K.bgzf(b'SAM\x01' + b'\0' * 100))
    with pytest.raises(VmxError) as e:
        BamReader(ctx, q)
    assert e.value.code == -1
    with pytest.raises(VmxError):
        BamReader(ctx, str(tmp_path / 'missing.bam'))


# ---------------------------------------------------------------- 3. malformed input: an error that names the place, or zlib's output

def _outcome(ctx, z):
    """(what zlib gives or None when it refuses, what the device gives or the VmxError)"""
    from vacmap_amd.lib import bgzf_decompress, VmxError
    try:
        want = gzip.decompress(z)
    except Exception:
        want = None
    try:
        got = bgzf_decompress(ctx, z)
    except VmxError as e:
        assert 'file offset' in str(e), str(e)
        return want, e
    assert want is not None and got == want, 'the device accepted what zlib refuses, or gives other bytes'
    return want, got


def _must_fail(ctx, z, word=None):
    from vacmap_amd.lib import VmxError
    want, got = _outcome(ctx, z)
    assert isinstance(got, VmxError), 'accepted'
    if word:
        assert word in str(got), str(got)
    return got


def test_malformed_members(ctx, bam_bytes):
    pl = bam_bytes[:30000]
    raw = K.deflate(pl, 6)
    good = K.member(raw, pl)
    first = K.member(K.deflate(b'hello'), b'hello')
    assert _outcome(ctx, first + good)[1] == b'hello' + pl
    e = _must_fail(ctx, first + good[:-5]); assert 'offset %d' % len(first) in str(e)              # truncated file
    _must_fail(ctx, first + good[:17])
    _must_fail(ctx, first + K.member(raw[:-40], pl), 'offset %d' % len(first))                         # truncated member (BSIZE consistent, deflate cut)
    _must_fail(ctx, first + K.member(raw, pl, crc=zlib.crc32(pl) ^ 1), 'CRC32')
    _must_fail(ctx, first + K.member(raw, pl, isize=len(pl) - 1), 'ISIZE')
    _must_fail(ctx, first + K.member(raw, pl, isize=len(pl) + 1), 'ISIZE')
    _must_fail(ctx, K.member(b'\x07' + raw[1:], pl), 'type 3')                                         # BTYPE 3
    st = K.deflate(pl[:1000], 0)
    bad = bytearray(st); bad[3] ^= 0x10                                                                # NLEN
    _must_fail(ctx, K.member(bytes(bad), pl[:1000]), 'LEN')
    far, _ = K.fixed_stream([65, 66, 67, (5, 4)])
    _must_fail(ctx, K.member(far, b'ABCABCAB'), 'before the member')
    ok, data = K.fixed_stream([65, 66, 67, (5, 3)])
    assert _outcome(ctx, K.member(ok, data))[1] == data
    # over-subscribed code lengths: a dynamic header whose code-length code gives three codes of one bit
    w = K.Bits(); w.put(1, 1); w.put(2, 2); w.put(0, 5); w.put(0, 5); w.put(15, 4)
    for i in range(19):
        w.put(1 if i < 3 else 0, 3)
    w.put(0, 64)
    _must_fail(ctx, K.member(w.bytes(), b''), 'code lengths')
    _must_fail(ctx, b'\x1f\x8b\x08\x04junk' + good)
    _must_fail(ctx, b'PK\x03\x04' + good)


def test_bit_flips_in_the_deflate_payload(ctx, bam_bytes):
    """200 seeded single-bit flips: an error that names the member, or exactly zlib's bytes. Nothing else"""
    from vacmap_amd.lib import VmxError
    pl = bam_bytes[:6000] + K.periodic(5, 1500) + bam_bytes[6000:9000]
    raws = [K.deflate(pl, 6), K.deflate(pl, 6, zlib.Z_FIXED), K.deflate(pl[:3000], 0), K.deflate(pl, 9, flushes=2)]
    rng = np.random.default_rng(99)
    first = K.member(K.deflate(b'abc'), b'abc')
    n_err = 0
    for k in range(200):
        raw = bytearray(raws[k % 4]); data = pl[:3000] if k % 4 == 2 else pl
        bit = int(rng.integers(0, 8 * len(raw))) if k % 2 else int(rng.integers(0, min(8 * len(raw), 1200)))      # half of them in the block header
        raw[bit >> 3] ^= 1 << (bit & 7)
        want, got = _outcome(ctx, first + K.member(bytes(raw), data) + K.BGZF_EOF)
        if isinstance(got, VmxError):
            n_err += 1
            assert 'offset %d' % len(first) in str(got), str(got)
    assert n_err >= 150                                                                                 # (a flip that keeps CRC32 and ISIZE right is the rare case)


def test_bit_flips_in_record_headers(ctx, tmp_path):
    """200 seeded single-bit flips in the 36 fixed bytes of a record: VmxError that names the record (or the member), or the records of the
    reference decoders. driver._bam_chunks is the reference wherever it accepts the bytes; where it raises (it decodes names and qualities
    as text, and slices past a record's end) the byte-level decoder of bam_input_cases decides, which refuses what SAMv1 §4.2 forbids"""
    from vacmap_amd import driver
    from vacmap_amd.lib import BamReader, VmxError
    recs = K.random_reads(12, 8, 20, 400)
    head = K.bam_header('@HD\tVN:1.6\n')
    parts = [K.bam_record(*r, tags=b'XYZ\0' * 3) for r in recs]
    starts = np.concatenate([[0], np.cumsum([len(x) for x in parts])])[:-1] + len(head)
    stream = head + b''.join(parts)
    rng = np.random.default_rng(123)
    outcomes = {'error': 0, 'same': 0}
    for k in range(200):
        s = bytearray(stream)
        at = int(starts[int(rng.integers(0, len(parts)))]) + int(rng.integers(0, 36)); s[at] ^= 1 << int(rng.integers(0, 8))
        p = str(tmp_path / 'f.bam')
        open(p, 'wb').write(K.bgzf(bytes(s), 1, block=3000))
        try:
            want = list(driver._bam_chunks(p, 5))
        except Exception:
            try:
                want = K.chunks_of_records(K.ref_records(bytes(s)), 5)
            except ValueError:
                want = None
        else:
            try:
                K.same_chunks(want, K.chunks_of_records(K.ref_records(bytes(s)), 5))                  # the two references agree where both accept
            except ValueError:
                pass
        rd = None
        try:
            rd = BamReader(ctx, p)
            got = K.read_all(rd, 5)
        except VmxError as e:
            assert 'record' in str(e) or 'offset' in str(e), str(e)
            outcomes['error'] += 1
            continue
        finally:
            if rd is not None:
                rd.close()
        assert want is not None, 'accepted what both references refuse (flip %d)' % k
        K.same_chunks(got, want)
        outcomes['same'] += 1
    assert outcomes['error'] > 0 and outcomes['same'] > 0, outcomes


# ---------------------------------------------------------------- 4. the driver

def _inputs(tmp_path):
    from vacmap_amd import synth
    from test_host_logic import _write_bam
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = tmp_path / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 6, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    reads = [cat[off[i]:off[i + 1]].tobytes().decode() for i in range(6)]
    quals = [B.ont_quals(len(r), 100 + i) for i, r in enumerate(reads)]
    recs = [('b%d' % i, reads[i] if i % 2 == 0 else synth.tostr(synth.revcomp(np.frombuffer(reads[i].encode(), np.uint8))), quals[i] if i % 2 == 0 else quals[i][::-1],
             0 if i % 2 == 0 else 16) for i in range(6)]
    bam = tmp_path / 'reads.bam'
    bam.write_bytes(K.bgzf(K.bam_header() + b''.join(K.bam_record(*r) for r in recs), 6, block=4000))
    plain = tmp_path / 'gz.bam'
    _write_bam(str(plain), recs)
    return fa, bam, plain


@pytest.mark.parametrize('extra', [['-mode', 'H', '--eqx', '--MD'], ['-mode', 'asm']])
def test_driver_native_reader_equals_python_reader(ctx, tmp_path, monkeypatch, capsys, extra):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bam, plain = _inputs(tmp_path)
    common = ['-ref', str(fa), '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd')] + extra

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@PG')]
    assert driver.main(common + ['-read', str(bam), '-o', str(tmp_path / 'py.sam')]) == 0
    assert driver.main(common + ['-read', str(bam), '-o', str(tmp_path / 'nat.sam'), '--bam-reader', 'native']) == 0
    a, b = body(tmp_path / 'py.sam'), body(tmp_path / 'nat.sam')
    assert a == b and sum(1 for x in a if not x.startswith('@')) >= 6
    capsys.readouterr()
    assert driver.main(common + ['-read', str(plain), '-o', str(tmp_path / 'fb.sam'), '--bam-reader', 'native']) == 0
    assert 'not BGZF' in capsys.readouterr().err
    assert body(tmp_path / 'fb.sam') == a
