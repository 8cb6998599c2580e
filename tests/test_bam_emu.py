"""Native BAM output (vm_bam_*, vm_bgzf_compress, vacmap_amd.bamout, driver --bam-writer native) on the CPU emulator build of the kernels
(tests/emu). Every BAM / BGZF byte is decoded by tests/bam_codec.py, a reader written from SAMv1 that shares no code with the product."""
import ctypes
import gzip
import os
import struct
import zlib

import numpy as np
import pytest

import bam_codec as B

HDR = '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:5000\n'
REFS = ['chr1', 'chr2']


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


def synth_sam(n_reads, seed, mean_len=1500):
    """SAM lines of ONT-shape reads with seeded Markov-chain qualities (the input of the ratio bar)"""
    from vacmap_amd import synth
    contigs = synth.make_reference([300000], seed=seed)
    cat, off, _ = synth.sample_reads_concat(contigs, n_reads, mean_len=mean_len, err=0.08, seed=seed + 1, min_len=300, max_len=6000)
    rng = np.random.default_rng(seed + 2)
    lines = []
    for i in range(n_reads):
        s = cat[off[i]:off[i + 1]].tobytes().decode()
        q = B.ont_quals(len(s), seed * 1000 + i)
        pos = int(rng.integers(1, 290000))
        nm = int(rng.integers(0, len(s) // 8 + 1))
        lines.append('%08x-%04x-read%d\t%d\tchr1\t%d\t%d\t%dM\t*\t0\t0\t%s\t%s\tNM:i:%d\tAS:i:%d\tde:f:%.4f\trl:i:%d\tRG:Z:1'
                     % (int(rng.integers(0, 1 << 31)), i, i, 16 * int(rng.integers(0, 2)), pos, int(rng.integers(0, 61)), len(s), s, q, nm, 2 * len(s) - 3 * nm,
                        nm / len(s), len(s)))
    return lines


def bam_like(codec, n_reads, seed):
    text = '\n'.join(synth_sam(n_reads, seed)) + '\n'
    return codec.encode(text)


# ---------------------------------------------------------------- 1. BGZF round trip

def _check_roundtrip(ctx, data):
    from vacmap_amd.lib import bgzf_compress
    z = bgzf_compress(ctx, data)
    assert bgzf_compress(ctx, data) == z                                 # deterministic
    assert gzip.decompress(z) == data
    mem = B.bgzf_members(z + B.BGZF_EOF)
    assert B.bgzf_decompress(z + B.BGZF_EOF) == data
    assert len(mem) == 1 + (len(data) + 65279) // 65280                  # + the EOF block
    assert all(len(pl) <= 65280 for _, pl in mem)
    return z, len(mem) - 1


@pytest.mark.parametrize('n', [0, 1, 65279, 65280, 65281])
def test_bgzf_roundtrip_sizes(ctx, n):
    data = np.random.default_rng(n).integers(0, 6, n).astype(np.uint8).tobytes()
    _check_roundtrip(ctx, data)


def test_bgzf_roundtrip_zeros_random_bam(ctx, codec):
    z, nm = _check_roundtrip(ctx, b'\0' * (1 << 20))
    assert len(z) < 20000
    rnd = np.random.default_rng(5).integers(0, 256, 1 << 20).astype(np.uint8).tobytes()
    z, nm = _check_roundtrip(ctx, rnd)
    assert len(z) <= len(rnd) + 31 * nm                                  # stored members: 18 + 5 + 8 bytes of framing each
    _check_roundtrip(ctx, bam_like(codec, 60, seed=7))


# ---------------------------------------------------------------- 2. ratio bar against zlib

def test_ratio_against_zlib_level1(ctx, codec):
    from vacmap_amd.lib import bgzf_compress
    data = bam_like(codec, 500, seed=21)
    mine = len(bgzf_compress(ctx, data))

    def zl(level):
        tot = 0
        for i in range(0, len(data), 65280):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            tot += len(c.compress(data[i:i + 65280]) + c.flush()) + 26
        return tot
    l1, l6 = zl(1), zl(6)
    print('BAM of 500 reads: %d bytes; device %d = %.3f x zlib -1 (%d), %.3f x zlib -6 (%d)' % (len(data), mine, mine / l1, l1, mine / l6, l6))
    assert mine <= 1.10 * l1


# ---------------------------------------------------------------- 3. encoder rules

LINES = [
    'r1\t0\tchr1\t100\t60\t5M2I3M\t=\t200\t50\tACGTAcgtnn\tABCDEFGHIJ\tNM:i:3\tXA:A:x\tXh:H:1AE3\tXZ:Z:hello world',
    'r2\t4\t*\t0\t0\t*\t*\t0\t0\tMRSVWYHKDB=Xacgtmrsvwyhkdbn\t*',
    'r3\t16\tchr2\t1\t255\t*\tchr1\t5\t-10\t*\t*\tCG:Z:10M5D3M',
    'r4\t0\tchr2\t4999\t7\t1S1M\tchr2\t1\t0\tAC\t!~\tXi:i:-129\tXj:i:-128\tXk:i:127\tXl:i:128\tXm:i:255\tXn:i:256\tXo:i:65535\tXp:i:65536'
    '\tXq:i:2147483647\tXr:i:4294967295\tXs:i:-32768\tXt:i:-32769\tXu:i:-2147483648',
    'r5\t0\tchr1\t16385\t60\t100M20D5N2=3X\t*\t0\t0\t' + 'A' * 110 + '\t' + 'I' * 110 + '\tf1:f:1.5\tf2:f:-0.1\tf3:f:123.456e-5\tf4:f:0'
    '\tf5:f:3.14159265358979323846\tf6:f:1e-40\tf7:f:3.4028235e38\tf8:f:inf\tf9:f:nan\tfa:f:-2.5E+30',
    'r6\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\t*\tBa:B:c,-128,0,127\tBb:B:C,0,255\tBc:B:s,-32768,32767\tBd:B:S,0,65535\tBe:B:i,-2147483648,2147483647'
    '\tBf:B:I,0,4294967295\tBg:B:f,1.5,-0.1,2.2250738585072014e-308,7e-46\tBh:B:i',
]


def test_encoder_rules_decode_back(codec):
    raw = codec.encode('\n'.join(LINES))                                 # (last line without its newline)
    recs = B.records(raw, REFS)
    assert len(recs) == len(LINES)
    for r, ln in zip(recs, LINES):
        assert B.same_as_sam(r, ln), (B.to_sam(r), ln)
    fields, tags = recs[3]
    types = {}
    p = 0
    for _ in range(3):
        p += 4 + struct.unpack_from('<i', raw, p)[0]
    rec = raw[p + 4:p + 4 + struct.unpack_from('<i', raw, p)[0]]
    q = rec.index(b'Xi')
    while q < len(rec):                                                  # the integer types chosen, as htslib chooses them
        tg, ty = rec[q:q + 2].decode(), chr(rec[q + 2])
        types[tg] = ty
        q += 3 + {'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4}[ty]
    assert types == {'Xi': 's', 'Xj': 'c', 'Xk': 'C', 'Xl': 'C', 'Xm': 'C', 'Xn': 'S', 'Xo': 'S', 'Xp': 'I', 'Xq': 'I', 'Xr': 'I',
                     'Xs': 's', 'Xt': 'i', 'Xu': 'i'}
    f = dict((t[0], t[2]) for t in recs[4][1])
    assert f['f5'] == np.float32(3.14159265358979323846) and f['f6'] == np.float32(1e-40) and f['f8'] == np.inf and f['f9'] != f['f9']


def test_encoder_long_cigar_uses_cg_tag(codec):
    cig = '1M1I' * 35000
    ln = 'rb\t0\tchr1\t1\t60\t%s\t*\t0\t0\t%s\t*\tNM:i:35000' % (cig, 'A' * 70000)
    raw = codec.encode(ln + '\n')
    ncig = struct.unpack_from('<H', raw, 4 + 12)[0]
    assert ncig == 2
    c0, c1 = struct.unpack_from('<II', raw, 4 + 32 + 3)
    assert (c0 & 15, c0 >> 4, c1 & 15, c1 >> 4) == (4, 70000, 3, 35000)     # 70000S35000N
    assert b'CGBI' in raw
    r = B.records(raw, REFS)[0]
    assert B.same_as_sam(r, ln)


def test_encoder_long_cigar_without_seq_and_oplen_limit(codec):
    from vacmap_amd.lib import VmxError
    ln = 'rc\t0\tchr1\t1\t60\t%s\t*\t0\t0\t*\t*' % ('2M1D' * 33000)
    raw = codec.encode(ln + '\n')
    c0, c1 = struct.unpack_from('<II', raw, 4 + 32 + 3)
    assert (c0 & 15, c0 >> 4, c1 & 15, c1 >> 4) == (4, 0, 3, 99000)          # <l_seq = 0>S<span>N, as htslib expects it
    assert B.same_as_sam(B.records(raw, REFS)[0], ln)
    assert B.records(codec.encode('r\t0\tchr1\t1\t60\t268435455N\t*\t0\t0\t*\t*\n'), REFS)[0][0][5] == '268435455N'
    with pytest.raises(VmxError) as e:                                    # 2^28 does not fit the 28-bit length field
        codec.encode('r\t0\tchr1\t1\t60\t268435456N\t*\t0\t0\t*\t*\n')
    assert e.value.code == -1 and 'line 1' in str(e.value)


def test_encoder_bytes_by_hand(codec):
    raw = codec.encode('r\t0\tchr1\t1\t60\t2M\t*\t0\t0\tAC\tII\tNM:i:1\nu\t4\t*\t0\t0\t*\t*\t0\t0\tA\t*\n')
    r1 = struct.pack('<iiiBBHHHiiii', 45, 0, 0, 2, 60, 4681, 1, 0, 2, -1, -1, 0) + b'r\0' + struct.pack('<I', 2 << 4) + bytes([0x12, 40, 40]) + b'NMC\x01'
    r2 = struct.pack('<iiiBBHHHiiii', 36, -1, -1, 2, 0, 4680, 0, 4, 1, -1, -1, 0) + b'u\0' + bytes([0x10, 0xff])
    assert raw == r1 + r2


# ---------------------------------------------------------------- 4. errors and the NULL context

@pytest.mark.parametrize('bad', ['x\t0\tchrZ\t1\t0\t*\t*\t0\t0\t*\t*', 'a\t0\t*\t1\t0\t*\t*\t0\t0\t*', 'a\t0\t*\t1\t0\t*\t*\t0\t0\tAC\tA',
                                 'n' * 255 + '\t0\t*\t1\t0\t*\t*\t0\t0\t*\t*', 'a\t0\t*\tx1\t0\t*\t*\t0\t0\t*\t*', 'a\t0\t*\t1\t0\t3Q\t*\t0\t0\t*\t*'])
def test_encoder_errors_name_the_line(codec, bad):
    from vacmap_amd.lib import VmxError
    with pytest.raises(VmxError) as e:
        codec.encode(LINES[1] + '\n' + LINES[2] + '\n' + bad + '\n')
    assert e.value.code == -1 and 'line 3' in str(e.value)


def test_null_context(ctx):
    L = ctx.lib.L
    p, n, h = ctypes.c_void_p(), ctypes.c_int64(), ctypes.c_void_p()
    assert L.vm_bgzf_compress(None, b'x', 1, ctypes.byref(p), ctypes.byref(n)) == -3
    assert L.vm_bam_writer_create(None, b'', 0, ctypes.byref(h)) == -3
    assert L.vm_bam_encode(None, b'x', 1, ctypes.byref(p), ctypes.byref(n)) == -3


# ---------------------------------------------------------------- 5. the driver end to end

def _inputs(tmp_path, ctx):
    from vacmap_amd import synth
    from test_host_logic import _write_bam
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = tmp_path / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 6, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    reads = [cat[off[i]:off[i + 1]].tobytes().decode() for i in range(6)]
    quals = [B.ont_quals(len(r), 100 + i) for i, r in enumerate(reads)]
    fq = tmp_path / 'r.fq.gz'
    with gzip.open(fq, 'wt') as f:
        for i in range(4):
            f.write('@q%d XI:i:%d\tXF:f:%s\tXB:B:s,1,-2,%d\n%s\n+\n%s\n' % (i, -129 * i, ['0.5', '3.14159265358979323846', '-1e-3', '1e30'][i], i,
                                                                         reads[i].lower() if i == 1 else reads[i], quals[i]))
    bam = tmp_path / 'more.bam'
    _write_bam(str(bam), [('b4', reads[4], quals[4], 0), ('b5', synth.tostr(synth.revcomp(np.frombuffer(reads[5].encode(), np.uint8))), quals[5][::-1], 16)])
    asm = tmp_path / 'asm.fa'
    asm.write_text(''.join('>ctg%d\n%s\n' % (i, reads[i]) for i in range(4)))
    return fa, fq, bam, asm


def _same(sam_path, bam_path):
    lines = [x for x in open(sam_path).read().split('\n') if x]
    hdr = [x for x in lines if x.startswith('@')]; body = [x for x in lines if not x.startswith('@')]
    text, refs, recs = B.read_bam(open(bam_path, 'rb').read())
    bh = [x for x in text.split('\n') if x]
    assert [x for x in bh if not x.startswith('@PG')] == [x for x in hdr if not x.startswith('@PG')] and any(x.startswith('@PG') for x in bh)
    assert [r[0] for r in refs] == [x.split('\t')[1][3:] for x in hdr if x.startswith('@SQ')]
    assert len(recs) == len(body) and body
    for r, ln in zip(recs, body):
        assert B.same_as_sam(r, ln), (B.to_sam(r)[:200], ln[:200])
    return body


@pytest.mark.parametrize('extra', [['-mode', 'H', '--eqx', '--MD', '--copycomments'], ['-mode', 'H', '--L', '--copycomments'], ['-mode', 'asm', '--copycomments']])
def test_driver_native_bam_equals_sam(ctx, tmp_path, monkeypatch, extra):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, fq, bam, asm = _inputs(tmp_path, ctx)
    reads = [str(asm)] if 'asm' in extra else [str(fq), str(bam)]
    common = ['-ref', str(fa), '-read'] + reads + ['-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2',
                                                  '-workdir', str(tmp_path / 'wd')] + extra
    assert driver.main(common + ['-o', str(tmp_path / 'x.sam')]) == 0
    assert driver.main(common + ['-o', str(tmp_path / 'x.bam'), '--bam-writer', 'native']) == 0
    body = _same(tmp_path / 'x.sam', tmp_path / 'x.bam')
    if 'asm' not in extra:
        txt = '\n'.join(body)
        assert 'XF:f:3.14159265358979323846' in txt and 'XB:B:s,1,-2,3' in txt and 'XI:i:-387' in txt   # the comments went through --copycomments


def test_driver_native_sorted_bam_and_missing_samtools(ctx, tmp_path, monkeypatch):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, fq, bam, asm = _inputs(tmp_path, ctx)
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2']
    with pytest.raises(SystemExit) as e:
        driver.main(common + ['-o', str(tmp_path / 'x.sorted.bam'), '--bam-writer', 'native'])
    assert 'unsorted' in str(e.value.code) and not os.path.exists(tmp_path / 'x.sorted.bam')
    monkeypatch.setenv('PATH', str(tmp_path))                            # no samtools: the default writer exits as before
    with pytest.raises(SystemExit) as e:
        driver.main(common + ['-o', str(tmp_path / 'y.bam')])
    assert 'samtools' in str(e.value.code)
