"""Native BAM input on the MI355X: the device's bytes against the emulator build's and Python's, the wave-ordering test of the match copy
(a back-reference reads what other lanes of the wave stored a moment ago: only real wavefronts can get that wrong), a 2 GB file read
through more than ten windows, and the two rejection paths that are safe to take on a shared GPU."""
import gzip
import os
import time
import zlib

import numpy as np
import pytest

import bam_input_cases as K

pytestmark = pytest.mark.gpu

HDR = '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:5000\n'


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def bam_bytes(ctx):
    from vacmap_amd.lib import BamCodec
    from test_bam_emu import synth_sam
    codec = BamCodec(ctx, HDR)
    b = codec.encode('\n'.join(synth_sam(120, 5)) + '\n')
    codec.close()
    return b


def test_gpu_bgzf_decompress_equals_emulator_and_zlib(ctx, bam_bytes):
    import emu_lib
    from vacmap_amd.lib import bgzf_decompress, bgzf_compress
    ectx = emu_lib.context()
    for name, z in K.inflate_cases(bam_bytes).items():
        got = bgzf_decompress(ctx, z)
        assert got == gzip.decompress(z), name
        assert got == bgzf_decompress(ectx, z), name
    for d in (b'', b'x', bam_bytes, b'\0' * 1000000, K.periodic(3, 700000)):
        assert bgzf_decompress(ctx, bgzf_compress(ctx, d)) == d


def test_gpu_reader_equals_bam_chunks(ctx, tmp_path, monkeypatch):
    """the record cases of the emulator suite on the device: unaligned (1 base to 200 kb, records over two and three members and over
    windows), a header over members and windows, aligned records of the product's codec"""
    import test_bam_input_emu as E
    from vacmap_amd.lib import BamCodec
    head, body = E._ubam_stream()
    p = str(tmp_path / 'u.bam')
    open(p, 'wb').write(K.bgzf(head + body, 6))
    E._check_file(ctx, p)
    codec = BamCodec(ctx, HDR)
    E.test_reader_aligned_bam_from_the_product_codec(ctx, codec, tmp_path)
    codec.close()
    E.test_reader_five_records_of_the_host_logic_test(ctx, tmp_path)
    E.test_reader_max_bases_stops_like_fastx(ctx, tmp_path)
    E._small_windows(monkeypatch)
    for block in (5000, 333):
        open(p, 'wb').write(K.bgzf(head + body, 6, block=block))
        E._check_file(ctx, p)
    E.test_reader_header_straddles_members_and_windows(ctx, tmp_path, monkeypatch)


def _mixed(period, variant):
    """short-period data with literal runs of 1 ... 70 bytes in between: matches at distances below, at and above 64, most with dist < len"""
    rng = np.random.default_rng(period * 100 + variant)
    out = bytearray()
    while len(out) < 2500:
        out += K.periodic(period, int(rng.integers(period + 3, 4 * period + 300)), seed=variant)
        out += rng.integers(0, 256, int(rng.integers(1, 71))).astype(np.uint8).tobytes()
    return bytes(out)


def test_gpu_wave_ordering_of_the_match_copy(ctx):
    """at least 4000 members in one launch, so that waves really overlap: periods 1 ... 130 deflated with Z_RLE and with level 9, and
    hand-assembled fixed-Huffman streams that force dist < len at every distance 1 ... 64. Byte for byte against zlib."""
    from vacmap_amd.lib import bgzf_decompress
    members, want = [], []
    for period in range(1, 131):
        for variant in range(30):
            d = _mixed(period, variant)
            members.append(K.member(K.deflate(d, 9 if variant % 2 else 6, zlib.Z_DEFAULT_STRATEGY if variant % 2 else zlib.Z_RLE), d)); want.append(d)
    for seed in range(120):
        m, d = K.overlap_member(seed)
        members.append(m); want.append(d)
    assert len(members) >= 4000
    z = b''.join(members)
    ref = gzip.decompress(z)
    assert ref == b''.join(want)
    for _ in range(3):
        got = bgzf_decompress(ctx, z)
        if got != ref:
            at = next(i for i in range(min(len(got), len(ref))) if got[i] != ref[i]) if len(got) == len(ref) else -1
            raise AssertionError('the device differs from zlib: lengths %d / %d, first difference at byte %d' % (len(got), len(ref), at))


def test_gpu_scale_two_files_of_2gb(ctx, tmp_path):
    """>= 2 GB of unaligned BAM (15 kb ONT-shape reads), once as zlib level 6 members and once through the device deflate: per-read
    checksums of names, bases and qualities equal the generator's, and the reader crosses at least 10 windows"""
    from vacmap_amd.lib import BamReader
    t0 = time.time()
    head, recs, want = K.scale_records(2 << 30)
    total = len(head) + sum(len(r) for r in recs)
    assert total >= 2 << 30
    print('generated %d reads, %.2f GB in %.0f s' % (len(recs), total / 1e9, time.time() - t0))
    for kind in ('zlib6', 'device'):
        p = str(tmp_path / (kind + '.bam'))
        t0 = time.time()
        if kind == 'zlib6':
            K.write_bgzf_zlib(p, [head] + recs)
        else:
            K.write_bgzf_device(p, [head] + recs, ctx)
        t1 = time.time()
        rd = BamReader(ctx, p)
        got = K.read_checksums(rd)
        st = rd.stats()
        rd.close()
        t2 = time.time()
        print('%s: file %.2f GB written in %.0f s; read with checksums in %.1f s; %s' % (kind, os.path.getsize(p) / 1e9, t1 - t0, t2 - t1, {k: round(v, 3) for k, v in st.items()}))
        assert len(got) == len(want)
        assert got == want
        assert st['windows'] >= 10 and st['inflated_bytes'] == total and st['dropped'] == 0
        os.remove(p)


def test_gpu_rejects_wrong_crc_and_truncated_file(ctx, bam_bytes, tmp_path):
    from vacmap_amd.lib import bgzf_decompress, BamReader, VmxError
    pl = bam_bytes[:50000]
    first = K.member(K.deflate(b'hello'), b'hello')
    with pytest.raises(VmxError) as e:
        bgzf_decompress(ctx, first + K.member(K.deflate(pl), pl, crc=zlib.crc32(pl) ^ 0x8000))
    assert 'CRC32' in str(e.value) and 'offset %d' % len(first) in str(e.value)
    z = K.bgzf(K.bam_header() + b''.join(K.bam_record(*r) for r in K.random_reads(50, 3, 100, 5000)), 6)
    p = str(tmp_path / 't.bam')
    open(p, 'wb').write(z[:len(z) * 2 // 3])
    rd = BamReader(ctx, p)
    try:
        with pytest.raises(VmxError) as e:
            K.read_all(rd, 1000)
    finally:
        rd.close()                                                          # (a reader is closed before its context)
    assert 'truncated' in str(e.value)
