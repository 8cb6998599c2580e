"""Native BAM output on the MI355X: BGZF round trip at scale, device bytes identical to the emulator build's, golden cases through the
driver with --bam-writer native. Decoding by tests/bam_codec.py (independent of the product)."""
import gzip
import json
import os

import numpy as np
import pytest

import bam_codec as B

pytestmark = pytest.mark.gpu

HDR = '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000000\n@SQ\tSN:chr2\tLN:5000\n'


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


def _bam_like(codec, n_reads, seed):
    from test_bam_emu import synth_sam
    return codec.encode('\n'.join(synth_sam(n_reads, seed, mean_len=3000)) + '\n')


def test_gpu_bgzf_roundtrip_at_scale(ctx):
    from vacmap_amd.lib import BamCodec, bgzf_compress
    rng = np.random.default_rng(3)
    for n in (0, 1, 65279, 65280, 65281):
        d = rng.integers(0, 6, n).astype(np.uint8).tobytes()
        z = bgzf_compress(ctx, d)
        assert gzip.decompress(z) == d and bgzf_compress(ctx, d) == z
    z = bgzf_compress(ctx, b'\0' * (1 << 20))
    assert B.bgzf_decompress(z + B.BGZF_EOF) == b'\0' * (1 << 20)
    rnd = rng.integers(0, 256, 1 << 20).astype(np.uint8).tobytes()
    z = bgzf_compress(ctx, rnd)
    assert B.bgzf_decompress(z + B.BGZF_EOF) == rnd and len(z) <= len(rnd) + 31 * 17
    codec = BamCodec(ctx, HDR)
    unit = _bam_like(codec, 400, seed=31)
    codec.close()
    big = unit * ((256 << 20) // len(unit) + 1)
    z = bgzf_compress(ctx, big)
    mem = B.bgzf_members(z + B.BGZF_EOF)
    assert len(mem) - 1 == (len(big) + 65279) // 65280 >= 4000
    assert b''.join(pl for _, pl in mem) == big
    assert bgzf_compress(ctx, big) == z                                  # the same bytes on every run
    print('BGZF of %.0f MB BAM-like bytes: %d members, ratio %.3f' % (len(big) / 1e6, len(mem) - 1, len(z) / len(big)))


def test_gpu_bam_matches_emulator(ctx):
    """the device's records and BGZF members equal the emulator build's byte for byte (no dependence on wave scheduling)"""
    import emu_lib
    from vacmap_amd.lib import BamCodec, bgzf_compress
    from test_bam_emu import synth_sam, LINES
    ectx = emu_lib.context()
    text = '\n'.join(synth_sam(150, seed=77, mean_len=3000) + LINES) + '\n'
    dc, ec = BamCodec(ctx, HDR), BamCodec(ectx, HDR)
    rec = dc.encode(text)
    assert rec == ec.encode(text)
    data = (rec * ((8 << 20) // len(rec) + 1))[:8 << 20]
    assert bgzf_compress(ctx, data) == bgzf_compress(ectx, data)
    assert dc.header() == ec.header()
    dc.close(); ec.close()


@pytest.fixture(scope='module')
def golden():
    meta = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'cases.json')))
    arrays = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'cases.npz'))
    return meta, arrays


def test_gpu_driver_native_bam_golden(ctx, golden, tmp_path):
    """golden cases A and B through the driver with --bam-writer native: the decoded body lines digest to the reference's lines"""
    import sam_cases as SC
    from vacmap_amd import driver
    meta, arrays = golden
    entries = [e for e in json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'sam.json')))
               if e['opt'] == {'md': False, 'shortcs': True, 'cigar2cg': False, 'markunbalancetra': True, 'H': False, 'fakecigar': False, 'rg': '1'}]
    for cid in ('A', 'B'):
        c = meta[cid]
        ref = tmp_path / ('ref%s.fa' % cid); fq = tmp_path / ('reads%s.fq' % cid); out = tmp_path / ('out%s.bam' % cid)
        with open(ref, 'w') as f:
            for i, n in enumerate(c['names']):
                s = arrays['%s_contig%d' % (cid, i)].tobytes().decode()
                f.write('>%s\n' % n)
                for x in range(0, len(s), 80):
                    f.write(s[x:x + 80] + '\n')
        expect = []
        with open(fq, 'w') as f:
            for ri, r in enumerate(c['reads']):
                q = arrays['%s_r%d_seq' % (cid, ri)].tobytes().decode()
                f.write('@%s\n%s\n+\n%s\n' % (r['name'], q, ''.join(chr(33 + (7 * i) % 40) for i in range(len(q)))))
                expect += [d for e in entries if e['case'] == cid and e['read'] == ri for d in e['digest']]
        assert driver.main(['-ref', str(ref), '-read', str(fq), '-mode', c['mode'], '-k', str(c['k']), '-o', str(out), '-t', '2', '--nowriteindex',
                            '--bam-writer', 'native']) == 0
        text, refs, recs = B.read_bam(open(out, 'rb').read())
        hdr = [x for x in text.split('\n') if x]
        assert hdr[0] == '@HD\tVN:1.0' and [r[0] for r in refs] == list(c['names']) and hdr[-1].startswith('@PG\tID:VACmap')
        assert [SC.digest(B.to_sam(r)) for r in recs] == expect, cid
