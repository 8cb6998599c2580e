"""Coordinate-sorted BAM and CSI on the MI355X: device bytes identical to the emulator build's, golden cases through the driver with
--bam-writer native-sort, and a 2 GB external sort. Decoding by tests/bam_codec.py and tests/csi_codec.py (independent of the product)."""
import json
import os
import time
import zlib

import numpy as np
import pytest

import bam_codec as B
import csi_codec as C
from test_bam_sorted_emu import HEAD, calls_of, check_index_by_use, check_index_structure, make_lines

pytestmark = pytest.mark.gpu


def _key(rec):
    """(offset, refID, pos, end, flag, bin) of csi_codec.Bam.scan -> the sort key"""
    return (rec[1] & 0xffffffff) << 32 | ((rec[2] + 1) & 0xffffffff) << 1 | (rec[4] >> 4 & 1)


def test_gpu_sorted_bam_and_csi_match_emulator(tmp_path):
    """a multi-call input with forced small chunks: the device's .sorted.bam and .csi equal the emulator build's byte for byte"""
    import emu_lib
    from vacmap_amd.bamout import SortedBamWriter
    calls = calls_of(make_lines())
    out = {}
    for name, lib in (('dev', None), ('emu', emu_lib.context().lib)):
        p = str(tmp_path / (name + '.sorted.bam'))
        w = SortedBamWriter(p, HEAD, lib=lib, chunk_bytes=20000)
        for c in calls:
            w.write_parts(*c)
        w.close()
        out[name] = (open(p, 'rb').read(), open(p + '.csi', 'rb').read())
    assert out['dev'][0] == out['emu'][0]
    assert out['dev'][1] == out['emu'][1]
    bam, idx = C.Bam(out['dev'][0]), C.parse(out['dev'][1])
    assert len(check_index_structure(bam, idx)) == len(make_lines())
    assert sorted(os.listdir(tmp_path)) == ['dev.sorted.bam', 'dev.sorted.bam.csi', 'emu.sorted.bam', 'emu.sorted.bam.csi']


def test_gpu_driver_native_sort_golden(tmp_path):
    """golden cases A and B through the driver with --bam-writer native-sort: the same multiset of lines as the reference's, in key order, and a usable index"""
    import sam_cases as SC
    from vacmap_amd import driver
    here = os.path.dirname(__file__)
    meta = json.load(open(os.path.join(here, 'golden', 'cases.json')))
    arrays = np.load(os.path.join(here, 'golden', 'cases.npz'))
    entries = [e for e in json.load(open(os.path.join(here, 'golden', 'sam.json')))
               if e['opt'] == {'md': False, 'shortcs': True, 'cigar2cg': False, 'markunbalancetra': True, 'H': False, 'fakecigar': False, 'rg': '1'}]
    for cid in ('A', 'B'):
        c = meta[cid]
        ref = tmp_path / ('ref%s.fa' % cid); fq = tmp_path / ('reads%s.fq' % cid); out = tmp_path / ('out%s.sorted.bam' % cid)
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
                            '--bam-writer', 'native-sort']) == 0
        data = open(out, 'rb').read()
        text, refs, recs = B.read_bam(data)
        hdr = [x for x in text.split('\n') if x]
        assert hdr[0] == '@HD\tVN:1.0\tSO:coordinate' and [r[0] for r in refs] == list(c['names']) and hdr[-1].startswith('@PG\tID:VACmap')
        assert sorted(SC.digest(B.to_sam(r)) for r in recs) == sorted(expect), cid
        bam, idx = C.Bam(data), C.parse(open(str(out) + '.csi', 'rb').read())
        scan = check_index_structure(bam, idx)
        keys = [_key(r) for r in scan]
        assert len(scan) == len(expect) and all(a <= b for a, b in zip(keys, keys[1:])), cid
        n, full = check_index_by_use(bam, idx, seed=31, per_ref=60)
        assert n == 60 * len(refs) and full > 0
        assert sorted(x for x in os.listdir(tmp_path) if x.startswith('out%s' % cid) or x.startswith('.bamsort')) == ['out%s.sorted.bam' % cid, 'out%s.sorted.bam.csi' % cid]


SCALE_REFS = [('chr1', 50000000), ('chr2', 20000000), ('chr3', 5000000)]
SCALE_HEAD = ['@HD\tVN:1.6'] + ['@SQ\tSN:%s\tLN:%d' % r for r in SCALE_REFS]


def test_gpu_sorted_bam_at_scale(tmp_path):
    """>= 2 GB of BAM-like records in >= 8 runs and >= 8 chunks: keys non-decreasing over the whole file, the multiset of records preserved
    (count and a sum of per-record CRCs), the index usable on 100 regions. 128 MB chunks and ~250 MB runs: keys (16 B per record), the staged
    chunk, the gathered chunk and its deflate slots are a few hundred MB of device memory."""
    from test_bam_emu import synth_sam
    from vacmap_amd.bamout import SortedBamWriter
    from vacmap_amd.lib import BamCodec
    unit = [ln.split('\t') for ln in synth_sam(300, seed=61, mean_len=3000)]
    rng = np.random.default_rng(62)
    path = str(tmp_path / 'big.sorted.bam')
    w = SortedBamWriter(path, SCALE_HEAD, chunk_bytes=128 << 20)
    codec = BamCodec(w.ctx, ''.join(x + '\n' for x in SCALE_HEAD))
    want_n = want_crc = want_bytes = 0
    n_calls = 0
    t0 = time.time()
    while want_bytes < (2 << 30) + (64 << 20) or n_calls < 8:
        lines, size = [], 0
        while size < 330 << 20:                                                       # about 250 MB of records per call
            rid = rng.choice(3, size=len(unit), p=[0.6, 0.3, 0.1])
            for f, r, x in zip(unit, rid, rng.random(len(unit))):                     # seeded references and positions: the keys are not periodic
                name, ln = SCALE_REFS[r]
                lines.append('\t'.join([f[0], f[1], name, str(1 + int(x * (ln - 7000)))] + f[4:]) + '\n')
                size += len(lines[-1])
        text = ''.join(lines).encode()
        del lines
        raw = codec.encode(text)                                                      # the expected multiset, from the unsorted encoder
        p = 0
        mv = memoryview(raw)
        while p < len(raw):
            bs = int.from_bytes(mv[p:p + 4], 'little')
            want_crc += zlib.crc32(mv[p:p + 4 + bs]); want_n += 1
            p += 4 + bs
        want_bytes += len(raw)
        del raw, mv
        w.write(text)
        n_calls += 1
    t_in = time.time() - t0
    assert n_calls >= 8 and len(w.runs) == n_calls and w.run_bytes == want_bytes >= 2 << 30
    codec.close()
    t0 = time.time()
    w.close()
    t_close = time.time() - t0
    assert sorted(os.listdir(tmp_path)) == ['big.sorted.bam', 'big.sorted.bam.csi']
    size = os.path.getsize(path)
    print('\nsorted BAM at scale: %d records, %.3f GB of records in %d runs; input + per-run sort %.1f s; close() (merge + index) %.2f s = %.2f GB/s of records; '
          'file %.3f GB, index %d bytes' % (want_n, want_bytes / 1e9, n_calls, t_in, t_close, want_bytes / 1e9 / t_close, size / 1e9, os.path.getsize(path + '.csi')))
    bam = C.Bam(open(path, 'rb').read())
    assert sum(1 for s in bam.sizes[1:-1] if 0 < s < 65280) >= 8                       # at least 8 chunks ended their last member early
    scan = bam.scan()
    assert len(scan) == want_n and len(bam.raw) - bam.body == want_bytes
    a = np.array(scan, dtype=np.int64)
    keys = (a[:, 1] & 0xffffffff) << 32 | ((a[:, 2] + 1) & 0xffffffff) << 1 | (a[:, 4] >> 4 & 1)
    assert _key(scan[7]) == int(keys[7]) and bool(np.all(keys[1:] >= keys[:-1]))
    got_crc = 0
    mv = memoryview(bam.raw)
    ends = list(a[1:, 0]) + [len(bam.raw)]
    for r, e in zip(scan, ends):
        got_crc += zlib.crc32(mv[r[0]:e])
    assert got_crc == want_crc
    idx = C.parse(open(path + '.csi', 'rb').read())
    assert idx['n_no_coor'] == 0 and sum(r['meta'][2] for r in idx['refs']) == want_n
    rng = np.random.default_rng(63)
    full = 0
    for i in range(100):
        rid = i % 3
        ln = SCALE_REFS[rid][1]
        beg = int(rng.integers(0, ln - 1))
        end = min(ln, beg + (1, 5000, 200000, 20000)[i % 4])
        want = [int(u) for u in a[(a[:, 1] == rid) & (a[:, 2] < end) & (a[:, 3] > beg), 0]]
        assert C.fetch(bam, idx, rid, beg, end) == want, (rid, beg, end)
        full += bool(want)
    assert full >= 50
