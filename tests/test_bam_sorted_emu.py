"""Coordinate-sorted BAM and its CSI index (vm_bam_sorter_*, vacmap_amd.bamout.SortedBamWriter, driver --bam-writer native-sort) on the CPU
emulator build of the kernels (tests/emu). The BAM is decoded by tests/bam_codec.py and the index by tests/csi_codec.py, readers written
from the specifications that share no code with the product.

Sort order under test: ascending uint32(refID) << 32 | uint32(pos + 1) << 1 | reverse-strand bit, ties in the order the lines were handed
over (refID -1 last). No samtools is involved anywhere: nothing here claims byte equality with it."""
import bisect
import os

import numpy as np
import pytest

import bam_codec as B
import csi_codec as C

REFS = [('chrA', 400000), ('chrB', 150000), ('chrC', 20000), ('chrD', 70000)]          # chrD gets no record
HEAD = ['@HD\tVN:1.6\tSO:unsorted\tGO:none'] + ['@SQ\tSN:%s\tLN:%d' % r for r in REFS] + ['@PG\tID:test\tPN:test']
CHUNK = 20000                                                                          # record bytes per output chunk: forces many chunks


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


def make_lines(seed=5, n=1300):
    """SAM lines over three references: both strands, many equal (reference, POS) pairs, secondary / supplementary lines, RNAME '*', one CIGAR of
    more than 65 535 operations, a read that ends in the last base of its contig, spans that cross 16 kb and 128 kb bin borders.
    chrA[300000, 360000) stays empty (regions without a record)."""
    rng = np.random.default_rng(seed)
    spots = {'chrA': [int(x) for x in rng.integers(1, 290000, 160)] + [16380, 131060, 262100], 'chrB': [int(x) for x in rng.integers(1, 140000, 60)],
             'chrC': [int(x) for x in rng.integers(1, 15000, 12)]}
    lines = []
    for i in range(n):
        ref = ('chrA', 'chrA', 'chrA', 'chrB', 'chrB', 'chrC')[int(rng.integers(0, 6))]
        pos = spots[ref][int(rng.integers(0, len(spots[ref])))]
        flag = 16 * int(rng.integers(0, 2)) + (256 if rng.random() < 0.1 else 0) + (2048 if rng.random() < 0.1 else 0)
        ln = int(rng.integers(8, 60))
        seq = ''.join('ACGT'[int(x)] for x in rng.integers(0, 4, ln))
        kind = rng.random()
        if kind < 0.7:
            cig = '%dM' % ln
        elif kind < 0.9:
            cig = '%dS%dM%dD%dM' % (2, ln - 6, int(rng.integers(1, 4000)), 4)
        else:
            cig = '%dM%dN%dM' % (4, int(rng.integers(10000, 140000)), ln - 4)
        span = sum(int(x) for x, op in _cigar(cig) if op in 'MDN=X')
        if pos + span - 1 > dict(REFS)[ref]:
            cig = '%dM' % ln
        lines.append('q%d\t%d\t%s\t%d\t%d\t%s\t*\t0\t0\t%s\t%s\tNM:i:%d\tXo:i:%d' % (i, flag, ref, pos, int(rng.integers(0, 61)), cig, seq, 'I' * ln, i % 7, i))
    for i in range(25):                                                                # RNAME '*': unplaced, on both strands
        lines.insert(int(rng.integers(0, len(lines))), 'u%d\t%d\t*\t0\t0\t*\t*\t0\t0\tACGTAC\t*\tXo:i:%d' % (i, 4 + 16 * (i % 2), i))
    for i in range(6):                                                                 # flagged unmapped but placed: indexed, counted as unmapped
        lines.insert(int(rng.integers(0, len(lines))), 'p%d\t4\tchrB\t%d\t0\t*\t*\t0\t0\tACGT\t*' % (i, 500 + 16384 * i))
    lines.insert(700, 'big\t0\tchrA\t20001\t60\t%s\t*\t0\t0\t*\t*\tNM:i:33000' % ('2M1D' * 33000))      # 66 000 operations, span 99 000
    lines.insert(300, 'last\t16\tchrC\t19991\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII')                # ends in chrC's last base
    lines.insert(100, 'first\t0\tchrA\t1\t60\t10M\t*\t0\t0\tACGTACGTAC\tIIIIIIIIII')
    return lines


def _cigar(c):
    out, num = [], ''
    for ch in c:
        if ch.isdigit():
            num += ch
        else:
            out.append((num, ch)); num = ''
    return out


def calls_of(lines, n_calls=7):
    """the lines as write_parts arguments: n_calls calls of two blobs each with interleaved order keys; call 2 is empty, call 4 holds one line"""
    cuts = sorted(set(int(x) for x in np.linspace(0, len(lines), n_calls - 1)))
    groups = [lines[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    groups.insert(2, []); groups.insert(4, [groups[4].pop()])
    calls = []
    for g in groups:
        parts = [g[0::2], g[1::2]]
        blobs, offs, keys = [], [], []
        for k, p in enumerate(parts):
            txt = [(x + '\n').encode() for x in p]
            blobs.append(np.frombuffer(b''.join(txt) or b'\0', np.uint8))
            offs.append(np.concatenate([[0], np.cumsum([len(t) for t in txt])]).astype(np.int64))
            keys.append(np.arange(k, 2 * len(p), 2, dtype=np.int64))
        calls.append((blobs, offs, keys))
    return calls


def sort_key(names):
    def key(rec):
        f = rec[0]
        rid = names.index(f[2]) if f[2] != '*' else 0xffffffff
        return rid << 32 | (int(f[3]) & 0xffffffff) << 1 | (int(f[1]) >> 4 & 1)
    return key


def write_both(lib, tmp, calls, head=HEAD, chunk=CHUNK):
    from vacmap_amd.bamout import BamWriter, SortedBamWriter
    wd = os.path.join(tmp, 'wd'); os.makedirs(wd, exist_ok=True)
    up, sp = os.path.join(tmp, 'u.bam'), os.path.join(tmp, 's.sorted.bam')
    for w in (BamWriter(up, head, lib=lib), SortedBamWriter(sp, head, lib=lib, workdir=wd, chunk_bytes=chunk)):
        for c in calls:
            w.write_parts(*c)
        w.close()
    assert os.listdir(wd) == []                                                        # the run files are gone
    return open(up, 'rb').read(), open(sp, 'rb').read(), open(sp + '.csi', 'rb').read()


@pytest.fixture(scope='module')
def files(ctx, tmp_path_factory):
    lines = make_lines()
    calls = calls_of(lines)
    assert len(calls) >= 5 and any(len(c[1][0]) + len(c[1][1]) == 2 for c in calls) and any(len(c[1][0]) + len(c[1][1]) == 3 for c in calls)
    return write_both(ctx.lib, str(tmp_path_factory.mktemp('sorted')), calls)


# ---------------------------------------------------------------- 1. order and content

def test_sorted_records_equal_python_sorted(files):
    ubam, sbam, _ = files
    ut, urefs, urecs = B.read_bam(ubam)
    st, srefs, srecs = B.read_bam(sbam)
    assert urefs == srefs == REFS and len(urecs) == len(make_lines())
    assert srecs == sorted(urecs, key=sort_key([r[0] for r in REFS]))                  # content, order and the stable tie-break at once
    assert srecs != urecs
    uh, sh = ut.split('\n'), st.split('\n')
    assert sh[0] == '@HD\tVN:1.6\tSO:coordinate\tGO:none' and uh[0] == HEAD[0] and sh[1:] == uh[1:]
    mem = B.bgzf_members(sbam)
    assert sum(1 for _, pl in mem[:-1] if len(pl) < 65280) >= 5                        # header + at least 4 chunks that end their last member


def test_header_without_hd_line_and_single_chunk(ctx, tmp_path):
    from vacmap_amd.bamout import coordinate_header
    assert coordinate_header(['@SQ\tSN:x\tLN:5']) == ['@HD\tVN:1.6\tSO:coordinate', '@SQ\tSN:x\tLN:5']
    assert coordinate_header(['@HD\tVN:1.0']) == ['@HD\tVN:1.0\tSO:coordinate']
    lines = make_lines(seed=9, n=60)
    ubam, sbam, csi = write_both(ctx.lib, str(tmp_path), calls_of(lines), head=HEAD[1:], chunk=256 << 20)
    st, _, srecs = B.read_bam(sbam)
    assert st.split('\n')[0] == '@HD\tVN:1.6\tSO:coordinate' and st.split('\n')[1:] == B.read_bam(ubam)[0].split('\n')
    assert srecs == sorted(B.read_bam(ubam)[2], key=sort_key([r[0] for r in REFS]))
    check_index_by_use(C.Bam(sbam), C.parse(csi), seed=3, per_ref=40)


def test_no_records_at_all(ctx, tmp_path):
    from vacmap_amd.bamout import SortedBamWriter
    p = str(tmp_path / 'e.sorted.bam')
    w = SortedBamWriter(p, HEAD, lib=ctx.lib)
    w.write(b'')
    w.close()
    assert B.read_bam(open(p, 'rb').read())[2] == []
    idx = C.parse(open(p + '.csi', 'rb').read())
    assert idx['n_no_coor'] == 0 and all(r['bins'] == {} and r['meta'] is None for r in idx['refs']) and len(idx['refs']) == len(REFS)
    assert sorted(os.listdir(tmp_path)) == ['e.sorted.bam', 'e.sorted.bam.csi']


def test_run_files_removed_when_a_write_raises(ctx, tmp_path):
    from vacmap_amd.bamout import SortedBamWriter
    from vacmap_amd.lib import VmxError
    wd = tmp_path / 'wd'; wd.mkdir()
    w = SortedBamWriter(str(tmp_path / 'x.sorted.bam'), HEAD, lib=ctx.lib, workdir=str(wd))
    w.write(('\n'.join(make_lines(n=20)) + '\n').encode())
    assert len(os.listdir(wd)) == 1                                                    # the run directory is there while the writer works
    with pytest.raises(VmxError) as e:
        w.write(b'a\t0\tchrA\t1\t0\t3Q\t*\t0\t0\t*\t*\n')
    assert 'line 1' in str(e.value) and os.listdir(wd) == []
    w.close()                                                                          # (harmless after the error)
    assert os.listdir(wd) == []


# ---------------------------------------------------------------- 2. the index, structurally

def voff_of(bam, u):
    """the virtual offset of decompressed offset u, in the member where the byte at u lies"""
    i = bisect.bisect_right(bam.ustart, u) - 1
    c = [k for k, v in bam.cstart.items() if v == i][0]
    return c << 16 | (u - bam.ustart[i])


def check_index_structure(bam, idx):
    recs = bam.scan()
    starts = set(r[0] for r in recs) | {len(bam.raw)}
    assert idx['min_shift'] == 14 and idx['depth'] == 5 and idx['aux'] == b'' and len(idx['refs']) == len(bam.refs)
    assert idx['n_no_coor'] == sum(1 for r in recs if r[1] < 0)
    nxt = {r[0]: (recs[i + 1][0] if i + 1 < len(recs) else len(bam.raw)) for i, r in enumerate(recs)}
    cof = {v: k for k, v in bam.cstart.items()}
    for rid, ref in enumerate(idx['refs']):
        mine = [r for r in recs if r[1] == rid]
        if not mine:
            assert ref['bins'] == {} and ref['meta'] is None
            continue
        # pseudo-bin: first record's start, last record's end, mapped and unmapped counts
        vb, ve, nm, nu = ref['meta']
        assert bam.u_of(vb) == mine[0][0] and bam.u_of(ve) == nxt[mine[-1][0]]
        assert (nm, nu) == (sum(1 for r in mine if not r[4] & 4), sum(1 for r in mine if r[4] & 4))
        # chunks: record boundaries, ascending and disjoint inside a bin
        spans = {}
        for b, (loff, chunks) in ref['bins'].items():
            us = [(bam.u_of(x), bam.u_of(y)) for x, y in chunks]
            assert all(x in starts and y in starts and x < y for x, y in us), (rid, b)
            assert all(us[i][1] <= us[i + 1][0] for i in range(len(us) - 1)), (rid, b)
            assert all(chunks[i][1] != chunks[i + 1][0] and chunks[i][1] >> 16 != chunks[i + 1][0] >> 16 for i in range(len(chunks) - 1)), 'unmerged chunks'
            spans[b] = us
        # every record: in exactly one chunk of the bin of its interval, which is the bin it stores
        used = set()
        for u, _, pos, end, flag, bn in mine:
            b = C.reg2bin(pos, end)
            assert b == bn and b in spans
            assert sum(1 for x, y in spans[b] if x <= u < y) == 1, (rid, b, u)
            used.add(b)
        assert used == set(spans)
        # loffset by brute force: first record in file order that reaches each 16 kb window
        first = {}
        for u, _, pos, end, flag, bn in mine:
            for wdw in range(pos >> 14, ((end - 1) >> 14) + 1):
                first.setdefault(wdw, u)
        wins = sorted(first)
        for b, (loff, chunks) in ref['bins'].items():
            w0 = C.bin_span(b)[0] >> 14
            k = bisect.bisect_left(wins, w0)
            assert k < len(wins)
            u = first[wins[k]]
            i = bisect.bisect_right(bam.ustart, u) - 1
            assert loff == cof[i] << 16 | (u - bam.ustart[i]), (rid, b)
    return recs


def test_index_structure(files):
    _, sbam, csi = files
    bam = C.Bam(sbam)
    recs = check_index_structure(bam, C.parse(csi))
    assert len(recs) == len(make_lines())
    assert B.bgzf_members(csi)[-1][0] == B.BGZF_EOF


# ---------------------------------------------------------------- 3. the index, by use

def regions_of(length, rng, per_ref):
    out = []
    for i in range(per_ref):
        k = i % 6
        if k == 0:                                                                     # a single base
            b = int(rng.integers(0, length)); out.append((b, b + 1))
        elif k == 1:                                                                   # across a 16 kb border
            c = 16384 * int(rng.integers(1, max(2, length // 16384 + 1))); b = max(0, c - int(rng.integers(1, 3000))); out.append((b, min(length, c + int(rng.integers(1, 3000))) if c < length else length))
        elif k == 2:                                                                   # across a 128 kb border (or the reference's start when it is shorter)
            c = 131072 * int(rng.integers(1, max(2, length // 131072 + 1))) if length > 131072 else 0
            b = max(0, c - int(rng.integers(1, 20000))); out.append((b, min(length, c + int(rng.integers(1, 20000)))))
        elif k == 3:                                                                   # the whole reference
            out.append((0, length))
        elif k == 4:                                                                   # the reference's far end and, on chrA, its empty stretch
            b = int(rng.integers(300000, 359000)) if length >= 400000 else int(rng.integers(length - length // 20, length)); out.append((b, min(length, b + int(rng.integers(1, 1000)))))
        else:                                                                          # anything
            b = int(rng.integers(0, length)); out.append((b, min(length, b + int(rng.integers(1, 60000)))))
    return [(b, e if e > b else b + 1) for b, e in out]


def check_index_by_use(bam, idx, seed, per_ref):
    """every region of every reference, none skipped: the records fetched through the index equal the brute-force overlap list, in file order"""
    rng = np.random.default_rng(seed)
    recs = bam.scan()
    n = full = 0
    for rid, (_, length) in enumerate(bam.refs):
        mine = [r for r in recs if r[1] == rid]
        for beg, end in regions_of(length, rng, per_ref):
            want = [r[0] for r in mine if r[2] < end and r[3] > beg]
            assert C.fetch(bam, idx, rid, beg, end) == want, (rid, beg, end)
            n += 1; full += bool(want)
    return n, full


def test_index_by_use(files):
    _, sbam, csi = files
    bam, idx = C.Bam(sbam), C.parse(csi)
    n, full = check_index_by_use(bam, idx, seed=17, per_ref=204)
    assert n == 204 * len(REFS) and 2 * full >= n, (n, full)


# ---------------------------------------------------------------- 4. the driver end to end

@pytest.mark.parametrize('extra', [['-mode', 'H', '--eqx', '--MD', '--copycomments'], ['-mode', 'H', '--L', '--copycomments'], ['-mode', 'asm', '--copycomments']])
def test_driver_native_sort(ctx, tmp_path, monkeypatch, extra, capsys):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    from test_bam_emu import _inputs
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, fq, bam, asm = _inputs(tmp_path, ctx)
    before = set(os.listdir(tmp_path))
    reads = [str(asm)] if 'asm' in extra else [str(fq), str(bam)]
    common = ['-ref', str(fa), '-read'] + reads + ['-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2',
                                                  '-workdir', str(tmp_path / 'wd')] + extra
    assert driver.main(common + ['-o', str(tmp_path / 'x.bam'), '--bam-writer', 'native']) == 0
    assert driver.main(common + ['-o', str(tmp_path / 'x.sorted.bam'), '--bam-writer', 'native-sort']) == 0
    assert 'x.sorted.bam.csi' in capsys.readouterr().err
    assert driver.main(common + ['-o', str(tmp_path / 'y.bam'), '--bam-writer', 'native-sort']) == 0
    assert os.listdir(tmp_path / 'wd') == []
    assert set(os.listdir(tmp_path)) - before == {'wd', 'x.bam', 'x.sorted.bam', 'x.sorted.bam.csi', 'y.bam'}
    xb, sb, yb = (open(tmp_path / n, 'rb').read() for n in ('x.bam', 'x.sorted.bam', 'y.bam'))
    ut, urefs, urecs = B.read_bam(xb)
    st, srefs, srecs = B.read_bam(sb)
    assert len(urecs) >= 3 and urefs == srefs
    assert srecs == sorted(urecs, key=sort_key([r[0] for r in urefs]))
    assert st.split('\n')[0].split('\t')[0] == '@HD' and 'SO:coordinate' in st.split('\n')[0].split('\t')
    # .bam through native-sort is the unsorted writer: the same bytes, but for the command line that the @PG header line quotes
    yt = B.read_bam(yb)[0]
    assert yt.replace('native-sort', 'native').replace('y.bam', 'x.bam') == ut

    def after_header(data):
        mem = B.bgzf_members(data)
        raw = b''.join(pl for _, pl in mem)
        head = len(raw) - sum(4 + len_ for len_ in _block_sizes(raw))
        k = u = 0
        while u < head:
            u += len(mem[k][1]); k += 1
        assert u == head
        return b''.join(m for m, _ in mem[k:])
    assert after_header(yb) == after_header(xb)
    sbam = C.Bam(sb)
    idx = C.parse(open(tmp_path / 'x.sorted.bam.csi', 'rb').read())
    check_index_structure(sbam, idx)
    check_index_by_use(sbam, idx, seed=23, per_ref=30)


def _block_sizes(raw):
    """block_size of every record of a decompressed BAM"""
    import struct
    lt = struct.unpack_from('<i', raw, 4)[0]
    p = 8 + lt
    nr = struct.unpack_from('<i', raw, p)[0]; p += 4
    for _ in range(nr):
        p += 8 + struct.unpack_from('<i', raw, p)[0]
    out = []
    while p < len(raw):
        bs = struct.unpack_from('<i', raw, p)[0]
        out.append(bs); p += 4 + bs
    return out
