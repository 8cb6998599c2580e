"""One round through every handle of the library that owns device or page-locked memory, at the smallest inputs the other case modules build: a fresh
Context, an Index over golden case D, one read through align_batch, the stage entries, ResidentReads, the device SAM emitter, BamCodec, BamSorter (two runs),
BamReader (without and with tags) and the free BGZF functions; everything is closed again, the context last. test_emu_ownership.py runs it on the emulator
build and counts the allocations left; test_gpu_ownership.py runs it on the device and compares two rounds."""
import os

import numpy as np

import bam_input_cases as K

CASE = 'D'
TAGGED = [('t1', 'ACGTACGT', 'IIIIIIII', 0), ('t2', 'GATTACA', None, 16), ('t3', 'AC', '!#', 4)]
FIVE = [('r1', 'ACGTNACGTA', 'IIIIIHHHHH', 0), ('r2', 'AACCGGTTA', 'ABCDEFGHI', 16), ('r3', 'GATTACA', None, 4), ('r4', '', None, 4), ('r5', 'ACGRYK', '!!!!!!', 0)]


def case_inputs(golden):
    """contig names, contigs and the shortest read of the case that the reference aligned"""
    meta, arrays = golden
    c = meta[CASE]
    contigs = [arrays['%s_contig%d' % (CASE, i)].tobytes().decode() for i in range(len(c['names']))]
    ok = [i for i, r in enumerate(c['reads']) if r['v6_status'] == 0 and r['v6_records']]
    ri = min(ok, key=lambda i: len(arrays['%s_r%d_seq' % (CASE, i)]))
    return c, contigs, arrays['%s_r%d_seq' % (CASE, ri)].tobytes().decode()


def blob(items):
    bs = [x.encode() for x in items]
    off = np.zeros(len(bs) + 1, np.int64)
    off[1:] = np.cumsum([len(b) for b in bs])
    return np.frombuffer(b''.join(bs) + b'\0', np.uint8)[:-1].copy(), off


def bam_files(tmp):
    """the five records of the reader's smallest test in members of 50 bytes, and three records that carry auxiliary fields"""
    plain, tagged = os.path.join(tmp, 'five.bam'), os.path.join(tmp, 'tagged.bam')
    if not os.path.exists(plain):
        open(plain, 'wb').write(K.bgzf(K.bam_header() + b''.join(K.bam_record(*r) for r in FIVE), 6, block=50))
        open(tagged, 'wb').write(K.bgzf(K.bam_header() + b''.join(K.bam_record(*r, tags=b'XAZab\0XBCz') for r in TAGGED), 6))
    return plain, tagged


def one_round(VL, lib, golden, tmp, tag, probe=lambda: None):
    """returns what the round computed (records, texts, BAM bytes); probe() is called once while every handle is open"""
    c, contigs, read = case_inputs(golden)
    out = {}
    ctx = VL.Context(0, lib=lib)
    idx = VL.Index.from_seqs(ctx, c['names'], contigs, k=c['k'], w=c['w'])
    prm = lib.params(c['mode'])
    status, recs, _ = VL.align_batch(ctx, idx, prm, [read])
    out['align'] = (status.tolist(), recs)
    out['map'] = [a.tolist() for a in ctx.map_batch(idx, [read[:400]])]
    out['ed'] = np.asarray(ctx.edit_distance_batch([read[:90], 'ACGT'], [read[3:100], 'AGT'])).tolist()
    cigars, scores = ctx.k_cigar_batch([read[:60], 'ACGTACGT'], [read[:20] + read[24:60], 'ACGACGT'])
    out['cigar'] = (cigars, scores.tolist())
    rr = VL.ResidentReads(ctx, seqs=[read])
    raw = rr.align_raw(idx, prm)
    assert raw.status.tolist() == out['align'][0] and raw.nrec == len(recs)
    names, name_off = blob(['read0']); seqs, seq_off = blob([read]); quals, qual_off = blob(['I' * len(read)])
    opts = VL.SamOpts(0, 0, 0, 0, 0, 0, None, 0)
    text, toff, nl, ns = VL.sam_emit_device(ctx, idx, opts, names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
    out['sam'] = (text.tobytes(), toff.tolist(), nl, ns)
    assert nl >= 1 and len(recs) >= 1, (nl, ns, len(recs))
    head = '@HD\tVN:1.6\n' + ''.join('@SQ\tSN:%s\tLN:%d\n' % (n, len(s)) for n, s in zip(c['names'], contigs))
    codec = VL.BamCodec(ctx, head)
    keys = [np.arange(len(toff) - 1, dtype=np.int64)]
    out['bam'] = codec.header() + codec.compress_parts([text], [toff], keys)
    sorter = VL.BamSorter(codec, 1 << 16)
    runs = []
    for k in range(2):
        run = sorter.add_parts([text], [toff], keys)
        assert run
        runs.append(os.path.join(tmp, 'run_%s_%d' % (tag, k)))
        open(runs[-1], 'wb').write(run)
    n_chunks = sorter.plan(runs, len(codec.header()))
    out['sorted'] = b''.join(sorter.chunk(k) for k in range(n_chunks))
    out['csi'] = sorter.index()
    plain, tagged = bam_files(tmp)
    rd, rt = VL.BamReader(ctx, plain), VL.BamReader(ctx, tagged, tags='*')
    out['reads'] = [(ch['names'].tobytes(), ch['seqs'].tobytes(), ch['quals'].tobytes()) for ch in K.read_all(rd, 3)]
    out['tagged'] = [(ch['names'].tobytes(), ch['comments'].tobytes(), ch['comments_off'].tolist()) for ch in K.read_all(rt, 4096)]
    assert b'XA:Z:ab' in out['tagged'][0][1] and len(out['reads']) == 2
    z = VL.bgzf_compress(ctx, out['sam'][0])
    assert VL.bgzf_decompress(ctx, z) == out['sam'][0]
    out['bgzf'] = z
    probe()
    for h in (rt, rd, sorter, codec, raw, rr, idx, ctx):
        h.close()
    return out


def error_round(VL, lib, tmp):
    """the two error paths other tests provoke: a reader opened on a file that is not BGZF, and a malformed SAM line in the encoder. Returns the error codes"""
    from test_host_logic import _write_bam
    ctx = VL.Context(0, lib=lib)
    p = os.path.join(tmp, 'plain_gzip.bam')
    _write_bam(p, [('r1', 'ACGT', 'IIII', 0)])
    codes = []
    try:
        VL.BamReader(ctx, p)
    except VL.VmxError as e:
        codes.append(e.code)
    codec = VL.BamCodec(ctx, '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n')
    try:
        codec.encode('a\t0\tchr1\t1\t0\t4M\t*\t0\t0\tACGT\tIIII\nb\t0\tchr1\t1\t0\t3Q\t*\t0\t0\t*\t*\n')
    except VL.VmxError as e:
        codes.append(e.code)
    codec.close()
    ctx.close()
    return codes
