"""Inputs for the depth of coverage (vm_depth_add, vm_depth_add_device, an attached accumulator), shared by the CPU, emulator and GPU tests. Built on
sam_device_cases (contigs of 6000 and 4000 bases): the smallest shapes at which k_depth_add can go wrong. A case is a batch, its options, a window
size and a MAPQ threshold. Expected results, all of which must agree: depth.py (python_expected), vm_depth_add (run_host), vm_depth_add_device
(run_device) and depth_codec applied to vm_sam_emit's lines of the same batch (codec_expected)."""
import numpy as np
import sam_device_cases as SD
import depth_codec as DC

LENS = [len(s) for s in SD.REF]
WINDOWS = (1, 7, 64, 100, 500, 6000, 8192)              # 6000 = 857 * 7 + 1: a last window of one base; 500 and 100: both contigs end on an edge; 8192: larger than either


class Case(SD.Case):
    def __init__(self, name, reads, window=64, min_mapq=0, err=None, **opts):
        SD.Case.__init__(self, name, reads, err=err, **opts)
        self.window, self.min_mapq = window, min_mapq


def run(rng, name, a, b, contig=0, strand='+', op='=', mapq=60):
    """a read whose one record covers [a, b) of the contig with one run"""
    return SD.one(rng, name, [(b - a, op)], contig=contig, r_st=a, strand=strand, mapq=mapq, qual=False)


def edge_reads(rng):
    """run edges against windows of 64 (and, at other window sizes, against whatever edges they meet)"""
    out = [run(rng, 'end_before', 70, 127), run(rng, 'end_on', 70, 128), run(rng, 'end_past', 70, 129, strand='-'), run(rng, 'start_on', 128, 158),
           run(rng, 'inside', 200, 210), run(rng, 'whole1', 64, 128), run(rng, 'interior1', 60, 130), run(rng, 'interior_many', 60, 400, strand='-'),
           run(rng, 'one_base', 255, 256), run(rng, 'long5000M', 3, 5003, op='M'), run(rng, 'interior70', 1000, 1000 + 72 * 64 + 5, contig=0),
           run(rng, 'last_base0', 5900, 6000), run(rng, 'last_base1', 3950, 4000, contig=1, strand='-'), run(rng, 'all_of_1', 0, 4000, contig=1, op='M'),
           run(rng, 'first_of_1', 0, 100, contig=1), run(rng, 'over_end', 3990, 4000, contig=1)]
    out[-1].recs[0].cigar = '30='; out[-1].name = 'past_contig_end'                      # positions at or beyond L_c count nothing
    r = run(rng, 'neg_start', 0, 45); r.recs[0].r_st = -5; r.recs[0].cigar = '5D45='; out.append(r)      # the D columns lie below 0
    return out


def gap_reads(rng):
    """operators that cover nothing: D and N over a boundary and over whole windows, I / S / H between runs, clips, the N stretch of contig 0"""
    one = SD.one
    return [one(rng, 'D_boundary', [(10, '='), (8, 'D'), (10, '=')], r_st=50, qual=False), one(rng, 'D_windows', [(10, '='), (200, 'D'), (10, '=')], r_st=50, qual=False),
            one(rng, 'N_windows', [(10, '='), (200, 'N'), (1, 'X'), (10, '=')], contig=1, r_st=50, strand='-', qual=False),
            one(rng, 'ISH', [(4, 'H'), (3, 'S'), (30, '='), (5, 'I'), (30, '='), (3, 'H'), (30, 'X'), (2, 'P'), (10, '='), (2, 'S'), (5, 'H')], r_st=100, qual=False),
            one(rng, 'clips_only', [(5, 'S'), (3, 'H')], r_st=100, qual=False), one(rng, 'I_only', [(9, 'I')], r_st=64, qual=False),
            one(rng, 'N_stretch', [(100, '='), (40, 'N'), (100, '=')], r_st=2900, qual=False), one(rng, 'M_over_N', [(140, 'M')], r_st=2950, qual=False),
            one(rng, 'D_first', [(70, 'D'), (5, '=')], r_st=60, qual=False), one(rng, 'zero_ops', [(0, '='), (5, '='), (0, 'D'), (3, '=')], r_st=126, cigar='0=5=0D3=', qual=False)]


def step_reads(rng):
    """the 64-byte text step: sam_device_cases' tokeniser set (operators on bytes 63 / 64 / 65, digits across the step, 0 ... 4097 operators, merged runs,
    unmerged pieces) and a record of 2000 alternating 1=1X operators"""
    return SD.tokeniser(rng) + [SD.one(rng, 'alt2000', [(1, '='), (1, 'X')] * 1000, r_st=100, qual=False)]


PIECES = [(700, '='), (1, 'X'), (650, '='), (130, 'D'), (300, '='), (65, 'X'), (70, '=')]


def overlap_reads(rng):
    m = SD.multi(rng, 'two_recs', 2, same_span=True, gaps=[300, 310])
    m2 = SD.multi(rng, 'four_recs', 4, contigs=(0, 1), gaps=[120, 0, 130, 3900])
    return [run(rng, 'ov%d' % i, 290 + i, 390 + 2 * i, strand='+-'[i % 2]) for i in range(3)] + [m, m2, run(rng, 'ov_c1', 0, 70, contig=1), run(rng, 'ov_c1-', 10, 64, contig=1, strand='-')]


def text_reads(rng):
    """means of 0.01 (a tie: count 1 over 200 bases at W = 200), 0.00, >= 10 and >= 100"""
    return [run(rng, 'single', 250, 251)] + [run(rng, 'x12_%d' % i, 1000, 1200) for i in range(12)] + [run(rng, 'x120_%d' % i, 2000, 2200, strand='+-'[i % 2]) for i in range(120)]


def cases():
    rng = np.random.default_rng(20250)
    ed = edge_reads(rng); gp = gap_reads(rng); st = step_reads(rng); ov = overlap_reads(rng); tx = text_reads(rng)
    out = []
    for w in WINDOWS:
        out.append(Case('edges_w%d' % w, ed, window=w)); out.append(Case('gaps_w%d' % w, gp, window=w))
    for w in (1, 7, 64, 500):
        out.append(Case('steps_w%d' % w, st, window=w))
    out += [Case('steps_asm_w64', st, window=64, asm_mode=1, min_mapq=60), Case('steps_md_w7', st, window=7, md=1, shortcs=1)]
    out += [Case('pieces_split', [SD.one(rng, 'p', PIECES, r_st=500, split=10, qual=False)], window=64), Case('pieces_merged', [SD.one(rng, 'p', PIECES, r_st=500, qual=False)], window=64)]
    for w in (1, 64, 100):
        out.append(Case('overlaps_w%d' % w, ov, window=w))
    out += [Case('overlaps_opts', ov, window=64, hardclip=1, fakecigar=1, cigar2cg=1, rg='grp'), Case('edges_md_w64', ed, window=64, md=1, shortcs=1), Case('overlaps_plain', ov, window=64)]
    # MAPQ: exactly Q and Q - 1; reassign_mapq taking records across the threshold; asm_mode's 60 / 1
    mq = [run(rng, 'mq%d' % q, 100 + q, 300 + q, mapq=q) for q in (0, 29, 30, 31, 255)]
    out += [Case('mapq_q30', mq, window=64, min_mapq=30), Case('mapq_q31', mq, window=64, min_mapq=31), Case('mapq_q255', mq, window=64, min_mapq=255), Case('mapq_q0', mq, window=64)]
    rc = SD.record_cases(rng)
    out +=[Case('records_mark_q30', rc, window=100, min_mapq=30, markunbalancetra=1), Case('records_q30', rc, window=100, min_mapq=30), Case('records_mark_q1', rc, window=100, min_mapq=1, markunbalancetra=1)]
    gaps = []
    for strand in '+-':                                     # four records of MAPQ 30 with covered columns; reassign_mapq zeroes those it leaves off the walk
        for gap in (9, 10):
            rd = SD.multi(rng, 'mark%d%s' % (gap, strand), 4, strands=strand, gaps=[1000, 1200 + gap, 2000, 1100])
            for x in rd.recs:
                x.mapq = 30
            gaps.append(rd)
    out += [Case('mark_on_q30', gaps, window=64, min_mapq=30, markunbalancetra=1), Case('mark_off_q30', gaps, window=64, min_mapq=30), Case('mark_on_q0', gaps, window=64, markunbalancetra=1)]
    am = SD.asm_cases(rng)
    out += [Case('asm_q60', am, window=64, min_mapq=60, asm_mode=1), Case('asm_q2', am, window=64, min_mapq=2, asm_mode=1), Case('asm_q1', am, window=64, min_mapq=1, asm_mode=1),
            Case('asm_q61', am, window=64, min_mapq=61, asm_mode=1), Case('asm_off_q60', am, window=64, min_mapq=60)]
    # reads that contribute nothing, between reads that count
    good = [run(rng, 'good%d' % i, 780 + 9 * i, 900 + 9 * i, strand='+-'[i % 2]) for i in range(4)]
    for k, r in enumerate(SD.raising(rng) + SD.md_raising(rng)):
        md = 1 if k >= 3 else 0
        mid = [good[0], SD.Read('failed', good[1].seq, good[1].recs, status=-10), good[2], r, SD.Read('empty', '', []), good[3], SD.Read('failed_norecs', 'ACGTA', [], status=-20)]
        out += [Case('nothing%d' % k, mid, window=64, md=md), Case('nothing%d_keep' % k, mid, window=64, md=md, keep_unmapped=1)]
    out += [Case('no_reads', [], window=64), Case('norecs_keep_w500', [SD.Read('u', 'ACGT', [])], window=500, keep_unmapped=1)]
    out += [Case('text_w200', tx, window=200), Case('text_w64', tx, window=64), Case('text_w6000', tx, window=6000)]
    r = SD.one(rng, 'big', [(10, '=')], r_st=10); r.recs[0].cigar = '5=2147483648D5='
    out.append(Case('count_2^31', [good[0], r], window=64, err='ARG'))
    return out


def sam_cases():
    """every batch of sam_device_cases at one window size: its options must change nothing that they should not"""
    return [Case(c.name, c.reads, window=100, err=c.err, **c.opts) for c in SD.cases()]


def bulk_cases():
    """300 reads in one call: more waves than a workgroup holds"""
    b = SD.bulk_cases()
    out = [Case(c.name + '_w100', c.reads, window=100, **c.opts) for c in b]
    out += [Case('bulk_w1_q30', b[0].reads, window=1, min_mapq=30, markunbalancetra=1), Case('bulk_w7_keep', b[0].reads, window=7, keep_unmapped=1, md=1, shortcs=1),
            Case('bulk_w8192', b[0].reads, window=8192)]
    return out


# ------------------------------------------------------------------------------------------------ running a case
def opts(VL, o):
    d = dict(md=0, shortcs=0, cigar2cg=0, markunbalancetra=0, hardclip=0, fakecigar=0, rg=None, asm_mode=0, keep_unmapped=0); d.update(o)
    return VL.SamOpts(d['md'], d['shortcs'], d['cigar2cg'], d['markunbalancetra'], d['hardclip'], d['fakecigar'], d['rg'].encode() if d['rg'] else None, d['asm_mode'],
                      d['keep_unmapped'])


def result(d, nl, ns):
    """what every implementation is compared by: (counts, win_off, regions bytes, summary bytes, n_lines, n_skipped)"""
    counts, off = d.counts()
    return counts.tolist(), off.tolist(), d.regions(), d.summary(), nl, ns


def run_host(VL, ctx, idx, case, nthreads=2):
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, case.window, case.min_mapq, lib=ctx.lib)
    try:
        nl, ns = d.add(idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw, nthreads=nthreads)
        return result(d, nl, ns)
    finally:
        d.close()


def run_device(VL, ctx, idx, case):
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, case.window, case.min_mapq, ctx=ctx)
    try:
        nl, ns = d.add_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw)
        return result(d, nl, ns)
    finally:
        d.close()


def run_attached(VL, ctx, idx, case, paf=False):
    """the case through an emit call on a context with an accumulator attached: (result, the emit call's return as bytes / lists)"""
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, case.window, case.min_mapq, ctx=ctx)
    try:
        ctx.attach_depth(d)
        if paf:
            t, off, nl, ns = VL.paf_emit_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw)
        else:
            t, off, nl, ns = VL.sam_emit_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
        return result(d, nl, ns), (t.tobytes(), off.tolist(), nl, ns)
    finally:
        ctx.attach_depth(None)
        d.close()


def run_emit(VL, ctx, idx, case, paf=False):
    """the emit call of run_attached with nothing attached"""
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, case)
    if paf:
        t, off, nl, ns = VL.paf_emit_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw)
    else:
        t, off, nl, ns = VL.sam_emit_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
    return t.tobytes(), off.tolist(), nl, ns


def sam_text(VL, ctx, idx, case):
    """vm_sam_emit's text of the case (without cigar2cg, whose CIGAR column is a placeholder and which changes no count), n_lines, n_skipped"""
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, case)
    o = dict(case.opts); o['cigar2cg'] = 0
    t, off, nl, ns = VL.sam_emit(ctx.lib, idx, opts(VL, o), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, nthreads=2)
    return t.tobytes().decode(), nl, ns


def codec_expected(VL, ctx, idx, case):
    text, nl, ns = sam_text(VL, ctx, idx, case)
    counts, off, reg, summ, seen = DC.expected(text, SD.NAMES, LENS, case.window, case.min_mapq)
    assert seen + (sum(1 for x in text.split('\n') if x and int(x.split('\t')[1]) & 4)) == nl
    return counts, off, reg, summ, nl, ns


def python_expected(case):
    """depth.py read by read, with vm_sam_emit's rule for which reads emit nothing"""
    from vacmap_amd import depth
    names, ref = SD.NAMES, SD.REF
    o = case.opts

    def refseq(c, a, b):
        s = ref[names.index(c)]
        a = min(max(a, 0), len(s)); b = min(max(b, 0), len(s))
        return s[a:max(a, b)]
    per_read, nl, ns = [], 0, 0
    for rd in case.reads:
        n = 0
        if rd.status != 0:
            ns += 1
        elif rd.recs:
            recs = [(rd.name, names[r.contig], r.strand, r.q_st, r.q_en, r.r_st, r.r_en, r.mapq, r.cigar) for r in rd.recs]
            try:
                per_read.append(depth.counts(recs, rd.seq, refseq, lambda c: len(ref[names.index(c)]), case.window, case.min_mapq, md=bool(o.get('md')),
                                             shortcs=bool(o.get('shortcs')), markunbalancetra=bool(o.get('markunbalancetra')), asm=bool(o.get('asm_mode'))))
                n = len(recs)
            except IndexError:
                ns += 1
        nl += n if n else (1 if o.get('keep_unmapped') else 0)
    table = depth.flat(names, LENS, case.window, per_read)
    return (table, depth.window_offsets(LENS, case.window), depth.regions_text(names, LENS, case.window, table).encode(),
            depth.summary_text(names, LENS, case.window, table).encode(), nl, ns)


def differ(name, exp, got, who):
    if got == exp:
        return
    assert got[1] == exp[1], '%s: win_off differs (%s): %r / %r' % (name, who, exp[1][-3:], got[1][-3:])
    bad = [(i, a, b) for i, (a, b) in enumerate(zip(exp[0], got[0])) if a != b]
    assert not bad, '%s: %d windows differ (%s), the first ones (window, expected, got): %r' % (name, len(bad), who, bad[:8])
    for k, what in ((2, 'regions'), (3, 'summary')):
        if exp[k] != got[k]:
            e, g = exp[k].split(b'\n'), got[k].split(b'\n')
            i = next((i for i in range(min(len(e), len(g))) if e[i] != g[i]), min(len(e), len(g)))
            raise AssertionError('%s: %s line %d differs (%s): %r / %r' % (name, what, i, who, e[i:i + 1], g[i:i + 1]))
    raise AssertionError('%s: n_lines / n_skipped differ (%s): %r / %r' % (name, who, exp[4:], got[4:]))


def check_device(VL, ctx, idx, case):
    """vm_depth_add_device against vm_depth_add of the same library; returns the device result (None for an error case)"""
    if case.err:
        d = VL.Depth.create(idx, case.window, case.min_mapq, ctx=ctx)
        try:
            names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
            try:
                d.add_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw)
            except VL.VmxError as e:
                assert e.code == {'ARG': -1, 'UNSUPPORTED': -7}[case.err], (case.name, e.args)
                assert not d.counts()[0].any(), case.name      # a call that returns an error adds nothing
                return None
            raise AssertionError('%s: expected VM_ERR_%s' % (case.name, case.err))
        finally:
            d.close()
    got = run_device(VL, ctx, idx, case)
    differ(case.name, run_host(VL, ctx, idx, case), got, 'device against host')
    return got
