"""Inputs for the PAF emitters (vm_paf_emit, vm_paf_emit_device), shared by the CPU, emulator and GPU tests: every batch of sam_device_cases
(cases() and bulk_cases(), their options passed on unchanged: the ones PAF ignores must change nothing) plus PAF-only batches at the smallest
shapes at which the PAF work can go wrong: clip runs around the 64-byte step of k_paf_lines, every operator's part in alen, signed and 2^40
numbers, names of 0 / 1 / 64 / 65 bytes, keep_unmapped. Expected bytes: paf.paf_lines (python_expected), vm_paf_emit, and on reads whose clips
agree with q_st / q_en the SAM emitter's lines through paf_codec.paf_from_sam_line."""
import numpy as np
import sam_device_cases as SD
import paf_codec as PC

NAMES4 = ['', 'c', 'n' * 64, 'm' * 65]                     # an index of the tests' own: contig names of 0, 1, 64 and 65 bytes
REF4 = [SD.REF[0], SD.REF[1], SD.REF[0], SD.REF[1]]


class Case(SD.Case):
    """a sam_device_cases.Case that may name its own index (names, sequences)"""

    def __init__(self, name, reads, err=None, index=None, **opts):
        SD.Case.__init__(self, name, reads, err=err, **opts)
        self.index = index


def clipped(rng, name, lead, body, trail, strand='+', r_st=300, contig=0):
    """a read with one record lead + body + trail whose q_st / q_en are the S bases of lead / trail (H takes no base), so that the walk with
    and without md agrees with the bases"""
    ops = lead + body + trail
    q, text, r_en = SD.apply_ops(rng, ops, contig, r_st)
    q_st = sum(n for n, op in lead if op == 'S'); q_en = len(q) - sum(n for n, op in trail if op == 'S')
    rec = SD.Rec(contig, strand, 37, q_st, q_en, r_st, r_en, text)
    return SD.Read(name, q if strand == '+' else SD.revcomp(q), [rec], qual=None)


def alternating(nbytes, first='S'):
    """1S1H1S... of nbytes bytes"""
    assert nbytes % 2 == 0
    return [(1, 'SH'[(i + (first == 'H')) % 2]) for i in range(nbytes // 2)]


def clip_reads(rng):
    out = []
    body = [(20, '='), (1, 'X'), (9, '=')]
    # the last leading clip operator on byte 62, 63 and 64 of the merged text (0-based), the body behind it
    for want in (62, 63, 64):
        lead = ([(10, 'S')] if want % 2 == 0 else []) + alternating(want + 1 - (3 if want % 2 == 0 else 0), first='H' if want % 2 == 0 else 'S')
        r = clipped(rng, 'leadclip%d' % want, lead, body, [(2, 'S')], strand='-' if want == 63 else '+')
        t = r.recs[0].cigar
        assert t[want] in 'SH' and t[want + 1:want + 4] == '20=', (want, t)
        out.append(r)
    out.append(clipped(rng, 'runs70', alternating(70), body, alternating(70, first='H')))
    out.append(clipped(rng, 'runs70-', alternating(70), body, alternating(70), strand='-'))
    out.append(clipped(rng, 'onlyclips', [(5, 'S'), (3, 'H')], [], []))
    out.append(clipped(rng, 'onlyclips70', alternating(70), [], []))
    out.append(clipped(rng, 'noclips', [], body, []))
    out.append(clipped(rng, 'interiorS', [(2, 'S')], [(10, '='), (3, 'S'), (10, '=')], [(2, 'S')]))
    out.append(clipped(rng, 'interiorH', [(2, 'H'), (2, 'S')], [(10, '='), (3, 'H'), (10, '=')], [(4, 'H')], strand='-'))
    out.append(clipped(rng, 'trailbody64', [], [(1, '='), (1, 'X')] * 15 + [(100, '=')], [(7, 'S')]))      # the last body operator on byte 63
    return out


def alen_reads(rng):
    out = []
    for op in 'M=XID':
        out.append(SD.one(rng, 'only' + op, [(5, op)], r_st=150, qual=False))
    out.append(SD.one(rng, 'withN', [(5, '='), (7, 'N'), (6, '=')], r_st=150, qual=False))
    out.append(SD.one(rng, 'join', [(10, '=')], r_st=150, cigar='5=5=', qual=False))
    out.append(SD.one(rng, 'joinclip', [(4, 'S'), (10, '='), (3, 'S')], r_st=150, cigar='1S3S5=5=2S1S', qual=False))
    out.append(SD.one(rng, 'M130', [(130, 'M')], r_st=400, m_mismatch=(0, 63, 64, 65, 129), qual=False))
    out.append(SD.one(rng, 'M130-', [(3, 'S'), (130, 'M'), (2, 'S')], r_st=400, m_mismatch=(63, 64), strand='-', qual=False))
    out.append(SD.one(rng, 'big', [(2, 'S'), (1234567, 'D'), (3, '=')], contig=0, r_st=10, cigar='2S1234567D3=', qual=False))      # (D columns are never read without md)
    return out


def number_reads(rng):
    out = []
    r = SD.one(rng, 'neg_qs', [(4, 'S'), (30, '='), (6, 'S')], r_st=200, strand='-', qual=False); r.recs[0].q_en = len(r.seq) + 9; out.append(r)
    r = SD.one(rng, 'neg_qs+', [(30, '=')], r_st=200, qual=False); r.recs[0].q_st = -12; out.append(r)
    r = SD.one(rng, 'r_st_2^40', [(10, 'I')], r_st=100, qual=False); r.recs[0].r_st = 1 << 40; r.recs[0].r_en = (1 << 40) + 10; out.append(r)
    r = SD.one(rng, 'r_neg', [(10, 'I')], r_st=100, qual=False); r.recs[0].r_st = -7; r.recs[0].r_en = -3; out.append(r)
    return out


def name_reads(rng):
    out = []
    for c in range(4):
        r = SD.one(rng, 'on%d' % c if c else '', [(3, 'S'), (25, '='), (1, 'X'), (5, '=')], contig=c % 2, r_st=100 + c, strand='+-'[c % 2], qual=False)
        r.recs[0].contig = c
        out.append(r)
    m = SD.multi(rng, 'q' * 65, 5, contigs=(0, 1))
    for i, rec in enumerate(m.recs):
        rec.contig = (rec.contig + 2 * i) % 4
    out.append(m)
    return out


def cases():
    """the PAF-only batches"""
    rng = np.random.default_rng(4711)
    cl = clip_reads(rng); al = alen_reads(rng); nu = number_reads(rng); na = name_reads(rng)
    good = [SD.one(rng, 'good%d' % i, [(3, 'S'), (30, '='), (1, 'X'), (20, '='), (2, 'D'), (10, '=')], r_st=800 + i, strand='+-'[i % 2]) for i in range(4)]
    out = [Case('clips', cl), Case('clips_md', cl, md=1, shortcs=1), Case('clips_opts', cl, hardclip=1, fakecigar=1, cigar2cg=1, rg='grp')]
    out += [Case('alen', al), Case('alen_md', al[:-1], md=1), Case('alen_asm', al, asm_mode=1), Case('alen_asm_md', al[:-1], asm_mode=1, md=1, shortcs=1)]
    out += [Case('numbers', nu), Case('numbers_keep', nu, keep_unmapped=1)]
    out += [Case('names', na, index=(NAMES4, REF4)), Case('names_md', na, index=(NAMES4, REF4), md=1, shortcs=1)]
    out += [Case('recs70', [SD.multi(rng, 'many', 70, contigs=(0, 1)), good[0]], markunbalancetra=1), Case('recs70_keep', [good[1], SD.multi(rng, 'many', 70)], keep_unmapped=1)]
    # keep_unmapped: nothing but reads without a record; a status, a raising read and an empty read between good ones
    none = [SD.Read('u1', 'ACGT', []), SD.Read('', 'AC', []), SD.Read('u3', '', [])]
    out += [Case('keep_norecs', none, keep_unmapped=1), Case('norecs', none)]
    for k, r in enumerate(SD.raising(rng) + SD.md_raising(rng)[:1]):
        mid = [good[0], SD.Read('failed', good[1].seq, good[1].recs, status=-10), good[2], r, SD.Read('empty', '', []), good[3], SD.Read('failed_norecs', 'ACGTA', [], status=-20)]
        out += [Case('keep_mixed%d' % k, mid, keep_unmapped=1, md=1 if k == 3 else 0, shortcs=1), Case('mixed%d' % k, mid, md=1 if k == 3 else 0)]
    out += [Case('keep_empty', [], keep_unmapped=1)]
    r = SD.one(rng, 'big', [(10, '=')], r_st=10); r.recs[0].cigar = '5=2147483648D5='
    out += [Case('count_2^31', [r], err='ARG')]
    return out


def all_cases():
    """(PAF-only batches, the SAM emitter's batches, its bulk batches)"""
    sam = [Case(c.name, c.reads, err=c.err, **c.opts) for c in SD.cases()]
    bulk = [Case(c.name, c.reads, err=c.err, **c.opts) for c in SD.bulk_cases()]
    bulk.append(Case('bulk_keep_md', bulk[0].reads, md=1, shortcs=1, markunbalancetra=1, keep_unmapped=1))
    return cases(), sam, bulk


# ------------------------------------------------------------------------------------------------ running a case
def opts(VL, o):
    d = dict(md=0, shortcs=0, cigar2cg=0, markunbalancetra=0, hardclip=0, fakecigar=0, rg=None, asm_mode=0, keep_unmapped=0); d.update(o)
    return VL.SamOpts(d['md'], d['shortcs'], d['cigar2cg'], d['markunbalancetra'], d['hardclip'], d['fakecigar'], d['rg'].encode() if d['rg'] else None, d['asm_mode'],
                      d['keep_unmapped'])


class Indexes:
    """the indexes of a context: sam_device_cases' two contigs, and NAMES4"""

    def __init__(self, VL, ctx):
        self.VL, self.ctx, self.made = VL, ctx, {}

    def of(self, case):
        key = 'own' if case.index else 'sd'
        if key not in self.made:
            self.made[key] = self.VL.Index.from_seqs(self.ctx, NAMES4, REF4, k=15, w=10) if case.index else SD.index(self.ctx)
        return self.made[key]


def ref_of(case):
    return (NAMES4, REF4) if case.index else (SD.NAMES, SD.REF)


def run_host(VL, ctx, idx, case, nthreads=2):
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    t, off, nl, ns = VL.paf_emit(ctx.lib, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw, nthreads=nthreads)
    return t.tobytes(), off.tolist(), nl, ns


def run_device(VL, ctx, idx, case):
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    t, off, nl, ns = VL.paf_emit_device(ctx, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw)
    return t.tobytes(), off.tolist(), nl, ns


def run_sam_host(VL, ctx, idx, case):
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, case)
    t, off, nl, ns = VL.sam_emit(ctx.lib, idx, opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, nthreads=2)
    return t.tobytes(), off.tolist(), nl, ns


def python_expected(case):
    """paf.paf_lines read by read, with vm_sam_emit's rule for which reads emit nothing: (text, text_off, n_lines, n_skipped)"""
    from vacmap_amd import paf
    names, ref = ref_of(case)
    o = case.opts

    def refseq(c, a, b):                                   # the host emitter's slice: both ends clamped to the contig, a negative one to 0
        s = ref[names.index(c)]
        a = min(max(a, 0), len(s)); b = min(max(b, 0), len(s))
        return s[a:max(a, b)]
    text, off, nl, ns = [], [0], 0, 0
    for rd in case.reads:
        lines = []
        if rd.status != 0:
            ns += 1
        elif rd.recs:
            recs = [(rd.name, names[r.contig], r.strand, r.q_st, r.q_en, r.r_st, r.r_en, r.mapq, r.cigar) for r in rd.recs]
            try:
                lines = paf.paf_lines(recs, rd.seq, refseq, lambda c: len(ref[names.index(c)]), md=bool(o.get('md')), shortcs=bool(o.get('shortcs')),
                                      markunbalancetra=bool(o.get('markunbalancetra')), asm=bool(o.get('asm_mode')))
            except IndexError:
                ns += 1
        if not lines and o.get('keep_unmapped'):
            lines = [paf.unmapped_line(rd.name, len(rd.seq))]
        nl += len(lines)
        text += [x + '\n' for x in lines]
        off.append(off[-1] + sum(len(x) + 1 for x in lines))
    return ''.join(text).encode(), off, nl, ns


def differ(name, exp, got, who):
    if got == exp:
        return
    el = exp[0].split(b'\n'); gl = got[0].split(b'\n')
    for i in range(max(len(el), len(gl))):
        a = el[i] if i < len(el) else None; b = gl[i] if i < len(gl) else None
        if a != b:
            raise AssertionError('%s: line %d differs (%s)\nexpected: %r\ngot:      %r\n(lines %d / %d, skipped %d / %d)' % (name, i, who, a and a[:600], b and b[:600], exp[2], got[2], exp[3], got[3]))
    raise AssertionError('%s: offsets or counts differ (%s): expected %r got %r' % (name, who, (exp[1][-5:], exp[2], exp[3]), (got[1][-5:], got[2], got[3])))


def check_device(VL, ctx, idx, case):
    """vm_paf_emit_device against vm_paf_emit of the same library; returns the device result (None for an error case)"""
    if case.err:
        try:
            run_device(VL, ctx, idx, case)
        except VL.VmxError as e:
            assert e.code == {'ARG': -1, 'UNSUPPORTED': -7}[case.err], (case.name, e.args)
            return None
        raise AssertionError('%s: expected VM_ERR_%s' % (case.name, case.err))
    got = run_device(VL, ctx, idx, case)
    differ(case.name, run_host(VL, ctx, idx, case), got, 'device against host')
    return got


def check_codec(case, paf, sam):
    """on the reads whose records' clips agree with q_st / q_en: paf_from_sam_line of every SAM line is the PAF line. Returns the lines compared."""
    names, ref = ref_of(case)
    clen = {n: len(s) for n, s in zip(names, ref)}
    assert len(paf[1]) == len(sam[1]) and (paf[2], paf[3]) == (sam[2], sam[3]), case.name
    n = 0
    for i, rd in enumerate(case.reads):
        pl = paf[0][paf[1][i]:paf[1][i + 1]].decode().split('\n')[:-1]
        sl = sam[0][sam[1][i]:sam[1][i + 1]].decode().split('\n')[:-1]
        assert len(pl) == len(sl), (case.name, rd.name)
        for x in pl:
            PC.parse(x)
        if not all(PC.clips_agree(r.cigar, r.q_st, r.q_en, r.r_st, r.r_en, len(rd.seq)) for r in rd.recs):
            continue
        for a, b in zip(pl, sl):                           # (the order inside a read is the SAM emitter's, line by line)
            assert a == PC.paf_from_sam_line(b, len(rd.seq), clen), (case.name, rd.name, a[:300], b[:300])
            n += 1
    return n
