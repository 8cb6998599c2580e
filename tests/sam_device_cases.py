"""Seeded inputs for the device SAM emitter (vm_sam_emit_device), shared by the emulator and the GPU tests. Every case is a batch (reads, their
records, options); the expected bytes are always vm_sam_emit's on the same batch and the same library. A builder applies an operator list to a
small reference (two contigs, ACGT with a stretch of N), so sequences and CIGARs agree and mismatches sit exactly where the case puts them.
The shapes are the smallest at which a kernel of k_sam.hip can go wrong: operators on bytes 63 / 64 / 65 of the text, numbers across the 64-byte
step, runs that merge across the 64-byte and the 64-operator steps, columns in the first and last place of 1 / 63 / 64 / 65 / 200-column runs, ..."""
import ctypes as C
import numpy as np

_COMP = bytes.maketrans(b'ACGTacgt', b'TGCAtgca')
NAMES = ['ctgA', 'chrB_long_name']
OPTSETS = {                                      # the option sets of tests/golden/sam.json that carry no comments (+ asm)
    'default': dict(),
    'hard_fake_rg': dict(hardclip=1, fakecigar=1, rg='grp1'),
    'md_short': dict(md=1, shortcs=1),
    'md_long': dict(md=1, shortcs=0),
    'cg': dict(cigar2cg=1, markunbalancetra=0),
    'asm': dict(asm_mode=1),
}


def reference():
    rng = np.random.default_rng(20240611)
    a = rng.choice(list(b'ACGT'), 6000).astype(np.uint8); b = rng.choice(list(b'ACGT'), 4000).astype(np.uint8)
    a[3000:3040] = ord('N')
    return [a.tobytes().decode(), b.tobytes().decode()]


REF = reference()


def revcomp(s):
    return s.encode().translate(_COMP)[::-1].decode()


def _other(rng, c):
    return 'ACGT'[('ACGT'.index(c) + int(rng.integers(1, 4))) % 4] if c in 'ACGT' else 'A'


def _rand(rng, n):
    return ''.join('ACGT'[i] for i in rng.integers(0, 4, n))


class Rec:
    def __init__(self, contig, strand, mapq, q_st, q_en, r_st, r_en, cigar):
        self.contig, self.strand, self.mapq, self.q_st, self.q_en, self.r_st, self.r_en, self.cigar = contig, strand, mapq, q_st, q_en, r_st, r_en, cigar


class Read:
    def __init__(self, name, seq, recs, qual=None, status=0):
        self.name, self.seq, self.recs, self.qual, self.status = name, seq, recs, qual, status


class Case:
    def __init__(self, name, reads, err=None, **opts):
        self.name, self.reads, self.opts, self.err = name, reads, opts, err

    def __repr__(self):
        return self.name


def apply_ops(rng, ops, contig, r_st, m_mismatch=()):
    """aligned-strand query and the text of an operator list [(n, op)] walked along REF[contig] from r_st. X columns differ from the reference, M
    columns equal it except at the column numbers (over all M columns) in m_mismatch; I / S bases are random; H takes nothing."""
    ref = REF[contig]; q = []; r = r_st; mcol = 0
    for n, op in ops:
        if op in '=M':
            for _ in range(n):
                c = ref[r] if r < len(ref) else 'A'
                q.append(_other(rng, c) if (op == 'M' and mcol in m_mismatch) else c)
                mcol += op == 'M'; r += 1
        elif op == 'X':
            for _ in range(n):
                q.append(_other(rng, ref[r] if r < len(ref) else 'A')); r += 1
        elif op in 'IS':
            q.append(_rand(rng, n))
        elif op in 'DN':
            r += n
    return ''.join(q), ''.join('%d%s' % (n, op) for n, op in ops), r


def one(rng, name, ops, contig=0, r_st=100, strand='+', mapq=60, m_mismatch=(), cigar=None, qual=True, lower=False, split=None):
    """a read with one record made from ops. cigar: the record's text when it is not the plain join (unmerged pieces); split: write every run of n
    as pieces of at most `split` columns (what the gap-fill joins look like)."""
    q, text, r_en = apply_ops(rng, ops, contig, r_st, m_mismatch)
    if split:
        text = ''.join(''.join('%d%s' % (min(split, n - i), op) for i in range(0, n, split)) if n else '0%s' % op for n, op in ops)
    if cigar is not None:
        text = cigar
    if lower:
        q = q.lower()
    soft = [n for n, op in ops if op == 'S'] + [0]                     # q_st / q_en: the query without its soft clips (H bases are not in the read)
    lead = soft[0] if [op for n, op in ops if op != 'H'][:1] == ['S'] else 0
    trail = soft[-2] if len(ops) > 1 and [op for n, op in ops if op != 'H'][-1:] == ['S'] else 0
    qlen = len(q)
    rec = Rec(contig, strand, mapq, lead, qlen - trail, r_st, r_en, text)
    seq = q if strand == '+' else revcomp(q)
    return Read(name, seq, [rec], qual=''.join(chr(33 + (5 * i) % 60) for i in range(qlen)) if qual else None)


def tokeniser(rng):
    out = []
    # an operator byte on byte 63, 64 and 65 of the text (0-based 62 / 63 / 64 and one beyond): '1=' pairs, then a number wide enough to land there
    for want in (62, 63, 64, 65):
        k = (want - 3) // 2                                             # k two-byte pieces, then a three-digit number ends on byte `want`
        pad = want - 3 - 2 * k
        ops = [(1, '='), (1, 'X')] * (k // 2) + ([(1, '=')] if k % 2 else [])
        ops += [(10 ** (2 + pad) + 7, 'D'), (3, '='), (2, 'I'), (4, '=')]
        r = one(rng, 'opbyte%d' % want, ops, contig=0, r_st=10)
        assert r.recs[0].cigar.index('D') == want, (want, r.recs[0].cigar)
        out.append(r)
    # a number whose digits straddle the 64-byte step: '1=1X' * 15 is 60 bytes, then 123456 begins on byte 60
    ops = [(1, '='), (1, 'X')] * 15 + [(1234, 'D'), (250, '='), (1, 'X')]
    r = one(rng, 'straddle', ops, r_st=20); assert r.recs[0].cigar[60:64] == '1234'; out.append(r)
    r = one(rng, 'straddle2', [(1, '='), (1, 'X')] * 15 + [(7, '='), (1500, 'D'), (30, '=')], r_st=25); assert r.recs[0].cigar[62:66] == '1500'; out.append(r)
    # 0, 1, 63, 64, 65 and 4097 operators
    for k in (0, 1, 63, 64, 65, 4097):
        ops = [((1, '='), (1, 'X'), (2, '='), (1, 'I'), (1, '='), (1, 'D'))[i % 6] for i in range(k)]
        if k == 0:
            out.append(Read('ops0', _rand(rng, 30), [Rec(0, '+', 60, 0, 30, 50, 50, '')], qual='I' * 30))
        else:
            out.append(one(rng, 'ops%d' % k, ops, contig=k % 2, r_st=40))
    # the same operator 2, 3, 64, 65 and 130 times in a row (one merged run), before and behind other operators
    for k in (2, 3, 64, 65, 130):
        for op in '=XDI':
            ops = [(5, 'S'), (3, '=' if op != '=' else 'X')] + [(k + 1, op)] + [(4, 'X' if op != 'X' else '='), (2, '=') if op != '=' else (2, 'X')]
            text = '5S3%s' % ops[1][1] + ('1%s' % op) * (k - 1) + '2%s' % op + '4%s2%s' % (ops[3][1], ops[4][1])
            out.append(one(rng, 'rep%d%s' % (k, op), ops, r_st=300, cigar=text, strand='-' if k % 2 else '+'))
    # long repeats written as two-digit pieces: merges that cross both the 64-byte and the 64-operator step
    out.append(one(rng, 'pieces', [(700, '='), (1, 'X'), (650, '='), (130, 'D'), (300, '=')], r_st=500, split=10))
    out.append(one(rng, 'nodigit', [(0, '='), (5, '=')], r_st=10, cigar='=5='))
    return out


def count_overflow(rng):
    r = one(rng, 'big', [(10, '=')], r_st=10)
    r.recs[0].cigar = '5=2147483648D5='
    return [Case('count_2^31', [r], err='ARG'), Case('count_2^31_md', [r], err='ARG', md=1)]


def nm_cases(rng):
    out = []
    for n in (1, 63, 64, 65, 200):
        for where in ('first', 'last', 'both', 'none'):
            mm = {'first': (0,), 'last': (n - 1,), 'both': (0, n - 1), 'none': ()}[where]
            out.append(one(rng, 'M%d%s' % (n, where), [(3, 'S'), (n, 'M'), (2, 'I'), (n, 'M'), (2, 'S')], r_st=200 + n, m_mismatch=mm, strand='-' if n & 1 else '+'))
            out.append(one(rng, 'M%d%slower' % (n, where), [(n, 'M')], r_st=900, m_mismatch=mm, lower=True))
            ops = [(n, '=')] if where == 'none' else ([(1, 'X'), (n - 1, '=')] if where == 'first' and n > 1 else [(n - 1, '='), (1, 'X')] if where == 'last' and n > 1 else [(1, 'X')] + ([(n - 2, '='), (1, 'X')] if n > 2 else []))
            out.append(one(rng, 'EX%d%s' % (n, where), [o for o in ops if o[0] > 0], r_st=1200))
    # N against N (equal) and N against a base
    r = one(rng, 'NvsN', [(70, 'M')], r_st=2990); r.seq = r.seq[:10] + 'N' * 40 + r.seq[50:]; out.append(r)
    r = one(rng, 'NvsBase', [(70, 'M')], r_st=2990); r.seq = r.seq[:10] + 'ACGTNRYK' * 5 + r.seq[50:]; out.append(r)
    # r_st / r_en outside the contig (clamped): the slice is shorter than the record says
    r = one(rng, 'neg_r_st', [(50, '=')], r_st=0); r.recs[0].r_st = -5; r.recs[0].cigar = '45='; out.append(r)
    r = one(rng, 'r_en_beyond', [(50, '=')], contig=1, r_st=3950); r.recs[0].r_en = 4100; out.append(r)
    r = one(rng, 'r_en_before_r_st', [(5, 'I')], r_st=100); r.recs[0].r_en = 50; out.append(r)
    return out


def raising(rng):
    """(name, the read that raises) — each is placed between two good neighbours"""
    out = []
    r = one(rng, 'M_past_read', [(40, 'M')], r_st=100); r.recs[0].cigar = '41M'; r.recs[0].r_en += 1; out.append(r)
    r = one(rng, 'M_past_slice', [(40, 'M')], r_st=100); r.recs[0].r_en -= 1; out.append(r)
    r = one(rng, 'M_past_contig', [(40, 'M'), (5, 'I')], contig=1, r_st=3961); r.recs[0].cigar = '40M5I'; r.recs[0].r_st = 3961; out.append(r)
    return out


def md_cases(rng):
    out = []
    L = [('EX', [(10, '='), (1, 'X'), (10, '=')]), ('Xfirst', [(1, 'X'), (10, '=')]), ('DX', [(5, '='), (3, 'D'), (1, 'X'), (5, '=')]), ('XD', [(5, '='), (1, 'X'), (3, 'D'), (5, '=')]),
         ('EIE', [(7, '='), (3, 'I'), (8, '=')]), ('EDE', [(7, '='), (3, 'D'), (8, '=')]), ('trailE', [(1, 'X'), (12, '=')]), ('SH', [(4, 'H'), (3, 'S'), (9, '='), (1, 'X'), (2, 'S'), (5, 'H')]),
         ('XIX', [(2, 'X'), (1, 'I'), (1, 'X'), (3, '=')]), ('DID', [(4, '='), (2, 'D'), (2, 'I'), (2, 'D'), (4, '=')]), ('IX', [(3, 'I'), (1, 'X'), (1, 'D'), (1, 'I'), (4, '=')]),
         ('opM', [(5, '='), (4, 'M'), (1, 'X'), (3, '=')]), ('opN', [(5, '='), (1, 'X'), (30, 'N'), (5, '=')]), ('zeroX', [(5, '='), (0, 'X'), (5, '=')]), ('zeroD', [(5, '='), (0, 'D'), (1, 'X'), (5, '=')])]
    for k in (1, 2, 64, 65):
        L.append(('X%d' % k, [(6, '='), (k, 'X'), (6, '=')]))
    for k in (1, 64, 65, 1000):
        L.append(('D%d' % k, [(6, '='), (k, 'D'), (6, '=')])); L.append(('I%d' % k, [(6, '='), (k, 'I'), (6, '=')]))
        L.append(('E%d' % k, [(1, 'X'), (k, '='), (1, 'X')]))
    for nm, ops in L:
        for strand in '+-':
            out.append(one(rng, 'md_%s%s' % (nm, strand), ops, contig=0, r_st=2950 if nm.startswith('D1000') else 700, strand=strand))
    # D and I past the end are clamped, an X run past the slice raises (kept apart: raising())
    r = one(rng, 'md_D_past', [(10, '='), (30, 'D')], contig=1, r_st=3970); r.recs[0].cigar = '10=45D'; out.append(r)
    r = one(rng, 'md_I_past', [(10, '='), (5, 'I')], r_st=100); r.recs[0].cigar = '10=9I'; out.append(r)
    r = one(rng, 'md_E_past', [(10, '=')], contig=1, r_st=3990); r.recs[0].cigar = '30='; out.append(r)
    r = one(rng, 'md_qslice', [(5, 'S'), (20, '='), (1, 'X'), (4, 'S')], r_st=100); r.recs[0].q_st = -3; r.recs[0].q_en = 500; out.append(r)
    return out


def md_raising(rng):
    out = []
    r = one(rng, 'X_past_slice', [(10, '='), (3, 'X')], contig=1, r_st=3987); r.recs[0].cigar = '10=4X'; out.append(r)
    r = one(rng, 'X_past_read', [(10, '='), (3, 'X')], r_st=100); r.recs[0].cigar = '10=3X1X'; r.recs[0].r_en += 1; out.append(r)
    r = one(rng, 'X65_past', [(10, '='), (64, 'X')], contig=1, r_st=3926); r.recs[0].cigar = '10=65X'; out.append(r)
    r = one(rng, 'X_after_abort', [(10, '='), (2, 'M'), (3, 'X')], contig=1, r_st=3985); r.recs[0].cigar = '10=2M9X'; out.append(r)      # (MD stops at M: no raise from X; NM has no M past the end)
    return out


def multi(rng, name, n, qlen=400, same_span=False, contigs=(0,), strands='+-', gaps=None):
    """a read with n records over pieces of one query"""
    q = _rand(rng, qlen); recs = []
    for i in range(n):
        span = 40 if same_span else int(rng.integers(20, 120))
        q_st = int(rng.integers(0, qlen - span)); contig = contigs[i % len(contigs)]; strand = strands[i % len(strands)]
        r_st = int(rng.integers(0, len(REF[contig]) - 200)) if gaps is None else gaps[i]
        ops = [(span // 2, '='), (1, 'X'), (span - span // 2 - 1, '=')]
        piece, text, r_en = apply_ops(rng, ops, contig, r_st)
        aligned = q if strand == '+' else revcomp(q)
        aligned = aligned[:q_st] + piece + aligned[q_st + span:]
        q = aligned if strand == '+' else revcomp(aligned)
        lead = '%dS' % q_st if q_st else ''; trail = '%dS' % (qlen - q_st - span) if qlen - q_st - span else ''
        recs.append(Rec(contig, strand, int(rng.integers(0, 61)), q_st, q_st + span, r_st, r_en, lead + text + trail))
    # the pieces overwrote one another: make every record's columns agree with the final query again by turning them into M
    for r in recs:
        r.cigar = r.cigar.replace('=', 'M').replace('X', 'M')
    return Read(name, q, recs, qual=''.join(chr(40 + i % 50) for i in range(qlen)))


def line_cases(rng):
    out = []
    for n in (1, 63, 64, 65, 129):
        for strand in '+-':
            r = one(rng, 'len%d%s' % (n, strand), [(n, 'M')], r_st=1500, strand=strand)
            s = list(r.seq); s[0] = 'N'; s[-1] = 'R' if n > 1 else s[-1]
            if n > 2:
                s[n // 2] = s[n // 2].lower()
            r.seq = ''.join(s); out.append(r)
    r = one(rng, 'noqual', [(50, 'M')], r_st=10, qual=False); out.append(r)
    r = one(rng, 'shortqual', [(50, 'M')], r_st=10); r.qual = r.qual[:-1]; out.append(r)
    r = one(rng, 'longqual', [(50, 'M')], r_st=10, strand='-'); r.qual = r.qual + 'I'; out.append(r)
    return out


def clip_cases(rng):
    out = []
    for k, (a, b) in enumerate(((0, None), (0, 0), (-4, 1000), (30, 10), (7, 33))):
        for strand in '+-':
            r = one(rng, 'clip%d%s' % (k, strand), [(5, 'S'), (40, '='), (5, 'S')], r_st=400, strand=strand)
            r.recs[0].q_st = a; r.recs[0].q_en = len(r.seq) if b is None else b
            out.append(r)
    return out


def record_cases(rng):
    out = [multi(rng, 'recs%d' % n, n, contigs=(0, 1)) for n in (1, 2, 3, 9, 70)]
    out.append(multi(rng, 'ties', 6, same_span=True))
    # reassign_mapq: reference gaps 9 / 10 and 100000 / 100001 against the record before, on both strands and across contigs (contig B is too
    # short for the long gaps: the coordinates only have to be numbers here, the CIGARs never touch the bases)
    for strand in '+-':
        for gap in (9, 10, 100000, 100001, -100000, -100001):
            rd = multi(rng, 'gap%d%s' % (gap, strand), 4, strands=strand, gaps=[1000, 1000, 1000, 1000])
            for r in rd.recs:
                r.cigar = '%dS%dI%dS' % (r.q_st, r.q_en - r.q_st, len(rd.seq) - r.q_en) if r.q_st and len(rd.seq) - r.q_en else '%dI' % len(rd.seq)
                r.mapq = 30
            base = rd.recs[0]
            x = rd.recs[1]
            if strand == '+':
                x.r_st = base.r_en + gap; x.r_en = x.r_st + 50
            else:
                x.r_en = base.r_st - gap; x.r_st = x.r_en - 50
            if x.r_st < 0:
                continue
            rd.recs[2].contig = 1; rd.recs[2].r_st = 10; rd.recs[2].r_en = 60
            out.append(rd)
    return out


def fake_cases(rng):
    """--fakecigar's shapes, fixed: a read of 300 bases with three records whose query span minus reference span is +7, 0 and -9, the first
    starting at the read's first base (no leading clip), the last ending at its last (no trailing clip), and one record that covers the whole
    read (no clip at all) next to one in the middle"""
    qlen = 300
    q = _rand(rng, qlen); qual = ''.join(chr(35 + i % 40) for i in range(qlen))

    def rec(q_st, q_en, r_st, r_en, contig=0, strand='+', mapq=20):
        return Rec(contig, strand, mapq, q_st, q_en, r_st, r_en, ('%dS' % q_st if q_st else '') + '%dI' % (q_en - q_st) + ('%dS' % (qlen - q_en) if qlen - q_en else ''))
    ends = Read('fake_ends', q, [rec(0, 100, 1000, 1093), rec(100, 180, 2000, 2080, contig=1, strand='-'), rec(180, 300, 500, 629)], qual=qual)
    whole = Read('fake_whole', q, [rec(0, 300, 1000, 1300), rec(120, 170, 3500, 3520, strand='-')], qual=qual)
    for rd in (ends, whole):
        for r in rd.recs:
            assert (r.q_en - r.q_st) - (r.r_en - r.r_st) in (7, 0, -9, 30)
    return [ends, whole]


def cg_cases(rng):
    out = []
    for k in (32767, 32768):
        ops = [((1, '='), (1, 'X'))[i % 2] for i in range(k)]
        half = len(REF[0]) - 50
        ops = ops[:half]                                              # the contig is shorter than 32 768 columns: the rest alternates I and D of one base
        rest = k - len(ops)
        ops += [((1, 'I'), (1, 'D'))[i % 2] for i in range(rest)]
        # D columns must stay inside the contig too: r_st 0 and at most 5950 + rest / 2 reference columns
        out.append(one(rng, 'cg%d' % k, ops, contig=0, r_st=0))
    return out


def asm_cases(rng):
    out = []
    out.append(one(rng, 'asm_continue', [(30, '='), (7, 'X'), (20, '='), (9, 'D'), (5, 'I'), (10, '=')], r_st=100, cigar='10=20=3X4X20=4D5D2I3I10='))
    out.append(one(rng, 'asm_M', [(30, 'M'), (7, 'X')], r_st=100, cigar='30M3X4X'))
    for m0, m1 in ((1, 1), (1, 0), (1, 5), (0, 1), (7, 1)):
        r = multi(rng, 'asm_mq%d_%d' % (m0, m1), 3)
        order = sorted(range(3), key=lambda i: (r.recs[i].q_en - r.recs[i].q_st, i), reverse=True)
        r.recs[order[0]].mapq = m0; r.recs[order[1]].mapq = m1; out.append(r)
    return out


def bulk(rng, n=300):
    """n reads of 200-3000 bases with 1-6 records each over disjoint pieces of the read (so every record's columns agree with the bases), two reads
    in three with =/X CIGARs and the rest with M; some reads failed, some without records, some without qualities"""
    reads = []
    for i in range(n):
        qlen = int(rng.integers(200, 3001)); nrec = int(rng.integers(1, 7)); eqx = i % 3 != 0
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, qlen), 2 * nrec - 1, replace=False))
        cuts = [0] + cuts + [qlen]
        read = list(_rand(rng, qlen)); recs = []
        for j in range(nrec):
            a, b = cuts[2 * j], cuts[2 * j + 1]                         # the piece of the read this record aligns
            contig = int(rng.integers(0, 2)); strand = '+-'[int(rng.integers(0, 2))]
            ops = []; left = b - a
            while left > 0:
                op = ('=X=I=D' if eqx else 'MMIMDM')[int(rng.integers(0, 6))]
                k = min(left, int(rng.integers(1, 90))) if op in '=M' else min(left, int(rng.integers(1, 6)))
                ops.append((k, op)); left -= 0 if op == 'D' else k
            ref_cols = sum(k for k, op in ops if op in '=XMD')
            r_st = int(rng.integers(0, len(REF[contig]) - ref_cols - 1))
            mm = set(int(x) for x in rng.integers(0, b - a, (b - a) // 15))
            piece, text, r_en = apply_ops(rng, ops, contig, r_st, mm)
            read[a:b] = piece if strand == '+' else revcomp(piece)
            lead, trail = (a, qlen - b) if strand == '+' else (qlen - b, a)
            text = ('%dS' % lead if lead else '') + text + ('%dS' % trail if trail else '')
            recs.append(Rec(contig, strand, int(rng.integers(0, 61)), lead, qlen - trail, r_st, r_en, text))
        if i % 37 == 5:
            recs = []
        q = ''.join(read)
        reads.append(Read('bulk%d' % i, q, recs, qual=None if i % 9 == 0 else ''.join(chr(33 + (i + k) % 70) for k in range(qlen)), status=-10 if i % 41 == 17 else 0))
    return reads


def cases():
    """every case but the bulk set: a list of Case"""
    rng = np.random.default_rng(77)
    out = []
    tk = tokeniser(rng); nm = nm_cases(rng); md = md_cases(rng); ln = line_cases(rng); cl = clip_cases(rng); rc = record_cases(rng); cg = cg_cases(rng); am = asm_cases(rng)
    good = [one(rng, 'good%d' % i, [(3, 'S'), (30, '='), (1, 'X'), (20, '='), (2, 'D'), (10, '=')], r_st=800 + i, strand='+-'[i % 2]) for i in range(4)]
    out.append(Case('tokeniser', tk)); out.append(Case('tokeniser_md', tk, md=1, shortcs=1)); out.append(Case('tokeniser_mdlong', tk, md=1)); out.append(Case('tokeniser_asm', tk, asm_mode=1))
    out += count_overflow(rng)
    out.append(Case('nm', nm)); out.append(Case('nm_md', nm, md=1, shortcs=1))
    for i, r in enumerate(raising(rng)):
        out.append(Case('raise_' + r.name, [good[0], r, good[1]])); out.append(Case('raise_md_' + r.name, [good[2], r, good[3]], md=1))
    out.append(Case('md_short', md, md=1, shortcs=1)); out.append(Case('md_long', md, md=1, shortcs=0)); out.append(Case('md_off', md))
    for r in md_raising(rng):
        out.append(Case('mdraise_' + r.name, [good[0], r, good[1]], md=1, shortcs=1)); out.append(Case('mdraise_off_' + r.name, [good[0], r, good[1]]))
    out.append(Case('lines', ln)); out.append(Case('lines_hard', ln, hardclip=1)); out.append(Case('lines_rg', ln, rg='RG-7'))
    out.append(Case('clip_hard', cl, hardclip=1)); out.append(Case('clip_soft', cl)); out.append(Case('clip_md', cl, md=1, hardclip=1))
    out.append(Case('records', rc)); out.append(Case('records_mark', rc, markunbalancetra=1)); out.append(Case('records_fake', rc, fakecigar=1))
    out.append(Case('records_fake_hard', rc, fakecigar=1, hardclip=1, markunbalancetra=1, rg='x'))
    fk = fake_cases(rng)
    out.append(Case('fake_clips', fk, fakecigar=1)); out.append(Case('fake_clips_hard', fk, fakecigar=1, hardclip=1)); out.append(Case('fake_clips_off', fk))
    out.append(Case('cg', cg, cigar2cg=1)); out.append(Case('cg_off', cg)); out.append(Case('cg_md', cg, cigar2cg=1, md=1))
    out.append(Case('asm', am + rc[:3], asm_mode=1)); out.append(Case('asm_md', am, asm_mode=1, md=1, shortcs=1)); out.append(Case('asm_mark', am + rc, asm_mode=1, markunbalancetra=1))
    # statuses and reads without records in the middle of a batch; a batch of nothing
    mid = [good[0], Read('failed', good[1].seq, good[1].recs, qual=good[1].qual, status=-10), good[2], Read('unmapped', _rand(rng, 50), []), good[3],
           Read('failed_norecs', _rand(rng, 20), [], status=-20)]
    out.append(Case('status', mid)); out.append(Case('status_md', mid, md=1)); out.append(Case('empty', [])); out.append(Case('no_records', [Read('u', 'ACGT', [])]))
    return out


def bulk_cases():
    reads = bulk(np.random.default_rng(4242))
    return [Case('bulk_' + k, reads, **v) for k, v in OPTSETS.items()]


# ------------------------------------------------------------------------------------------------ running a case
def pack(VL, case):
    """(names, name_off, seqs, seq_off, quals, qual_off, raw) of a case: blobs as the driver hands them to sam_emit"""
    reads = case.reads

    def blob(items):
        bs = [x.encode() for x in items]
        off = np.zeros(len(bs) + 1, np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        return np.frombuffer(b''.join(bs) + b'\0', np.uint8)[:-1].copy(), off
    names, name_off = blob([r.name for r in reads]); seqs, seq_off = blob([r.seq for r in reads])
    quals, qual_off = blob([r.qual or '' for r in reads])
    nrec = sum(len(r.recs) for r in reads)
    R = (VL.Record * max(nrec, 1))(); cig = b''; k = 0
    for i, rd in enumerate(reads):
        for r in rd.recs:
            t = r.cigar.encode()
            R[k].read_idx = i; R[k].contig = r.contig; R[k].strand = 1 if r.strand == '+' else -1; R[k].mapq = r.mapq
            R[k].q_st, R[k].q_en, R[k].r_st, R[k].r_en = r.q_st, r.q_en, r.r_st, r.r_en
            R[k].cigar_off = len(cig); R[k].cigar_len = len(t); cig += t + b'\0'; k += 1

    class Raw:
        pass
    raw = Raw(); raw.recs = R; raw.nrec = nrec; raw._keep = C.create_string_buffer(cig + b'\0'); raw.blob = C.cast(raw._keep, C.c_void_p)
    raw.status = np.array([r.status for r in reads], np.int32)
    return names, name_off, seqs, seq_off, quals, qual_off, raw


def sam_opts(VL, opts):
    o = dict(md=0, shortcs=0, cigar2cg=0, markunbalancetra=0, hardclip=0, fakecigar=0, rg=None, asm_mode=0); o.update(opts)
    return VL.SamOpts(o['md'], o['shortcs'], o['cigar2cg'], o['markunbalancetra'], o['hardclip'], o['fakecigar'], o['rg'].encode() if o['rg'] else None, o['asm_mode'])


def index(ctx):
    from vacmap_amd.lib import Index
    return Index.from_seqs(ctx, NAMES, REF, k=15, w=10)


def run_host(VL, ctx, idx, case):
    names, name_off, seqs, seq_off, quals, qual_off, raw = pack(VL, case)
    t, off, nl, ns = VL.sam_emit(ctx.lib, idx, sam_opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, nthreads=2)
    return t.tobytes(), off.tolist(), nl, ns


def run_device(VL, ctx, idx, case):
    names, name_off, seqs, seq_off, quals, qual_off, raw = pack(VL, case)
    t, off, nl, ns = VL.sam_emit_device(ctx, idx, sam_opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
    return t.tobytes(), off.tolist(), nl, ns


def check(VL, ctx, idx, case):
    """the device emitter against vm_sam_emit of the same library on one case; returns the device result"""
    if case.err:
        try:
            run_device(VL, ctx, idx, case)
        except VL.VmxError as e:
            assert e.code == {'ARG': -1, 'UNSUPPORTED': -7}[case.err], (case.name, e.args)
            return None
        raise AssertionError('%s: expected VM_ERR_%s' % (case.name, case.err))
    exp = run_host(VL, ctx, idx, case)
    got = run_device(VL, ctx, idx, case)
    if got != exp:
        el = exp[0].split(b'\n'); gl = got[0].split(b'\n')
        for i in range(max(len(el), len(gl))):
            a = el[i] if i < len(el) else None; b = gl[i] if i < len(gl) else None
            if a != b:
                raise AssertionError('%s: line %d differs\nhost:   %r\ndevice: %r\n(lines %d / %d, skipped %d / %d)' % (case.name, i, a and a[:600], b and b[:600], exp[2], got[2], exp[3], got[3]))
        raise AssertionError('%s: offsets or counts differ: host %r device %r' % (case.name, (exp[1][-5:], exp[2], exp[3]), (got[1][-5:], got[2], got[3])))
    return got
