"""Seeded inputs for vm_sam_opts.keep_unmapped (--keep-unmapped): a read that emits no record line (no record, a status other than 0, or an
emission that raises) stays in the text as one FLAG 4 line at its place. Shared by the host, emulator and GPU tests; built on sam_device_cases
(reference, reads, records) and the comment shapes of sam_comment_cases.

The reference has no such output, so the yardstick is the SAM specification, stated here in `unmapped_line` by plain string formatting, without
vacmap_amd.sam and without the library:

    QNAME 4 * 0 0 * * 0 0 SEQ QUAL [RG:Z:id] [comment fields]

MAPQ 0; SEQ the read as given, whole, in its own orientation, '*' when empty; QUAL the string when its length is the read's and not 0, else '*';
the comment fields by the rule of the record lines (`kept_fields`), the line's own tags being SA, NM, MD, cs always and RG under a read group.
Which reads emit no record line is known by construction (`emits`); a read that does emit keeps the bytes the emitter writes for it with the
option off. The shapes are the smallest at which the per-read wave can go wrong: reads of 0 / 1 / 63 / 64 / 65 / 128 / 129 bases, names of 1 and
254 characters, a batch without any record, unmapped reads first, last and in a row, comment tabs on both sides of the 64-byte step."""
import numpy as np

import sam_comment_cases as CC
import sam_device_cases as SD

LENGTHS = (0, 1, 63, 64, 65, 128, 129)
TYPES = (b'A', b'i', b'f', b'Z', b'H', b'B')


# ------------------------------------------------------------------------------------------------ the rule, by string formatting
def kept_fields(comment, rg):
    """the tab-separated XX:T:value fields of a comment that an unmapped line carries, each behind a tab"""
    out, seen = b'', {b'SA', b'NM', b'MD', b'cs'} | ({b'RG'} if rg else set())
    for f in (comment or b'').split(b'\t'):
        parts = f.split(b':')
        if len(parts) == 3 and len(parts[0]) == 2 and parts[1] in TYPES and parts[0] not in seen:
            out += b'\t' + f
            seen.add(parts[0])
    return out


def unmapped_line(read, rg):
    seq = read.seq.encode() or b'*'
    qual = read.qual.encode() if read.qual and read.seq and len(read.qual) == len(read.seq) else b'*'
    line = b'%s\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s' % (read.name.encode(), seq, qual)
    if rg:
        line += b'\tRG:Z:' + rg.encode()
    return line + kept_fields(getattr(read, 'comment', None), rg) + b'\n'


def emits(read):
    """the read writes record lines"""
    return read.status == 0 and bool(read.recs) and not getattr(read, 'raises', False)


def expected(case, off_text, off_off, off_lines, with_comments=True):
    """(text, text_off, n_lines, n_skipped) of a case under keep_unmapped, from the emitter's result with the option off"""
    parts = []
    for k, r in enumerate(case.reads):
        mine = off_text[off_off[k]:off_off[k + 1]]
        if emits(r):
            assert mine.count(b'\n') >= 1
            parts.append(mine)
        else:
            assert mine == b'', (case.name, r.name)
            bare = SD.Read(r.name, r.seq, [], qual=r.qual)
            bare.comment = getattr(r, 'comment', None) if with_comments else None
            parts.append(unmapped_line(bare, case.opts.get('rg')))
    off = [0]
    for p in parts:
        off.append(off[-1] + len(p))
    skipped = sum(1 for r in case.reads if r.status != 0 or (r.recs and getattr(r, 'raises', False)))
    return b''.join(parts), off, off_lines + sum(1 for r in case.reads if not emits(r)), skipped


# ------------------------------------------------------------------------------------------------ builders
def qual_of(n, k=0):
    return ''.join(chr(33 + (7 * i + k) % 60) for i in range(n))


def U(rng, name, n, qual='same', comment=None, status=0):
    """a read of n bases without records. qual: 'same' (of the read's length), None, 'short' (one less; one for an empty read), 'long' (one more)"""
    q = {'same': qual_of(n), None: None, 'short': qual_of(n - 1 if n else 1), 'long': qual_of(n + 1)}[qual]
    r = SD.Read(name, SD._rand(rng, n), [], qual=q, status=status)
    r.comment = comment
    return r


def good(rng, k, comment=None):
    r = SD.one(rng, 'good%d' % k, CC.OPS, r_st=800 + 7 * k, strand='+-'[k % 2])
    r.comment = comment
    return r


def raisers(rng, md):
    """reads whose emission raises: under every option set (an M run past a sequence end) or, md, under MD / cs only (an X run past one)"""
    out = SD.md_raising(rng)[:3] if md else SD.raising(rng)
    for r in out:
        r.raises = True
        r.comment = b'XF:Z:raises\t' + CC.field('XL', 70)
    return out


def length_reads(rng):
    out = []
    for n in LENGTHS:
        out.append(U(rng, 'len%d' % n, n)); out.append(U(rng, 'len%d_noqual' % n, n, qual=None))
        out.append(U(rng, 'len%d_short' % n, n, qual='short')); out.append(U(rng, 'len%d_long' % n, n, qual='long'))
    out.append(U(rng, 'n', 70)); out.append(U(rng, 'N' * 254, 70)); out.append(U(rng, 'e', 0, qual=None)); out.append(U(rng, 'M' * 254, 129, qual=None))
    return out


def comment_reads(rng):
    out = [U(rng, 'c_none', 40), U(rng, 'c_empty', 40, comment=b''), U(rng, 'c_one', 40, comment=b'XC:Z:one'), U(rng, 'c_words', 40, comment=b'just words')]
    for at in (63, 64, 65):
        com = CC.field('XA', at) + b'\t' + b'XB:i:5'
        assert com.index(b'\t') == at
        out.append(U(rng, 'c_tab%d' % at, 30 + at, comment=com))
    out.append(U(rng, 'c_line_tags', 64, comment=b'SA:Z:x\tNM:i:5\tMD:Z:3\tcs:Z:=A\tXK:i:1\tRG:Z:other\tCG:Z:mine'))
    out.append(U(rng, 'c_dup', 65, qual=None, comment=b'XA:i:1\tXA:i:2\tXB:Z:b\tXA:Z:3\tXB:c:1'))
    T = CC.tags(130)
    out.append(U(rng, 'c_tags130', 1, comment=b'\t'.join([('%s:i:%d' % (t, k)).encode() for k, t in enumerate(T)] + [('%s:Z:again' % t).encode() for t in (T[0], T[64], T[129])])))
    out.append(U(rng, 'c_long', 0, comment=b'MM:Z:C+m?,1,2;\t' + CC.ml_field(3000) + b'\tMN:i:0'))
    return out


def mixed_reads(rng, tag):
    """unmapped reads first, last and three in a row between mapped reads; a failed read with records (minus strand) and one without; all commented"""
    g = [good(rng, k, b'XG:i:%d\t' % k + CC.field('XL', 60 + 3 * k)) for k in range(4)]
    failed = SD.Read('failed', g[1].seq, g[1].recs, qual=g[1].qual, status=-10); failed.comment = b'XF:Z:failed\tRG:Z:mine'
    u = [U(rng, '%s_u%d' % (tag, k), (65, 1, 129, 64, 200)[k], qual=(None, 'same', 'same', 'short', 'same')[k], comment=(b'XU:i:%d' % k) if k != 3 else None) for k in range(5)]
    return [u[0], g[0], u[1], u[2], u[3], g[2], failed, U(rng, 'failed_norecs', 20, status=-20, comment=b'XF:Z:norecs'), g[3], u[4]]


def cases():
    rng = np.random.default_rng(4141)
    out = [SD.Case('lengths', length_reads(rng)), SD.Case('lengths_rg_hard', length_reads(rng), rg='grp', hardclip=1)]      # batches without any record
    out.append(SD.Case('one_empty', [U(rng, 'only', 0, qual=None)])); out.append(SD.Case('nothing', []))
    cm = comment_reads(rng)
    out.append(SD.Case('comments', cm)); out.append(SD.Case('comments_rg', cm, rg='g1'))
    for k, v in SD.OPTSETS.items():
        out.append(SD.Case('mixed_' + k, mixed_reads(rng, k), **v))
    g = [good(rng, 10 + k, b'XG:i:%d' % k) for k in range(2)]
    for r in raisers(rng, md=False):
        out.append(SD.Case('raise_' + r.name, [g[0], r, g[1]])); out.append(SD.Case('raise_md_rg_' + r.name, [g[0], r, g[1]], md=1, rg='r1')); out.append(SD.Case('raise_hard_' + r.name, [g[0], r, g[1]], hardclip=1, fakecigar=1))
    for r in raisers(rng, md=True):
        out.append(SD.Case('mdraise_' + r.name, [g[0], r, g[1]], md=1, shortcs=1))
    for c in out:
        c.opts['keep_unmapped'] = 1
    return out


def bulk_cases():
    """300 reads (more than one scan block of line slots), every third without records, some failed, all but a few commented"""
    reads = CC.commented(SD.bulk(np.random.default_rng(4242)), seed=8)
    for k, r in enumerate(reads):
        if k % 3 == 1:
            r.recs = []
        if k % 7 == 3:
            r.comment = None
    assert 100 <= sum(1 for r in reads if not emits(r)) <= 120
    # (the option sets under which no read of the bulk set raises: which reads emit is then known by construction; raising reads are cases of their own)
    return [SD.Case('bulk_u_' + k, reads, keep_unmapped=1, **SD.OPTSETS[k]) for k in ('default', 'hard_fake_rg', 'cg', 'asm')]


# ------------------------------------------------------------------------------------------------ running a case
def sam_opts(VL, opts, keep=None):
    o = dict(md=0, shortcs=0, cigar2cg=0, markunbalancetra=0, hardclip=0, fakecigar=0, rg=None, asm_mode=0, keep_unmapped=0); o.update(opts)
    return VL.SamOpts(o['md'], o['shortcs'], o['cigar2cg'], o['markunbalancetra'], o['hardclip'], o['fakecigar'], o['rg'].encode() if o['rg'] else None, o['asm_mode'],
                      o['keep_unmapped'] if keep is None else keep)


def run(VL, ctx, idx, case, keep=None, device=False, with_comments=True):
    """(text, text_off, n_lines, n_skipped) of the host emitter (of ctx's library) or the device emitter; keep: the option, when not the case's"""
    (names, name_off, seqs, seq_off, quals, qual_off, raw), cb, co = CC.pack(VL, case)
    o = sam_opts(VL, case.opts, keep)
    if device:
        kw = dict(comments=cb, com_off=co) if with_comments and cb is not None else {}
        t, off, nl, ns = VL.sam_emit_device(ctx, idx, o, names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, **kw)
    else:
        kw = dict(comments=cb, com_off=co) if with_comments and cb is not None else {}
        t, off, nl, ns = VL.sam_emit(ctx.lib, idx, o, names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, nthreads=2, **kw)
    return t.tobytes(), off.tolist(), nl, ns


def differ(name, exp, got, what):
    """raises with the first line that differs"""
    if got == exp:
        return
    el = exp[0].split(b'\n'); gl = got[0].split(b'\n')
    for i in range(max(len(el), len(gl))):
        a = el[i] if i < len(el) else None; b = gl[i] if i < len(gl) else None
        if a != b:
            raise AssertionError('%s: line %d differs from %s\nwant: %r\ngot:  %r' % (name, i, what, a and a[:300], b and b[:300]))
    raise AssertionError('%s: offsets or counts differ from %s: want %r got %r' % (name, what, (exp[1][-4:], exp[2:]), (got[1][-4:], got[2:])))


def check_host(VL, ctx, idx, case):
    """vm_sam_emit under the option against `expected`, with and without comments; returns its result with comments"""
    res = None
    for wc in (False, True):
        off = run(VL, ctx, idx, case, keep=0, with_comments=wc)
        got = run(VL, ctx, idx, case, with_comments=wc)
        differ(case.name, expected(case, off[0], off[1], off[2], with_comments=wc), got, 'the specification')
        assert off[3] == got[3]
        res = got
    return res


def check_device(VL, ctx, idx, case):
    """the device emitter against vm_sam_emit of the same library: option on and off, with and without comments; returns the on / commented result"""
    res = None
    for keep in (0, 1):
        for wc in (False, True):
            got = run(VL, ctx, idx, case, keep=keep, device=True, with_comments=wc)
            differ(case.name, run(VL, ctx, idx, case, keep=keep, with_comments=wc), got, 'vm_sam_emit (keep_unmapped %d, comments %d)' % (keep, wc))
            res = got
    return res


# ------------------------------------------------------------------------------------------------ the driver, run by both suites
def driver_inputs(d, n_aligned, n_random, n_tiny, ref_lens=(1200000, 300000), mean_len=4000):
    """a reference, and a FASTQ of n_aligned synthetic reads with n_random random 500-base reads and n_tiny twelve-base reads spread among them;
    every read has an XC:Z: comment. Returns (reference path, FASTQ path, read names in input order)."""
    from vacmap_amd import synth
    contigs = synth.make_reference(list(ref_lens), seed=5)
    donor = synth.implant_svs(contigs[0], [('INV', ref_lens[0] // 3, 4000), ('DEL', 2 * ref_lens[0] // 3, 900)])
    reads = [synth.tostr(r[1]) for r in synth.sample_reads([donor, contigs[1]], n_aligned, mean_len=mean_len, err=0.08, seed=6, min_len=800, max_len=3 * mean_len)]
    rng = np.random.default_rng(31)
    named = [('read%d' % i, s) for i, s in enumerate(reads)]
    extra = [('rnd%d' % i, SD._rand(rng, 500)) for i in range(n_random)] + [('tiny%d' % i, SD._rand(rng, 12)) for i in range(n_tiny)]
    for k, e in enumerate(extra):                                      # first, last, and spread in between
        at = 0 if k == 0 else (len(named) if k == 1 else int(rng.integers(1, len(named))))
        named.insert(at, e)
    fa = d / 'ref.fa'; fq = d / 'reads.fq'
    fa.write_text(''.join('>%s\n%s\n' % (n, synth.tostr(c)) for n, c in zip(['chr1', 'chr2'], contigs)))
    fq.write_text(''.join('@%s XC:Z:c%d\tNM:i:77\n%s\n+\n%s\n' % (n, i, s, qual_of(len(s), i)) for i, (n, s) in enumerate(named)))
    return fa, fq, [n for n, _ in named]


def check_driver(d, fa, fq, names, least, t='4', batch='64', bam=True):
    """-mode H without --keep-unmapped and with it, on the host emitter, the device-comments emitter, --bam-writer native and native-sort (five runs). Which reads
    are unmapped is read off the run without the flag: the names that have no line (at least `least`, so that nothing passes empty). bam=False: the
    SAM runs alone (the emulator suite, where tests/test_bam_sorted_emu.py already takes FLAG 4 lines through the writers)."""
    import bam_codec as B
    import csi_codec as CS
    from vacmap_amd import driver
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', t, '--nowriteindex', '--batch-reads', batch, '--copycomments', '-workdir', str(d / 'wd')]

    def body(tag, extra):
        assert driver.main(common + extra + ['-o', str(d / (tag + '.sam'))]) == 0
        return [x for x in open(d / (tag + '.sam')).read().split('\n') if x and not x.startswith('@')]
    off = body('off', [])
    on = body('on', ['--keep-unmapped'])
    dev = body('dev', ['--keep-unmapped', '--sam-emitter', 'device-comments'])
    mapped = set(x.split('\t')[0] for x in off)
    lost = [n for n in names if n not in mapped]
    assert len(lost) >= least, (len(lost), least)
    assert all(x.split('\t')[1] != '4' for x in off)
    # the mapped lines are the same lines; every name occurs; the FLAG 4 lines stand where their reads stood in the input
    assert [x for x in on if x.split('\t')[1] != '4'] == off
    four = [x for x in on if x.split('\t')[1] == '4']
    assert [x.split('\t')[0] for x in four] == lost
    order = []
    for x in on:
        if not order or order[-1] != x.split('\t')[0]:
            order.append(x.split('\t')[0])
    assert order == names
    at = {n: i for i, n in enumerate(names)}
    for x in four:
        f = x.split('\t')
        assert f[2:9] == ['*', '0', '0', '*', '*', '0', '0'] and len(f[9]) == len(f[10]) > 0 and f[11:] == ['RG:Z:1', 'XC:Z:c%d' % at[f[0]]], f[:9] + f[11:]
    assert dev == on
    if not bam:
        return lost
    # BAM (unsorted from the host emitter's lines, sorted from the device emitter's): the same records; sorted, the FLAG 4 records come last and the
    # index counts them
    assert driver.main(common + ['--keep-unmapped', '--bam-writer', 'native', '-o', str(d / 'host.bam')]) == 0
    assert driver.main(common + ['--keep-unmapped', '--sam-emitter', 'device-comments', '--bam-writer', 'native-sort', '-o', str(d / 's.sorted.bam')]) == 0
    hrecs = B.read_bam(open(d / 'host.bam', 'rb').read())[2]
    assert len(hrecs) == len(on) and all(B.same_as_sam(r, ln) for r, ln in zip(hrecs, on))
    sdata = open(d / 's.sorted.bam', 'rb').read()
    srecs = B.read_bam(sdata)[2]
    k = len(srecs) - len(lost)
    assert all(r[0][1] != '4' and r[0][2] != '*' for r in srecs[:k]) and [r[0][0] for r in srecs[k:]] == lost and all(r[0][1] == '4' and r[0][2] == '*' for r in srecs[k:])
    assert sorted(srecs, key=repr) == sorted(hrecs, key=repr)
    assert all(('XC', 'Z', 'c%d' % at[r[0][0]]) in r[1] for r in srecs[k:])
    assert CS.parse(open(d / 's.sorted.bam.csi', 'rb').read())['n_no_coor'] == len(lost)
    return lost
