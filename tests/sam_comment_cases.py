"""Seeded inputs for the comment stage of the device SAM emitter (sam_comment in k_sam.hip, vm_sam_emit_device_comments), shared by the emulator
and the GPU tests. Built on sam_device_cases: the same reference, reads and records, each read with a comment (bytes, or None). The expected
bytes are vm_sam_emit's on the same batch and library; `appended` states the rule of emit_read() a second time in Python, on the lines the host
emitter writes without comments. The shapes are the smallest at which the stage can go wrong: tabs and field ends on both sides of the 64-byte
step, fields longer than many steps, a decision that falls steps after the field's start, 64 / 65 / 130 kept tags."""
import struct

import numpy as np

import sam_device_cases as SD

OPS = [(3, 'S'), (30, '='), (1, 'X'), (20, '='), (2, 'D'), (10, '=')]
TYPES_KEPT, TYPES_DROPPED = 'AifZHB', 'cSz '
ALWAYS = (b'SA', b'NM', b'MD', b'cs')


# ------------------------------------------------------------------------------------------------ the rule, in Python
def qualifies(f, rg, cg):
    """a field (bytes between two tabs) by its own bytes and the line's tags"""
    if not (len(f) >= 5 and f[2:3] == b':' and f[4:5] == b':' and f.count(b':') == 2 and f[3:4] in tuple(t.encode() for t in TYPES_KEPT)):
        return False
    return not (f[:2] in ALWAYS or (f[:2] == b'RG' and rg) or (f[:2] == b'CG' and cg))


def appended(comment, rg, cg):
    """what a line gains from its read's comment: every qualifying field that no earlier qualifying field shares its tag with, each behind a tab"""
    if not comment:
        return b''
    fields = comment.split(b'\t')
    ok = [qualifies(f, rg, cg) for f in fields]
    return b''.join(b'\t' + f for k, f in enumerate(fields) if ok[k] and not any(ok[j] and fields[j][:2] == f[:2] for j in range(k)))


def with_rule(plain_text, plain_off, comments, rg):
    """the host emitter's text of a batch without comments -> the text with them, by `appended`"""
    out, off = [], [0]
    for r, com in enumerate(comments):
        part = plain_text[plain_off[r]:plain_off[r + 1]]
        new = b''.join(line + appended(com, rg, b'\tCG:Z:' in line) + b'\n' for line in part.split(b'\n')[:-1])
        out.append(new); off.append(off[-1] + len(new))
    return b''.join(out), off


# ------------------------------------------------------------------------------------------------ builders
def rd(rng, name, comment, strand='+', **kw):
    r = SD.one(rng, name, OPS, r_st=300 + int(rng.integers(0, 400)), strand=strand, **kw)
    r.comment = comment
    return r


def fill(k, start=0):
    """k bytes of value text without tab or colon"""
    return bytes(b'abcdefghijklmnopqrstuvwxyz0123456789,;+-'[(start + j) % 40] for j in range(k))


def field(tag, n, ty='Z'):
    """a valid field of exactly n bytes (n >= 5)"""
    return tag.encode() + b':' + ty.encode() + b':' + fill(n - 5)


def tags(n):
    """n distinct two-character tags, none of them a tag of the line"""
    out = [chr(97 + k // 10) + chr(48 + k % 10) for k in range(n)]
    assert len(set(out)) == n and not {'SA', 'NM', 'MD', 'cs', 'RG', 'CG'} & set(out)
    return out


def ml_field(n):
    """an ML-shaped field of exactly n bytes: ML:B:C,v,v,..."""
    body = b'ML:B:C'
    k = 0
    while len(body) < n:
        body += b',%d' % ((k * 37 + 11) % 256); k += 1
    return body[:n] if body[n - 1:n] != b',' else body[:n - 1] + b'7'


def lengths_and_edges(rng):
    out = []
    for n, com in ((0, b''), (1, b'X'), (4, b'XC:Z'), (5, b'XC:Z:')):
        out.append(rd(rng, 'len%d' % n, com))
    for at in (62, 63, 64, 65):                                       # a tab at byte `at`: the first field has `at` bytes
        com = field('XA', at) + b'\t' + b'XB:i:5'
        assert com.index(b'\t') == at
        out.append(rd(rng, 'tab%d' % at, com, strand='+-'[at & 1]))
    for end in (63, 64, 65):                                          # a field that ends with the comment at byte `end`, alone and behind another
        out.append(rd(rng, 'end%d' % end, field('XA', end)))
        out.append(rd(rng, 'end%d_second' % end, b'XB:i:7\t' + field('XA', end - 7)))
    out.append(rd(rng, 'field200', b'XS:i:1\t' + ml_field(200) + b'\tXT:i:2'))
    out.append(rd(rng, 'field10000', b'MM:Z:C+m?,1,2;\t' + ml_field(10000) + b'\tMN:i:15000'))
    late = b'XD:Z:' + fill(124) + b':'                                # 130 bytes, the third colon is the last: dropped two steps after its start
    assert len(late) == 130 and late.count(b':') == 3
    out.append(rd(rng, 'late_colon', late + b'\tXE:i:1'))
    out.append(rd(rng, 'late_colon_last', b'XE:i:1\t' + late))
    return out


def empty_fields(rng):
    return [rd(rng, 'lead_tab', b'\tXA:i:1'), rd(rng, 'trail_tab', b'XA:i:1\t'), rd(rng, 'double_tab', b'XA:i:1\t\tXB:i:2'), rd(rng, 'only_tab', b'\t'),
            rd(rng, 'tabs3', b'\t\t\t'), rd(rng, 'tabs_around', b'\t\tXA:i:1\t\t')]


def field_shapes(rng):
    out = [rd(rng, 'tag1', b'X:Z:abc\tXK:i:1'), rd(rng, 'tag3', b'XYZ:Z:abc\tXK:i:1'), rd(rng, 'type2', b'XY:ZZ:abc\tXK:i:1'), rd(rng, 'tag0', b':Z:abc'),
           rd(rng, 'colon_in_tag', b'X::Z:a\tXK:i:1'), rd(rng, 'no_type', b'XY::abc'), rd(rng, 'words', b'just words here')]
    for t in TYPES_KEPT:
        out.append(rd(rng, 'type_%s' % t, b'Xa:' + t.encode() + b':q'))
    for t in TYPES_DROPPED:
        out.append(rd(rng, 'type_bad_%d' % ord(t), b'Xa:' + t.encode() + b':q\tXK:i:1'))
    out.append(rd(rng, 'colon_value', b'st:Z:2024-01-01T00:00:00\tXK:i:1'))
    out.append(rd(rng, 'nul_ff', b'XN:Z:a\x00b\xffc\tXO:Z:\xff\x00\tXP:i:\x80'))
    out.append(rd(rng, 'tag_bytes', b'\x00\xff:Z:v\t\x00\xff:Z:w\t  :i:1'))
    return out


def line_tags(rng):
    com = b'SA:Z:x\tNM:i:5\tMD:Z:3\tcs:Z:=A\tXK:i:1\tRG:Z:other\tCG:Z:mine'
    return [rd(rng, 'fixed', com), rd(rng, 'fixed_rev', com, strand='-')]


def cg_read(rng):
    """the 32 768-operator record (its line carries CG:Z: under cigar2cg) and a second, short record of the same read (its line does not)"""
    r = SD.cg_cases(rng)[1]
    qlen = len(r.seq)
    r.recs.append(SD.Rec(1, '+', 30, 10, qlen, 100, 100, '10S%dI' % (qlen - 10)))
    r.name = 'cg_two_lines'
    r.comment = b'CG:Z:mine\tXQ:i:1\tCG:Z:again'
    return r


def duplicates(rng):
    out = [rd(rng, 'dup_first_wins', b'XA:i:1\tXA:i:2\tXB:Z:b\tXA:Z:3'),
           rd(rng, 'dup_bad_first', b'XB:c:1\tXB:Z:a:b\tXB:i:3\tXB:i:4\tXC:Z:\tXC:Z:x')]
    for n in (64, 65, 130):
        T = tags(n)
        fields = [('%s:i:%d' % (t, k)).encode() for k, t in enumerate(T)]
        if n == 130:                                                  # a tag whose first, bad, occurrences lie behind the 64th kept field
            fields.insert(100, b'zz:c:1'); fields.insert(110, b'zz:Z:a:b')
        reps = [T[0], T[min(64, n - 1)], T[n - 1]]
        tail = [('%s:Z:again' % t).encode() for t in reps] + ([b'zz:i:2', b'zz:i:3'] if n == 130 else [])
        out.append(rd(rng, 'tags%d' % n, b'\t'.join(fields + tail), strand='+-'[n & 1]))
    return out


def commented(reads, seed=5):
    """every read of a list of plain reads with a comment of its own"""
    rng = np.random.default_rng(seed)
    for k, r in enumerate(reads):
        r.comment = b'XC:Z:c%d\tXI:i:%d\tNM:i:9\t' % (k, int(rng.integers(0, 1000))) + field('XL', 20 + int(rng.integers(0, 120))) + b'\tXC:Z:twice'
    return reads


def cases():
    rng = np.random.default_rng(99)
    out = []
    le = lengths_and_edges(rng); ef = empty_fields(rng); fs = field_shapes(rng); lt = line_tags(rng); du = duplicates(rng)
    out.append(SD.Case('lengths', le)); out.append(SD.Case('lengths_md', le, md=1, shortcs=1))
    out.append(SD.Case('empty_fields', ef)); out.append(SD.Case('shapes', fs)); out.append(SD.Case('shapes_md_rg', fs, md=1, rg='g1'))
    out.append(SD.Case('line_tags', lt)); out.append(SD.Case('line_tags_rg', lt, rg='grp'))
    cgr = cg_read(rng)
    out.append(SD.Case('cg_on', [cgr], cigar2cg=1)); out.append(SD.Case('cg_off', [cgr], cigar2cg=0))
    out.append(SD.Case('duplicates', du)); out.append(SD.Case('duplicates_md', du, md=1))
    three = SD.multi(rng, 'three', 3, strands='+-+'); three.comment = b'XA:i:1\tSA:Z:no\t' + field('XL', 150) + b'\tXA:i:2'
    nine = SD.multi(rng, 'nine', 9, contigs=(0, 1)); nine.comment = b'XR:Z:nine'
    out.append(SD.Case('records', [three, nine])); out.append(SD.Case('records_hard', [three, nine], hardclip=1, fakecigar=1))
    out.append(SD.Case('records_md_hard', [three, nine], md=1, hardclip=1, rg='x'))
    am = commented(SD.asm_cases(rng))
    out.append(SD.Case('asm', am, asm_mode=1)); out.append(SD.Case('asm_md', am[:2], asm_mode=1, md=1, shortcs=1))
    # a failed read and a raising read, each with a comment, between commented neighbours; reads without a comment between reads with one
    good = [rd(rng, 'good%d' % i, b'XG:i:%d\t' % i + field('XL', 60 + 3 * i), strand='+-'[i % 2]) for i in range(4)]
    failed = SD.Read('failed', good[1].seq, good[1].recs, qual=good[1].qual, status=-10); failed.comment = b'XF:Z:failed'
    out.append(SD.Case('skip_status', [good[0], failed, good[2]]))
    for r in SD.raising(rng):
        r.comment = b'XF:Z:raises\t' + field('XL', 100)
        out.append(SD.Case('skip_raise_' + r.name, [good[0], r, good[3]]))
    bare = [rd(rng, 'bare%d' % i, None) for i in range(3)]
    norecs = SD.Read('unmapped', 'ACGTACGT', []); norecs.comment = b'XU:Z:unmapped'
    out.append(SD.Case('mixed', [bare[0], good[0], bare[1], norecs, good[1], rd(rng, 'empty_comment', b''), good[2], bare[2]]))
    out.append(SD.Case('mixed_md', [good[3], bare[0], good[0]], md=1))
    out.append(SD.Case('no_comments', bare)); out.append(SD.Case('empty', []))
    return out


def bulk_cases():
    reads = commented(SD.bulk(np.random.default_rng(4242), n=120), seed=6)
    for k, r in enumerate(reads):
        if k % 7 == 3:
            r.comment = None
        if k % 11 == 5:
            r.comment = ml_field(700 + 13 * k) + b'\tMM:Z:C+m?;'
    return [SD.Case('bulk_c_' + k, reads, **SD.OPTSETS[k]) for k in ('default', 'hard_fake_rg', 'md_short', 'asm')]


# ------------------------------------------------------------------------------------------------ running a case
def comments_of(case):
    return [getattr(r, 'comment', None) for r in case.reads]


def pack(VL, case, lead=0):
    """SD.pack's tuple and (comments, com_off): the comment blob as the driver hands it to sam_emit. lead: bytes of something else before the first
    comment (com_off[0] = lead). (None, None) for a case without reads."""
    base = SD.pack(VL, case)
    coms = [c or b'' for c in comments_of(case)]
    if not coms:
        return base, None, None
    off = np.zeros(len(coms) + 1, np.int64)
    off[1:] = np.cumsum([len(c) for c in coms])
    blob = np.frombuffer(b'?' * lead + b''.join(coms) + b'\0', np.uint8)[:-1].copy()
    return base, blob, off + lead


def run_host(VL, ctx, idx, case, with_comments=True, lead=0):
    (names, name_off, seqs, seq_off, quals, qual_off, raw), cb, co = pack(VL, case, lead)
    kw = dict(comments=cb, com_off=co) if with_comments and cb is not None else {}
    t, off, nl, ns = VL.sam_emit(ctx.lib, idx, SD.sam_opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, nthreads=2, **kw)
    return t.tobytes(), off.tolist(), nl, ns


def run_device(VL, ctx, idx, case, with_comments=True, lead=0):
    (names, name_off, seqs, seq_off, quals, qual_off, raw), cb, co = pack(VL, case, lead)
    kw = dict(comments=cb, com_off=co) if with_comments and cb is not None else dict(comments=None, com_off=None)
    t, off, nl, ns = VL.sam_emit_device(ctx, idx, SD.sam_opts(VL, case.opts), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off, **kw)
    return t.tobytes(), off.tolist(), nl, ns


def _first_difference(name, exp, got, what):
    el = exp[0].split(b'\n'); gl = got[0].split(b'\n')
    for i in range(max(len(el), len(gl))):
        a = el[i] if i < len(el) else None; b = gl[i] if i < len(gl) else None
        if a != b:
            k = next((j for j in range(min(len(a or b''), len(b or b''))) if a[j] != b[j]), min(len(a or b''), len(b or b'')))
            raise AssertionError('%s: line %d differs from %s at byte %d\nwant: %r\ngot:  %r' % (name, i, what, k, a and a[max(0, k - 80):k + 200], b and b[max(0, k - 80):k + 200]))
    raise AssertionError('%s: offsets or counts differ from %s: want %r got %r' % (name, what, exp[1:], got[1:]))


def check(VL, ctx, idx, case, lead=0):
    """the device emitter with comments against vm_sam_emit of the same library (text, text_off, lines, skipped) and against the Python statement
    of the rule applied to vm_sam_emit's lines without comments; returns the device result"""
    exp = run_host(VL, ctx, idx, case, lead=lead)
    got = run_device(VL, ctx, idx, case, lead=lead)
    if got != exp:
        _first_difference(case.name, exp, got, 'vm_sam_emit')
    plain = run_host(VL, ctx, idx, case, with_comments=False)
    text, off = with_rule(plain[0], plain[1], comments_of(case), bool(case.opts.get('rg')))
    if (got[0], got[1]) != (text, off):
        _first_difference(case.name, (text, off), got, 'the Python rule')
    assert got[2:] == plain[2:]
    return got


# ------------------------------------------------------------------------------------------------ the driver, run by both suites
def _lines(path):
    return [x for x in open(path).read().split('\n') if not x.startswith('@PG')]


def _counted(VL, monkeypatch):
    calls = {'device': 0, 'commented': 0}
    dev = VL.sam_emit_device

    def counted(*a, **kw):
        calls['device'] += 1
        calls['commented'] += kw.get('comments') is not None
        return dev(*a, **kw)
    monkeypatch.setattr(VL, 'sam_emit_device', counted)
    return calls


def fastq_inputs(d):
    """a two-contig 70 kb reference, 8 reads of ~1.5 kb with FASTQ comments (one field repeated, one the line carries), a 6 kb assembly contig with one"""
    from vacmap_amd import synth
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = d / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 8, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    fq = d / 'r.fq'
    fq.write_text(''.join('@q%d XC:Z:c%d\tNM:i:77\tXI:i:%d\tXC:Z:again\n%s\n+\n%s\n' % (i, i, i, cat[off[i]:off[i + 1]].tobytes().decode(),
                                                                                      ''.join(chr(40 + (i + k) % 50) for k in range(int(off[i + 1] - off[i])))) for i in range(8)))
    asm = d / 'asm.fa'
    piece = synth.implant_svs(contigs[0][10000:16000], [('DEL', 3000, 200)])
    asm.write_text('>tig1 XT:Z:tig\tcs:Z:no\n%s\n' % piece.tobytes().decode())
    return fa, fq, asm


def check_driver_copycomments(VL, d, monkeypatch, capture, t='2', batch='3'):
    """--copycomments --sam-emitter device-comments writes the --copycomments host file through sam_emit_device, with no fallback line; without
    comments the choice is `device`; -mode asm hands its comments over too"""
    from vacmap_amd import driver
    calls = _counted(VL, monkeypatch)
    fa, fq, asm = fastq_inputs(d)
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', t, '--nowriteindex', '--batch-reads', batch, '--inflight', '2', '--eqx', '--MD']
    out = {}
    for tag, extra in (('host_c', ['--copycomments']), ('devc_c', ['--copycomments', '--sam-emitter', 'device-comments']), ('device', ['--sam-emitter', 'device']),
                       ('devc', ['--sam-emitter', 'device-comments'])):
        capture.readouterr(); calls['device'] = calls['commented'] = 0
        assert driver.main(common + extra + ['-o', str(d / (tag + '.sam'))]) == 0
        out[tag] = (_lines(d / (tag + '.sam')), capture.readouterr().err, calls['device'], calls['commented'])
    body = [x for x in out['host_c'][0] if x and not x.startswith('@')]
    assert len(body) >= 8 and all('\tXC:Z:c' in x and '\tXI:i:' in x and 'XC:Z:again' not in x and 'NM:i:77' not in x for x in body)
    assert out['devc_c'][0] == out['host_c'][0] and out['devc_c'][2] >= 3 and out['devc_c'][3] >= 3 and out['host_c'][2] == 0
    assert 'host SAM emitter' not in out['devc_c'][1] and 'host SAM emitter' not in out['devc'][1]
    assert out['devc'][0] == out['device'][0] != out['host_c'][0] and out['devc'][3] == 0 and out['devc'][2] == out['device'][2]
    for tag, extra in (('asm_host_c', ['--copycomments']), ('asm_devc_c', ['--copycomments', '--sam-emitter', 'device-comments'])):
        calls['device'] = calls['commented'] = 0
        assert driver.main(['-ref', str(fa), '-read', str(asm), '-mode', 'asm', '-workdir', str(d / 'wd'), '-t', t, '--nowriteindex', '-o', str(d / (tag + '.sam'))] + extra) == 0
        out[tag] = (_lines(d / (tag + '.sam')), calls['device'], calls['commented'])
    assert out['asm_devc_c'][0] == out['asm_host_c'][0] and out['asm_devc_c'][1:] == (1, 1) and out['asm_host_c'][1] == 0
    body = [x for x in out['asm_host_c'][0] if x and not x.startswith('@')]
    assert body and all(x.endswith('\tXT:Z:tig') for x in body)


def check_driver_bam_tags(VL, d, monkeypatch, capture):
    """--bam-tags MM,ML,MN --bam-reader native --sam-emitter device-comments writes the file of the Python reader and the host emitter; written as
    BAM by the native writer it decodes to the same tag values"""
    import bam_codec as B
    import bam_tag_cases as BT
    from vacmap_amd import driver
    calls = _counted(VL, monkeypatch)
    fa, bam, reads = BT.driver_inputs(d)
    common = ['-ref', str(fa), '-t', '2', '--nowriteindex', '--batch-reads', '4', '--window-batches', '2', '--inflight', '2', '-workdir', str(d / 'wd'), '-mode', 'H',
              '-read', str(bam), '--bam-tags', 'MM,ML,MN']

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@')]
    assert driver.main(common + ['-o', str(d / 'py.sam')]) == 0
    assert calls['device'] == 0
    capture.readouterr()
    assert driver.main(common + ['-o', str(d / 'devc.sam'), '--bam-reader', 'native', '--sam-emitter', 'device-comments']) == 0
    err = capture.readouterr().err
    a = body(d / 'py.sam')
    assert body(d / 'devc.sam') == a and len(a) >= len(reads) - 2 and 'host SAM emitter' not in err and calls['commented'] >= 4
    want = {nm: BT.aux_text(aux, ['MM', 'ML', 'MN'])[0] for nm, _, _, _, aux in reads}
    assert all(x.endswith('\t' + want[x.split('\t')[0]]) for x in a)
    assert driver.main(common + ['-o', str(d / 'host.bam'), '--bam-reader', 'native', '--bam-writer', 'native']) == 0
    assert driver.main(common + ['-o', str(d / 'devc.bam'), '--bam-reader', 'native', '--bam-writer', 'native', '--sam-emitter', 'device-comments']) == 0
    _, _, hrecs = B.read_bam(open(d / 'host.bam', 'rb').read())
    _, _, drecs = B.read_bam(open(d / 'devc.bam', 'rb').read())
    assert len(drecs) == len(a) and drecs == hrecs
    by = {nm: aux for nm, _, _, _, aux in reads}
    for f, tags in drecs:
        exp = [t for t in BT.aux_values(by[f[0]]) if t[0] in ('MM', 'ML', 'MN')]
        got = [(tg, ty, struct.pack('<f', v) if ty == 'f' else v) for tg, ty, v in tags if tg in ('MM', 'ML', 'MN', 'rq', 'np', 'st')]
        assert got == exp, (f[0], got[:3], exp[:3])
