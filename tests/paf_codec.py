"""An independent PAF parser, and PAF lines derived from SAM record lines: a second statement of the PAF rule (include/vacmapx.h) that shares no
code with vacmap_amd/paf.py or the emitters. paf_from_sam_line is valid where the record's q_st / q_en equal its end clips (what the aligner
returns; constructed cases say so per read: clips_agree)."""
import re

_OP = re.compile(r'(\d+)([MIDNSHP=X])')
_INT = re.compile(r'-?\d+\Z')


def parse(line):
    """the columns of a PAF line as a dict; AssertionError on anything the format does not allow"""
    assert not line.endswith('\n') and '\n' not in line
    c = line.split('\t')
    assert len(c) >= 12, line
    for k in (1, 2, 3, 6, 7, 8, 9, 10, 11):
        assert _INT.match(c[k]), (k, c[k])
    d = dict(qname=c[0], qlen=int(c[1]), qs=int(c[2]), qe=int(c[3]), strand=c[4], tname=c[5], tlen=int(c[6]), ts=int(c[7]), te=int(c[8]), nmatch=int(c[9]), alen=int(c[10]),
             mapq=int(c[11]), tags={})
    assert d['strand'] in ('+', '-', '*')
    order = []
    for t in c[12:]:
        m = re.match(r'([A-Za-z][A-Za-z0-9]):([AifZ]):(.*)\Z', t, re.S)
        assert m, t
        assert m.group(1) not in d['tags'], t
        d['tags'][m.group(1)] = (m.group(2), m.group(3)); order.append(m.group(1))
    d['tag_order'] = order
    if d['strand'] == '*':                          # the line of a read without a record line
        assert c[2:12] == ['0', '0', '*', '*', '0', '0', '0', '0', '0', '0'] and not order
        return d
    assert 0 <= d['mapq'] <= 255 and d['tags']['tp'] == ('A', 'P') and d['tags']['NM'][0] == 'i'
    assert d['nmatch'] == d['alen'] - int(d['tags']['NM'][1])
    assert order[:2] == ['tp', 'NM'] and order[2:] in ([], ['cg'], ['MD', 'cs'], ['cg', 'MD', 'cs'])
    if 'cg' in d['tags']:
        cg = d['tags']['cg'][1]
        ops = _OP.findall(cg)
        assert cg and ''.join(n + o for n, o in ops) == cg and ops[0][1] not in 'SH' and ops[-1][1] not in 'SH'
        assert sum(int(n) for n, o in ops if o in 'M=XID') == d['alen']       # (te - ts is not checked: constructed records may carry any r_en)
    else:
        assert d['alen'] == 0
    return d


def paf_from_sam_line(line, qlen, contig_len):
    """the PAF line of a SAM line of the emitters. Record line: strand from FLAG, r_st from POS, MAPQ and NM from the line's own fields, r_en from
    the CIGAR's reference span, qs / qe from the end clips and the strand, cg by stripping the end clips, alen from the CIGAR (taken from CG:Z: where
    the column holds '*'). FLAG 4: the unmapped line. qlen: the read's length; contig_len: name -> length."""
    c = line.split('\t')
    flag = int(c[1])
    if flag & 4:
        return '%s\t%d\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0' % (c[0], qlen)
    tags = {}
    for t in c[11:]:
        k, ty, v = t.split(':', 2)
        tags.setdefault(k, v)
    cigar = c[5] if c[5] != '*' else tags['CG']
    ops = [(int(n), o) for n, o in _OP.findall(cigar)]
    assert ''.join('%d%s' % x for x in ops) == cigar
    a = 0
    while a < len(ops) and ops[a][1] in 'SH':
        a += 1
    b = len(ops)
    while b > a and ops[b - 1][1] in 'SH':
        b -= 1
    lead = sum(n for n, o in ops[:a]); trail = sum(n for n, o in ops[b:])
    strand = '-' if flag & 16 else '+'
    qs, qe = (lead, qlen - trail) if strand == '+' else (trail, qlen - lead)
    r_st = int(c[3]) - 1
    r_en = r_st + sum(n for n, o in ops if o in 'M=XDN')
    alen = sum(n for n, o in ops if o in 'M=XID')
    nm = int(tags['NM'])
    out = [c[0], str(qlen), str(qs), str(qe), strand, c[2], str(contig_len[c[2]]), str(r_st), str(r_en), str(alen - nm), str(alen), c[4], 'tp:A:P', 'NM:i:%d' % nm]
    if b > a:
        out.append('cg:Z:' + ''.join('%d%s' % x for x in ops[a:b]))
    if 'MD' in tags:
        out.append('MD:Z:' + tags['MD']); out.append('cs:Z:' + tags['cs'])
    return '\t'.join(out)


def clips_agree(cigar, q_st, q_en, r_st, r_en, qlen):
    """paf_from_sam_line's precondition on a record: its q_st / q_en are its end clips, its r_en its reference span"""
    ops = [(int(n), o) for n, o in _OP.findall(cigar)]
    if not ops or ''.join('%d%s' % x for x in ops) != cigar:
        return False
    a = 0
    while a < len(ops) and ops[a][1] in 'SH':
        a += 1
    b = len(ops)
    while b > a and ops[b - 1][1] in 'SH':
        b -= 1
    return q_st == sum(n for n, o in ops[:a]) and q_en == qlen - sum(n for n, o in ops[b:]) and r_en == r_st + sum(n for n, o in ops if o in 'M=XDN')
