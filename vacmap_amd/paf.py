"""PAF emission for the records of vm_align_batch: the Python statement of the rule that vm_paf_emit and vm_paf_emit_device implement
(include/vacmapx.h states it once). A sibling of sam.py: a PAF line exists exactly where `sam.sam_lines` makes a record line, with the same
reassign_mapq, the same order inside a read and the same raises, and its MAPQ, NM, MD and cs are that line's. Pure Python; no GPU involved.

    QNAME qlen qs qe strand TNAME tlen r_st r_en nmatch alen MAPQ tp:A:P NM:i:nm [cg:Z:cg] [MD:Z:md cs:Z:cs]
"""
from .sam import merge_cigar, merge_cigar_nm, nm_from_cigar, md_cs, reassign_mapq, revcomp


def strip_clips(ops):
    """the flat [count, op, ...] list without its leading and its trailing maximal run of S / H operators (interior ones stay)"""
    a, b = 0, len(ops)
    while a < b and ops[a + 1] in 'SH':
        a += 2
    while b > a and ops[b - 1] in 'SH':
        b -= 2
    return ops[a:b]


def aligned_length(ops):
    """alen: the lengths of the M = X I D operators (N, S, H, P are not counted)"""
    return sum(int(ops[i - 1]) for i in range(1, len(ops), 2) if ops[i] in 'M=XID')


def _clamp(v, hi):
    return 0 if v < 0 else (hi if v > hi else v)


def unmapped_line(name, qlen):
    """the line of a read that emits no record line, under keep_unmapped"""
    return '%s\t%d\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0' % (name, qlen)


def paf_lines(records, query, refseq, contig_len, md=False, shortcs=True, markunbalancetra=True, asm=False):
    """PAF lines of one read. records, query, refseq as sam.sam_lines takes them (refseq clamps its range to the contig, a negative
    start to 0, as vm_sam_emit does); contig_len(contig) -> the contig's length in the index. Raises
    what sam.sam_lines raises for the same arguments (the caller skips the read). hardclip, fakecigar, cigar2cg, rg_id and comments do not exist
    here: they change nothing on a PAF line."""
    recs = reassign_mapq(records) if markunbalancetra else [list(r) for r in records]
    rc_query = revcomp(query)
    recs.sort(key=lambda x: x[4] - x[3])          # stable, then reversed: longest first, later ones first among equals
    recs = recs[::-1]
    qlen = len(query)
    lines = []
    for r in recs:
        ops, nm_asm = merge_cigar_nm(r[8]) if asm else (merge_cigar(r[8]), None)
        text = ''.join(ops)
        t = refseq(r[1], r[5], r[6])
        if not md:
            nm = nm_asm if asm else nm_from_cigar(text, query if r[2] == '+' else rc_query, t)
            tags = ''
        else:
            qa, qb = _clamp(r[3], qlen), _clamp(r[4], qlen)      # (vm_sam_emit's slice: both ends clamped to the read, a negative one to 0)
            q = (query if r[2] == '+' else rc_query)[qa:max(qa, qb)]
            m_, c_ = md_cs(ops, t, q, shortcs)
            nm = nm_asm if asm else nm_from_cigar(text, q, t)
            tags = '\tMD:Z:%s\tcs:Z:%s' % (m_, c_)
        alen = aligned_length(ops)
        qs, qe = (r[3], r[4]) if r[2] == '+' else (qlen - r[4], qlen - r[3])
        mapq = (60 if r[7] != 0 else 1) if asm else r[7]
        cg = ''.join(strip_clips(ops))
        lines.append('%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:P\tNM:i:%d%s%s' % (
            r[0], qlen, qs, qe, r[2], r[1], contig_len(r[1]), r[5], r[6], alen - nm, alen, mapq, nm, '\tcg:Z:' + cg if cg else '', tags))
    return lines
