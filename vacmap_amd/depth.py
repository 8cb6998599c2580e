"""Per-window depth of coverage from the records of vm_align_batch: the Python statement of the rule that vm_depth_add and vm_depth_add_device
implement (include/vacmapx.h states it once, at vm_depth_add). A sibling of paf.py: a record counts exactly where `sam.sam_lines` makes a record
line for it and that line's MAPQ column is at least the threshold; every reference position under an M, = or X of its CIGAR counts 1, positions
under D and N count 0, and `counts[w]` sums the counted (record, position) pairs inside window w. Pure Python and integers only; no GPU involved."""
from .paf import paf_lines
from .sam import merge_cigar, reassign_mapq


def window_offsets(lens, window):
    """win_off[nseq + 1]: contig c has ceil(L_c / window) windows, concatenated in index order"""
    off = [0]
    for L in lens:
        off.append(off[-1] + (L + window - 1) // window)
    return off


def counts(records, query, refseq, contig_len, window, min_mapq=0, md=False, shortcs=True, markunbalancetra=True, asm=False):
    """{(contig name, window number inside the contig): counted positions} of one read. records, query, refseq, contig_len and the options as
    paf.paf_lines takes them; raises what sam.sam_lines raises for the same arguments (the caller skips the read: it contributes nothing)."""
    paf_lines(records, query, refseq, contig_len, md=md, shortcs=shortcs, markunbalancetra=markunbalancetra, asm=asm)      # the emitter's raises, by construction
    recs = reassign_mapq(records) if markunbalancetra else [list(r) for r in records]
    out = {}
    for r in recs:
        mapq = (60 if r[7] != 0 else 1) if asm else r[7]
        if mapq < min_mapq:
            continue
        L = contig_len(r[1])
        ops = merge_cigar(r[8])
        pos = r[5]
        for i in range(1, len(ops), 2):
            n, op = int(ops[i - 1]), ops[i]
            if op in 'M=X':
                a, b = max(pos, 0), min(pos + n, L)
                while a < b:                               # split at the window boundaries
                    w = a // window
                    stop = min(b, (w + 1) * window)
                    out[(r[1], w)] = out.get((r[1], w), 0) + stop - a
                    a = stop
            if op in 'M=XDN':
                pos += n
    return out


def flat(names, lens, window, per_read):
    """the table counts[n_windows] from the dictionaries `counts` returned for any number of reads"""
    off = window_offsets(lens, window)
    at = {n: off[i] for i, n in enumerate(names)}
    table = [0] * off[-1]
    for d in per_read:
        for (name, w), v in d.items():
            table[at[name] + w] += v
    return table


def mean_text(count, length):
    """two decimals, half up, from integers: h = (200 count + length) div (2 length) hundredths (0 for an empty range)"""
    h = (200 * count + length) // (2 * length) if length else 0
    return '%d.%02d' % (h // 100, h % 100)


def regions_text(names, lens, window, table):
    """one line per window, empty ones included: TNAME start end mean"""
    off = window_offsets(lens, window)
    out = []
    for c, (name, L) in enumerate(zip(names, lens)):
        for w in range(off[c], off[c + 1]):
            start = (w - off[c]) * window
            end = min(start + window, L)
            out.append('%s\t%d\t%d\t%s\n' % (name, start, end, mean_text(table[w], end - start)))
    return ''.join(out)


def summary_text(names, lens, window, table):
    """one line per contig, TNAME length bases mean, and a last line `total`"""
    off = window_offsets(lens, window)
    out = []; total = 0
    for c, (name, L) in enumerate(zip(names, lens)):
        bases = sum(table[off[c]:off[c + 1]])
        total += bases
        out.append('%s\t%d\t%d\t%s\n' % (name, L, bases, mean_text(bases, L)))
    out.append('total\t%d\t%d\t%s\n' % (sum(lens), total, mean_text(total, sum(lens))))
    return ''.join(out)
