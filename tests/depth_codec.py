"""An independent check of the depth of coverage: from the SAM lines an emitter returned (RNAME, POS, MAPQ and CIGAR columns only) a brute-force
per-base numpy array per contig, the window sums taken from it, and the two texts. Shares no code with vacmap_amd/depth.py (the mean is taken with
fractions here). Not for lines made under cigar2cg, whose CIGAR column is a placeholder."""
import re
from fractions import Fraction
import numpy as np

_OP = re.compile(r'(\d+)([MIDNSHP=X])')


def per_base(sam_text, names, lens, min_mapq=0):
    """one int64 array per contig: how many record lines with MAPQ >= min_mapq cover each base with an M, = or X column"""
    cov = {n: np.zeros(L, np.int64) for n, L in zip(names, lens)}
    n_lines = 0
    for line in sam_text.split('\n'):
        if not line or line.startswith('@'):
            continue
        f = line.split('\t')
        if int(f[1]) & 4:                                   # an unmapped line counts nothing
            continue
        n_lines += 1
        if int(f[4]) < min_mapq:
            continue
        a = cov[f[2]]
        pos = int(f[3]) - 1
        assert f[5] != '*' and ''.join(n + o for n, o in _OP.findall(f[5])) == f[5], f[5][:80]
        for n, op in _OP.findall(f[5]):
            n = int(n)
            if op in 'M=X':
                lo, hi = max(pos, 0), min(pos + n, len(a))
                if lo < hi:
                    a[lo:hi] += 1
            if op in 'M=XDN':
                pos += n
    return [cov[n] for n in names], n_lines


def window_sums(arrays, window):
    """(counts over all windows, win_off) of per-base arrays"""
    parts, off = [], [0]
    for a in arrays:
        nw = -(-len(a) // window)
        padded = np.zeros(nw * window, np.int64); padded[:len(a)] = a
        parts.append(padded.reshape(nw, window).sum(axis=1) if nw else np.zeros(0, np.int64))
        off.append(off[-1] + nw)
    return (np.concatenate(parts) if parts else np.zeros(0, np.int64)), off


def _mean(count, length):
    if length == 0:
        return '0.00'
    h = int((Fraction(100 * int(count), int(length)) + Fraction(1, 2)) // 1)     # hundredths, half up
    return str(h // 100) + '.' + str(h % 100).rjust(2, '0')


def regions(names, arrays, window):
    out = []
    for name, a in zip(names, arrays):
        for s in range(0, len(a), window):
            e = min(s + window, len(a))
            out.append('\t'.join([name, str(s), str(e), _mean(a[s:e].sum(), e - s)]) + '\n')
    return ''.join(out).encode()


def summary(names, arrays):
    out = []
    for name, a in zip(names, arrays):
        out.append('\t'.join([name, str(len(a)), str(int(a.sum())), _mean(a.sum(), len(a))]) + '\n')
    tot = sum(int(a.sum()) for a in arrays); L = sum(len(a) for a in arrays)
    out.append('\t'.join(['total', str(L), str(tot), _mean(tot, L)]) + '\n')
    return ''.join(out).encode()


def expected(sam_text, names, lens, window, min_mapq=0):
    """(counts list, win_off list, regions bytes, summary bytes, record lines seen) from SAM text"""
    arrays, n_lines = per_base(sam_text, names, lens, min_mapq)
    counts, off = window_sums(arrays, window)
    return counts.tolist(), off, regions(names, arrays, window), summary(names, arrays), n_lines
