"""Shared checks: the HIP entries (real library on a GPU, or its emulator build in CPU tests) against the spec references of spec_ref.py,
at the shapes, parameters and edges where the kernels switch layouts or tie-break. `ctx` is a vacmap_amd.lib.Context."""
import numpy as np
import pytest
import spec_ref as R
from kernel_cases import rand_seq, mutate

GAP_SCORES = [(2, -4, 4, 2, 24, 1), (1, -3, 3, 2, 12, 1)]                  # (match, mismatch, o1, e1, o2, e2); the product's first
EXT_SCORES = [(2, -4, 4, 4), (1, -3, 2, 1), (3, -2, 6, 2)]                 # (match, mismatch, o, e); the product's first


def _iupac(rng, s, n=3):
    s = list(s)
    for _ in range(n):
        if s:
            s[int(rng.integers(0, len(s)))] = 'NRYKMSWn'[int(rng.integers(0, 8))]
    return ''.join(s)


# ------------------------------------------------------------------------------------------------ VMX-ED
def edit_distance_pairs(rng, lens):
    qs, ts = [], []
    for L in lens:
        a = rand_seq(rng, L)
        for b in (mutate(rng, a, 0.03), mutate(rng, a, 0.25), rand_seq(rng, max(L + int(rng.integers(-3, 4)), 0))):
            qs += [a, b]; ts += [b, a]                                      # both argument orders
        qs.append(_iupac(rng, a).lower()); ts.append(_iupac(rng, a))      # lower case, N and IUPAC codes (one code, case ignored)
    qs += ['', 'A', '', 'N', 'n', 'ACGT']; ts += ['', '', 'ACGT', 'N', 'R', 'acgt']
    return qs, ts


def check_edit_distance(ctx, lens, seed):
    qs, ts = edit_distance_pairs(np.random.default_rng(seed), lens)
    got = ctx.edit_distance_batch(qs, ts).tolist()
    exp = [R.levenshtein(q, t) for q, t in zip(qs, ts)]
    bad = [(len(q), len(t), g, e) for q, t, g, e in zip(qs, ts, got, exp) if g != e]
    assert not bad, bad[:5]


def check_edit_distance_bound(ctx, lens, seed, tier):
    """the banded bound is EXACT on near-diagonal pairs (the optimal path stays inside its band) and never below the distance"""
    rng = np.random.default_rng(seed)
    qs, ts, exact = [], [], []
    for L in lens:
        a = rand_seq(rng, L)
        for rate in (0.0, 0.05, 0.15):
            b = mutate(rng, a, rate)
            qs += [a, b]; ts += [b, a]; exact += [True, True]
        b = _iupac(rng, a, 5)
        qs += [a.lower(), b]; ts += [b, a]; exact += [True, True]
        qs.append(rand_seq(rng, L)); ts.append(rand_seq(rng, L)); exact.append(False)
    qs += ['', 'ACGTN']; ts += ['ACGT', '']; exact += [True, True]
    got = ctx.edit_distance_bound_batch(qs, ts, tier=tier).tolist()
    for q, t, ex, g in zip(qs, ts, exact, got):
        e = R.levenshtein(q, t)
        assert (g == e) if ex else (g >= e), (len(q), len(t), tier, g, e)


# ------------------------------------------------------------------------------------------------ VMX-DP-G
def gapfill_pairs(rng, totals, base=(40, 150)):
    """(target, query) pairs: every tl + ql in `totals` (layout thresholds +-1) in a square and an oblong shape, random sizes, long gaps
    (second affine piece), N on both sides, lower case, tandem repeats (many co-optimal paths)"""
    out = []
    for tot in totals:
        for tl in (tot // 2, tot // 3):
            ql = tot - tl
            a = rand_seq(rng, tl)
            b = (mutate(rng, a, 0.08) + rand_seq(rng, ql))[:ql]
            out.append((a, b))
    for _ in range(6):
        a = rand_seq(rng, int(rng.integers(*base)))
        out.append((a, mutate(rng, a, float(rng.choice([0.02, 0.1, 0.3]))) or 'A'))
    a = rand_seq(rng, base[1])
    out += [(a, a[:20] + a[60:]), (a[:20] + a[60:], a), (a, a[:30] + rand_seq(rng, 35) + a[30:])]
    out += [(_iupac(rng, a, 6), _iupac(rng, a, 6)), (a.lower(), _iupac(rng, a)), ('ACGT' * 12, 'ACGT' * 10 + 'AC'), ('A' * 30, 'A' * 25)]
    out += [('', 'ACG'), ('ACGTA', ''), ('A', 'A'), ('N', 'N'), ('A', 'C')]
    return out


def check_gapfill(ctx, pairs, scores=GAP_SCORES[0], banded=True, ksw2_cells=2500):
    """k_cigar_batch (and the batched path's banded schedule): score = the optimum, each CIGAR rescores to it, '='/'X' are right, and on
    problems small enough for the cell-by-cell DP the CIGAR is the one of ksw2's published tie order"""
    ts = [t for t, _ in pairs]; qs = [q for _, q in pairs]
    exp = [R.dpg_score(t, q, *scores) for t, q in pairs]
    small = [len(t) * len(q) <= ksw2_cells for t, q in pairs]
    ref = [R.ksw2_order_cigar(t, q, *scores)[0] if sm else None for (t, q), sm in zip(pairs, small)]
    for eqx in (False, True):
        forms = [ctx.k_cigar_batch(ts, qs, *scores, eqx=eqx)[0]]
        sc = ctx.k_cigar_batch(ts, qs, *scores, eqx=eqx)[1].tolist()
        assert sc == exp, [(len(t), len(q), g, e) for t, q, g, e in zip(ts, qs, sc, exp) if g != e][:5]
        if banded:
            forms.append(ctx.k_cigar_batch_banded(ts, qs, *scores, eqx=eqx)[0])
        for cg in forms:
            for c, t, q, e, r in zip(cg, ts, qs, exp, ref):
                assert R.cigar_score(c, t, q, *scores) == e, (len(t), len(q), c)
                assert ('M' not in c) if eqx else ('=' not in c and 'X' not in c), c
                if r is not None:
                    plain = ''.join('%d%s' % (L, 'M' if op in '=X' else op) for L, op in R.parse_cigar(c))
                    merged = R.parse_cigar(plain); runs = []
                    for L, op in merged:
                        if runs and runs[-1][1] == op:
                            runs[-1][0] += L
                        else:
                            runs.append([L, op])
                    assert ''.join('%d%s' % (L, op) for L, op in runs) == r, (t, q, c, r)


# ------------------------------------------------------------------------------------------------ VMX-DP-X
def extend_random(rng, n, maxlen):
    out = []
    for i in range(n):
        a = rand_seq(rng, int(rng.integers(1, maxlen)))
        b = mutate(rng, a, float(rng.choice([0.0, 0.05, 0.15, 0.3])))
        cut = int(rng.integers(0, len(b) + 1))
        out.append((a, b[:cut] + rand_seq(rng, int(rng.integers(0, 60)))))
    return out + [('', 'ACGT'), ('ACGT', ''), ('', ''), ('NNNN', 'NNNN'), ('ACNGT', 'ACNGT'), ('acgtac', 'ACGTAC')]


def zdrop_threshold(t, q, p, bw):
    """smallest zdrop at which the extension crosses the valley of (t, q): at z0 - 1 it stops before it (None if the answer never changes)"""
    lo_r, hi_r = R.dpx(t, q, *p, bw, 0), R.dpx(t, q, *p, bw, 10 ** 6)
    if lo_r == hi_r:
        return None
    lo, hi = 0, 10 ** 6
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if R.dpx(t, q, *p, bw, mid) == hi_r:
            hi = mid
        else:
            lo = mid
    return hi


def extend_constructed(rng, p, L=60):
    """(t, q, bw, zdrop, tag) problems built at the rule boundaries of VMX-DP-X for the score set p"""
    out = []
    P, S = rand_seq(rng, L), rand_seq(rng, L)
    for g in (5, 40, 120):                                  # one deletion of g bases: the path runs g off the main diagonal
        X = rand_seq(rng, g)
        for bw in (g, g - 1):                               # exactly on the band edge, and one beyond it
            out.append((P + X + S, P + S, bw, 10 ** 6, 'del %d bw %d' % (g, bw)))
            out.append((P + S, P + X + S, bw, 10 ** 6, 'ins %d bw %d' % (g, bw)))
    # a valley between two matching stretches: a drop of exactly zdrop is crossed, zdrop + 1 ... is not
    for vlen in (3, 8, 20):
        t = P + rand_seq(rng, vlen) + S; q = P + rand_seq(rng, vlen) + S
        for bw in (100, 1):
            z0 = zdrop_threshold(t, q, p, bw)
            if z0 is not None:
                out += [(t, q, bw, z0, 'valley %d z0' % vlen), (t, q, bw, z0 - 1, 'valley %d z0-1' % vlen)]
    # equal best scores on two diagonals (the earlier one stays) and, by symmetry, within one diagonal (the smaller i stays)
    out.append((P + 'AGG', P + 'CGG', 100, 10 ** 6, 'tie across diagonals'))
    for m in (4, 6, 9):                                     # (AC)^m against (CA)^m: a deletion and an insertion reach the same score
        u, v = P[:20] + 'AC' * m, P[:20] + 'CA' * m          # on the same diagonal, (i, i - 1) and (i - 1, i)
        for bw in (100, 2):
            a, b = R.dpx(u, v, *p, bw, 10 ** 6), R.dpx(v, u, *p, bw, 10 ** 6)
            if (a[1], a[2]) != (b[2], b[1]):                 # transposing reverses the i order on each diagonal: a tie inside one
                out += [(u, v, bw, 10 ** 6, 'tie in a diagonal'), (v, u, bw, 10 ** 6, 'tie in a diagonal (t)')]
    # longer than the 512-entry ring (rows wrap), diagonals wider than 64 cells, N on either side
    a = rand_seq(rng, 700)
    out += [(a, mutate(rng, a, 0.05), 100, 50, 'ring wrap'), (a, mutate(rng, a, 0.05), 300, 10 ** 6, 'wide diagonals')]
    out += [(_iupac(rng, a[:200], 8), a[:200], 100, 50, 'N in t'), (a[:200], _iupac(rng, a[:200], 8), 100, 50, 'N in q')]
    return out


def check_extend(ctx, pairs, p, bw, zdrop):
    ts = [t for t, _ in pairs]; qs = [q for _, q in pairs]
    sc, te, qe = ctx.k_extend_batch(ts, qs, *p, bw, zdrop)
    for i, (t, q) in enumerate(pairs):
        assert (int(sc[i]), int(te[i]), int(qe[i])) == R.dpx(t, q, *p, bw, zdrop), (len(t), len(q), p, bw, zdrop)


def check_extend_constructed(ctx, seed, min_ties=3):
    rng = np.random.default_rng(seed)
    n_tie = 0
    for p in EXT_SCORES:
        cases = extend_constructed(rng, p)
        n_tie += sum(1 for c in cases if c[4].startswith('tie in'))
        assert any(c[4].endswith('z0') for c in cases), p
        for t, q, bw, zd, tag in cases:
            sc, te, qe = ctx.k_extend_batch([t], [q], *p, bw, zd)
            assert (int(sc[0]), int(te[0]), int(qe[0])) == R.dpx(t, q, *p, bw, zd), (tag, p, bw, zd)
    assert n_tie >= min_ties


def check_extend_no_band(ctx, seed):
    """bw < 0 is no band: exact where a diagonal fits the kernel (a side of <= 496 bases, the other side any length), refused otherwise —
    never the answer of some other band (the issue's case: 1500 bases against the same with 520 inserted after base 50)"""
    from vacmap_amd.lib import VmxError
    rng = np.random.default_rng(seed)
    a = rand_seq(rng, 1500)
    pairs = [(a[:300], a[:50] + rand_seq(rng, 520) + a[50:300]), (a[:50] + rand_seq(rng, 700) + a[50:400], a[:400]), (a[:496], mutate(rng, a[:496], 0.05)),
             (a[:120], a[:120])]
    for p in EXT_SCORES[:2]:
        check_extend(ctx, pairs, p, -1, 10 ** 6)
        check_extend(ctx, pairs, p, -1, 50)
    t, q = a, a[:50] + rand_seq(rng, 520) + a[50:]
    assert R.dpx(t, q, 2, -4, 4, 4, -1, 10 ** 6) == R.dpx(t, q, 2, -4, 4, 4, 10 ** 6, 10 ** 6) != R.dpx(t, q, 2, -4, 4, 4, 496, 10 ** 6)
    for args in (([t], [q]), ([a[:100], t], [a[:100], q]), ([a[:497]], [a[:497]])):
        with pytest.raises(VmxError) as ei:
            ctx.k_extend_batch(*args, 2, -4, 4, 4, -1, 10 ** 6)
        assert ei.value.code == -7
    with pytest.raises(VmxError) as ei:
        ctx.k_cigar(t, q, 2, -4, 4, 4, 4, 4, bw=-1, zdropvalue=10 ** 6)
    assert ei.value.code == -7
    _, _, q_e, t_e, _, _ = ctx.k_cigar(a[:300], pairs[0][1], 2, -4, 4, 4, 4, 4, bw=-1, zdropvalue=10 ** 6)
    assert (t_e, q_e) == R.dpx(a[:300], pairs[0][1], 2, -4, 4, 4, -1, 10 ** 6)[1:]


# ------------------------------------------------------------------------------------------------ VMX-S1
def sketch_seqs(rng, k, w, long_len=5000):
    """shorter than k, shorter than k + w - 1, N runs, lower case, homopolymers and tandem repeats (ties everywhere), one spanning several tiles"""
    out = [rand_seq(rng, max(k - 1, 0)), rand_seq(rng, k), rand_seq(rng, k + max(w - 2, 0)), rand_seq(rng, k + w - 1), rand_seq(rng, k + w + 5)]
    a = rand_seq(rng, 400)
    out += [a[:100] + 'N' * 40 + a[100:200] + 'n' + a[200:], a.lower(), 'A' * 300, 'T' * 150 + 'A' * 150, 'AT' * 150, 'ACGT' * 80, ('ACG' * 90)[:260]]
    out.append(rand_seq(rng, long_len))
    return out


def check_sketch(ctx, k, w, seqs):
    got = ctx.sketch_batch(k, w, seqs)
    for s, (h, p, z) in zip(seqs, got):
        eh, ep, ez = R.sketch(s, k, w)
        assert np.array_equal(h, eh) and np.array_equal(p, ep) and np.array_equal(z, ez), (k, w, len(s), s[:20])


def check_index(ctx, k, w, contigs):
    from vacmap_amd.lib import Index
    gi = Index.from_seqs(ctx, ['c%d' % i for i in range(len(contigs))], contigs, k=k, w=w)
    h, p = gi.minimizers()
    eh, ep = R.index_minimizers(contigs, k, w)
    gi.close()
    assert np.array_equal(h, eh) and np.array_equal(p, ep), (k, w, len(h), len(eh))
