"""Cases and checks for the gap fill's second launch (k_gapfill_redo): the larger problems of the redo list (tl + ql >= VMX_REDO_PK_MIN) go two
per wavefront through a wave-wide anti-diagonal band whose traceback bytes land in the packed two-rows-per-lane layout, and only those whose
band result is not proven are filled in full. Shared by test_redo_wide_emu.py (emulator build: small constants) and test_gpu_redo_wide.py."""
import numpy as np
import kernel_cases as KC

GF_SCORE = (2, -4, 4, 2, 24, 1)
NS_MIN, NS_MAX = 2, 4            # VMX_ADW_NS_MIN, VMX_AD_NS_MAX
PCT, PCT_MIN = 100, 65           # VMX_ADW_PCT, VMX_ADW_PCT_MIN


class Shape:
    """the build's constants: dpn = VMX_ADW_DPN (claimed diagonals of the wide band per unit of ns), pk_min = VMX_REDO_PK's lower bound,
    x4_max = VMX_DP16X4_MAX"""
    def __init__(self, dpn, pk_min, x4_max):
        self.dpn, self.pk_min, self.x4_max = dpn, pk_min, x4_max

    def pk(self, t, q):
        return len(t) > 0 and len(q) > 0 and self.pk_min <= len(t) + len(q) <= self.x4_max


EMU = Shape(36, 120, 160)
GPU = Shape(128, 384, 1024)


def geom_nd(tl, ql, nd):
    """mirror of vmx_ad_geom_nd: (g, dlo)"""
    dl = ql - tl; lo = min(0, dl); hi = max(0, dl)
    slack = nd - (hi - lo + 1)
    if slack < 0:
        return 0, 0
    mb = slack // 2; dlo = lo - mb
    if dlo & 1:
        if mb + 1 <= slack:
            mb += 1; dlo -= 1
        elif mb >= 1:
            mb -= 1; dlo += 1
        else:
            return 0, 0
    return min(mb, slack - mb) + 1, dlo


def wide_ns(sh, tl, ql):
    """mirror of vmx_ad_ns_nd with the second launch's constants: the width a problem asks for (0: no wide attempt)"""
    mn = min(tl, ql); g = 0
    for ns in range(NS_MIN, NS_MAX + 1):
        g, _ = geom_nd(tl, ql, sh.dpn * ns)
        if g >= 1 and (g > mn or KC.ad_margin(g) * 100 >= PCT * mn):
            return ns
    return NS_MAX if (g >= 1 and KC.ad_margin(g) * 100 >= PCT_MIN * mn) else 0


def fit(rng, s, n):
    """s cut or padded with random bases to n"""
    return (s + KC.rand_seq(rng, max(0, n - len(s))))[:n]


def noisy(rng, a, ql, rate=0.10):
    return fit(rng, KC.mutate(rng, a, rate), ql)


def two_gaps(rng, parts, d, i, first='D'):
    """target / query that differ by a deletion of d and an insertion of i bases, `parts` = the lengths of the three shared stretches"""
    P = [KC.rand_seq(rng, n) for n in parts]
    D, I = KC.rand_seq(rng, d), KC.rand_seq(rng, i)
    if first == 'D':
        return P[0] + D + P[1] + P[2], P[0] + P[1] + I + P[2]
    return P[0] + P[1] + D + P[2], P[0] + I + P[1] + P[2]


def check(ctx, O, sh, cases, scores=GF_SCORE):
    """cases: (target, query, label). CIGARs of the batched gap fill == the oracle's == the full-matrix entry's, eqx off and on; the second launch's
    two counters add up to the problems that carry the packed layout's flag. Returns (stats, flags) of the eqx run."""
    ts = [c[0] for c in cases]; qs = [c[1] for c in cases]
    for eqx in (False, True):
        exp = [O.k_cigar_global(t, q, *scores, eqx=eqx)[0] for t, q in zip(ts, qs)]
        cg, flag, st = ctx.k_cigar_batch_banded(ts, qs, *scores, eqx=eqx)
        cg0, _ = ctx.k_cigar_batch(ts, qs, *scores, eqx=eqx)
        for i, (t, q, lab) in enumerate(cases):
            assert cg[i] == exp[i], (lab, len(t), len(q), int(flag[i]), eqx)
            assert cg0[i] == exp[i], (lab, len(t), len(q), 'full-matrix entry', eqx)
            assert int(flag[i]) != 1 or sh.pk(t, q), (lab, len(t), len(q))
        n1 = int((flag == 1).sum())
        assert st['redo_wide'] + st['redo_full'] == n1, (st, n1)
        assert st['proven'] == int((flag > 16).sum()) and st['redo'] >= n1, st
    return st, flag


def shuffled(rng, cases):
    return [cases[i] for i in rng.permutation(len(cases))]
