"""The gap fill's second launch on the GPU (k_gapfill_redo): refilled problems of perimeter >= 384 run two per wavefront in a wave-wide
anti-diagonal band of 256 .. 512 diagonals whose traceback bytes go into the packed layout (128-row stripes); what the proof does not keep is
filled in full. Through vm_k_cigar_batch_banded, eqx off and on, against the oracle's full DP and the full-matrix entry (redo_wide_cases.check)."""
import numpy as np
import pytest
import kernel_cases as KC
import redo_wide_cases as RW
from redo_wide_cases import GPU as SH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)


@pytest.fixture(autouse=True)
def first_launch_rule(monkeypatch):
    # the first launch's band-width rule at its default (90 / 65); tests that want every problem in the second launch pin it below
    monkeypatch.delenv('VMX_AD_PCT', raising=False)
    monkeypatch.delenv('VMX_AD_PCT_MIN', raising=False)


def nothing_in_the_first_launch(monkeypatch):
    monkeypatch.setenv('VMX_AD_PCT', '60000')
    monkeypatch.setenv('VMX_AD_PCT_MIN', '60000')


def clean_refill(rng, L, gap=70, extra=0):
    """tl = L, ql = L + extra; a deletion of `gap` and an insertion of `gap + extra` bases apart: beyond the margin (64 at the most) of the first launch's
    band, whose result is therefore not proven; well inside 256 diagonals, where the proof holds for clean flanks"""
    n = L - gap
    t, q = RW.two_gaps(rng, (n // 3, n // 3, n - 2 * (n // 3)), gap, gap + extra)
    return t, q


def test_gpu_redo_wide_kept(ctx, oracle):
    rng = np.random.default_rng(801)
    clean = []
    for L in (200, 270, 400, 467):
        t, q = clean_refill(rng, L)
        clean.append((t, q, 'clean 70/70 at %d' % L))
    st, flag = RW.check(ctx, oracle, SH, clean)
    assert list(flag) == [1] * len(clean) and st['redo_wide'] == len(clean) and st['redo_full'] == 0, (st, list(flag))
    cases = list(clean)
    for L in (200, 270, 400, 470, 500, 511):
        a = KC.rand_seq(rng, L)
        if L > 467:                      # never tried in the 16-lane band (its widest margin is below 65 % of the problem)
            cases.append((a, RW.noisy(rng, a, L), '10%% at %d' % L))
        else:
            t, q = clean_refill(rng, L)
            cases.append((t, RW.noisy(rng, q, L), '10%% + 70/70 at %d' % L))
    for L in (300, 400):
        for d in (1, 25, 100, 200):
            for sign in (1, -1):
                tl, ql = (L, L + d) if sign > 0 else (L + d, L)
                if tl + ql > SH.x4_max:
                    continue
                t, q = RW.two_gaps(rng, (L // 3 - 23, L // 3 - 23, L - 70 - 2 * (L // 3 - 23)), 70 + (d if sign < 0 else 0), 70 + (d if sign > 0 else 0))
                assert (len(t), len(q)) == (tl, ql)
                cases.append((t, RW.noisy(rng, q, ql), '10%% + gaps, %d x %d' % (tl, ql)))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, cases))
    assert st['redo_wide'] >= len(clean), (st, list(flag))


def test_gpu_redo_wide_stripe_edges(ctx, oracle, monkeypatch):
    """rows around the 128-row stripes of the packed layout, and gaps that cross a stripe's last row"""
    rng = np.random.default_rng(802)
    cases = []
    for tl in (127, 128, 129, 255, 256, 257, 383, 384, 385):
        a = KC.rand_seq(rng, tl)
        for ql in (tl - 3, tl + 3):
            cases.append((a, RW.noisy(rng, a, ql), 'stripe %d x %d' % (tl, ql)))
        ql = min(2 * tl, SH.x4_max - tl)
        cases.append((a, RW.noisy(rng, a[:tl // 2] + KC.rand_seq(rng, ql - tl) + a[tl // 2:], ql, 0.02), 'stripe %d x %d' % (tl, ql)))
    a = KC.rand_seq(rng, 400)
    cross = [(a, a[:100] + a[160:], 'deletion across row 128'), (a, a[:230] + a[290:], 'deletion across row 256'),
             (a, a[:100] + a[170:300] + KC.rand_seq(rng, 70) + a[300:], 'deletion across row 128, insertion later')]
    # the first two are not tried in the first launch (a margin of 34 beside the 60 diagonals between the corners), the third leaves its margin of 64
    # and is not proven there; all three are proven in 256 diagonals
    st, flag = RW.check(ctx, oracle, SH, cross)
    assert list(flag) == [1, 1, 1] and st['redo_wide'] == 3, (st, list(flag))
    nothing_in_the_first_launch(monkeypatch)
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, cases + cross))
    assert st['redo_wide'] >= 10, st


def test_gpu_redo_wide_band_edges(ctx, oracle):
    """two opposite gaps of g - 1, g, g + 1 bases, g = the wide band's margin: with clean flanks the path of g - 1 is proven, the others fall back"""
    rng = np.random.default_rng(803)
    cases = []
    for tl, ql, ns in ((500, 500, 2), (400, 500, 3)):
        assert RW.wide_ns(SH, tl, ql) == ns
        g = RW.geom_nd(tl, ql, SH.dpn * ns)[0]
        for x in (g - 1, g, g + 1):
            n = tl - x
            for pos, parts in (('start', (3, n // 2, n - 3 - n // 2)), ('middle', (n // 3, n // 3, n - 2 * (n // 3))), ('end', (n - 3 - n // 2, n // 2, 3))):
                for first in 'DI':
                    t, q = RW.two_gaps(rng, parts, x, x + ql - tl, first)
                    assert (len(t), len(q)) == (tl, ql)
                    cases.append((t, q, 'ns %d, gaps of %d, %s, %s first' % (ns, x, pos, first)))
    st, flag = RW.check(ctx, oracle, SH, cases)
    assert int((flag == 1).sum()) == len(cases) and st['redo_wide'] >= 1 and st['redo_full'] >= 1, st


def test_gpu_redo_wide_fallback(ctx, oracle):
    rng = np.random.default_rng(804)
    a = KC.rand_seq(rng, 900)
    cases = [(KC.rand_seq(rng, 300), KC.rand_seq(rng, 300), 'unrelated') for _ in range(3)]
    cases += [(a[:60], a, 'oblong 60 x 900'), (a, a[400:460], 'oblong 900 x 60')]            # no band of 512 diagonals holds both corners
    st, flag = RW.check(ctx, oracle, SH, cases)
    assert list(flag) == [1] * 5 and st['redo_full'] == 5 and st['redo_wide'] == 0, (st, list(flag))
    # a scoring outside the tagged range (vmx_ad_scores_ok: bias 4096 + 1025 * 3 + 24, highest value 2 * 513): no band anywhere, every problem still right
    more = []
    for L in (200, 270, 400):
        t, q = clean_refill(rng, L)
        more.append((t, q, 'clean 70/70 at %d' % L))
    st, flag = RW.check(ctx, oracle, SH, cases + more, scores=(2, -4, 4, 3, 24, 2))
    assert st['proven'] == 0 and st['redo_wide'] == 0 and st['redo_full'] == 8, st


def test_gpu_redo_wide_pairing(ctx, oracle):
    rng = np.random.default_rng(805)
    refill = []
    for L in (270, 300, 330, 400, 450):
        t, q = clean_refill(rng, L)
        refill.append((t, q, 'clean 70/70 at %d' % L))
    for n in (1, 2, 3, 5):               # an idle Y, an odd tail
        st, flag = RW.check(ctx, oracle, SH, refill[:n])
        assert list(flag) == [1] * n and st['redo_wide'] == n and st['redo_full'] == 0, (n, st)
    # a pair whose members want different widths: both run in the wider one
    a = KC.rand_seq(rng, 500)
    t3, q3 = clean_refill(rng, 400, gap=70, extra=100)
    pair = [(a, RW.noisy(rng, a, 500), 'ns 2'), (t3, q3, 'ns 3')]
    assert [RW.wide_ns(SH, len(t), len(q)) for t, q, _ in pair] == [2, 3]
    st, flag = RW.check(ctx, oracle, SH, pair)
    assert list(flag) == [1, 1], list(flag)
    # very different lengths: the short one idles through most of the long one's steps
    ts, qs = clean_refill(rng, 190, gap=70, extra=10)
    b = KC.rand_seq(rng, 505)
    pair = [(ts, qs, '190 x 200'), (b, RW.noisy(rng, b, 510), '505 x 510')]
    st, flag = RW.check(ctx, oracle, SH, pair)
    assert list(flag) == [1, 1] and st['redo_wide'] >= 1, (st, list(flag))
    # proven outright: in its partner's 512 diagonals nothing can leave the band of the 11-base problem (g > min(tl, ql))
    c = KC.rand_seq(rng, 600)
    pair = [(c[:11], c[:373], '11 x 373'), (c[:150] + c[450:], c, '300 x 600')]
    assert [RW.wide_ns(SH, len(t), len(q)) for t, q, _ in pair] == [3, 4] and RW.geom_nd(11, 373, SH.dpn * 4)[0] > 11
    st, flag = RW.check(ctx, oracle, SH, pair)
    assert list(flag) == [1, 1] and st['redo_wide'] >= 1, (st, list(flag))
    # among problems the first launch keeps and refilled problems below the whole-wave class
    others = []
    for L in (60, 150, 270):
        for _ in range(6):
            d = KC.rand_seq(rng, L)
            others.append((d, KC.mutate(rng, d, 0.08), 'first launch %d' % L))
    for _ in range(8):
        others.append((KC.rand_seq(rng, 150), KC.rand_seq(rng, 170), 'unrelated, four per wave'))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, refill + others + pair))
    assert st['proven'] >= 1 and st['redo_wide'] >= len(refill) and int((flag == 0).sum()) >= 8, (st, list(flag))


def test_gpu_redo_wide_ties_and_n(ctx, oracle, monkeypatch):
    nothing_in_the_first_launch(monkeypatch)           # clean repeats would be kept by the first launch: here the wide band's bytes are what the walk reads
    rng = np.random.default_rng(806)
    cases = []
    for unit in (1, 2, 3, 7):
        u = KC.rand_seq(rng, unit)
        a = (u * (300 // unit + 2))[:300]
        cases.append((a, a[6:], 'tandem %d shift' % unit))
        cases.append((a, RW.fit(rng, KC.mutate(rng, a, 0.05), 294), 'tandem %d err' % unit))
    cases += [('A' * 300, 'A' * 294, 'homopolymer'), ('A' * 300, 'A' * 150 + 'C' + 'A' * 149, 'homopolymer, one C'), ('AC' * 150, 'CA' * 147, 'dinucleotide, out of phase')]
    a = list(KC.rand_seq(rng, 300))
    for p0 in (3, 150, 294):
        a[p0:p0 + 3] = 'NNN'
    a = ''.join(a)
    cases += [(a, a, 'N both'), (a, KC.mutate(rng, a, 0.05), 'N both err'), (a.replace('N', 'A'), a, 'N query'), (a, a.replace('N', 'C'), 'N target')]
    F1, F2 = KC.rand_seq(rng, 200), KC.rand_seq(rng, 200)
    for t, q in KC.gapfill_tie_cases(seed=int(rng.integers(1 << 30))):
        cases.append((F1 + t + F2, F1 + q + F2, 'E2 = F1 tie in flanks'))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, cases))
    cases = [c for c in cases if SH.pk(c[0], c[1])]      # (the largest tie case in its flanks is past the small class)
    assert st['proven'] == 0 and int((flag == 1).sum()) == len(cases) and st['redo_wide'] >= len(cases) // 2, st
