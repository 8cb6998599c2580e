"""The gap fill's second launch (k_gapfill_redo) on the emulator build, whose constants are small: the small class ends at tl + ql = 160, the
whole-wave class of the redo list starts at 120, and the wave-wide band claims 36 ns of its diagonals (ns = 2 .. 4: 72 .. 144), so that problems
this small reach all three outcomes — kept by the proof, proven outright (g > min(tl, ql)), filled in full after all. The same checks as
test_gpu_redo_wide.py (redo_wide_cases.check), with its sizes scaled down; rows beyond the first 128-row stripe of the packed layout only occur in
problems that fall back here (an oblong problem's one long gap is more than the proof's bound allows)."""
import numpy as np
import pytest
import kernel_cases as KC
import redo_wide_cases as RW
from redo_wide_cases import EMU as SH


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(autouse=True)
def nothing_in_the_first_launch(monkeypatch):
    # the first launch tries no band (its rule asks for a margin no band has): every small problem is on the redo list, those of the class go wide
    monkeypatch.setenv('VMX_AD_PCT', '60000')
    monkeypatch.setenv('VMX_AD_PCT_MIN', '60000')


def clean_refill(rng, L, gap=20, extra=0):
    """tl = L, ql = L + extra; a deletion of `gap` and an insertion of `gap + extra` bases apart, clean flanks: proven in the wide band's 72 diagonals"""
    n = L - gap
    return RW.two_gaps(rng, (n // 3, n // 3, n - 2 * (n // 3)), gap, gap + extra)


def test_emu_redo_wide_kept_and_outright(ctx, oracle):
    rng = np.random.default_rng(811)
    clean = []
    for L in (66, 70, 80):                # (up to 64 x 64 the first launch's widest band proves a problem outright, whatever its rule)
        t, q = clean_refill(rng, L)
        clean.append((t, q, 'clean 20/20 at %d' % L))
    st, flag = RW.check(ctx, oracle, SH, clean)
    assert list(flag) == [1] * 3 and st['redo_wide'] == 3 and st['redo_full'] == 0, (st, list(flag))
    # g > min(tl, ql) in the problem's own band: nothing can leave it
    a = KC.rand_seq(rng, 130)
    outright = [(a[40:50], a, '10 x 130'), (a, a[3:12], '130 x 9')]
    for t, q, _ in outright:
        ns = RW.wide_ns(SH, len(t), len(q))
        assert ns > 0 and RW.geom_nd(len(t), len(q), SH.dpn * ns)[0] > min(len(t), len(q))
    st, flag = RW.check(ctx, oracle, SH, outright)
    assert list(flag) == [1, 1] and st['redo_wide'] == 2, (st, list(flag))
    cases = clean + outright
    for L in (65, 68, 73, 80):
        b = KC.rand_seq(rng, L)
        cases.append((b, RW.noisy(rng, b, L), '10%% at %d' % L))
        for d in (1, 6, 25):
            for sign in (1, -1):
                tl, ql = (L, L + d) if sign > 0 else (L + d, L)
                if tl + ql > SH.x4_max:
                    continue
                t, q = RW.two_gaps(rng, (L // 3 - 5, L // 3 - 5, L - 12 - 2 * (L // 3 - 5)), 12 + (d if sign < 0 else 0), 12 + (d if sign > 0 else 0))
                assert (len(t), len(q)) == (tl, ql)
                cases.append((t, RW.noisy(rng, q, ql), '10%% + gaps, %d x %d' % (tl, ql)))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, cases))
    assert st['redo_wide'] >= 5, st


def test_emu_redo_wide_band_edges(ctx, oracle):
    """two opposite gaps of g - 1, g, g + 1 bases, g = the margin of the band the proof claims"""
    rng = np.random.default_rng(812)
    cases = []
    for tl, ql, ns in ((76, 76, 2), (45, 107, 3)):
        assert RW.wide_ns(SH, tl, ql) == ns
        g = RW.geom_nd(tl, ql, SH.dpn * ns)[0]
        for x in (g - 1, g, g + 1):
            n = tl - x
            for pos, parts in (('start', (2, n // 2, n - 2 - n // 2)), ('middle', (n // 3, n // 3, n - 2 * (n // 3))), ('end', (n - 2 - n // 2, n // 2, 2))):
                for first in 'DI':
                    t, q = RW.two_gaps(rng, parts, x, x + ql - tl, first)
                    assert (len(t), len(q)) == (tl, ql)
                    cases.append((t, q, 'ns %d, gaps of %d, %s, %s first' % (ns, x, pos, first)))
    st, flag = RW.check(ctx, oracle, SH, cases)
    assert int((flag == 1).sum()) == len(cases) and st['redo_wide'] >= 1 and st['redo_full'] >= 1, st


def test_emu_redo_wide_fallback(ctx, oracle):
    rng = np.random.default_rng(813)
    a = KC.rand_seq(rng, 152)
    cases = [('A' * 75, 'C' * 75, 'nothing matches'), (''.join('AC'[i] for i in rng.integers(0, 2, 75)), ''.join('GT'[i] for i in rng.integers(0, 2, 75)), 'unrelated'),
             (a[:8], a, 'oblong 8 x 152'), (a, a[70:78], 'oblong 152 x 8'),                  # no band of 144 diagonals holds both corners
             (a[:140], a[60:75], 'oblong 140 x 15'),                                         # a band holds it; the 125-base gap is more than the bound allows
             (a[:140], a[:8] + a[132:140], 'deletion across row 128')]
    st, flag = RW.check(ctx, oracle, SH, cases)
    assert list(flag) == [1] * 6 and st['redo_full'] == 6 and st['redo_wide'] == 0, (st, list(flag))
    # a scoring outside the tagged range (as test_ad_tags.py: e = 26 over 161 steps): no band anywhere, every problem still right
    more = []
    for L in (66, 70, 80):
        t, q = clean_refill(rng, L)
        more.append((t, q, 'clean 20/20 at %d' % L))
    st, flag = RW.check(ctx, oracle, SH, cases + more, scores=(2, -4, 4, 26, 24, 25))
    assert st['proven'] == 0 and st['redo_wide'] == 0 and st['redo_full'] == 9, st


def test_emu_redo_wide_pairing(ctx, oracle, monkeypatch):
    rng = np.random.default_rng(814)
    refill = []
    for L in (66, 68, 70, 75, 80):
        t, q = clean_refill(rng, L)
        refill.append((t, q, 'clean 20/20 at %d' % L))
    for n in (1, 2, 3, 5):               # an idle Y, an odd tail
        st, flag = RW.check(ctx, oracle, SH, refill[:n])
        assert list(flag) == [1] * n and st['redo_wide'] == n and st['redo_full'] == 0, (n, st)
    # a pair whose members want different widths; a pair of very different lengths
    t3, q3 = clean_refill(rng, 45, gap=10, extra=62)
    pair = [refill[2], (t3, q3, 'ns 3')]
    assert [RW.wide_ns(SH, len(t), len(q)) for t, q, _ in pair] == [2, 3]
    st, flag = RW.check(ctx, oracle, SH, pair)
    assert list(flag) == [1, 1] and st['redo_wide'] >= 1, (st, list(flag))
    b = KC.rand_seq(rng, 79)
    pair = [refill[0], (b, RW.noisy(rng, b, 80, 0.05), '79 x 80')]
    st, flag = RW.check(ctx, oracle, SH, pair)
    assert list(flag) == [1, 1] and st['redo_wide'] == 2, (st, list(flag))
    # with the first launch's rule at its default: among problems it keeps, refilled problems below the whole-wave class (four per wave in the same
    # launch) and one outside the small class
    monkeypatch.delenv('VMX_AD_PCT'); monkeypatch.delenv('VMX_AD_PCT_MIN')
    others = []
    for L in (20, 45, 55):
        for _ in range(5):
            d = KC.rand_seq(rng, L)
            others.append((d, KC.mutate(rng, d, 0.08), 'first launch %d' % L))
    for _ in range(8):
        others.append((''.join('AC'[i] for i in rng.integers(0, 2, 45)), ''.join('GT'[i] for i in rng.integers(0, 2, 50)), 'unrelated, four per wave'))
    others.append((KC.rand_seq(rng, 100), KC.rand_seq(rng, 90), 'packed class'))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, refill + others + pair))
    assert st['proven'] >= 1 and st['redo_wide'] >= len(refill) and int((flag == 0).sum()) >= 9, (st, list(flag))


def test_emu_redo_wide_ties_and_n(ctx, oracle):
    rng = np.random.default_rng(815)
    cases = []
    for unit in (1, 2, 3, 7):
        u = KC.rand_seq(rng, unit)
        a = (u * (78 // unit + 2))[:78]
        cases.append((a, a[6:], 'tandem %d shift' % unit))
        cases.append((a, RW.fit(rng, KC.mutate(rng, a, 0.05), 72), 'tandem %d err' % unit))
    cases += [('A' * 78, 'A' * 72, 'homopolymer'), ('A' * 78, 'A' * 40 + 'C' + 'A' * 37, 'homopolymer, one C'), ('AC' * 39, 'CA' * 36, 'dinucleotide, out of phase')]
    a = list(KC.rand_seq(rng, 76))
    for p0 in (3, 38, 70):
        a[p0:p0 + 3] = 'NNN'
    a = ''.join(a)
    cases += [(a, a, 'N both'), (a, RW.fit(rng, KC.mutate(rng, a, 0.05), 76), 'N both err'), (a.replace('N', 'A'), a, 'N query'), (a, a.replace('N', 'C'), 'N target')]
    for t, q in KC.gapfill_tie_cases(seed=int(rng.integers(1 << 30))):
        pad = max(0, min((SH.x4_max - len(t) - len(q)) // 4, 10))          # flanks as far as the small class allows
        F1, F2 = KC.rand_seq(rng, pad), KC.rand_seq(rng, pad)
        cases.append((F1 + t + F2, F1 + q + F2, 'E2 = F1 tie'))
    st, flag = RW.check(ctx, oracle, SH, RW.shuffled(rng, cases))
    n_pk = sum(1 for t, q, _ in cases if SH.pk(t, q))
    assert int((flag == 1).sum()) == n_pk and n_pk >= 15 and st['redo_wide'] >= 10, (st, n_pk)
