"""The anti-diagonal band fill in its tagged score domain (vmx_dp_ad.h: 8 * (score + bias) + tag per unsigned 16-bit half, the winner of
each max carrying its traceback code): tie-heavy problems (homopolymers, tandem repeats, gap lengths at which the two affine pieces cost
the same, E2 = F1 ties), problems at the small class's tl + ql limit, and every gap-fill scoring, through vm_k_cigar_batch_banded (the
batched path's gap-fill chunk) against the oracle's full DP: identical CIGARs, and each CIGAR rescores to the oracle's score. A scoring
outside the tagged range (vmx_ad_scores_ok) must send every problem to the second launch and still give the same CIGARs."""
import numpy as np
import pytest
import kernel_cases as KC
import spec_cases as SC
import spec_ref as R

GF_SCORE = (2, -4, 4, 2, 24, 1)          # the product's gap-fill scoring (vmx_stage_extend.hip: gf_score, every mode)


def _cross_len(o1, e1, o2, e2):
    """gap length at which the two affine pieces cost the same (o1 + e1 L = o2 + e2 L), or None"""
    if e1 == e2 or (o2 - o1) % (e1 - e2):
        return None
    L = (o2 - o1) // (e1 - e2)
    return L if L > 0 else None


def tag_cases(rng, limit, scores):
    """(target, query, label) pairs whose DP is full of exact ties, plus problems with tl + ql at `limit` (the small class's bound)"""
    o1, e1, o2, e2 = scores[2:]
    out = []
    rs = lambda n: KC.rand_seq(rng, n)
    # homopolymers and tandem repeats: every gap position in a run scores the same
    for unit in ('A', 'AC', 'ACG', 'AACG'):
        for n1, n2 in ((40, 34), (33, 41), (50, 47)):
            out.append(((unit * 60)[:n1], (unit * 60)[:n2], 'repeat %s %d/%d' % (unit, n1, n2)))
            P = rs(12)
            out.append((P + (unit * 30)[:n1] + P, P + (unit * 30)[:n2] + rs(3) + P, 'flanked repeat %s' % unit))
    # gaps at, below and above the length where the two pieces tie (E1 = E2, F1 = F2)
    L0 = _cross_len(o1, e1, o2, e2)
    for L in sorted({x for x in ((L0 - 1, L0, L0 + 1) if L0 else ()) + (1, 2, 5) if x > 0}):
        a = rs(30) + rs(L) + rs(30)
        b = a[:30] + a[30 + L:]
        out.append((a, b, 'deletion %d' % L))
        out.append((b, a, 'insertion %d' % L))
        out.append((a.replace('G', 'A'), b.replace('G', 'A'), 'deletion %d, 3 letters' % L))
    # deletion next to an insertion of another alphabet: E2 = F1 ties (ksw2 takes F1)
    out += [(t, q, 'E2=F1 tie') for t, q in KC.gapfill_tie_cases(seed=int(rng.integers(1 << 30)))[:12]]
    # mismatch against gap pairs: a substitution costs the same as one base deleted and one inserted when match - mismatch = 2 (o1 + e1)
    for i in range(4):
        a = rs(45)
        b = a[:20] + ('T' if a[20] != 'T' else 'G') + a[21:]
        out.append((a, b, 'one substitution %d' % i))
    # the small class's tl + ql limit (and one over), square and oblong
    for tot in (limit - 1, limit, limit + 1):
        for tl in (tot // 2, tot // 2 - 3, (2 * tot) // 5):
            ql = tot - tl
            a = rs(tl)
            b = (KC.mutate(rng, a, 0.02) + rs(ql))[:ql]
            out.append((a, b, 'limit %d (%d + %d)' % (tot, tl, ql)))
        h = ('A' * tot)[:tot // 2]
        out.append((h, h[:tot - len(h)], 'homopolymer limit %d' % tot))
    return out


def check_tags(ctx, O, limit, scores, seed, expect_band=True):
    """expect_band: some problems are proven in a band, among them one at the limit; else none is tried in a band at all"""
    rng = np.random.default_rng(seed)
    cases = tag_cases(rng, limit, scores)
    perm = rng.permutation(len(cases))
    cases = [cases[i] for i in perm]
    ts = [t for t, _, _ in cases]; qs = [q for _, q, _ in cases]
    for eqx in (False, True):
        exp = [O.k_cigar_global(t, q, *scores, eqx=eqx) for t, q in zip(ts, qs)]
        cg, flag, st = ctx.k_cigar_batch_banded(ts, qs, *scores, eqx=eqx)
        for i, (t, q, lab) in enumerate(cases):
            assert cg[i] == exp[i][0], (lab, len(t), len(q), int(flag[i]), eqx)
            assert R.cigar_score(cg[i], t, q, *scores) == exp[i][1], (lab, cg[i])
        small = [len(t) + len(q) <= limit for t, q in zip(ts, qs)]
        if expect_band:
            assert st['proven'] > 0, st
            # both sides of the limit were present and the ones at the limit ran in a band
            assert any(f > 16 and len(t) + len(q) == limit for f, t, q in zip(flag, ts, qs)), st
        else:
            assert int((flag > 16).sum()) == 0 and st['proven'] == 0 and st['redo'] == sum(small), st
    return st


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def gpu():
    from vacmap_amd.lib import Context
    return Context(0)


EMU_LIMIT = 160       # VMX_DP16X4_MAX of the emulator build
GPU_LIMIT = 1024      # VMX_DP16X4_MAX of the product build


@pytest.mark.parametrize('scores', [GF_SCORE] + [s for s in SC.GAP_SCORES if s != GF_SCORE])
def test_emu_ad_tags(emu, oracle, monkeypatch, scores):
    # wide bands (VMX_AD_PCT=330) on problems this small: nearly every one is proven, so the band's bytes are what the walk reads
    monkeypatch.setenv('VMX_AD_PCT', '330')
    check_tags(emu, oracle, EMU_LIMIT, scores, seed=71)


def test_emu_ad_scores_out_of_range(emu, oracle):
    """-infinity loses e per step: with e = 26 over 161 steps the bias alone passes 8191, the tagged halves cannot hold the values and every
    small problem goes to the second launch"""
    check_tags(emu, oracle, EMU_LIMIT, (2, -4, 4, 26, 24, 25), seed=72, expect_band=False)


@pytest.mark.gpu
@pytest.mark.parametrize('scores', [GF_SCORE] + [s for s in SC.GAP_SCORES if s != GF_SCORE])
def test_gpu_ad_tags(gpu, oracle, monkeypatch, scores):
    # narrow bands for everything (VMX_AD_PCT=20): the 1024-base problems at the limit are tried in a band too
    monkeypatch.setenv('VMX_AD_PCT', '20')
    monkeypatch.setenv('VMX_AD_PCT_MIN', '20')
    check_tags(gpu, oracle, GPU_LIMIT, scores, seed=73)


@pytest.mark.gpu
def test_gpu_ad_scores_out_of_range(gpu, oracle):
    # bias 4096 + 1025 * 3 + 24 = 7195, highest value 2 * 513: 8221 > 8191
    check_tags(gpu, oracle, GPU_LIMIT, (2, -4, 4, 3, 24, 2), seed=74, expect_band=False)
