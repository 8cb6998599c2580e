"""GPU tests (run with -m gpu on an MI355X): the real library's kernels against the spec references of tests/spec_ref.py — not the oracle —
at the gfx950 layout switches (vmx_kernels.h: VMX_DP16X4_MAX 1024, VMX_DP16_MAX 6000), past the edit distance's 4096-column pass and its
16384-base long-pattern launch, and on a multi-Mb index. test_emu_spec.py runs the same checks on the emulator build's thresholds."""
import numpy as np
import pytest
import spec_cases as SC
import spec_ref as R
from kernel_cases import rand_seq, mutate

pytestmark = pytest.mark.gpu

X4_MAX, DP16_MAX = 1024, 6000


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)


def test_spec_edit_distance(ctx):
    SC.check_edit_distance(ctx, (0, 1, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 8193), seed=201)
    rng = np.random.default_rng(202)
    qs, ts = [], []
    for L in (16383, 16385, 17000):                         # around VMX_ED_LONG: the 16-wave launch
        a = rand_seq(rng, L)
        qs += [a, mutate(rng, a, 0.1)]; ts += [mutate(rng, a, 0.1), a[:L // 3] + a[L // 2:]]
    assert ctx.edit_distance_batch(qs, ts).tolist() == [R.levenshtein(q, t) for q, t in zip(qs, ts)]


@pytest.mark.parametrize('tier', [1, 2])
def test_spec_edit_distance_bound(ctx, tier):
    SC.check_edit_distance_bound(ctx, (1, 63, 64, 65, 129, 4095, 4096, 4097, 9000), seed=210 + tier, tier=tier)


def test_spec_gapfill(ctx):
    rng = np.random.default_rng(220)
    totals = [t + d for t in (X4_MAX, DP16_MAX) for d in (-1, 0, 1)]
    pairs = SC.gapfill_pairs(rng, totals)
    for _ in range(3):
        a = rand_seq(rng, 3000)
        pairs.append((a, (mutate(rng, a, 0.1) + rand_seq(rng, 3000))[:3000]))
    SC.check_gapfill(ctx, pairs)
    SC.check_gapfill(ctx, SC.gapfill_pairs(rng, totals[:3], base=(20, 80)), scores=SC.GAP_SCORES[1])


@pytest.mark.parametrize('p', SC.EXT_SCORES)
def test_spec_extend_grid(ctx, p):
    rng = np.random.default_rng(230 + SC.EXT_SCORES.index(p))
    for bw in (0, 1, 63, 64, 65, 100, 496, -1):
        pairs = SC.extend_random(rng, 8, 400)
        for zdrop in (0, 1, 50, 10 ** 6):
            SC.check_extend(ctx, pairs, p, bw, zdrop)


def test_spec_extend_large(ctx):
    """up to 6000 x 6000 with the widest band: thousands of ring wraps, diagonals of ~500 cells"""
    rng = np.random.default_rng(240)
    a = rand_seq(rng, 6000)
    pairs = [(a, mutate(rng, a, 0.04)), (a[:5000], a[:2000] + rand_seq(rng, 300) + a[2000:5000]), (a[:3000], mutate(rng, a[:3000], 0.15))]
    SC.check_extend(ctx, pairs, SC.EXT_SCORES[0], 496, 10 ** 6)
    SC.check_extend(ctx, pairs, SC.EXT_SCORES[0], 100, 50)


def test_spec_extend_constructed(ctx):
    SC.check_extend_constructed(ctx, seed=250)


def test_spec_extend_without_band(ctx):
    SC.check_extend_no_band(ctx, seed=260)


def test_spec_sketch(ctx):
    rng = np.random.default_rng(270)
    for k in (1, 2, 15, 16, 17, 27, 28):
        for w in (1, 2, 9, 10, 11, 255):
            SC.check_sketch(ctx, k, w, SC.sketch_seqs(rng, k, w, long_len=20000))


def test_spec_index(ctx):
    rng = np.random.default_rng(280)
    big = [rand_seq(rng, 2_000_000), rand_seq(rng, 1_200_000)]
    big[1] = big[1][:500_000] + 'N' * 2000 + big[1][:300_000].lower() + 'AC' * 5000 + big[1][500_000:]
    for k, w in ((15, 10), (17, 11), (28, 255)):
        SC.check_index(ctx, k, w, big + [rand_seq(rng, max(k - 1, 1))])
    for k, w in ((1, 1), (2, 255), (16, 9), (27, 2)):
        SC.check_index(ctx, k, w, [rand_seq(rng, 30000), 'A' * 700 + rand_seq(rng, 2100), 'ACGT' * 30 + 'N' * 10 + rand_seq(rng, 300).lower()])
