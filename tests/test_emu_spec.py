"""CPU tests (no GPU): the PRODUCT's kernels, compiled unchanged against the fiber emulator (tests/emu), against the spec references of
tests/spec_ref.py — not the oracle. Sizes straddle THIS build's layout switches (vmx_kernels.h: VMX_DP16X4_MAX 160, VMX_DP16_MAX 420);
test_gpu_spec.py runs the same checks at the gfx950 thresholds."""
import numpy as np
import pytest
import spec_cases as SC

EMU_X4_MAX, EMU_DP16_MAX = 160, 420


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


def test_emu_spec_edit_distance(ctx):
    SC.check_edit_distance(ctx, (0, 1, 63, 64, 65, 127, 128, 129), seed=101)
    SC.check_edit_distance(ctx, (4095, 4096, 4097), seed=102)              # the last pattern block of a 64-block pass, and one past it


@pytest.mark.parametrize('tier', [1, 2])
def test_emu_spec_edit_distance_bound(ctx, tier):
    SC.check_edit_distance_bound(ctx, (1, 63, 64, 65, 127, 128, 129, 700), seed=110 + tier, tier=tier)


def test_emu_spec_gapfill(ctx):
    rng = np.random.default_rng(120)
    totals = [t + d for t in (EMU_X4_MAX, EMU_DP16_MAX) for d in (-1, 0, 1)]
    SC.check_gapfill(ctx, SC.gapfill_pairs(rng, totals))
    SC.check_gapfill(ctx, SC.gapfill_pairs(rng, totals[:3], base=(20, 80)), scores=SC.GAP_SCORES[1])


@pytest.mark.parametrize('p', SC.EXT_SCORES)
def test_emu_spec_extend_grid(ctx, p):
    rng = np.random.default_rng(130 + SC.EXT_SCORES.index(p))
    for bw in (0, 1, 63, 64, 65, 100, 496, -1):
        pairs = SC.extend_random(rng, 6, 300)
        for zdrop in (0, 1, 50, 10 ** 6):
            SC.check_extend(ctx, pairs, p, bw, zdrop)


def test_emu_spec_extend_constructed(ctx):
    SC.check_extend_constructed(ctx, seed=140)


def test_emu_spec_extend_without_band(ctx):
    SC.check_extend_no_band(ctx, seed=150)


def test_emu_spec_sketch(ctx):
    rng = np.random.default_rng(160)
    for k in (1, 2, 15, 16, 17, 27, 28):
        for w in (1, 2, 9, 10, 11, 255):
            SC.check_sketch(ctx, k, w, SC.sketch_seqs(rng, k, w))


def test_emu_spec_index(ctx):
    rng = np.random.default_rng(170)
    from kernel_cases import rand_seq
    for k, w in ((1, 1), (2, 255), (15, 10), (16, 9), (17, 11), (27, 2), (28, 255)):
        contigs = [rand_seq(rng, 5000), 'ACGT' * 30 + 'N' * 10 + rand_seq(rng, 300).lower(), rand_seq(rng, max(k - 1, 1)), 'A' * 700 + rand_seq(rng, 2100)]
        SC.check_index(ctx, k, w, contigs)
