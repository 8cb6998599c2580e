"""CPU tests (no GPU): the PRODUCT's lookup and cluster kernels, compiled unchanged against the fiber emulator (tests/emu), on the constructed hit
sets of seed_cases.py — against spec_ref.map_read, row for row, at the emulator build's thresholds and under each routing: the default one, with
VMX_CLUSTER_SMALL_MAX lowered (every read with a hit goes to the filtered form k_cluster_big), and with VMX_CLUSTER_HUGE_MIN lowered too (straight to
the LONG form). The emulator build's counters (vmx_emu_cf_count) must show that every read was answered, or declined and handed on, by the forms
seed_cases.path() names: a case meant for a filtered form cannot pass through the general path unnoticed. test_gpu_seed_edges.py runs the same
families at the gfx950 thresholds."""
import ctypes
import numpy as np
import pytest
import seed_cases as S
import spec_ref as R

BUILD = 'emu'
FAMILIES = ('cut', 'bins', 'rank', 'overflow', 'occ', 'kform', 'sizes')
ANSWERS = {'default': {'small'}, 'big': {'big', 'gen'}, 'long': {'long', 'gen'}}      # the forms that must answer reads of every family's own, by routing


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def counter(ctx):
    f = ctx.lib.L.vmx_emu_cf_count; f.argtypes = [ctypes.c_int]; f.restype = ctypes.c_int
    return f


@pytest.fixture(scope='module')
def indexes(ctx):
    """one index per case, built on first use and kept for the three routings"""
    from vacmap_amd.lib import Index
    built = {}

    def get(case):
        if case.label not in built:
            built[case.label] = Index.from_seqs(ctx, ['c%d' % i for i in range(len(case.contigs))], case.contigs, k=case.k, w=case.w)
        return built[case.label]
    yield get
    for gi in built.values():
        gi.close()


@pytest.mark.parametrize('routing', list(S.ROUTINGS))
@pytest.mark.parametrize('family', FAMILIES)
def test_emu_seed_edges(ctx, counter, indexes, monkeypatch, family, routing):
    for name, v in S.ROUTINGS[routing].items():
        monkeypatch.setenv(name, v)
    seen = set()
    for c in S.constructed(BUILD):
        if c.family == family:
            S.check_case(ctx, indexes(c), c, S.spec_of(c), BUILD, routing, counter, seen)
    assert seen >= ANSWERS[routing], (family, routing, seen)                # (the counters have shown it for each of them)


def test_emu_seed_edges_default_cap(ctx, indexes):
    """Index.mid_occ is the spec's quantile rule on references that put the quantile index on the floor, on the second largest count and on the
    largest, and map_batch(mid_occ=-1) uses it"""
    caps = set()
    for c in S.constructed(BUILD):
        sp = S.spec_of(c); gi = indexes(c)
        assert gi.mid_occ == R.default_mid_occ(sp.IH), (c.label, gi.mid_occ, R.default_mid_occ(sp.IH))
        if c.family == 'defcap':
            h, p = gi.minimizers()
            assert np.array_equal(h, sp.IH) and np.array_equal(p, sp.IP), c.label
            S.check_case(ctx, gi, c, sp, BUILD, 'default'); caps.add(gi.mid_occ)
    assert caps == {10, 31, 51}
