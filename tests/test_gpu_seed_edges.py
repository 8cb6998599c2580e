"""GPU tests (run with -m gpu on an MI355X): k_lookup, k_fill_hits and the four cluster forms (k_cluster, k_cluster_big, k_cluster_long,
k_cluster_gen) on the constructed hit sets of seed_cases.py at the gfx950 thresholds — against spec_ref.map_read alone, row for row. The small
cases reach the filtered forms through the two routing knobs (VMX_CLUSTER_SMALL_MAX, VMX_CLUSTER_HUGE_MIN); the size-class family is routed by
its real hit counts (4096 / 4097, the candidate caps and one above, 0x3fff / 0x4000, 0xffff / 0x10000 and beyond). Every map_batch call holds
reads of several size classes, declined and answered ones side by side. test_emu_seed_edges.py asserts on the emulator build which form answers."""
import numpy as np
import pytest
import seed_cases as S
import spec_ref as R

pytestmark = pytest.mark.gpu
BUILD = 'gfx950'


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)


@pytest.fixture(scope='module')
def indexes(ctx):
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
@pytest.mark.parametrize('family', ('cut', 'bins', 'rank', 'overflow', 'occ', 'kform'))
def test_seed_edges(ctx, indexes, monkeypatch, family, routing):
    for name, v in S.ROUTINGS[routing].items():
        monkeypatch.setenv(name, v)
    n = 0
    for c in S.constructed(BUILD):
        if c.family == family:
            S.check_case(ctx, indexes(c), c, S.spec_of(c), BUILD, routing); n += 1
    assert n


@pytest.mark.parametrize('routing', list(S.ROUTINGS))
def test_seed_edges_size_classes(ctx, indexes, monkeypatch, routing):
    for name, v in S.ROUTINGS[routing].items():
        monkeypatch.setenv(name, v)
    c = [x for x in S.constructed(BUILD) if x.family == 'sizes'][0]
    S.check_case(ctx, indexes(c), c, S.spec_of(c), BUILD, routing)


def test_seed_edges_default_cap(ctx, indexes):
    caps = set()
    for c in S.constructed(BUILD):
        sp = S.spec_of(c); gi = indexes(c)
        assert gi.mid_occ == R.default_mid_occ(sp.IH), (c.label, gi.mid_occ, R.default_mid_occ(sp.IH))
        if c.family == 'defcap':
            h, p = gi.minimizers()
            assert np.array_equal(h, sp.IH) and np.array_equal(p, sp.IP), c.label
            S.check_case(ctx, gi, c, sp, BUILD, 'default'); caps.add(gi.mid_occ)
    assert caps == {10, 31, 51}
