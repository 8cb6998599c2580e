"""GPU tests (run with -m gpu on an MI355X): the local re-seeding stage (k_local_prep, k_local_seed_band, k_local_seed) on the constructed cases of
local_cases.py at the gfx950 chunk, tile and slice sizes — against spec_ref.local_raw alone, row for row, with the banded form on
(VMX_LSEED_BAND=1) and with the general form alone (0). The trace line of vmx_local_stage (VMX_LSEED_TRACE) must show that the banded form kept
every read built for it and handed back exactly the reads built to be handed back ('windows', 'open runs', 'hit tile'). 'mix' is one call
with the reads of all mode-H families side by side; 'reuse' cycles 40 distinct reads through a launch of one workgroup per CU, so that every
workgroup slot's HBM pools (log, keys, offsets) serve a sparse read after a dense one. test_emu_local_edges.py runs the families at the emulator
build's sizes."""
import numpy as np
import pytest
import local_cases as LC

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
            built[case.label] = Index.from_seqs(ctx, ['c%d' % i for i in range(len(case.contigs))], case.contigs, k=15, w=10)
        return built[case.label]
    yield get
    for gi in built.values():
        gi.close()


@pytest.mark.parametrize('band', (1, 0))
@pytest.mark.parametrize('family', LC.FAMILIES)
def test_local_edges(ctx, indexes, monkeypatch, capfd, family, band):
    monkeypatch.setenv('VMX_LSEED_BAND', str(band)); monkeypatch.setenv('VMX_LSEED_TRACE', '1')
    n = 0
    for c in LC.constructed(BUILD):
        if c.family == family:
            LC.check_case(ctx, indexes(c), c, BUILD, band, lambda: capfd.readouterr().err); n += 1
    assert n


def test_local_edges_slot_reuse(ctx, indexes, monkeypatch, capfd):
    """one workgroup per CU (VMX_LSEED_BAND_WGS=1) and more than three reads per workgroup slot: the launch takes the reads longest first, so
    every slot runs sparse chunk-boundary reads, then the dense tandem-repeat reads, then the short sparse window reads, on the same pools"""
    from vacmap_amd.lib import local_chain_batch
    monkeypatch.setenv('VMX_LSEED_BAND', '1'); monkeypatch.setenv('VMX_LSEED_TRACE', '1'); monkeypatch.setenv('VMX_LSEED_BAND_WGS', '1')
    case = [c for c in LC.constructed(BUILD) if c.family == 'mix'][0]
    mine = [i for i, rd in enumerate(case.reads) if not rd.expect and rd.label.split('/')[0] in ('tile', 'windows', 'chunks')]
    dense = [i for i in mine if case.reads[i].label.startswith('tile')]
    sparse = [i for i in mine if i not in dense]
    assert len(dense) == 4 and len(sparse) >= 36
    pick = [i for j in range(4) for i in sparse[9 * j:9 * j + 9] + [dense[j]]]          # 40 distinct reads, every tenth one dense
    import torch
    slots = torch.cuda.get_device_properties(0).multi_processor_count                  # one workgroup per CU
    ids = pick * (3 * slots // len(pick) + 1)
    capfd.readouterr()
    res = local_chain_batch(ctx, indexes(case), ctx.lib.params(case.mode, local_kmersize=case.k), [case.reads[i].seq for i in ids], [case.reads[i].paths for i in ids])
    assert LC.parse_trace(capfd.readouterr().err) == [(len(ids), 0, {})]
    for i, g in zip(ids, res):
        assert g['status'] == 0, (case.reads[i].label, g['status'])
        LC.same(g['raw'], case.rows(i), case, case.reads[i], 'slot reuse')
