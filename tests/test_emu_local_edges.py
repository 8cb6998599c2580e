"""CPU tests (no GPU): the PRODUCT's local re-seeding stage (k_local_prep, k_local_seed_band, k_local_seed), compiled unchanged against the fiber
emulator (tests/emu), on the constructed cases of local_cases.py at the emulator build's chunk, tile and slice sizes — against
spec_ref.local_raw, row for row, with the banded form on (VMX_LSEED_BAND=1) and with the general form alone (0). The trace line of
vmx_local_stage (VMX_LSEED_TRACE) must show that the banded form kept every read built for it and handed back exactly the reads built to be
handed back, for the reason they were built for. test_gpu_local_edges.py runs the same families at the gfx950 sizes."""
import pytest
import local_cases as LC

BUILD = 'emu'


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def indexes(ctx):
    """one index per case, built on first use and kept for both kernels"""
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
def test_emu_local_edges(ctx, indexes, monkeypatch, capfd, family, band):
    monkeypatch.setenv('VMX_LSEED_BAND', str(band)); monkeypatch.setenv('VMX_LSEED_TRACE', '1')
    n = 0
    for c in LC.constructed(BUILD):
        if c.family == family:
            LC.check_case(ctx, indexes(c), c, BUILD, band, lambda: capfd.readouterr().err); n += 1
    assert n
