"""GPU twin of test_emu_ad_block_store.py: the band fill's block stores (vmx_dp_ad.h, one 16- / 8- / 4-byte store per lane, problem and four anti-diagonals, into
the lane-major lines of vmx_gapfill.h) and the walk that reads them, on the real library through vm_k_cigar_batch_banded — CIGARs and scores against the
full-matrix entry and the oracle, problem for problem (ad_block_store_cases.py)."""
import pytest
import ad_block_store_cases as BS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)     # raises loudly when the HIP library or the device is missing


def test_gpu_ad_block_store(ctx, oracle, monkeypatch):
    BS.check(ctx, oracle, monkeypatch)
