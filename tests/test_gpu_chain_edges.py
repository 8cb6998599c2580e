"""GPU tests (run with -m gpu on an MI355X): the chain kernels on the constructed anchor sets of chain_cases.py — against the reference's recorded
results (tests/golden/chain_edges.*) and the oracle run live, bit for bit. The forms: four reads per wavefront (k_chain_global_rows), the same with
the 3-entry window built into the library as test kernels (VMX_RW_WIN=3; the device counters must show that scans left the window and insertions
went through HBM — a store -> load order inside one wavefront, which the CPU emulator cannot get wrong), one wavefront per read (k_chain_global:
VMX_CHAIN_ROWS=0 is read once, so a freshly started child process runs it), GC-fast, and the linked DPs of -mode asm in both forms (k_chain_linked_win,
and k_chain_linked with VMX_LINK_PLAIN=1 in the child)."""
import os, subprocess, sys
import numpy as np
import pytest
import chain_cases as CC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)


@pytest.fixture(scope='module')
def cases():
    return CC.constructed()


def test_chain_edges_rows(ctx, oracle, cases):
    assert os.environ.get('VMX_CHAIN_ROWS', '1') != '0' and 'VMX_RW_WIN' not in os.environ
    CC.check_global(ctx, oracle, cases, 'rows')
    CC.check_long_beside_short(ctx, oracle)


def test_chain_edges_rows_small_window(ctx, oracle, cases, monkeypatch):
    from vacmap_amd.lib import chain_counters
    chain_counters(ctx.lib, 1); chain_counters(ctx.lib, -1)
    monkeypatch.setenv('VMX_RW_WIN', '3')
    n = CC.check_global(ctx, oracle, cases, 'rows, window of 3')
    CC.check_long_beside_short(ctx, oracle)
    c = chain_counters(ctx.lib, -1)
    assert c['global_anchors'] > 100 * n and c['global_scans_past_window'] > 1000 and c['global_insertions_through_hbm'] > 1000, c
    monkeypatch.delenv('VMX_RW_WIN')
    # the product's window: the isolated equal anchors and the layout sets leave it too
    CC.check_global(ctx, oracle, [x for x in cases if x.label.startswith(('ties/isolated', 'layout'))], 'rows')
    c = chain_counters(ctx.lib, -1)
    assert c['global_scans_past_window'] > 0 and c['global_insertions_through_hbm'] > 0, c


def test_chain_edges_random(ctx, oracle, monkeypatch):
    rng = np.random.default_rng(4200)
    rnd = [c for mode in 'HLSR' for c in CC.random_cases(rng, mode, 750)]
    CC.check_global(ctx, oracle, rnd, 'random')
    monkeypatch.setenv('VMX_RW_WIN', '3')
    CC.check_global(ctx, oracle, rnd[::3], 'random, window of 3')


def test_chain_edges_one_wavefront_per_read():
    out = subprocess.run([sys.executable, os.path.join(HERE, 'chain_cases.py'), 'gpu'], env=dict(os.environ, VMX_CHAIN_ROWS='0', VMX_LINK_PLAIN='1'), capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and 'chain edges ok' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_chain_edges_refusals(ctx, oracle):
    CC.check_refusals(ctx, oracle)


def test_chain_edges_linked(ctx, oracle, cases):
    CC.check_linked(ctx, oracle, cases)
