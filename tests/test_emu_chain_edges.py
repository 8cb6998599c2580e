"""CPU tests (no GPU): the PRODUCT's chain kernels, compiled unchanged against the fiber emulator (tests/emu), on the constructed anchor sets of
chain_cases.py — against the reference's recorded results (tests/golden/chain_edges.*) and the oracle run live, bit for bit, in three forms:
four reads per wavefront with the 16-entry window, the same with the 3-entry window (VMX_RW_WIN=3), and one wavefront per read
(VMX_CHAIN_ROWS=0, read once: a child process, which also runs the linked DPs in their plain form, VMX_LINK_PLAIN=1). The 3-entry-window run leaves
out the sets of more than 1100 anchors (the bail-out pair and the larger layout sizes) to keep this file's time down; test_gpu_chain_edges.py runs the
same checks on the device, all sets in every form."""
import os, subprocess, sys
import numpy as np
import pytest
import chain_cases as CC

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def cases():
    return CC.constructed()


def test_emu_chain_edges_rows(ctx, oracle, cases):
    assert os.environ.get('VMX_CHAIN_ROWS', '1') != '0' and 'VMX_RW_WIN' not in os.environ
    CC.check_global(ctx, oracle, cases, 'rows')
    CC.check_long_beside_short(ctx, oracle)


def test_emu_chain_edges_rows_small_window(ctx, oracle, cases, monkeypatch):
    monkeypatch.setenv('VMX_RW_WIN', '3')
    CC.check_global(ctx, oracle, [c for c in cases if len(c.anchors) <= 1100], 'rows, window of 3')
    CC.check_long_beside_short(ctx, oracle)


def test_emu_chain_edges_random(ctx, oracle, monkeypatch):
    rng = np.random.default_rng(4100)
    rnd = [c for mode in 'HLSR' for c in CC.random_cases(rng, mode, 150, nmax=500)]
    CC.check_global(ctx, oracle, rnd, 'random')
    monkeypatch.setenv('VMX_RW_WIN', '3')
    CC.check_global(ctx, oracle, rnd[::3], 'random, window of 3')


def test_emu_chain_edges_one_wavefront_per_read():
    out = subprocess.run([sys.executable, os.path.join(HERE, 'chain_cases.py'), 'emu'], env=dict(os.environ, VMX_CHAIN_ROWS='0', VMX_LINK_PLAIN='1'), capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'chain edges ok' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_emu_chain_edges_refusals(ctx, oracle):
    CC.check_refusals(ctx, oracle)


def test_emu_chain_edges_linked(ctx, oracle, cases):
    CC.check_linked(ctx, oracle, cases)
