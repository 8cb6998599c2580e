"""CPU tests (no GPU): the PRODUCT's local chain DPs, compiled unchanged against the fiber emulator (tests/emu), through the stage entry vm_local_dp_batch on
the constructed rows of local_dp_cases.py — against the reference's recorded results (tests/golden/local_dp_edges.*), the plain spec (spec_ref.local_dp) and
the oracle run live, with no tolerance: status, variant, twin used, score as bits, chain rows, S / P where the form that ran leaves them in HBM. The forms:
four reads per wavefront with the 16-entry window, the same with the 3-entry window (VMX_RW_WIN=3), each with the host-built and the device-built read
list, and one wavefront per read (VMX_CHAIN_ROWS=0, read once: child processes, LDS-resident under the product's limit and with VMX_LC_LDS_MAX=0). The
3-entry-window run leaves out the sets of more than 1100 rows; the largest LDS bucket (13 056 rows) is left to test_gpu_local_dp_edges.py."""
import os, subprocess, sys
import numpy as np
import pytest
import local_dp_cases as D

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def tables(oracle):
    return D.oracle_tables(oracle)


@pytest.fixture(scope='module')
def cases(tables):
    return D.constructed(tables, largest=False)


@pytest.mark.parametrize('device_list', [False, True], ids=['host_list', 'device_list'])
def test_emu_local_dp_rows(ctx, oracle, tables, cases, device_list):
    assert os.environ.get('VMX_CHAIN_ROWS', '1') != '0' and 'VMX_RW_WIN' not in os.environ
    D.check(ctx, oracle, tables, cases, 'rows', device_list, need_s=lambda c: True)
    D.check_long_beside_short(ctx, oracle, tables, device_list=device_list)


@pytest.mark.parametrize('device_list', [False, True], ids=['host_list', 'device_list'])
def test_emu_local_dp_rows_small_window(ctx, oracle, tables, cases, monkeypatch, device_list):
    monkeypatch.setenv('VMX_RW_WIN', '3')
    D.check(ctx, oracle, tables, [c for c in cases if len(c.rows) <= 1100], 'rows, window of 3', device_list, need_s=lambda c: True)
    D.check_long_beside_short(ctx, oracle, tables, device_list=device_list)


def test_emu_local_dp_random(ctx, oracle, tables, monkeypatch):
    rnd = D.random_cases(np.random.default_rng(4600), 60)
    D.check(ctx, oracle, tables, rnd, 'random')
    D.check(ctx, oracle, tables, rnd[::2], 'random', device_list=True)
    monkeypatch.setenv('VMX_RW_WIN', '3')
    D.check(ctx, oracle, tables, rnd[::3], 'random, window of 3')


@pytest.mark.parametrize('lds', ['512', '0'])
def test_emu_local_dp_one_wavefront_per_read(lds):
    out = subprocess.run([sys.executable, os.path.join(HERE, 'local_dp_cases.py'), 'emu'], env=dict(os.environ, VMX_CHAIN_ROWS='0', VMX_LC_LDS_MAX=lds),
                         capture_output=True, text=True, timeout=3000)
    assert out.returncode == 0 and 'local dp edges ok' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_emu_local_dp_long_row_0_switches(ctx, oracle, tables):
    """l = 32 768 as row 0 of a set that switches (9 301 rows, 35 M candidates: the one slow set, run in one form): k_chain_local_fast indexes its score table with it"""
    D.check(ctx, oracle, tables, D.a0_cases()[:1], 'rows', need_s=lambda c: True)


def test_emu_local_dp_refusals(ctx, oracle, tables):
    D.check_refusals(ctx, oracle, tables)
