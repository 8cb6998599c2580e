"""GPU tests (run with -m gpu on an MI355X): the local chain DPs through the stage entry vm_local_dp_batch on the constructed rows of local_dp_cases.py —
against the reference's recorded results (tests/golden/local_dp_edges.*), the plain spec (spec_ref.local_dp) and the oracle run live, with no tolerance:
status, variant, twin used, score as bits, chain rows, S / P where the form that ran leaves them in HBM. The forms: four reads per wavefront
(k_chain_local_rows), the same with the 3-entry window built into the library as test kernels (VMX_RW_WIN=3; the device counters must show that scans left
the window and insertions went through HBM — a store -> load order inside one wavefront, which the CPU emulator cannot get wrong), each with the host-built
and the device-built read list; one wavefront per read (k_chain_local: VMX_CHAIN_ROWS=0 is read once, so freshly started child processes run it, LDS-resident
up to the largest bucket with VMX_LC_LDS_MAX=13056 and with nothing in LDS, VMX_LC_LDS_MAX=0); and the `_fast` twins behind either."""
import os, subprocess, sys
import numpy as np
import pytest
import local_dp_cases as D

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    return Context(0)


@pytest.fixture(scope='module')
def tables(oracle):
    return D.oracle_tables(oracle)


@pytest.fixture(scope='module')
def cases(tables):
    return D.constructed(tables, largest=True)


@pytest.mark.parametrize('device_list', [False, True], ids=['host_list', 'device_list'])
def test_local_dp_rows(ctx, oracle, tables, cases, device_list):
    assert os.environ.get('VMX_CHAIN_ROWS', '1') != '0' and 'VMX_RW_WIN' not in os.environ
    D.check(ctx, oracle, tables, cases, 'rows', device_list, need_s=lambda c: True)
    D.check_long_beside_short(ctx, oracle, tables, device_list=device_list)


def test_local_dp_rows_small_window(ctx, oracle, tables, cases, monkeypatch):
    from vacmap_amd.lib import chain_counters
    chain_counters(ctx.lib, 1); chain_counters(ctx.lib, -1)
    monkeypatch.setenv('VMX_RW_WIN', '3')
    n = D.check(ctx, oracle, tables, cases, 'rows, window of 3', need_s=lambda c: True)
    D.check(ctx, oracle, tables, cases, 'rows, window of 3', device_list=True, need_s=lambda c: True)
    D.check_long_beside_short(ctx, oracle, tables)
    c = chain_counters(ctx.lib, -1)
    assert c['local_anchors'] > 50 * n and c['local_scans_past_window'] > 1000 and c['local_insertions_through_hbm'] > 1000, c
    monkeypatch.delenv('VMX_RW_WIN')
    # the product's window: the tie and layout families leave it too
    D.check(ctx, oracle, tables, [x for x in cases if x.label.startswith(('ties', 'layout'))], 'rows')
    c = chain_counters(ctx.lib, -1)
    assert c['local_scans_past_window'] > 0 and c['local_insertions_through_hbm'] > 0, c
    chain_counters(ctx.lib, 0)


def test_local_dp_random(ctx, oracle, tables, monkeypatch):
    rnd = D.random_cases(np.random.default_rng(4700), 150)
    D.check(ctx, oracle, tables, rnd, 'random')
    D.check(ctx, oracle, tables, rnd[::2], 'random', device_list=True)
    monkeypatch.setenv('VMX_RW_WIN', '3')
    D.check(ctx, oracle, tables, rnd[::3], 'random, window of 3')


@pytest.mark.parametrize('lds', ['13056', '0'])
def test_local_dp_one_wavefront_per_read(lds):
    out = subprocess.run([sys.executable, os.path.join(HERE, 'local_dp_cases.py'), 'gpu'], env=dict(os.environ, VMX_CHAIN_ROWS='0', VMX_LC_LDS_MAX=lds),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and 'local dp edges ok' in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize('l', [32767, 32768, 65535])
def test_local_dp_long_row_0_switches(ctx, oracle, tables, l):
    """l at the 16-bit edge as row 0 of a set that switches (9 301 / 12 751 rows): k_chain_local_fast indexes its score table with it"""
    cs = D.a0_cases((l,))
    D.check(ctx, oracle, tables, cs, 'rows', need_s=lambda c: True)
    D.check(ctx, oracle, tables, cs[:1], 'rows', device_list=True)


def test_local_dp_refusals(ctx, oracle, tables):
    D.check_refusals(ctx, oracle, tables)
