"""CPU tests (no GPU, no emulator): the constructed rows of local_dp_cases.py for the local chain DPs, the plain statement of LC-exact, LC-mm and `_scar`
in spec_ref.local_dp, the fixture the reference's own Python recorded on the sets (tests/golden/local_dp_edges.*, tools/harness/gen_golden_local_dp_edges.py)
and the CPU oracle. The generator's claims are proven from the spec's counters alone; the spec must reproduce the reference bit for bit on every recorded
set, and the oracle must equal both — which is what entitles the emulator and GPU tests to use spec and oracle live on the sets that are not recorded."""
import os, re
import numpy as np
import pytest
import local_dp_cases as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tables(oracle):
    return D.oracle_tables(oracle)


@pytest.fixture(scope='module')
def cases(tables):
    return D.constructed(tables, largest=False)


def test_generator_is_deterministic_and_covers_every_family(cases, tables):
    D._constructed.clear()
    again = D.constructed(tables, largest=False)
    assert [D.key(c) for c in cases] == [D.key(c) for c in again]
    assert all(np.array_equal(a.rows, b.rows) and (a.readlen, a.ng, a.skip, a.maxdiff) == (b.readlen, b.ng, b.skip, b.maxdiff) for a, b in zip(cases, again))
    fam = {(c.mode, c.label.split('/')[0]) for c in cases}
    for mode in D.MODES:
        assert {(mode, f) for f in ('colinear', 'overlap', 'ties', 'lengths')} <= fam
    for mode in 'HLS':
        assert {(mode, f) for f in ('noncolinear', 'mm', 'switch')} <= fam
    assert ('R', 'scar') in fam and ('H', 'layout') in fam and ('R', 'layout') in fam
    # every set is in the DP's input order, and — outside mode R — every rule family runs as LC-exact and as LC-mm
    for c in cases:
        k = c.rows[:, 0] + (0 if c.mode == 'R' else c.rows[:, 3])
        assert (np.diff(k) >= 0).all(), D.key(c)
    assert {c.ng for c in cases if c.mode == 'H' and c.label.startswith('colinear')} == {1, 2}
    assert sorted({len(c.rows) for c in cases if c.label.startswith('layout')}) == D.layout_sizes(False)


def test_claims_hold_under_the_spec(cases, tables):
    """every family reaches its branch: the claims of every set, and per family no counter it is about at zero"""
    tot = {}
    for c in cases:
        D.check_claims(c, tables)
        e = D.expected_spec(c, tables)
        if e is not None and not e['switch']:
            t = tot.setdefault((c.label.split('/')[0], c.variant), {})
            for k, v in e['counters'].items():
                t[k] = t.get(k, 0) + v
    need = {'colinear': ('colinear_wins', 'noncolinear_wins', 'overlaps', 'gapcost_above10', 'breaks'), 'overlap': ('trimmed', 'trimmed_to_1', 'overlaps'),
            'ties': ('eq_break_evals', 'tie_tests', 'insert_among_equals', 'below16', 'below3', 'scans_past16', 'scans_past3'),
            'noncolinear': ('cross_strand_wins', 'noncolinear_wins'), 'lengths': ('trimmed', 'colinear_wins'), 'layout': ('colinear_wins', 'noncolinear_wins', 'overlaps', 'breaks')}
    for (f, v), t in tot.items():
        for k in need.get(f, ()):
            assert t[k] > 0, (f, v, k)
    assert tot[('noncolinear', 0)]['extra_saturated'] > 0 and tot[('mm', 1)]['l2c_saturated'] > 0
    s = tot[('scar', 2)]
    assert s['refunds'] > 0 and s['debts_carried'] > 0 and s['bonus_skips'] > 0 and s['held'] > 0 and s['kind_flips'] > 0
    # `bonus <= 0`: in every variant (LC-exact and LC-mm reach it against row 0 only: local_dp_cases.py, the module text)
    assert all(tot[('overlap', v)]['bonus_skips'] > 0 for v in (0, 1, 2))
    # the switch: both sides of opcount 100 000 and of the ratio 1000, in both variants
    sw = {D.key(c): D.expected_spec(c, tables)['switch'] for c in cases if c.label.startswith('switch')}
    assert sw['H:switch/ops100000/exact'] is False and sw['H:switch/ops100001/exact'] is True and sw['L:switch/ops100000/mm'] is False and sw['S:switch/ops100001/mm'] is True
    assert (sw['H:switch/ratio_below/exact'], sw['H:switch/ratio_at/exact'], sw['H:switch/ratio_above/exact']) == (False, False, True)


def test_twin_rules_are_reached(cases, oracle):
    """the `_fast` twins' own rules, proven on the oracle's twin: a bucket of 5 (every entry tried) and of 6 (the closest diagonal key stands for it), a tie of two
    keys, int(S) on both sides of an integer, row 0 above every later score level; and a row of l = 32 768 as row 0 of a set that switches"""
    assert sum(D.check_twin_claims(c, oracle) for c in cases) == 7
    for c in D.a0_cases():
        o = D.expected_oracle(c, oracle)
        assert o['rc'] == 0 and o['fast_used'] and o['opcount'] > 1000 * (c.rows[0, 3] + 14) and o['S'][0] == c.rows[0, 3] == 32768 and o['score'] >= 32768, D.key(c)


def test_spec_equals_the_reference_fixture(cases, tables):
    """score as bits and the trimmed chain of every recorded set; where the reference took the `_fast` twin the spec must have said so"""
    meta, _ = D.fixture()
    n = n_twin = 0
    for c in cases:
        if not c.record:
            continue
        e, r = D.expected_spec(c, tables), D.expected_recorded(c)
        if e['switch']:
            n_twin += 1
            continue
        assert D.bits(e['score']) == D.bits(r['score']), (D.key(c), e['score'], r['score'])
        D.same_chain(e['chain'], r['chain'], D.key(c))
        n += 1
    assert n + n_twin == len(meta) and n > 800 and n_twin >= 10, (n, n_twin, len(meta))


def test_oracle_equals_spec_and_fixture(cases, tables, oracle):
    """vmo_local_dp against the spec (S and P of every row, opcount, the switch) and against the recorded reference (the twins included)"""
    n = 0
    for c in cases:
        if not len(c.rows):
            continue
        e, o = D.expected_spec(c, tables), D.expected_oracle(c, oracle)
        assert o['fast_used'] == e['switch'], D.key(c)
        if c.label.startswith('switch/score_outside_table'):
            assert o['rc'] != 0, D.key(c)                      # the reference indexes its score table out of range: a raised read
            continue
        assert o['rc'] == 0, D.key(c)
        if not e['switch']:
            assert D.bits(o['score']) == D.bits(e['score']) and np.array_equal(o['P'], e['P']) and np.array_equal(D.bits(o['S']), D.bits(e['S'])), D.key(c)
            D.same_chain(o['chain'], e['chain'], D.key(c))
            assert c.variant == 2 or o['opcount'] == e['opcount'], (D.key(c), o['opcount'], e['opcount'])
        else:
            assert o['opcount'] == e['opcount'] and (o['opcount'], ) == e['tests'][-1][:1], (D.key(c), o['opcount'], e['tests'][-1])
        if c.record:
            r = D.expected_recorded(c)
            assert D.bits(o['score']) == D.bits(r['score']), (D.key(c), o['score'], r['score'])
            D.same_chain(o['chain'], r['chain'], D.key(c))
        n += 1
    assert n > 900


def test_random_sets_spec_equals_oracle(tables, oracle):
    for c in D.random_cases(np.random.default_rng(4500), 40):
        e, o = D.expected_spec(c, tables), D.expected_oracle(c, oracle)
        assert o['rc'] == 0 and not o['fast_used'] and not e['switch'], D.key(c)
        assert D.bits(o['score']) == D.bits(e['score']) and np.array_equal(o['P'], e['P']) and np.array_equal(D.bits(o['S']), D.bits(e['S'])), D.key(c)
        D.same_chain(o['chain'], e['chain'], D.key(c))


def test_constants_are_the_sources():
    """the row counts of the layout family and the switch sets straddle constants of the sources; if one of them changes, the generator (and the fixture) follows"""
    csrc = os.path.join(ROOT, 'vacmap_amd', 'csrc')
    kh = open(os.path.join(csrc, 'vmx_kernels.h')).read(); st = open(os.path.join(csrc, 'vmx_stage_local.hip')).read()
    rows = open(os.path.join(csrc, 'k_chain_rows.hip')).read(); one = open(os.path.join(csrc, 'k_chain_local.hip')).read()
    assert re.search(r'#define VMX_CHAIN_LDS_MAX_SHARED %d\b' % D.LDS_SHARED, kh) and re.search(r'#define VMX_LC_LDS_MAX_DEFAULT %d\b' % D.LDS_LARGEST, kh)
    assert 'caps[NB] = {512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 13056}' in st and D.LDS_CAPS == (512, 768, 1024)
    assert 'WW: entries the window holds (16;' in rows and 'VMX_RW_WIN=3' in rows and 'hi -= 16' in rows and (D.WINDOW, D.WINDOW_TEST) == (16, 3)
    assert 'if ((i & 63) == 0)' in one and D.WAVE_BLOCK == 64
    assert 'opcount > 100000 && ((double)opcount / (double)prereadloc) > 1000.0' in one and 'opcount > 100000 && (long long)opcount > 1000LL * (long long)prereadloc' in rows
    assert (D.SWITCH_OPS, D.SWITCH_RATIO) == (100000, 1000)
    import spec_ref
    assert (spec_ref.LOCAL_SWITCH_OPS, spec_ref.LOCAL_SWITCH_RATIO, spec_ref.LOCAL_NOPRE) == (100000, 1000, D.NOPRE)


def test_table_sizes_the_generator_assumes(tables):
    assert len(tables['log2cache']) == 100000 and len(tables['large_readgap']) == 100 and len(tables['readgap_h']) == 100 and len(tables['readgap_r']) == 100
    assert tables['extra'][-1] == 36.0 and tables['extra'][-2] < 36.0 and 100000 < len(tables['extra']) < 2 ** 20
    assert tables['large_readgap'][29] < 1 and tables['large_readgap'][30] == 15.0
