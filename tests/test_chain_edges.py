"""CPU tests (no GPU, no emulator): the constructed anchor sets of chain_cases.py, the fixture the reference's own Python recorded on them
(tests/golden/chain_edges.*, tools/harness/gen_golden_chain_edges.py) and the CPU oracle. The oracle must reproduce the reference bit for bit on
every recorded set — which is what entitles the emulator and GPU tests to use it live on the sets that are too many or too large to record."""
import numpy as np
import pytest
import chain_cases as CC


@pytest.fixture(scope='module')
def cases():
    return CC.constructed()


def test_generator_is_deterministic_and_covers_every_family(cases):
    again = CC.constructed()
    assert [CC.key(c) for c in cases] == [CC.key(c) for c in again]
    assert all(np.array_equal(a.anchors, b.anchors) and a.readlen == b.readlen for a, b in zip(cases, again))
    fam = {(c.mode, c.label.split('/')[0]) for c in cases}
    for mode in 'HLSR':
        assert {(mode, f) for f in ('gap', 'overlap', 'coverage', 'ties', 'extra', 'form')} <= fam
    assert ('R', 'modeR') in fam and ('H', 'layout') in fam and ('R', 'layout') in fam
    # both orientations of the strand flip, and the tie
    meta, _ = CC.fixture()
    flips = [meta[CC.key(c)].get('need_reverse') for c in cases if c.record and len(c.anchors) > 2]
    assert flips.count(True) > 300 and flips.count(False) > 300
    for c in cases:
        if c.label.startswith('form/strand_tie'):
            assert (c.anchors[:, 2] == 1).sum() == (c.anchors[:, 2] == -1).sum() and meta[CC.key(c)]['need_reverse'] is False


def test_geometry_helper_inverts_the_reference_rule():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        aj = (int(rng.integers(0, 5000)), int(rng.integers(10 ** 6, 10 ** 7)), int(rng.choice([-1, 1])), int(rng.integers(5, 40)))
        li = int(rng.integers(5, 40))
        readgap = int(rng.integers(-min(aj[3], li - 1), 50)) or 1
        refgap = int(rng.integers(-5, 3000))
        ai = CC.place(aj, int(rng.choice([-1, 1])), li, readgap, refgap)
        rg, fg, bonus = CC.geometry(ai, aj)
        assert (rg, fg) == (max(readgap, 0), refgap) and bonus == (li if readgap >= 0 else li + readgap)


def test_form_switches_are_hit(cases):
    """the sets meant to sit on either side of a switch do: the fixture says which DP the reference ran"""
    meta, _ = CC.fixture()
    for mode in 'HLSR':
        assert meta['%s:form/per_base/300_over_60' % mode]['fast_used'] is False
        assert meta['%s:form/per_base/301_over_60' % mode]['fast_used'] is True
        assert meta['%s:form/per_base/300_over_61' % mode]['fast_used'] is False
    for mode in 'HR':
        assert meta['%s:form/bailout/2002' % mode]['fast_used'] is False and meta['%s:form/bailout/2003' % mode]['fast_used'] is True
        assert meta['%s:form/l65535' % mode]['gmax'] >= 0 and meta['%s:form/l65535' % mode]['score'] >= 40 * 65535
    assert any(meta[CC.key(c)]['mapq'] > 0 for c in cases if c.record) and any(len(meta[CC.key(c)]['path_lens']) > 1 for c in cases if c.record)


def test_oracle_equals_the_reference_fixture(cases, oracle):
    n = 0
    for c in cases:
        if not c.record:
            continue
        e, o = CC.expected_recorded(c), CC.expected_oracle(c, oracle)
        g = dict(o, paths=[np.array(p, dtype=np.int64).reshape(-1, 4) for p in o['paths']])
        if e['n'] <= 2:
            g['gmax'] = -1
        CC.same(e, g, CC.key(c))
        n += 1
    meta, _ = CC.fixture()
    assert n == len(meta) > 700


def test_long_row_sets_reach_gc_fast(cases, oracle):
    """the bail-out set with a row of l = 32 768 (oracle only): GC-fast ran, did not raise, and the long row is in the primary path"""
    n = 0
    for c in cases:
        if c.label.startswith('form/bailout/l32768'):
            e = CC.expected_oracle(c, oracle)
            assert e['fast_used'] and e['gmax'] >= 0 and e['score'] > 32768, (c.label, e['fast_used'], e['gmax'], e['score'])
            assert any(32768 in [row[3] for row in p] for p in e['paths'][:1]), c.label
            n += 1
    assert n == 1


def test_opcount_rule_of_the_oracle(cases, oracle):
    """the reference does not return opcount; its bail-out (:24914) shows it: isolated equal anchors never end a scan, so opcount is i (i - 1) / 2 at anchor i"""
    for c in cases:
        if c.label == 'form/bailout/2002':
            assert CC.expected_oracle(c, oracle)['opcount'] == 2002 * 2001 // 2


def test_oracle_linked_equals_the_reference_fixture(cases, oracle):
    """chain_linked_raw (which 0 and 2), with and without carried state, against what the reference's linked DPs returned for the same calls"""
    n_state, _ = CC.check_linked(None, oracle, cases)
    meta, _ = CC.linked_fixture()
    assert n_state >= 40 and len(meta) >= 180


def test_layout_thresholds_are_the_sources(cases):
    """the anchor counts of the layout family straddle constants of the kernels' sources; if one of them changes, the family (and the fixture) has to follow"""
    import os, re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vacmap_amd', 'csrc')
    kh = open(os.path.join(csrc, 'vmx_kernels.h')).read(); al = open(os.path.join(csrc, 'vmx_align.hip')).read(); rows = open(os.path.join(csrc, 'k_chain_rows.hip')).read()
    assert re.search(r'#define VMX_SORT_LDS 4096\b', kh) and re.search(r'#define VMX_CHAIN_LDS_MAX_SHARED 512\b', kh) and re.search(r'#define VMX_SELECT_LDS 3072\b', kh)
    assert 'caps[NC] = {192, 384, 768, 1536, 3072, 0}' in al and 'caps[NB] = {384, 512, 768,' in al
    assert 'WW: entries the window holds (16;' in rows and 'VMX_RW_WIN=3' in rows
    sizes = {len(c.anchors) for c in cases if c.label.startswith('layout/')}
    for t in (3, 16, 64, 128, 192, 384, 512, 768, 1536, 3072, 4096):
        assert {t, t + 1} <= sizes and (t - 1 in sizes or t == 3)
