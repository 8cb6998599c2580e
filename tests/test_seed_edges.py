"""CPU tests (no GPU, no emulator): the constructed hit sets of seed_cases.py. The generator's self-check — the hits it intends are the ones
spec_ref.map_read sees, and every property a case names holds (the cut falls inside a tie, ncand = cap + 1, the path a read takes through the
cluster forms ...) — and the CPU oracle's Index.map against spec_ref.map_read on every case: the oracle's map() is pinned to the spec here,
which is what entitles the other tests to use it live."""
import re, os
import numpy as np
import pytest
import seed_cases as S
import spec_ref as R

BUILD_NAMES = sorted(S.BUILDS)


@pytest.fixture(scope='module', params=BUILD_NAMES)
def cases(request):
    return request.param, S.constructed(request.param)


def test_generator_is_deterministic_and_covers_every_family(cases):
    build, cs = cases
    again = S.generate() + S.size_cases(np.random.default_rng(20240608), build)
    assert [c.label for c in cs] == [c.label for c in again] and len({c.label for c in cs}) == len(cs)
    for a, b in zip(cs, again):
        assert a.contigs == b.contigs and [r.seq for r in a.reads] == [r.seq for r in b.reads] and a.params == b.params
    assert {c.family for c in cs} == {'cut', 'bins', 'rank', 'overflow', 'occ', 'defcap', 'kform', 'sizes'}
    assert {(c.k, c.w) for c in cs} >= {(15, 1), (17, 1), (28, 1), (15, 10)}
    for c in cs:                                                         # every family runs reverse-complemented too, beside reads of other size classes
        if c.family not in ('defcap', 'sizes') and c.w == 1:
            labels = {r.label for r in c.reads}
            assert any(l.endswith('/rc') for l in labels) and {'ballast/320', 'ballast/4224'} <= labels, c.label


def test_probes_and_plant():
    rng = np.random.default_rng(1)
    P = S.Plan('x', rng, k=3, ballast=False)                             # 4^3 = 64 k-mers, none its own reverse complement: 32 probes and no more
    ids = [P.probe() for _ in range(32)]
    ps = [P.probes[i] for i in ids]
    assert len(set(ps) | {S.revcomp(p) for p in ps}) == 64 and all(p != S.revcomp(p) for p in ps)
    assert S.plant([(2, 'ACG'), (7, 'TTA')], [6, 10]) == ['NNACGN', 'NTTANNNNNN']
    assert S.read_of(['ACG', 'TTA']) == 'ACGNTTA'
    for bad in ([(2, 'ACG'), (5, 'TTA')], [(4, 'ACG')], [(2, 'ACG'), (3, 'T')]):      # touching, across a contig end, overlapping
        with pytest.raises(AssertionError):
            S.plant(bad, [6, 10])


def test_intended_hits_are_the_specs_and_every_stated_property_holds(cases):
    build, cs = cases
    n = 0
    for c in cs:
        S.check_claims(c, S.spec_of(c))
        n += len(c.claims)
    assert n > 150


def test_default_cap_cases_sit_on_every_place_of_the_quantile(cases):
    caps = {c.label: [x[1] for x in c.claims if x[0] == 'mid_occ'][0] for c in cases[1] if c.family == 'defcap'}
    assert caps['defcap/floor'] == 10 and caps['defcap/nd1/30'] == 31 and caps['defcap/nd1/3'] == 10 and caps['defcap/nd10001'] == 10
    assert caps['defcap/nd4999'] == 51 and caps['defcap/nd5001'] == caps['defcap/nd5002'] == 31 and caps['defcap/nd5000'] in (31, 51)


def test_every_form_is_named_by_every_family_it_can_take(cases):
    """before any kernel runs: under the three routings the expected paths end in each of the four forms for every family with its own reads of
    more than one hit (test_emu_seed_edges.py then asserts the paths with the emulator's counters)"""
    build, cs = cases
    seen = set()
    for c in cs:
        sp = S.spec_of(c)
        for rt in S.ROUTINGS:
            for cn, mo in c.params:
                for i in S.reads_for(c, cn, mo):
                    if not c.reads[i].label.startswith('ballast'):
                        seen.add((c.family, S.path(sp.hits(i, mo)[:, 1], cn, build, rt)[-1]))
    assert seen >= {(f, x) for f in ('cut', 'bins', 'rank', 'overflow', 'occ', 'kform', 'sizes') for x in ('small', 'big', 'long', 'gen')}, seen


def test_size_classes_are_the_sources(cases):
    """the hit and candidate counts of the size-class family straddle constants of the kernels' sources; if one changes, the table has to follow"""
    build, cs = cases
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'vacmap_amd', 'csrc')
    kh = open(os.path.join(csrc, 'vmx_kernels.h')).read(); ks = open(os.path.join(csrc, 'k_seed.hip')).read(); ix = open(os.path.join(csrc, 'vmx_index.hip')).read()
    E, G = S.BUILDS['emu'], S.BUILDS['gfx950']
    assert re.search(r'#define VMX_SORT_LDS %d\b' % E['SORT_LDS'], kh) and E['SORT_LDS'] == G['SORT_LDS']
    assert re.search(r'#define VMX_SORT_LDS_BIG %d\b.*emulator' % E['SORT_LDS_BIG'], kh) and re.search(r'#define VMX_SORT_LDS_BIG %d\b' % G['SORT_LDS_BIG'], kh)
    assert re.search(r'#ifdef VMX_EMU\n#define VMX_CF_SLOT_BITS 15 .*\n#define VMX_CF_CAND %d\n' % E['CF_CAND'], ks) and re.search(r'#else\n#define VMX_CF_SLOT_BITS 18\n#define VMX_CF_CAND %d\n' % G['CF_CAND'], ks)
    assert '#define VMX_CFB_CAP (VMX_SORT_LDS_BIG - 1024)' in ks and all(B['CFB_CAP'] == B['SORT_LDS_BIG'] - 1024 for B in (E, G))
    assert 'if (n > (LONG ? 0xffff : 0x3fff)) return false;' in ks and 'check_num > 0 && check_num <= 1024' in ks and 'int64_t huge_min = 0x3fff;' in ix
    assert 'sz < 1023 ? sz : 1023' in ks and '>> 28) >> 13)' in ks and '> 5000)' in ks
    B = S.BUILDS[build]
    c = [x for x in cs if x.family == 'sizes'][0]; sp = S.spec_of(c)
    nh = {len(sp.hits(i, 64)) for i in range(len(c.reads))}
    for t in (64, 256, 1024, 2048, 4096, B['SORT_LDS_BIG'], S.BIG_MAX_HITS + 1):
        assert {t - 1, t, t + 1} <= nh | {S.BIG_MAX_HITS + 2}, t
    assert {S.LONG_MAX_HITS, S.LONG_MAX_HITS + 1} <= nh and max(nh) > S.LONG_MAX_HITS + 1
    nc = {S.ncand(sp.hits(i, 64)[:, 1]) for i in range(len(c.reads))}
    assert {B['CF_CAND'], B['CF_CAND'] + 1, B['CFB_CAP'], B['CFB_CAP'] + 1} <= nc
    big = sp.rows(c.read('hits/65801'), 0, 64)                              # the read above 0xffff hits keeps dense clusters
    assert len(big) == 65801 and 100 < len(sp.sizes(c.read('hits/65801'), 64)) < 200 and sp.sizes(c.read('hits/65801'), 64)[0] == 768 and len(set(sp.sizes(c.read('hits/65801'), 64))) >= 8


def test_oracle_map_is_spec(cases, oracle):
    build, cs = cases
    n = 0
    for c in cs:
        if build != BUILD_NAMES[0] and c.family != 'sizes':
            continue                                                        # (the other families are the same objects for both builds)
        sp = S.spec_of(c)
        oi = oracle.Index.from_seqs(['c%d' % i for i in range(len(c.contigs))], c.contigs, k=c.k, w=c.w)
        assert oi.mid_occ == R.default_mid_occ(sp.IH), c.label
        oh, op = oi.minimizers()
        assert np.array_equal(oh, sp.IH) and np.array_equal(op, sp.IP), c.label
        for cn, mo in c.params:
            for i in S.reads_for(c, cn, mo):
                S.same(oi.map(c.reads[i].seq, cn, mo), sp.rows(i, cn, mo), c, c.reads[i], cn, mo, 'oracle'); n += 1
    assert n > (800 if build == BUILD_NAMES[0] else 80)
