"""CPU test of the batched path's host decisions (vacmap_amd/csrc/vmx_batch_policy.h): pool geometry of the extend stage, the gap fill's band-width rule, the
per-read status, the splice of side batches and the result-size guess. tests/host/batch_policy_main.cpp is built with plain g++ under AddressSanitizer and
UBSan and run as a child process; every row it prints carries its inputs, and is compared here with a Python restatement of the rule. The asserts on the case
list itself (which inputs must be present) keep a case from being dropped on the C++ side without this file noticing."""
import json, os, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHORT, EXACT = -9001, -9002                      # VMX_EXT_SHORT_INTERNAL, VMX_EXT_EXACT_INTERNAL
RAISED, CAPACITY, UNSUPPORTED = -10, -20, -22    # VM_READ_*
EXT_CAPACITY_DEV, EXT_NEED_EXACT_DEV, READ_CAPACITY_DEV, READ_BANDFALL_DEV = -24, -25, -20, -23


@pytest.fixture(scope='module')
def out(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('batch_policy') / 'batch_policy')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-I', os.path.join(ROOT, 'vacmap_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host', 'batch_policy_main.cpp'), '-o', exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()[-2000:]
    return json.loads(p.stdout.decode())


# ---- pool geometry
def pool(bit, x, mul, tmask, tdiv):
    y = x * mul
    return max(y // tdiv, 1) if tmask & bit else y


def geometry(cl, ln, mul, tmask, tdiv):
    if cl <= 0:
        return [0, 0, 0, 0]
    return [pool(1, 3 * cl + 8, mul, tmask, tdiv), pool(2, cl + 2, mul, tmask, tdiv), (pool(4, 3 * ln + 64 * (cl // 2 + 2) + 56, mul, tmask, tdiv) + 7) // 8 * 8, cl + 2]


def test_pool_geometry(out):
    rows = out['geometry']
    for row in rows:
        assert row['out'] == geometry(*row['in']), row
        assert row['out'][2] % 8 == 0
    ins = [tuple(r['in']) for r in rows]
    assert any(i[0] == 0 for i in ins) and any(i[0] == 1 for i in ins)
    assert all(r['out'] == [0, 0, 0, 0] for r in rows if r['in'][0] == 0)
    for bit in (1, 2, 4):                        # every mask bit reaches the floor of 1 (the blob's 1 rounds up to 8) and leaves the other two pools alone
        r = [r for r in rows if r['in'][3] == bit and r['in'][4] >= 10 ** 9]
        assert r and all([x['out'][0] == 1, x['out'][1] == 1, x['out'][2] == 8].count(True) == 1 for x in r)
    sizes = {(3 * i[1] + 64 * (i[0] // 2 + 2) + 56) % 8 for i in ins if i[2] == 1 and i[3] == 0 and i[0] > 0}
    assert {0, 1, 7} <= sizes                    # the 8-byte rounding meets a size that is 0, 1 and 7 mod 8 ...
    assert {0, 1, 7} <= {i[1] % 8 for i in ins if i[0] == 5}      # ... and a read length that is
    for row in out['pool']:
        assert row['out'] == pool(*row['in']), row
    assert any(r['out'] == 1 for r in out['pool'] if r['in'][0] == 8) and any(r['out'] == 1 for r in out['pool'] if r['in'][0] == 16)


# ---- band-width rule
def vote(state, ad_cur, not_proven, problems):
    pct, floor, hold = state
    if problems < 2000 or ad_cur != pct:
        return [pct, floor, hold]
    f = not_proven / problems
    if f > 0.03 and pct < 100:
        pct = min(100, pct + 10); floor = pct; hold = 256
    elif hold > 0:
        hold -= 1
        if hold == 0:
            floor = 20
    elif f < 0.025 and pct > floor:
        pct = max(floor, pct - (20 if f < 0.01 else 10))
    return [pct, floor, hold]


def test_band_width_rule(out):
    assert out['start_pct'] == [90, 40, 90, 90, 90]          # mode L starts at 40
    for p, packed in out['packed']:
        assert packed == p | (max(20, p - 25) << 16)
    by_name = {}
    for case in out['rule']:
        state = case['start']
        for step in case['steps']:
            state = vote(state, *step['in'])
            assert step['out'] == state, (case['name'], step)
        by_name[case['name']] = [s['out'] for s in case['steps']]
    # the edges, by value: one vote on each side of 2000 problems and of f = 0.01, 0.025 and 0.03
    assert by_name['too few problems to vote'] == [[90, 20, 0]] * 2 and by_name['2000 problems vote'] == [[70, 20, 0]]
    assert by_name['f just below 0.01'] == [[70, 20, 0]] and by_name['f at 0.01'] == [[80, 20, 0]]
    assert by_name['f just below 0.025'] == [[80, 20, 0]] and by_name['f at 0.025'] == [[90, 20, 0]]
    assert by_name['f at 0.03'] == [[90, 20, 0]] and by_name['f just above 0.03'] == [[100, 100, 256]]
    assert by_name['a stale vote'] == [[90, 20, 0], [90, 20, 0], [70, 20, 0], [70, 20, 0]]
    assert by_name['up stops at 100'][0] == [100, 100, 256] and by_name['pinned at 100'] == [[100, 20, 0]] * 2
    assert by_name['at the floor'] == [[60, 60, 0]] and by_name['down stops at the floor'] == [[60, 60, 0], [60, 60, 0]] and by_name['down stops at 20'] == [[20, 20, 0]] * 2
    hold = by_name['the 256-batch hold']
    assert hold[0] == [60, 60, 256] and hold[255] == [60, 60, 1] and hold[256] == [60, 20, 0] and hold[257] == [40, 20, 0]


# ---- per-read status
def status(s):
    e = s['er_status']
    st = SHORT if e == EXT_CAPACITY_DEV else (EXACT if e == EXT_NEED_EXACT_DEV else e)
    if s['fast_local'] and e in (READ_CAPACITY_DEV, READ_BANDFALL_DEV):
        st = EXACT
    if st == 0 and not s['do_pass1'] and s['er_active'] and s['er_redo'] == 1 and s['er_pass'] == 1:
        st = EXACT
    if st == 0 and s['test_side_every'] > 0 and not s['force_exact'] and s['r'] % s['test_side_every'] == 0:
        st = EXACT
    if s['gmax'] == -2 and s['n_anchors'] > 2:
        st = RAISED
    if s['gmax'] == -4:
        st = UNSUPPORTED
    if s['asm_override'] != 0:
        st = s['asm_override']
    if s['rmode'] == 1 and s['n_anchors'] <= 2:
        st = RAISED
    return [st, int(st == 0 and s['er_nrec'] == 0)]


def test_read_status(out):
    rows = out['status']
    for row in rows:
        assert row['out'] == status(row['in']), row

    def find(**kw):
        base = dict(er_status=0, er_active=1, er_redo=0, er_pass=0, er_nrec=1, fast_local=0, do_pass1=0, force_exact=0, test_side_every=0, r=3, gmax=0, n_anchors=50, rmode=0, asm_override=0)
        base.update(kw)
        hit = [r['out'] for r in rows if r['in'] == base]
        assert len(hit) >= 1, kw
        return hit[0]
    assert find() == [0, 0] and find(er_nrec=0) == [0, 1] and find(er_status=RAISED, er_nrec=0) == [RAISED, 0]
    assert find(er_status=EXT_CAPACITY_DEV) == [SHORT, 0] and find(er_status=EXT_NEED_EXACT_DEV) == [EXACT, 0]
    for code in (READ_CAPACITY_DEV, READ_BANDFALL_DEV):      # the local stage's codes: run again only from the fast path
        assert find(er_status=code) == [code, 0] and find(er_status=code, fast_local=1) == [EXACT, 0]
    assert find(er_redo=1, er_pass=1) == [EXACT, 0] and find(er_redo=1, er_pass=1, do_pass1=1) == [0, 0] and find(er_redo=1, er_pass=1, er_status=RAISED) == [RAISED, 0]
    assert find(test_side_every=2, r=4) == [EXACT, 0] and find(test_side_every=2, r=3) == [0, 0] and find(test_side_every=2, r=4, force_exact=1) == [0, 0]
    # the order of the overrides: each later rule wins over the one before
    assert find(gmax=-2, n_anchors=3, test_side_every=1) == [RAISED, 0] and find(gmax=-2, n_anchors=2, test_side_every=1) == [EXACT, 0]
    assert find(gmax=-4, er_status=EXT_CAPACITY_DEV) == [UNSUPPORTED, 0]
    assert find(gmax=-4, asm_override=CAPACITY) == [CAPACITY, 0] and find(gmax=-2, n_anchors=3, asm_override=CAPACITY) == [CAPACITY, 0]
    assert find(rmode=1, n_anchors=2, asm_override=CAPACITY) == [RAISED, 0] and find(rmode=1, n_anchors=3, asm_override=CAPACITY) == [CAPACITY, 0]
    assert find(rmode=0, n_anchors=2) == [0, 0] and find(rmode=2, n_anchors=2) == [0, 0]


# ---- splice
def cigars(res):
    blob = bytes.fromhex(res['blob'])
    return [(r[0], r[1], r[2], blob[r[3]:r[3] + r[4]].decode(), blob[r[3] + r[4]]) for r in res['recs']]


def test_splice(out):
    names = [c['name'] for c in out['splice']]
    assert names == ['middle read again', 'side batch without records', 'two side rounds', 'given up']
    for case in out['splice']:
        n, st = case['n'], list(case['status_in'])
        again = set(case['rounds'][0]['sub'] if case['rounds'] else case['given_up'])
        want = [t for t in cigars(case['main']) if t[0] not in again]
        for rnd in case['rounds']:
            want += [(rnd['sub'][t[0]],) + t[1:] for t in cigars(rnd['res'])]
            for j, r in enumerate(rnd['sub']):
                st[r] = rnd['status'][j]
        for r in case['given_up']:
            st[r] = CAPACITY
        want.sort(key=lambda t: t[0])            # stable: a read's records keep their order
        got = cigars(case['out'])
        assert got == want and all(t[4] == 0 for t in got), case['name']      # read_idx, coordinates, and each cigar_off names its own NUL-terminated text
        recs = case['out']['recs']
        spans = sorted((r[3], r[3] + r[4] + 1) for r in recs)
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (not spans or spans[-1][1] <= len(bytes.fromhex(case['out']['blob']))), case['name']
        has = {t[0] for t in got}
        assert case['counters'] == {'n_records': len(got), 'aligned_bases': sum(t[2] - t[1] for t in got), 'cigar_bytes': sum(len(t[3]) for t in got),
                                    'n_failed': sum(1 for r in range(n) if st[r] != 0), 'n_unmapped': sum(1 for r in range(n) if st[r] == 0 and r not in has)}, case['name']
    c = {x['name']: x for x in out['splice']}
    assert [t[0] for t in cigars(c['middle read again']['out'])] == [0, 0, 1, 1, 2] and [t[3] for t in cigars(c['middle read again']['out'])] == ['10M', '5M2D3M', '4M', '6M1I', '3M1I3M']
    assert c['side batch without records']['counters']['n_unmapped'] == 2 and c['side batch without records']['counters']['n_failed'] == 1
    assert [t[3] for t in cigars(c['two side rounds']['out'])] == ['11M', '9M', '12M', '13M'] and [t[0] for t in cigars(c['two side rounds']['out'])] == [0, 2, 2, 2]
    assert c['given up']['counters'] == {'n_records': 1, 'aligned_bases': 10, 'cigar_bytes': 3, 'n_failed': 1, 'n_unmapped': 0}


def test_side_batch_statistics_add_exactly_the_listed_fields(out):
    st, st2, got = out['stats_add']['st'], out['stats_add']['st2'], out['stats_add']['out']
    want = dict(st)
    want['ms_total'] = st['ms_total'] + st2['ms_total']
    want['ms_stage'] = [a + b if i < 14 else a for i, (a, b) in enumerate(zip(st['ms_stage'], st2['ms_stage']))]
    for k in ('n_host_syncs', 'n_ed_tier2', 'n_ed_full', 'n_local_anchors', 'n_local_general'):
        want[k] = st[k] + st2[k]
    assert got == want
    assert all(st2[k] != 0 for k in ('n_dp_problems', 'dp_cells', 'n_dp_redo', 'ms_gapfill_fill', 'n_ed_tier1'))      # the fields that stay out had something to add


def test_result_size_guess(out):
    for row in out['guess']:
        rpr, bpb, n, bases, cS, cB = row['in']
        want = [min(cS, int(rpr * 2.0 * n) + 256), min(cB, int(bpb * 1.5 * bases) + 65536)] if rpr > 0.0 else [0, 0]
        assert row['out'] == want, row
    assert [0, 0] in [r['out'] for r in out['guess']] and any(r['out'][0] == r['in'][4] for r in out['guess']) and any(r['out'][1] == r['in'][5] for r in out['guess'])
    for row in out['learn']:
        rpr, bpb, nr, nb, n, bases = row['in']
        want = [max(rpr, nr / n), max(bpb, nb / bases)] if n > 0 and bases > 0 else [rpr, bpb]
        assert row['out'] == want, row
