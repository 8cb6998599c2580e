"""The host PAF emitter (vm_paf_emit, through the emulator build's library: host code only) against the Python statement of the rule
(vacmap_amd/paf.py) on every case, every line through the independent parser, and against the SAM emitter's lines through
paf_codec.paf_from_sam_line where the records' clips agree with q_st / q_en. CPU only."""
import json, os
import numpy as np
import pytest
import paf_cases as P
import paf_codec as PC
import sam_cases as SC
import test_sam as TS

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
OWN, SAM, BULK = P.all_cases()
ALL = [c for c in OWN + SAM + BULK if not c.err]


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, P.Indexes(VL, ctx)


@pytest.mark.parametrize('case', ALL, ids=repr)
def test_host_emitter_matches_python_rule(env, case):
    VL, ctx, ix = env
    got = P.run_host(VL, ctx, ix.of(case), case)
    P.differ(case.name, P.python_expected(case), got, 'vm_paf_emit against paf.paf_lines')
    assert P.run_host(VL, ctx, ix.of(case), case, nthreads=1) == got


@pytest.mark.parametrize('case', ALL, ids=repr)
def test_lines_parse_and_follow_the_sam_lines(env, case):
    """a PAF line exists where a SAM record line does; where the codec's precondition holds it is that line's PAF form"""
    VL, ctx, ix = env
    paf = P.run_host(VL, ctx, ix.of(case), case)
    sam = P.run_sam_host(VL, ctx, ix.of(case), case)
    n = P.check_codec(case, paf, sam)
    if case.name.startswith('bulk_'):
        assert n >= 600


def test_cases_hold_the_shapes_they_name(env):
    VL, ctx, ix = env
    by = {c.name: c for c in OWN}
    text = {c.name: P.run_host(VL, ctx, ix.of(c), c)[0].decode() for c in OWN if not c.err}
    rd = {r.name: r for r in by['clips'].reads}
    for want in (62, 63, 64):
        assert rd['leadclip%d' % want].recs[0].cigar[want] in 'SH'
    assert len(''.join('1' + o for _, o in P.alternating(70))) == 70 and rd['runs70'].recs[0].cigar.startswith('1S1H') and rd['runs70'].recs[0].cigar.endswith('9=' + '1H1S' * 17 + '1H')
    lines = {x.split('\t')[0]: x for x in text['clips'].split('\n')[:-1]}
    assert lines['runs70'].endswith('\tcg:Z:20=1X9=') and lines['leadclip64'].endswith('\tcg:Z:20=1X9=') and 'cg:Z:' not in lines['onlyclips'] and 'cg:Z:' not in lines['onlyclips70']
    assert lines['interiorS'].endswith('\tcg:Z:10=3S10=') and lines['interiorH'].endswith('\tcg:Z:10=3H10=') and lines['noclips'].endswith('\tcg:Z:20=1X9=')
    al = {x.split('\t')[0]: x.split('\t') for x in text['alen'].split('\n')[:-1]}
    assert [al['only' + o][10] for o in 'M=XID'] == ['5'] * 5 and al['withN'][10] == '11' and al['join'][10] == '10' and al['join'][-1] == 'cg:Z:10='
    assert al['joinclip'][-1] == 'cg:Z:10=' and al['M130'][9:11] == ['125', '130'] and al['onlyX'][9] == '0' and al['big'][10] == '1234570'
    nu = {x.split('\t')[0]: x.split('\t') for x in text['numbers'].split('\n')[:-1]}
    assert nu['neg_qs'][2] == '-9' and nu['neg_qs+'][2] == '-12' and nu['r_st_2^40'][7:9] == [str(1 << 40), str((1 << 40) + 10)] and nu['r_neg'][7:9] == ['-7', '-3']
    na = [x.split('\t') for x in text['names'].split('\n')[:-1]]
    assert na[0][0] == '' and sorted(set(x[5] for x in na)) == sorted(P.NAMES4) and len(na) == 9
    assert text['recs70'].count('\n') == 71 and text['keep_norecs'] == 'u1\t4\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n\t2\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\nu3\t0\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n'
    assert text['norecs'] == '' and text['keep_empty'] == ''
    for k in range(4):
        kept = P.run_host(VL, ctx, ix.of(by['keep_mixed%d' % k]), by['keep_mixed%d' % k]); plain = P.run_host(VL, ctx, ix.of(by['mixed%d' % k]), by['mixed%d' % k])
        assert kept[2] == plain[2] + 4 and kept[3] == plain[3] == 3 and plain[1][3] == plain[1][4] == plain[1][5]
        assert [x.split('\t')[4] for x in kept[0].decode().split('\n')[:-1]] == ['+', '*', '+', '*', '*', '-', '*']


def test_asm_rule_and_ignored_options(env):
    """asm_mode: MAPQ 60 / 1 and the X / D / I NM; hardclip, fakecigar, cigar2cg and rg_id change no byte"""
    VL, ctx, ix = env
    by = {c.name: c for c in OWN}
    idx = ix.of(by['alen'])
    a = [x.split('\t') for x in P.run_host(VL, ctx, idx, by['alen_asm'])[0].decode().split('\n')[:-1]]
    assert all(x[11] == '60' for x in a) and [x for x in a if x[0] == 'M130'][0][9:11] == ['130', '130']
    zero = P.Case('mq0', by['alen'].reads[:2], asm_mode=1)
    for r in zero.reads:
        r.recs[0].mapq = 0
    try:
        assert [x.split('\t')[11] for x in P.run_host(VL, ctx, idx, zero)[0].decode().split('\n')[:-1]] == ['1', '1']
    finally:
        for r in zero.reads:
            r.recs[0].mapq = 60
    assert P.run_host(VL, ctx, idx, by['clips_opts']) == P.run_host(VL, ctx, idx, by['clips'])


def test_reference_inputs_as_paf(env, golden, oracle):
    """the inputs of tests/golden/sam.json (the path goldens' records, regenerated as test_sam_device_emu.py regenerates them): vm_paf_emit gives
    paf.paf_lines' lines, raises where the reference's SAM emitter raised, and every line is the PAF form of vm_sam_emit's line"""
    import kernel_cases as KC
    from vacmap_amd import paf
    VL, ctx, _ = env
    meta, arrays = golden
    entries = json.load(open(os.path.join(GOLD, 'sam.json')))
    idx = {}
    nlines = nraised = 0
    for e in entries:
        cid, o = e['case'], e['opt']
        if 'comments' in o:
            continue
        if cid not in idx:
            idx[cid] = KC._case_index(ctx, oracle, meta, arrays, cid)[0]
        recs, query, qual, contigs = SC.inputs(e, meta, arrays)
        names = meta[cid]['names']
        raw = TS._raw_from_tuples(VL, recs, names)
        opts = VL.SamOpts(int(o['md']), int(o['shortcs']), int(o['cigar2cg']), int(o['markunbalancetra']), int(o['H']), int(o['fakecigar']), o['rg'].encode() if 'rg' in o else None)
        nm = recs[0][0].encode()
        a = (np.frombuffer(nm, np.uint8), [0, len(nm)], np.frombuffer(query.encode(), np.uint8), [0, len(query)], raw)
        buf, off, nl, ns = VL.paf_emit(ctx.lib, idx[cid], opts, *a, nthreads=2)
        lines = buf.tobytes().decode().split('\n')[:-1] if len(buf) else []
        if e['raised']:
            assert ns == 1 and not lines and nl == 0, (cid, e['read'], o)
            nraised += 1
            continue
        exp = paf.paf_lines(recs, query, lambda c, x, y: contigs[c][max(x, 0):max(y, 0)], lambda c: len(contigs[c]), md=bool(o['md']), shortcs=bool(o['shortcs']),
                            markunbalancetra=bool(o['markunbalancetra']))
        assert lines == exp and nl == len(lines) and ns == 0 and off.tolist() == [0, len(buf)], (cid, e['read'], o)
        sbuf = VL.sam_emit(ctx.lib, idx[cid], opts, *a, nthreads=2)[0]
        sl = sbuf.tobytes().decode().split('\n')[:-1]
        assert len(sl) == len(lines)
        clen = {n: len(contigs[n]) for n in names}
        for x, y in zip(lines, sl):
            PC.parse(x)
            assert x == PC.paf_from_sam_line(y, len(query), clen), (cid, e['read'], o)
        nlines += len(lines)
    assert nraised >= 10 and nlines >= 100
