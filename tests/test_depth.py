"""Depth of coverage, host side (vm_depth_add and the host texts, through the emulator build's library: host code only): every case of depth_cases
against the Python statement of the rule (vacmap_amd/depth.py) and against depth_codec applied to vm_sam_emit's lines of the same batch — counts,
win_off and both texts byte for byte; the shapes the cases name; accumulation, merge and the refusals of create. CPU only."""
import numpy as np
import pytest
import depth_cases as D
import depth_codec as DC
import sam_device_cases as SD

OWN, SAM, BULK = D.cases(), D.sam_cases(), D.bulk_cases()
ALL = [c for c in OWN + SAM + BULK if not c.err]
assert len(set(c.name for c in ALL)) == len(ALL)


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.fixture(scope='module')
def host(env):
    """vm_depth_add's result per case, computed once and left unchanged"""
    VL, ctx, idx = env
    return {c.name: D.run_host(VL, ctx, idx, c) for c in ALL}


@pytest.mark.parametrize('case', ALL, ids=repr)
def test_host_matches_python_rule_and_codec(env, host, case):
    VL, ctx, idx = env
    got = host[case.name]
    D.differ(case.name, D.python_expected(case), got, 'vm_depth_add against depth.py')
    D.differ(case.name, D.codec_expected(VL, ctx, idx, case), got, 'vm_depth_add against the codec on vm_sam_emit\'s lines')
    if case in BULK or case.name.startswith('edges'):
        assert D.run_host(VL, ctx, idx, case, nthreads=1) == got
    if case in BULK:
        assert got[4] >= 600 and got[5] >= 7 and sum(got[0]) > 50000


def test_cases_hold_the_shapes_they_name(host):
    w64 = dict(zip(range(10 ** 6), host['edges_w64'][0]))
    rd = {r.name: r.recs[0] for r in D.edge_reads(np.random.default_rng(20250))}
    assert (rd['end_before'].r_en, rd['end_on'].r_en, rd['end_past'].r_en) == (127, 128, 129) and rd['start_on'].r_st == 128 and rd['long5000M'].cigar == '5000M'
    assert rd['interior70'].r_en - rd['interior70'].r_st > 64 * 66        # more interior windows than the wave has lanes
    # window 1 = [64, 128): three runs from 70 (57, 58, 58 bases), the whole window, two runs from 60, 5000M
    assert w64[1] == 57 + 58 + 58 + 64 + 64 + 64 + 64 and w64[0] == 4 + 4 + 61 + 45      # ... and neg_start's 45 bases from 0
    assert host['edges_w7'][1] == [0, 858, 858 + 572] and host['edges_w7'][2].split(b'\n')[857] == b'ctgA\t5999\t6000\t1.00'
    assert host['edges_w500'][1] == [0, 12, 20] and host['edges_w8192'][1] == [0, 1, 2] and host['edges_w1'][1] == [0, 6000, 10000]
    assert host['edges_w6000'][2].startswith(b'ctgA\t0\t6000\t') and b'chrB_long_name\t0\t4000\t' in host['edges_w6000'][2]
    g = host['gaps_w64'][0]
    # D_boundary 10 + ISH 28 + zero_ops 2; ISH 2 + 30 + 30 + 2, D_first 5, zero_ops 3 + 3; ISH 8: D_windows' [60, 260) adds nothing to windows 1 .. 3
    assert g[1:4] == [40, 75, 8]
    c1 = host['gaps_w64'][1][1]
    assert host['gaps_w64'][0][c1 + 1:c1 + 4] == [0, 0, 0] and host['gaps_w64'][0][c1] == 10 and host['gaps_w64'][0][c1 + 4] == 11      # N_windows: [60, 260) of contig 1 is empty
    st = {r.name: r.recs[0].cigar for r in D.step_reads(np.random.default_rng(1))}
    assert st['alt2000'].count('=') == 1000 and st['alt2000'].count('X') == 1000 and st['straddle'][60:64] == '1234' and [st['opbyte%d' % k].index('D') for k in (62, 63, 64, 65)] == [62, 63, 64, 65]
    assert host['pieces_split'][:4] == host['pieces_merged'][:4] and sum(host['pieces_split'][0]) == 700 + 1 + 650 + 300 + 65 + 70
    assert host['overlaps_opts'] == host['overlaps_plain'] and host['edges_md_w64'] == host['edges_w64']       # hardclip, fakecigar, cigar2cg, rg, md and shortcs change nothing
    # MAPQ exactly Q counts, Q - 1 does not
    assert [sum(host[n][0]) for n in ('mapq_q0', 'mapq_q30', 'mapq_q31', 'mapq_q255')] == [1000, 600, 400, 200]
    assert sum(host['mark_on_q30'][0]) < sum(host['mark_off_q30'][0]) == sum(host['mark_on_q0'][0]) > 0        # reassign_mapq takes records below the threshold
    assert sum(host['asm_q60'][0]) == sum(host['asm_q2'][0]) > 0 and sum(host['asm_q1'][0]) > sum(host['asm_q60'][0]) and sum(host['asm_q61'][0]) == 0
    for k in range(6):                                     # a status, no records, a raising read between reads that count: only the three good reads add
        assert sum(host['nothing%d' % k][0]) == 3 * 120 and host['nothing%d' % k][5] == 3 and host['nothing%d_keep' % k][:4] == host['nothing%d' % k][:4]
        assert host['nothing%d_keep' % k][4] == host['nothing%d' % k][4] + 4
    assert sum(host['no_reads'][0]) == 0 and host['no_reads'][2].count(b'\t0.00\n') == 94 + 63
    t = host['text_w200'][2].split(b'\n')
    assert t[1] == b'ctgA\t200\t400\t0.01' and t[0] == b'ctgA\t0\t200\t0.00' and t[5] == b'ctgA\t1000\t1200\t12.00' and t[10] == b'ctgA\t2000\t2200\t120.00'
    assert host['text_w200'][3] == b'ctgA\t6000\t26401\t4.40\nchrB_long_name\t4000\t0\t0.00\ntotal\t10000\t26401\t2.64\n'


def test_mean_rounds_half_up_from_integers():
    from vacmap_amd import depth
    assert [depth.mean_text(c, n) for c, n in ((1, 200), (1, 201), (0, 5), (5, 1), (1, 3), (2, 3), (12345, 100), (1, 0))] == ['0.01', '0.00', '0.00', '5.00', '0.33', '0.67', '123.45', '0.00']
    assert [DC._mean(c, n) for c, n in ((1, 200), (1, 201), (2, 3), (12345, 100), (3, 200))] == ['0.01', '0.00', '0.67', '123.45', '0.02']


def test_two_calls_accumulate_like_one(env, host):
    VL, ctx, idx = env
    case = next(c for c in BULK if c.name == 'bulk_default_w100')
    a = D.Case('a', case.reads[:131], window=100, **case.opts); b = D.Case('b', case.reads[131:], window=100, **case.opts)
    d = VL.Depth.create(idx, 100, 0, lib=ctx.lib)
    nl = ns = 0
    for part in (a, b):
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, part)
        x, y = d.add(idx, D.opts(VL, part.opts), names, name_off, seqs, seq_off, raw, nthreads=3)
        nl += x; ns += y
    assert D.result(d, nl, ns) == host[case.name]
    d.close()


def test_merge_host_accumulators_and_layout_mismatch(env, host):
    VL, ctx, idx = env
    ca, cb = (next(c for c in OWN if c.name == n) for n in ('edges_w64', 'gaps_w64'))
    acc = []
    for c in (ca, cb):
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, c)
        d = VL.Depth.create(idx, 64, 0, lib=ctx.lib)
        d.add(idx, D.opts(VL, c.opts), names, name_off, seqs, seq_off, raw)
        acc.append(d)
    acc[0].merge(acc[1])
    assert acc[0].counts()[0].tolist() == [x + y for x, y in zip(host['edges_w64'][0], host['gaps_w64'][0])] and acc[1].counts()[0].tolist() == host['gaps_w64'][0]
    acc[0].add_counts(acc[1].counts()[0])
    assert acc[0].counts()[0].tolist() == [x + 2 * y for x, y in zip(host['edges_w64'][0], host['gaps_w64'][0])]
    other_w = VL.Depth.create(idx, 100, 0, lib=ctx.lib)
    idx2 = VL.Index.from_seqs(ctx, SD.NAMES, [SD.REF[0][:5999], SD.REF[1]], k=15, w=10)
    other_len = VL.Depth.create(idx2, 64, 0, lib=ctx.lib)
    for bad in (other_w, other_len):
        with pytest.raises(VL.VmxError) as ei:
            acc[0].merge(bad)
        assert ei.value.code == -1
    with pytest.raises(VL.VmxError) as ei:
        acc[0].add_counts(np.zeros(3, np.int64))
    assert ei.value.code == -1
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, ca)
    with pytest.raises(VL.VmxError) as ei:                 # an accumulator adds only for the index it was made for
        other_len.add(idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -1
    for d in acc + [other_w, other_len]:
        d.close()
    idx2.close()


def test_create_refuses(env):
    VL, ctx, idx = env
    for window, q in ((0, 0), (-5, 0), (64, -1), (64, 256)):
        with pytest.raises(VL.VmxError) as ei:
            VL.Depth.create(idx, window, q, lib=ctx.lib)
        assert ei.value.code == -1
    d = VL.Depth.create(idx, 1, 255, lib=ctx.lib)
    assert d.counts()[1].tolist() == [0, 6000, 10000]
    d.close()


def test_window_cap():
    """more than 2^28 windows in all are refused: a reference of 2^28 + 1 bases at W = 1 (the index is not needed for the arithmetic: depth.py's layout)"""
    from vacmap_amd import depth
    assert depth.window_offsets([(1 << 28) + 1], 1)[-1] > 1 << 28 and depth.window_offsets([3_100_000_000], 500)[-1] == 6_200_000


def test_bad_records_are_refused_and_add_nothing(env):
    VL, ctx, idx = env
    rng = np.random.default_rng(2)
    case = D.Case('x', [SD.one(rng, 'a', [(40, '=')]), SD.one(rng, 'b', [(40, '=')])])
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, 64, 0, lib=ctx.lib)
    for field, value in (('read_idx', 2), ('read_idx', -1), ('contig', 2), ('contig', -1), ('cigar_len', -1)):
        old = getattr(raw.recs[1], field); setattr(raw.recs[1], field, value)
        with pytest.raises(VL.VmxError) as ei:
            d.add(idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
        assert ei.value.code == -1
        setattr(raw.recs[1], field, old)
    raw.recs[0].read_idx = 1; raw.recs[1].read_idx = 0                     # not ordered by read
    with pytest.raises(VL.VmxError) as ei:
        d.add(idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -1 and not d.counts()[0].any()
    d.close()
