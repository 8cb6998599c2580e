"""The comment stage of the device SAM emitter (sam_comment in k_sam.hip, vm_sam_emit_device_comments, --sam-emitter device-comments) on the CPU
emulator build: every case of sam_comment_cases against vm_sam_emit of the same library and against the Python statement of the rule, the
reference's own commented lines (tests/golden/sam.json) through the device path, the argument errors, and the driver's third choice.
CPU only; the same cases run on the device in test_gpu_sam_comments.py."""
import json, os
import numpy as np
import pytest
import sam_cases as SC
import sam_comment_cases as CC
import sam_device_cases as SD
import test_sam as TS

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
CASES = CC.cases()
BULK = CC.bulk_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.mark.parametrize('case', CASES + BULK, ids=repr)
def test_case_matches_host_emitter_and_rule(env, case):
    VL, ctx, idx = env
    got = CC.check(VL, ctx, idx, case)
    if case.name.startswith('skip_'):
        # the failed / raising read emits nothing and is counted; its commented neighbours are the lines they are on their own
        assert got[3] == 1 and got[1][1] == got[1][2] and got[2] == 2
        for k in (0, 2):
            alone = CC.run_device(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts))
            assert got[0][got[1][k]:got[1][k + 1]] == alone[0] and alone[0].count(b'\tXG:i:') == 1


def test_cases_hold_the_shapes_they_name(env):
    """the builders' claims, checked on the comments they made and on the lines the emitter wrote for them"""
    VL, ctx, idx = env
    by = {r.name: r for c in CASES for r in c.reads}
    for at in (62, 63, 64, 65):
        assert by['tab%d' % at].comment[at] == 9 and by['tab%d' % at].comment.count(b'\t') == 1
    for end in (63, 64, 65):
        assert len(by['end%d' % end].comment) == end == len(by['end%d_second' % end].comment) and b'\t' not in by['end%d' % end].comment
    f = by['field10000'].comment.split(b'\t')
    assert len(f[1]) == 10000 and f[1].startswith(b'ML:B:C,') and len(by['field200'].comment.split(b'\t')[1]) == 200
    assert [CC.appended(by[n].comment, False, False) for n in ('len0', 'len1', 'len4', 'len5')] == [b'', b'', b'', b'\tXC:Z:']
    assert CC.appended(by['late_colon'].comment, False, False) == b'\tXE:i:1' == CC.appended(by['late_colon_last'].comment, False, False)
    for n in (64, 65, 130):
        kept = CC.appended(by['tags%d' % n].comment, False, False).split(b'\t')[1:]
        assert len(kept) == n + (1 if n == 130 else 0) and len(by['tags%d' % n].comment.split(b'\t')) == n + 3 + (4 if n == 130 else 0)
    assert CC.appended(by['tags130'].comment, False, False).endswith(b'\tzz:i:2')
    assert CC.appended(by['dup_bad_first'].comment, False, False) == b'\tXB:i:3\tXC:Z:'
    assert CC.appended(by['fixed'].comment, True, True) == b'\tXK:i:1' and CC.appended(by['fixed'].comment, False, False) == b'\tXK:i:1\tRG:Z:other\tCG:Z:mine'
    # CG: dropped only on the line that carries CG:Z:, kept on the read's other line and everywhere with cigar2cg 0
    on = CC.run_device(VL, ctx, idx, [c for c in CASES if c.name == 'cg_on'][0])[0].split(b'\n')[:-1]
    off = CC.run_device(VL, ctx, idx, [c for c in CASES if c.name == 'cg_off'][0])[0].split(b'\n')[:-1]
    assert len(on) == len(off) == 2
    assert sorted((b'\tCG:Z:1=' in x, x.endswith(b'\tXQ:i:1'), x.endswith(b'\tCG:Z:mine\tXQ:i:1')) for x in on) == [(False, True, True), (True, True, False)]
    assert all(x.endswith(b'\tCG:Z:mine\tXQ:i:1') and b'\tCG:Z:1=' not in x for x in off)
    # RG kept without rg_id, dropped with it
    lines = {c.name: CC.run_device(VL, ctx, idx, c)[0] for c in CASES if c.name in ('line_tags', 'line_tags_rg')}
    assert lines['line_tags'].count(b'\tRG:Z:other') == 2 and lines['line_tags_rg'].count(b'\tRG:Z:other') == 0 and lines['line_tags_rg'].count(b'\tRG:Z:grp\t') == 2
    # NUL and 0xFF travel unchanged
    shapes = CC.run_device(VL, ctx, idx, [c for c in CASES if c.name == 'shapes'][0])[0]
    assert b'\tXN:Z:a\x00b\xffc\tXO:Z:\xff\x00\tXP:i:\x80\n' in shapes and b'st:Z:' not in shapes


def test_com_off_may_begin_past_zero(env):
    """the blob is used from com_off[0] on: the text is the one of the blob that begins at its first comment"""
    VL, ctx, idx = env
    for name in ('lengths', 'mixed', 'duplicates'):
        case = [c for c in CASES if c.name == name][0]
        assert CC.check(VL, ctx, idx, case, lead=7) == CC.run_device(VL, ctx, idx, case)


def test_without_comments_the_call_is_the_old_one(env):
    VL, ctx, idx = env
    for name in ('lengths', 'records_hard', 'asm'):
        case = [c for c in CASES if c.name == name][0]
        none = CC.run_device(VL, ctx, idx, case, with_comments=False)
        assert none == SD.run_device(VL, ctx, idx, case) == CC.run_host(VL, ctx, idx, case, with_comments=False)
        assert none != CC.run_device(VL, ctx, idx, case)


def test_argument_errors(env):
    VL, ctx, idx = env
    case = [c for c in CASES if c.name == 'mixed'][0]
    (names, name_off, seqs, seq_off, quals, qual_off, raw), cb, co = CC.pack(VL, case)
    a = (ctx, idx, SD.sam_opts(VL, {}), names, name_off, seqs, seq_off, raw)
    bad = co.copy(); bad[2] = bad[1] - 1
    for kw in (dict(comments=cb, com_off=bad), dict(comments=None, com_off=co)):         # decreasing offsets; a null blob under a span of bytes
        with pytest.raises(VL.VmxError) as ei:
            VL.sam_emit_device(*a, quals=quals, qual_off=qual_off, **kw)
        assert ei.value.code == -1
    # a null blob under offsets that span nothing is no comment at all
    t = VL.sam_emit_device(*a, quals=quals, qual_off=qual_off, comments=None, com_off=np.zeros(len(co), np.int64))
    assert t[0].tobytes() == CC.run_device(VL, ctx, idx, case, with_comments=False)[0]
    with pytest.raises(TypeError):                                                        # keywords only
        VL.sam_emit_device(*a, quals, qual_off, cb, co)


def test_reference_commented_lines_through_the_device_emitter(env, golden, oracle):
    """the 21 entries of sam.json with comments, run through the device path with their comments, give the reference's lines"""
    import kernel_cases as KC
    VL, ctx, _ = env
    meta, arrays = golden
    idx = {}
    ncom = nlines = 0
    for e in json.load(open(os.path.join(GOLD, 'sam.json'))):
        cid, o = e['case'], e['opt']
        if 'comments' not in o:
            continue
        if cid not in idx:
            idx[cid] = KC._case_index(ctx, oracle, meta, arrays, cid)[0]
        recs, query, qual, contigs = SC.inputs(e, meta, arrays)
        raw = TS._raw_from_tuples(VL, recs, meta[cid]['names'])
        opts = VL.SamOpts(int(o['md']), int(o['shortcs']), int(o['cigar2cg']), int(o['markunbalancetra']), int(o['H']), int(o['fakecigar']), o['rg'].encode() if 'rg' in o else None)
        nm = recs[0][0].encode(); com = o['comments'].replace('\\t', '\t').encode()
        buf, off, nl, ns = VL.sam_emit_device(ctx, idx[cid], opts, np.frombuffer(nm, np.uint8), [0, len(nm)], np.frombuffer(query.encode(), np.uint8), [0, len(query)], raw,
                                              quals=np.frombuffer(qual.encode(), np.uint8) if qual else None, qual_off=[0, len(qual)] if qual else None,
                                              comments=np.frombuffer(com, np.uint8), com_off=[0, len(com)])
        ncom += 1
        lines = buf.tobytes().decode().split('\n')[:-1] if len(buf) else []
        if e['raised']:
            assert ns == 1 and not lines and nl == 0, (cid, e['read'], o)
            continue
        assert [SC.head(x) for x in lines] == e['head'], (cid, e['read'], o)
        assert [SC.digest(x) for x in lines] == e['digest'], (cid, e['read'], o)
        assert nl == len(lines) and ns == 0 and off.tolist() == [0, len(buf)]
        nlines += len(lines)
    assert ncom == 21 and nlines >= 21


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_copycomments_on_the_device(env, tmp_path, monkeypatch, capsys):
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    CC.check_driver_copycomments(VL, tmp_path, monkeypatch, capsys)


def test_driver_bam_tags_on_the_device(env, tmp_path, monkeypatch, capsys):
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    CC.check_driver_bam_tags(VL, tmp_path, monkeypatch, capsys)
