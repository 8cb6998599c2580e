"""The device SAM emitter (vm_sam_emit_device, k_sam.hip) on the CPU emulator build: every constructed case of sam_device_cases against vm_sam_emit
of the same library, the reference's own lines (tests/golden/sam.json, sam_asm.json) through the device path, and three cases against the pure-Python
emitter as a third witness. CPU only; the same cases run on the device in test_gpu_sam_device.py."""
import json, os
import numpy as np
import pytest
import sam_cases as SC
import sam_device_cases as SD
import test_sam as TS

GOLD = os.path.join(os.path.dirname(__file__), 'golden')
CASES = SD.cases()
BULK = SD.bulk_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.mark.parametrize('case', CASES + BULK, ids=repr)
def test_case_matches_host_emitter(env, case):
    VL, ctx, idx = env
    got = SD.check(VL, ctx, idx, case)
    if case.name.startswith(('raise_', 'mdraise_X_past', 'mdraise_X65')):
        # the read that raises emits nothing and is counted; its neighbours are the lines they are on their own
        assert got[3] == 1 and got[1][1] == got[1][2]
        for k in (0, 2):
            alone = SD.run_device(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts))
            assert got[0][got[1][k]:got[1][k + 1]] == alone[0]
    if case.name.startswith('bulk_'):
        assert got[2] >= 600 and got[3] >= 7


def test_cases_cover_what_they_claim():
    """the builders' own claims, checked on the texts they made"""
    by = {r.name: r for c in CASES for r in c.reads}
    for want in (62, 63, 64, 65):
        assert by['opbyte%d' % want].recs[0].cigar[want] == 'D'
    assert by['straddle'].recs[0].cigar[60:64] == '1234' and by['ops4097'].recs[0].cigar.count('=') + by['ops4097'].recs[0].cigar.count('X') > 2000
    assert len(by['recs70'].recs) == 70 and len(by['rep130D'].recs[0].cigar) > 260
    for k in (32767, 32768):
        import re
        assert len(re.findall(r'\d+\D', by['cg%d' % k].recs[0].cigar)) == k


def _emit_entry(VL, ctx, idx, recs, names, query, qual, o, asm=0, device=True):
    raw = TS._raw_from_tuples(VL, recs, names)
    opts = VL.SamOpts(int(o['md']), int(o['shortcs']), int(o['cigar2cg']), int(o['markunbalancetra']), int(o['H']), int(o['fakecigar']), o['rg'].encode() if 'rg' in o else None, asm)
    nm = recs[0][0].encode()
    a = (np.frombuffer(nm, np.uint8), [0, len(nm)], np.frombuffer(query.encode(), np.uint8), [0, len(query)], raw)
    kw = dict(quals=np.frombuffer(qual.encode(), np.uint8) if qual else None, qual_off=[0, len(qual)] if qual else None)
    if device:
        return VL.sam_emit_device(ctx, idx, opts, *a, **kw)
    return VL.sam_emit(ctx.lib, idx, opts, *a, nthreads=2, **kw)


def test_reference_lines_through_the_device_emitter(env, golden, oracle):
    """the 105 entries of sam.json without comments give the reference's lines; the 21 with comments, run without them, give vm_sam_emit's"""
    import kernel_cases as KC
    VL, ctx, _ = env
    meta, arrays = golden
    entries = json.load(open(os.path.join(GOLD, 'sam.json')))
    idx = {}
    nplain = ncom = nraised = nlines = 0
    for e in entries:
        cid, o = e['case'], e['opt']
        if cid not in idx:
            idx[cid] = KC._case_index(ctx, oracle, meta, arrays, cid)[0]
        recs, query, qual, contigs = SC.inputs(e, meta, arrays)
        buf, off, nl, ns = _emit_entry(VL, ctx, idx[cid], recs, meta[cid]['names'], query, qual, o)
        if 'comments' in o:
            hb, ho, hl, hs = _emit_entry(VL, ctx, idx[cid], recs, meta[cid]['names'], query, qual, o, device=False)
            assert (buf.tobytes(), off.tolist(), nl, ns) == (hb.tobytes(), ho.tolist(), hl, hs), (cid, e['read'], o)
            ncom += 1
            continue
        nplain += 1
        lines = buf.tobytes().decode().split('\n')[:-1] if len(buf) else []
        if e['raised']:
            assert ns == 1 and not lines and nl == 0, (cid, e['read'], o)
            nraised += 1
            continue
        assert [SC.head(x) for x in lines] == e['head'], (cid, e['read'], o)
        assert [SC.digest(x) for x in lines] == e['digest'], (cid, e['read'], o)
        assert nl == len(lines) and ns == 0 and off.tolist() == [0, len(buf)]
        nlines += len(lines)
    assert nplain == 105 and ncom == 21 and nraised >= 10 and nlines >= 100


def test_reference_asm_lines_through_the_device_emitter(env):
    VL, ctx, _ = env
    idx = {}
    nlines = 0
    for e, recs, query, contigs, c in TS._asm_sam_entries():
        cid, ci, o = e['case'], e['contig'], e['opt']
        if cid not in idx:
            idx[cid] = VL.Index.from_seqs(ctx, c['names'], [contigs[n] for n in c['names']], k=c['k'], w=c['w'])
        if 'comments' in o:
            got = _emit_entry(VL, ctx, idx[cid], recs, c['names'], query, None, o, asm=1)
            exp = _emit_entry(VL, ctx, idx[cid], recs, c['names'], query, None, o, asm=1, device=False)
            assert (got[0].tobytes(), got[1].tolist(), got[2], got[3]) == (exp[0].tobytes(), exp[1].tolist(), exp[2], exp[3]), (cid, ci, o)
            continue
        buf, off, nl, ns = _emit_entry(VL, ctx, idx[cid], recs, c['names'], query, None, o, asm=1)
        lines = buf.tobytes().decode().split('\n')[:-1] if len(buf) else []
        if e['raised']:
            assert ns == 1 and not lines, (cid, ci, o)
            continue
        assert [SC.head(x) for x in lines] == e['head'], (cid, ci, o)
        assert [SC.digest(x) for x in lines] == e['digest'], (cid, ci, o)
        nlines += len(lines)
    assert nlines >= 60


def test_reference_with_other_letters_is_unsupported(env):
    """an R in the index's host copy of the reference: vm_sam_emit prints it, the device codes hold N -> VM_ERR_UNSUPPORTED with a message"""
    VL, ctx, _ = env
    ref = [SD.REF[0][:500] + 'R' + SD.REF[0][501:], SD.REF[1]]
    idx = VL.Index.from_seqs(ctx, SD.NAMES, ref, k=15, w=10)
    case = SD.Case('r', [SD.one(np.random.default_rng(1), 'r', [(40, '=')], r_st=480)])
    with pytest.raises(VL.VmxError) as ei:
        SD.run_device(VL, ctx, idx, case)
    assert ei.value.code == -7 and 'ACGTN' in str(ei.value)
    assert b'\tNM:i:' in SD.run_host(VL, ctx, idx, case)[0]                 # the host emitter still serves it
    low = VL.Index.from_seqs(ctx, SD.NAMES, [SD.REF[0].lower(), SD.REF[1][:100] + 'n' + SD.REF[1][101:]], k=15, w=10)      # lower case and n are fine
    SD.check(VL, ctx, low, case)


def test_contig_names_follow_the_index_not_its_address(env):
    """the context keeps the contig-name blob of the index it last emitted for. An index that is closed hands its address to the next one, which has
    other names: the lines must carry the new names. (Indexes are made and closed until one lands on the first one's address; the lines are checked
    against the host emitter either way.)"""
    VL, ctx, _ = env
    case = SD.Case('addr', [SD.one(np.random.default_rng(3), 'r', [(40, '=')], r_st=480)])
    first = VL.Index.from_seqs(ctx, ['oldA', 'oldB'], SD.REF, k=15, w=10)
    assert b'\toldA\t' in SD.check(VL, ctx, first, case)[0]
    addr = first.h.value if hasattr(first.h, 'value') else first.h
    first.close()
    for i in range(8):
        nxt = VL.Index.from_seqs(ctx, ['new%dA' % i, 'new%dB' % i], SD.REF, k=15, w=10)
        same = (nxt.h.value if hasattr(nxt.h, 'value') else nxt.h) == addr
        text = SD.check(VL, ctx, nxt, case)[0]
        assert b'\tnew%dA\t' % i in text and b'oldA' not in text, (i, same)
        nxt.close()
        if same:
            break


def test_bad_records_are_refused(env):
    VL, ctx, idx = env
    rng = np.random.default_rng(2)
    a, b = SD.one(rng, 'a', [(40, '=')]), SD.one(rng, 'b', [(40, '=')])
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, SD.Case('x', [a, b]))
    for field, value in (('read_idx', 2), ('read_idx', -1), ('contig', 2), ('contig', -1), ('cigar_len', -1)):
        old = getattr(raw.recs[1], field); setattr(raw.recs[1], field, value)
        with pytest.raises(VL.VmxError) as ei:
            VL.sam_emit_device(ctx, idx, SD.sam_opts(VL, {}), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
        assert ei.value.code == -1
        setattr(raw.recs[1], field, old)
    raw.recs[0].read_idx = 1; raw.recs[1].read_idx = 0                     # not ordered by read
    with pytest.raises(VL.VmxError):
        VL.sam_emit_device(ctx, idx, SD.sam_opts(VL, {}), names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)


@pytest.mark.parametrize('name,opts', [('straddle', dict(md=True, shortcs=True)), ('rep65D', dict(md=True, shortcs=False)), ('md_DX+', dict(md=True, shortcs=True)),
                                       ('pieces', dict())])
def test_third_witness_python_emitter(env, name, opts):
    """the pure-Python emitter (vacmap_amd/sam.py, pinned to the reference line by line) on tokeniser and MD cases"""
    from vacmap_amd import sam
    VL, ctx, idx = env
    rd = {r.name: r for c in CASES for r in c.reads}[name]
    recs = [(rd.name, SD.NAMES[r.contig], r.strand, r.q_st, r.q_en, r.r_st, r.r_en, r.mapq, r.cigar) for r in rd.recs]
    exp = sam.sam_lines(recs, rd.seq, rd.qual, lambda c, a, b: SD.REF[SD.NAMES.index(c)][a:b], markunbalancetra=False, **opts)
    got = SD.run_device(VL, ctx, idx, SD.Case(name, [rd], md=int(opts.get('md', 0)), shortcs=int(opts.get('shortcs', 0))))
    assert got[0].decode().split('\n')[:-1] == exp


@pytest.fixture(scope='module')
def driver_inputs(tmp_path_factory):
    """a two-contig 70 kb reference, 8 reads of ~1.5 kb with FASTQ comments, and a 6 kb assembly contig"""
    from vacmap_amd import synth
    d = tmp_path_factory.mktemp('samdev')
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = d / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 8, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    fq = d / 'r.fq'
    fq.write_text(''.join('@q%d XC:Z:c%d\n%s\n+\n%s\n' % (i, i, cat[off[i]:off[i + 1]].tobytes().decode(), ''.join(chr(40 + (i + k) % 50) for k in range(int(off[i + 1] - off[i]))))
                          for i in range(8)))
    asm = d / 'asm.fa'
    piece = synth.implant_svs(contigs[0][10000:16000], [('DEL', 3000, 200)])
    asm.write_text('>tig1\n%s\n' % piece.tobytes().decode())
    return d, fa, fq, asm


def _lines(path):
    return [x for x in open(path).read().split('\n') if not x.startswith('@PG')]


def test_driver_sam_emitter_switch(env, driver_inputs, monkeypatch, capsys):
    """driver.main on the emulator build: --sam-emitter device writes the host emitter's file (read mode and -mode asm), its contexts are
    closed, and with --copycomments the host emitter serves the whole run and one stderr line says so"""
    from vacmap_amd import driver
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    d, fa, fq, asm = driver_inputs
    made = []
    init = VL.Context.__init__

    def init_recorded(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(VL.Context, '__init__', init_recorded)
    calls = {'device': 0}
    dev = VL.sam_emit_device

    def counted(*a, **kw):
        calls['device'] += 1
        return dev(*a, **kw)
    monkeypatch.setattr(VL, 'sam_emit_device', counted)
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '3', '--inflight', '2', '--eqx', '--MD']
    out = {}
    for tag, extra in (('host', []), ('device', ['--sam-emitter', 'device']), ('host_c', ['--copycomments']), ('device_c', ['--copycomments', '--sam-emitter', 'device'])):
        capsys.readouterr(); calls['device'] = 0; n_ctx = len(made)
        assert driver.main(common + extra + ['-o', str(d / (tag + '.sam'))]) == 0
        out[tag] = (_lines(d / (tag + '.sam')), capsys.readouterr().err, calls['device'], len(made) - n_ctx)
    assert all(c.h is None for c in made)
    assert len([x for x in out['host'][0] if x and not x.startswith('@')]) >= 8 and out['device'][0] == out['host'][0]
    assert out['host'][2] == 0 and out['device'][2] >= 3 + 2             # three batches, and the two emit contexts' sizing calls
    assert out['device'][3] == out['host'][3] + 2                        # VMX_EMIT_CONTEXTS contexts more, the aligners' as they were
    assert out['device_c'][0] == out['host_c'][0] != out['host'][0] and out['device_c'][2] == 0
    assert out['device_c'][1].count('--copycomments needs the host SAM emitter') == 1 and 'host SAM emitter' not in out['device'][1]
    # -mode asm honours the switch on the run's own context
    for tag, extra in (('asm_host', []), ('asm_device', ['--sam-emitter', 'device'])):
        calls['device'] = 0
        assert driver.main(['-ref', str(fa), '-read', str(asm), '-mode', 'asm', '-workdir', str(d / 'wd'), '-t', '2', '--nowriteindex', '-o', str(d / (tag + '.sam'))] + extra) == 0
        out[tag] = (_lines(d / (tag + '.sam')), calls['device'])
    assert out['asm_device'][0] == out['asm_host'][0] and out['asm_device'][1] == 1 and out['asm_host'][1] == 0
    assert any(x and not x.startswith('@') for x in out['asm_host'][0])


def test_driver_falls_back_when_the_reference_has_other_letters(env, driver_inputs, monkeypatch, capsys):
    from vacmap_amd import driver
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    d, fa, fq, _ = driver_inputs
    fa2 = d / 'ref_r.fa'
    text = fa.read_text()
    fa2.write_text(text[:2000] + 'R' + text[2001:])
    errs = {}
    # the host run; the device run (the sizing run meets the reference: no batch is tried on the device); the same without a sizing run (the first batch meets it)
    for tag, extra, nowarm in (('r_host', [], '1'), ('r_device', ['--sam-emitter', 'device'], '0'), ('r_device_nowarm', ['--sam-emitter', 'device'], '1')):
        monkeypatch.setenv('VMX_NO_WARM', nowarm)
        capsys.readouterr()
        assert driver.main(['-ref', str(fa2), '-read', str(fq), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '3', '--inflight', '2', '-o', str(d / (tag + '.sam'))] + extra) == 0
        errs[tag] = capsys.readouterr().err
    assert _lines(d / 'r_device.sam') == _lines(d / 'r_host.sam') == _lines(d / 'r_device_nowarm.sam')
    for tag in ('r_device', 'r_device_nowarm'):
        assert errs[tag].count('the host SAM emitter is used for the whole run') == 1 and 'ACGTN' in errs[tag]
    assert 'host SAM emitter' not in errs['r_host']


def test_fakecigar_cases_hold_the_shapes_they_name():
    """zero clips at both ends and all three signs of diff, in reads of more than one record (SA is where the approximate CIGAR is printed)"""
    ends, whole = [r for c in CASES if c.name == 'fake_clips' for r in c.reads]
    diffs = [(r.q_en - r.q_st) - (r.r_en - r.r_st) for r in ends.recs]
    assert diffs == [7, 0, -9] and ends.recs[0].q_st == 0 and ends.recs[-1].q_en == len(ends.seq)
    assert whole.recs[0].q_st == 0 and whole.recs[0].q_en == len(whole.seq) and len(whole.recs) == 2
