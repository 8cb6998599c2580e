"""Depth of coverage on the CPU emulator build: vm_depth_add_device (k_depth.hip) and the device texts against vm_depth_add and the host texts of the
same library on every case of depth_cases; an accumulator attached to a context; accumulation over calls; merge of device and host accumulators;
refusals; the driver's --depth under both emitters. CPU only; the same cases run on the device in test_gpu_depth.py."""
import os
import numpy as np
import pytest
import depth_cases as D
import depth_codec as DC
import sam_device_cases as SD

OWN, SAM, BULK = D.cases(), D.sam_cases(), D.bulk_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.mark.parametrize('case', OWN + SAM + BULK, ids=repr)
def test_device_matches_host(env, case):
    VL, ctx, idx = env
    got = D.check_device(VL, ctx, idx, case)
    if case in BULK:
        assert got[4] >= 600 and got[5] >= 7 and sum(got[0]) > 50000


ATTACH = [c for c in OWN + BULK if c.name in ('edges_w64', 'gaps_w7', 'steps_w1', 'mark_on_q30', 'asm_q60', 'nothing1_keep', 'nothing4', 'text_w200', 'bulk_md_short_w100', 'bulk_w7_keep')]


@pytest.mark.parametrize('case', ATTACH, ids=repr)
def test_attached_accumulator_counts_and_leaves_the_bytes(env, case):
    """an emit call with an accumulator attached returns the bytes it returns unattached and adds what a stand-alone vm_depth_add_device adds"""
    VL, ctx, idx = env
    alone = D.run_device(VL, ctx, idx, case)
    for paf in (False, True):
        plain = D.run_emit(VL, ctx, idx, case, paf=paf)
        got, emitted = D.run_attached(VL, ctx, idx, case, paf=paf)
        D.differ(case.name, alone, got, 'attached %s call against vm_depth_add_device' % ('PAF' if paf else 'SAM'))
        assert emitted == plain and plain[2] == alone[4]


def test_sam_and_paf_calls_both_add_and_detaching_stops(env):
    VL, ctx, idx = env
    case = next(c for c in OWN if c.name == 'edges_w64')
    one = D.run_device(VL, ctx, idx, case)[0]
    names, name_off, seqs, seq_off, quals, qual_off, raw = SD.pack(VL, case)
    o = D.opts(VL, case.opts)
    d = VL.Depth.create(idx, 64, 0, ctx=ctx)
    ctx.attach_depth(d)
    VL.sam_emit_device(ctx, idx, o, names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
    VL.paf_emit_device(ctx, idx, o, names, name_off, seqs, seq_off, raw)
    assert d.counts()[0].tolist() == [2 * x for x in one]
    ctx.attach_depth(None)
    VL.sam_emit_device(ctx, idx, o, names, name_off, seqs, seq_off, raw, quals=quals, qual_off=qual_off)
    assert d.counts()[0].tolist() == [2 * x for x in one]
    ctx.attach_depth(d)
    bad = next(c for c in OWN if c.name == 'count_2^31')                  # a call that returns an error adds nothing
    bn = SD.pack(VL, bad)
    with pytest.raises(VL.VmxError):
        VL.paf_emit_device(ctx, idx, o, bn[0], bn[1], bn[2], bn[3], bn[6])
    assert d.counts()[0].tolist() == [2 * x for x in one]
    d.close()                                              # (closing detaches)
    VL.paf_emit_device(ctx, idx, o, names, name_off, seqs, seq_off, raw)
    host = VL.Depth.create(idx, 64, 0, lib=ctx.lib)        # only an accumulator made on the context attaches
    with pytest.raises(VL.VmxError) as ei:
        ctx.attach_depth(host)
    assert ei.value.code == -1
    with pytest.raises(VL.VmxError) as ei:
        host.add_device(ctx, idx, o, names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -1
    host.close()


def test_two_device_calls_accumulate_like_one(env):
    VL, ctx, idx = env
    case = next(c for c in BULK if c.name == 'bulk_default_w100')
    whole = D.run_device(VL, ctx, idx, case)
    d = VL.Depth.create(idx, 100, 0, ctx=ctx)
    nl = ns = 0
    for part in (D.Case('a', case.reads[:131], **case.opts), D.Case('b', case.reads[131:], **case.opts)):
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, part)
        x, y = d.add_device(ctx, idx, D.opts(VL, part.opts), names, name_off, seqs, seq_off, raw)
        nl += x; ns += y
    assert D.result(d, nl, ns) == whole
    d.close()


def test_merge_device_and_host(env):
    """the rank sum is a merge: device += host, host += device, device += device give the sums, texts included"""
    VL, ctx, idx = env
    ca, cb = (next(c for c in OWN if c.name == n) for n in ('edges_w64', 'gaps_w64'))
    a = D.run_host(VL, ctx, idx, ca); b = D.run_host(VL, ctx, idx, cb)
    both = D.run_host(VL, ctx, idx, D.Case('both', ca.reads + cb.reads, window=64))

    def made(case, on_device):
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
        d = VL.Depth.create(idx, 64, 0, ctx=ctx if on_device else None, lib=ctx.lib)
        (d.add_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw) if on_device else d.add(idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw))
        return d
    for dst_dev, src_dev in ((True, False), (False, True), (True, True)):
        x, y = made(ca, dst_dev), made(cb, src_dev)
        x.merge(y)
        assert D.result(x, 0, 0)[:4] == both[:4] and y.counts()[0].tolist() == b[0]
        x.add_counts(np.asarray(a[0], np.int64))
        assert x.counts()[0].tolist() == [2 * p + q for p, q in zip(a[0], b[0])]
        x.close(); y.close()
    x = made(ca, True); w = VL.Depth.create(idx, 100, 0, lib=ctx.lib)
    with pytest.raises(VL.VmxError) as ei:
        x.merge(w)
    assert ei.value.code == -1
    x.close(); w.close()


def test_bad_records_are_refused_and_add_nothing(env):
    VL, ctx, idx = env
    rng = np.random.default_rng(2)
    case = D.Case('x', [SD.one(rng, 'a', [(40, '=')]), SD.one(rng, 'b', [(40, '=')])])
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, 64, 0, ctx=ctx)
    for field, value in (('read_idx', 2), ('read_idx', -1), ('contig', 2), ('contig', -1), ('cigar_len', -1)):
        old = getattr(raw.recs[1], field); setattr(raw.recs[1], field, value)
        with pytest.raises(VL.VmxError) as ei:
            d.add_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
        assert ei.value.code == -1
        setattr(raw.recs[1], field, old)
    raw.recs[0].read_idx = 1; raw.recs[1].read_idx = 0                     # not ordered by read
    with pytest.raises(VL.VmxError) as ei:
        d.add_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -1 and not d.counts()[0].any()
    idx2 = VL.Index.from_seqs(ctx, SD.NAMES, [SD.REF[0][:5999], SD.REF[1]], k=15, w=10)       # an accumulator adds only for the index it was made for
    raw.recs[0].read_idx = 0; raw.recs[1].read_idx = 1
    with pytest.raises(VL.VmxError) as ei:
        d.add_device(ctx, idx2, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -1
    d.close(); idx2.close()


def test_reference_with_other_letters_is_unsupported(env):
    VL, ctx, _ = env
    ref = [SD.REF[0][:500] + 'R' + SD.REF[0][501:], SD.REF[1]]
    idx = VL.Index.from_seqs(ctx, SD.NAMES, ref, k=15, w=10)
    case = D.Case('r', [SD.one(np.random.default_rng(1), 'r', [(40, '=')], r_st=480)])
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    d = VL.Depth.create(idx, 64, 0, ctx=ctx)
    with pytest.raises(VL.VmxError) as ei:
        d.add_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert ei.value.code == -7 and not d.counts()[0].any()
    h = VL.Depth.create(idx, 64, 0, lib=ctx.lib)           # the host accumulator still serves it
    h.add(idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
    assert h.counts()[0].sum() == 40
    d.close(); h.close(); idx.close()


# ------------------------------------------------------------------------------------------------ the driver
@pytest.fixture(scope='module')
def driver_inputs(tmp_path_factory):
    """a two-contig 70 kb reference, 8 reads of ~1.5 kb plus one of random bases, and a 6 kb assembly contig"""
    from vacmap_amd import synth
    d = tmp_path_factory.mktemp('depthdev')
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = d / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 8, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    reads = [cat[off[i]:off[i + 1]].tobytes().decode() for i in range(8)] + [''.join('ACGT'[i] for i in np.random.default_rng(9).integers(0, 4, 700))]
    fq = d / 'r.fq'
    fq.write_text(''.join('@q%d\n%s\n+\n%s\n' % (i, s, 'I' * len(s)) for i, s in enumerate(reads)))
    asm = d / 'asm.fa'
    piece = synth.implant_svs(contigs[0][10000:16000], [('DEL', 3000, 200)])
    asm.write_text('>tig1\n%s\n' % piece.tobytes().decode())
    return d, fa, fq, asm


def _files(prefix):
    return open(str(prefix) + '.regions.bed', 'rb').read(), open(str(prefix) + '.summary.txt', 'rb').read()


def test_driver_writes_depth_under_both_emitters(env, driver_inputs, monkeypatch):
    """driver.main on the emulator build with --depth: --sam-emitter host and device, .sam and .paf outputs give equal files, which are the codec's
    from that run's .sam record lines; without --depth the .sam is byte-equal and no depth file exists; -mode asm too"""
    from vacmap_amd import driver
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    d, fa, fq, asm = driver_inputs
    names, lens = ['cA', 'cB'], [50000, 20000]
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '3', '--inflight', '2', '--eqx', '--keep-unmapped']
    out = {}
    for tag, extra in (('host.sam', []), ('device.sam', ['--sam-emitter', 'device']), ('host.paf', []), ('device.paf', ['--sam-emitter', 'device'])):
        assert driver.main(common + extra + ['-o', str(d / tag), '--depth', str(d / tag), '--depth-window', '100', '--depth-mapq', '1']) == 0
        out[tag] = _files(d / tag)
    assert out['host.sam'] == out['device.sam'] == out['host.paf'] == out['device.paf']
    sam = open(d / 'device.sam').read()
    _, _, reg, summ, n = DC.expected(sam, names, lens, 100, 1)
    assert n >= 8 and out['host.sam'] == (reg, summ) and int(summ.split(b'\n')[-2].split(b'\t')[2]) > 8 * 600
    assert driver.main(common + ['--sam-emitter', 'device', '-o', str(d / 'plain.sam')]) == 0
    body = lambda t: [x for x in t.split('\n') if not x.startswith('@PG')]      # (the @PG line holds the command line)
    assert body(open(d / 'plain.sam').read()) == body(sam) and not os.path.exists(str(d / 'plain.sam') + '.regions.bed') and not os.path.exists(str(d / 'plain.sam') + '.summary.txt')
    for tag, extra in (('asm_host.sam', []), ('asm_device.sam', ['--sam-emitter', 'device'])):
        assert driver.main(['-ref', str(fa), '-read', str(asm), '-mode', 'asm', '-workdir', str(d / 'wd'), '-t', '2', '--nowriteindex', '-o', str(d / tag), '--depth', str(d / tag)] + extra) == 0
        out[tag] = _files(d / tag)
    _, _, reg, summ, n = DC.expected(open(d / 'asm_host.sam').read(), names, lens, 500, 0)
    assert n >= 1 and out['asm_host.sam'] == out['asm_device.sam'] == (reg, summ) and int(summ.split(b'\n')[-2].split(b'\t')[2]) > 5000
    for bad in (['--depth-window', '0'], ['--depth-mapq', '256']):
        with pytest.raises(SystemExit) as ei:
            driver.main(common + ['-o', str(d / 'no.sam'), '--depth', str(d / 'no')] + bad)
        assert '--depth' in str(ei.value.code)


def test_driver_rank_sum_on_rank_zero(env, tmp_path, monkeypatch):
    """the driver's end of run with two ranks, the gather replaced by its result: rank 0 adds the other rank's table to its merged accumulators (one on
    the device, one on the host) and writes the files of the sum; the other rank writes nothing"""
    import types
    from vacmap_amd import driver, dist
    VL, ctx, idx = env
    ca, cb, cc = (next(c for c in D.cases() if c.name == n) for n in ('edges_w64', 'gaps_w64', 'overlaps_w64'))
    other = D.run_host(VL, ctx, idx, cc)[0]
    want = D.run_host(VL, ctx, idx, D.Case('all', ca.reads + cb.reads + cc.reads, window=64))
    for rank in (0, 1):
        args = types.SimpleNamespace(depth=str(tmp_path / ('r%d' % rank)), depth_window=64, depth_mapq=0)
        sink = driver.DepthSink(args, ctx.lib, idx)
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, ca)
        sink.attach(ctx)
        VL.paf_emit_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)
        names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, cb)
        sink.add_host(D.opts(VL, {}), names, name_off, seqs, seq_off, raw, 2)
        sent = []
        monkeypatch.setattr(dist, 'gather_lines', lambda mine, dst=0, group=None: (sent.append(mine), [mine, np.asarray(other, np.int64)] if rank == 0 else None)[1])
        sink.finish(types.SimpleNamespace(world=2, rank=rank, text_group=None))
        assert len(sent) == 1 and sent[0].tolist() == [x + y for x, y in zip(D.run_host(VL, ctx, idx, ca)[0], D.run_host(VL, ctx, idx, cb)[0])]
        if rank == 0:
            assert _files(tmp_path / 'r0') == (want[2], want[3])
        else:
            assert not os.path.exists(str(tmp_path / 'r1') + '.regions.bed')
    VL.paf_emit_device(ctx, idx, D.opts(VL, {}), names, name_off, seqs, seq_off, raw)       # finish() detached and closed the accumulator
