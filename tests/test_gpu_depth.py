"""Depth of coverage on the MI355X: vm_depth_add_device and the device texts against vm_depth_add of the same library on every case of depth_cases,
the bulk set and three edge cases also against the emulator build's results, aligned synthetic reads accumulated through an attached context
against the host and the codec on the SAM emitter's lines, and the driver's --depth under both emitters."""
import numpy as np
import pytest
import depth_cases as D
import depth_codec as DC
import sam_device_cases as SD

pytestmark = pytest.mark.gpu

OWN, SAM, BULK = D.cases(), D.sam_cases(), D.bulk_cases()


@pytest.fixture(scope='module')
def env():
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    idx = SD.index(ctx)
    yield VL, ctx, idx
    idx.close()
    ctx.close()


@pytest.mark.parametrize('case', OWN + SAM, ids=repr)
def test_gpu_case_matches_host(env, case):
    VL, ctx, idx = env
    D.check_device(VL, ctx, idx, case)


_EMU = []


def _emu():
    if not _EMU:
        import emu_lib
        ectx = emu_lib.context()
        _EMU.append((ectx, SD.index(ectx)))
    return _EMU[0]


@pytest.mark.parametrize('case', BULK + [c for c in OWN if c.name in ('edges_w64', 'steps_w7', 'gaps_w1')], ids=repr)
def test_gpu_bulk_matches_host_and_emulator(env, case):
    """300 reads in one call: more waves than a workgroup holds; the device's counts and texts are the emulator build's"""
    VL, ctx, idx = env
    got = D.check_device(VL, ctx, idx, case)
    if case in BULK:
        assert got[4] >= 600 and got[5] >= 7 and sum(got[0]) > 50000
    ectx, eidx = _emu()
    assert D.run_device(VL, ectx, eidx, case) == got


def test_gpu_attached_calls_add_and_leave_the_bytes(env):
    VL, ctx, idx = env
    for case in (next(c for c in BULK if c.name == 'bulk_md_short_w100'), next(c for c in OWN if c.name == 'nothing4_keep')):
        alone = D.run_device(VL, ctx, idx, case)
        for paf in (False, True):
            plain = D.run_emit(VL, ctx, idx, case, paf=paf)
            got, emitted = D.run_attached(VL, ctx, idx, case, paf=paf)
            D.differ(case.name, alone, got, 'attached call against vm_depth_add_device')
            assert emitted == plain


@pytest.fixture(scope='module')
def aligned(env):
    """200 synthetic ONT-shape reads over a 1.5 Mb reference with three implanted SVs, and 3 reads of random bases (no record)"""
    from vacmap_amd import synth
    contigs = synth.make_reference([1200000, 300000], seed=5)
    donor = synth.implant_svs(contigs[0], [('INV', 400000, 4000), ('DEL', 800000, 900), ('DUP', 600000, 1500, 2)])
    reads = synth.sample_reads([donor, contigs[1]], 200, mean_len=4000, err=0.08, seed=6, min_len=800, max_len=12000)
    rng = np.random.default_rng(8)
    rand = [''.join('ACGT'[i] for i in rng.integers(0, 4, 900)) for _ in range(3)]
    return ['chr1', 'chr2'], [synth.tostr(c) for c in contigs], [('read%d' % i, synth.tostr(r[1])) for i, r in enumerate(reads)] + [('rand%d' % i, s) for i, s in enumerate(rand)]


@pytest.mark.parametrize('opts', [dict(), dict(md=1, shortcs=1, eqx=1), dict(md=1, eqx=1, hardclip=1, markunbalancetra=1, keep_unmapped=1)], ids=['default', 'eqx_md', 'eqx_mdlong_hard_keep'])
def test_gpu_aligned_reads_through_an_attached_context(env, aligned, opts):
    """the 203-read set in two emit calls (SAM, then PAF) on a context with an accumulator attached, at W = 100 and 500: the counts are the host's
    and the codec's from the SAM emitter's lines"""
    VL, ctx, _ = env
    names, contigs, reads = aligned
    idx = VL.Index.from_seqs(ctx, names, contigs, k=15, w=10)
    opts = dict(opts)
    prm = ctx.lib.params('H', eqx=opts.pop('eqx', 0))
    o = D.opts(VL, opts)
    half = len(reads) // 2
    parts = []
    for sub in (reads[:half], reads[half:]):
        nb, no = SD.pack(VL, SD.Case('n', [SD.Read(n, s, []) for n, s in sub]))[:2]
        sb = np.frombuffer(''.join(s for _, s in sub).encode(), np.uint8)
        so = np.concatenate([[0], np.cumsum([len(s) for _, s in sub])]).astype(np.int64)
        parts.append((nb, no, sb, so, VL.align_batch_raw(ctx, idx, prm, sb, so)))
    lens = [len(c) for c in contigs]
    sam = ''.join(VL.sam_emit(ctx.lib, idx, o, nb, no, sb, so, raw, nthreads=4)[0].tobytes().decode() for nb, no, sb, so, raw in parts)
    for window in (100, 500):
        dev = VL.Depth.create(idx, window, 0, ctx=ctx); host = VL.Depth.create(idx, window, 0, lib=ctx.lib)
        ctx.attach_depth(dev)
        nl = 0
        for k, (nb, no, sb, so, raw) in enumerate(parts):
            emit = VL.paf_emit_device if k else VL.sam_emit_device
            nl += emit(ctx, idx, o, nb, no, sb, so, raw)[2]
            host.add(idx, o, nb, no, sb, so, raw, nthreads=4)
        ctx.attach_depth(None)
        got = D.result(dev, 0, 0); exp = D.result(host, 0, 0)
        dev.close(); host.close()
        D.differ('aligned_w%d' % window, exp, got, 'attached device accumulator against vm_depth_add')
        counts, off, reg, summ, seen = DC.expected(sam, names, lens, window, 0)
        D.differ('aligned_w%d' % window, (counts, off, reg, summ, 0, 0), got, 'device against the codec on vm_sam_emit\'s lines')
        assert seen >= 200 and sum(got[0]) > 200 * 800 and int(got[3].split(b'\n')[-2].split(b'\t')[2]) == sum(got[0])
    for p in parts:
        p[4].close()
    idx.close()


def test_gpu_driver_writes_depth(aligned, tmp_path):
    """driver.main with --depth under --sam-emitter host and device writes the same two files, the codec's from the run's .sam record lines"""
    from vacmap_amd import driver
    names, contigs, reads = aligned
    ref = tmp_path / 'ref.fa'; fq = tmp_path / 'reads.fq'
    with open(ref, 'w') as f:
        for n, s in zip(names, contigs):
            f.write('>%s\n%s\n' % (n, s))
    with open(fq, 'w') as f:
        for n, s in reads:
            f.write('@%s\n%s\n+\n%s\n' % (n, s, 'I' * len(s)))
    common = ['-ref', str(ref), '-read', str(fq), '-mode', 'H', '-t', '4', '--nowriteindex', '--batch-reads', '64', '--eqx', '--keep-unmapped', '--depth-mapq', '5']
    out = {}
    for tag, extra in (('host', ['--sam-emitter', 'host']), ('device', ['--sam-emitter', 'device'])):
        assert driver.main(common + extra + ['-o', str(tmp_path / (tag + '.sam')), '--depth', str(tmp_path / tag)]) == 0
        out[tag] = (open(str(tmp_path / tag) + '.regions.bed', 'rb').read(), open(str(tmp_path / tag) + '.summary.txt', 'rb').read())
    assert out['host'] == out['device']
    _, _, reg, summ, seen = DC.expected(open(tmp_path / 'device.sam').read(), names, [len(c) for c in contigs], 500, 5)
    assert seen >= 200 and out['device'] == (reg, summ) and int(summ.split(b'\n')[-2].split(b'\t')[2]) > 200 * 800
