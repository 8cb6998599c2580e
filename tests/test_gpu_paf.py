"""The device PAF emitter on the MI355X: the cases of paf_cases against vm_paf_emit of the same library, the bulk set also against the emulator
build's bytes, aligned synthetic reads through both emitters with every line checked against the SAM emitter's line, and the driver's -o x.paf."""
import numpy as np
import pytest
import paf_cases as P
import paf_codec as PC
import sam_device_cases as SD

pytestmark = pytest.mark.gpu

OWN, SAM, BULK = P.all_cases()


@pytest.fixture(scope='module')
def env():
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    yield VL, ctx, P.Indexes(VL, ctx)
    ctx.close()


@pytest.mark.parametrize('case', OWN + SAM, ids=repr)
def test_gpu_case_matches_host_emitter(env, case):
    VL, ctx, ix = env
    P.check_device(VL, ctx, ix.of(case), case)


_EMU = []


def _emu():
    if not _EMU:
        import emu_lib
        from vacmap_amd import lib as VL
        ectx = emu_lib.context()
        _EMU.append((ectx, P.Indexes(VL, ectx)))
    return _EMU[0]


@pytest.mark.parametrize('case', BULK + [c for c in OWN if c.name in ('clips', 'names_md', 'keep_mixed3')], ids=repr)
def test_gpu_bulk_matches_host_emitter_and_emulator(env, case):
    """300 reads in one call: more waves than a workgroup, more workgroups than a scan block; the device's bytes are the emulator build's"""
    VL, ctx, ix = env
    got = P.check_device(VL, ctx, ix.of(case), case)
    if case.name.startswith('bulk_'):
        assert got[2] >= 600 and got[3] >= 7
    ectx, eix = _emu()
    assert P.run_device(VL, ectx, eix.of(case), case) == got


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
def test_gpu_aligned_reads_through_both_emitters(env, aligned, opts):
    VL, ctx, _ = env
    names, contigs, reads = aligned
    idx = VL.Index.from_seqs(ctx, names, contigs, k=15, w=10)
    opts = dict(opts)
    prm = ctx.lib.params('H', eqx=opts.pop('eqx', 0))
    nb, no = SD.pack(VL, SD.Case('n', [SD.Read(n, s, []) for n, s in reads]))[:2]
    sb = np.frombuffer(''.join(s for _, s in reads).encode(), np.uint8)
    so = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
    raw = VL.align_batch_raw(ctx, idx, prm, sb, so)
    o = P.opts(VL, opts)
    ht, hoff, hl, hs = VL.paf_emit(ctx.lib, idx, o, nb, no, sb, so, raw, nthreads=4)
    dt, doff, dl, ds = VL.paf_emit_device(ctx, idx, o, nb, no, sb, so, raw)
    st, soff, sl, ss = VL.sam_emit(ctx.lib, idx, o, nb, no, sb, so, raw, nthreads=4)
    raw.close()
    idx.close()
    assert hl >= 200 and (dl, ds) == (hl, hs) == (sl, ss) and doff.tolist() == hoff.tolist()
    assert dt.tobytes() == ht.tobytes()
    clen = {n: len(c) for n, c in zip(names, contigs)}; qlen = dict((n, len(s)) for n, s in reads)
    pl = dt.tobytes().decode().split('\n')[:-1]; sam = st.tobytes().decode().split('\n')[:-1]
    assert len(pl) == len(sam) == hl
    for a, b in zip(pl, sam):
        PC.parse(a)
        assert a == PC.paf_from_sam_line(b, qlen[b.split('\t')[0]], clen), (a[:300], b[:300])
    assert sum(x.split('\t')[4] == '*' for x in pl) == sum(int(x.split('\t')[1]) & 4 != 0 for x in sam)


def test_gpu_driver_writes_paf(aligned, tmp_path, capfd):
    """driver.main with -o x.paf under --sam-emitter host and device writes the same file, one line per record line of the .sam run"""
    from vacmap_amd import driver
    names, contigs, reads = aligned
    ref = tmp_path / 'ref.fa'; fq = tmp_path / 'reads.fq'
    with open(ref, 'w') as f:
        for n, s in zip(names, contigs):
            f.write('>%s\n%s\n' % (n, s))
    with open(fq, 'w') as f:
        for i, (n, s) in enumerate(reads):
            f.write('@%s XC:Z:c%d\n%s\n+\n%s\n' % (n, i, s, 'I' * len(s)))
    common = ['-ref', str(ref), '-read', str(fq), '-mode', 'H', '-t', '4', '--nowriteindex', '--batch-reads', '64', '--eqx', '--MD', '--keep-unmapped']
    out = {}
    for tag, extra in (('host.paf', ['--sam-emitter', 'host']), ('device.paf', ['--sam-emitter', 'device']), ('host.sam', ['--sam-emitter', 'host'])):
        capfd.readouterr()
        assert driver.main(common + extra + ['-o', str(tmp_path / tag)]) == 0
        out[tag] = (open(tmp_path / tag).read().split('\n')[:-1], capfd.readouterr().err)
    sam = [x for x in out['host.sam'][0] if not x.startswith('@')]
    assert len(out['host.paf'][0]) > 200 and out['device.paf'][0] == out['host.paf'][0] and len(sam) == len(out['host.paf'][0])
    assert 'host SAM emitter' not in out['device.paf'][1] and ' PAF lines' in out['device.paf'][1]
    clen = {n: len(c) for n, c in zip(names, contigs)}; qlen = dict((n, len(s)) for n, s in reads)
    assert [PC.paf_from_sam_line(x, qlen[x.split('\t')[0]], clen) for x in sam] == out['host.paf'][0]
