"""The device SAM emitter on the MI355X: the constructed cases of sam_device_cases against vm_sam_emit of the same library, the bulk set also
against the emulator build's bytes, aligned synthetic reads through both emitters, and the driver's --sam-emitter switch."""
import numpy as np
import pytest
import sam_device_cases as SD

pytestmark = pytest.mark.gpu

CASES = SD.cases()
BULK = SD.bulk_cases()


@pytest.fixture(scope='module')
def env():
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    yield VL, ctx, SD.index(ctx)
    ctx.close()


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_gpu_case_matches_host_emitter(env, case):
    VL, ctx, idx = env
    got = SD.check(VL, ctx, idx, case)
    if case.name.startswith(('raise_', 'mdraise_X_past', 'mdraise_X65')):
        assert got[3] == 1 and got[1][1] == got[1][2]
        for k in (0, 2):
            alone = SD.run_device(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts))
            assert got[0][got[1][k]:got[1][k + 1]] == alone[0]


@pytest.mark.parametrize('case', BULK, ids=repr)
def test_gpu_bulk_matches_host_emitter_and_emulator(env, case):
    """300 reads in one call: more waves than a workgroup, more workgroups than a scan block; the device's bytes are the emulator build's"""
    import emu_lib
    VL, ctx, idx = env
    got = SD.check(VL, ctx, idx, case)
    assert got[2] >= 600 and got[3] >= 7
    ectx = emu_lib.context()
    assert SD.run_device(VL, ectx, _emu_index(ectx), case) == got


_EMU_INDEX = []


def _emu_index(ectx):
    if not _EMU_INDEX:
        _EMU_INDEX.append(SD.index(ectx))
    return _EMU_INDEX[0]


@pytest.fixture(scope='module')
def aligned(env):
    """200 synthetic ONT-shape reads over a 1.5 Mb reference with two implanted SVs, their blobs and the reference"""
    from vacmap_amd import synth
    contigs = synth.make_reference([1200000, 300000], seed=5)
    donor = synth.implant_svs(contigs[0], [('INV', 400000, 4000), ('DEL', 800000, 900), ('DUP', 600000, 1500, 2)])
    reads = synth.sample_reads([donor, contigs[1]], 200, mean_len=4000, err=0.08, seed=6, min_len=800, max_len=12000)
    return ['chr1', 'chr2'], [synth.tostr(c) for c in contigs], [('read%d' % i, synth.tostr(r[1])) for i, r in enumerate(reads)]


@pytest.mark.parametrize('opts', [dict(), dict(md=1, shortcs=1, eqx=1), dict(md=1, eqx=1, hardclip=1, fakecigar=1, markunbalancetra=1, rg='g')], ids=['default', 'eqx_md', 'eqx_mdlong_hard'])
def test_gpu_aligned_reads_through_both_emitters(env, aligned, opts):
    VL, ctx, _ = env
    names, contigs, reads = aligned
    idx = VL.Index.from_seqs(ctx, names, contigs, k=15, w=10)
    opts = dict(opts)
    prm = ctx.lib.params('H', eqx=opts.pop('eqx', 0))
    nb, no = SD.pack(VL, SD.Case('n', [SD.Read(n, s, []) for n, s in reads]))[:2]
    sb = np.frombuffer(''.join(s for _, s in reads).encode(), np.uint8)
    so = np.concatenate([[0], np.cumsum([len(s) for _, s in reads])]).astype(np.int64)
    qb = np.frombuffer(bytes(33 + (i * 7) % 50 for i in range(len(sb))), np.uint8)
    raw = VL.align_batch_raw(ctx, idx, prm, sb, so)
    o = SD.sam_opts(VL, opts)
    ht, hoff, hl, hs = VL.sam_emit(ctx.lib, idx, o, nb, no, sb, so, raw, quals=qb, qual_off=so, nthreads=4)
    dt, doff, dl, ds = VL.sam_emit_device(ctx, idx, o, nb, no, sb, so, raw, quals=qb, qual_off=so)
    raw.close()
    assert hl >= 200 and (dl, ds) == (hl, hs) and doff.tolist() == hoff.tolist()
    assert dt.tobytes() == ht.tobytes()


def _body(path):
    lines = open(path).read().split('\n')
    return [x for x in lines if not x.startswith('@PG')]


def test_gpu_driver_sam_emitter_switch(aligned, tmp_path, capfd):
    """driver.main with --sam-emitter host and device writes the same file; with --copycomments the device switch falls back to the host
    emitter for the whole run and says so on stderr"""
    from vacmap_amd import driver
    names, contigs, reads = aligned
    ref = tmp_path / 'ref.fa'; fq = tmp_path / 'reads.fq'
    with open(ref, 'w') as f:
        for n, s in zip(names, contigs):
            f.write('>%s\n%s\n' % (n, s))
    with open(fq, 'w') as f:
        for i, (n, s) in enumerate(reads):
            f.write('@%s XC:Z:c%d\tXI:i:%d\n%s\n+\n%s\n' % (n, i, i, s, ''.join(chr(33 + (i + k) % 60) for k in range(len(s)))))
    common = ['-ref', str(ref), '-read', str(fq), '-mode', 'H', '-t', '4', '--nowriteindex', '--batch-reads', '64', '--eqx', '--MD']
    out = {}
    for tag, extra in (('host', ['--sam-emitter', 'host']), ('device', ['--sam-emitter', 'device']), ('host_c', ['--copycomments']),
                       ('device_c', ['--copycomments', '--sam-emitter', 'device'])):
        capfd.readouterr()
        assert driver.main(common + extra + ['-o', str(tmp_path / (tag + '.sam'))]) == 0
        out[tag] = (_body(tmp_path / (tag + '.sam')), capfd.readouterr().err)
    assert len(out['host'][0]) > 200 and out['device'][0] == out['host'][0]
    assert 'host SAM emitter' not in out['device'][1] and 'host SAM emitter' not in out['host'][1]
    assert out['device_c'][0] == out['host_c'][0] and out['host_c'][0] != out['host'][0]
    assert out['device_c'][1].count('--copycomments needs the host SAM emitter') == 1
