"""The device PAF emitter (vm_paf_emit_device, k_paf.hip) on the CPU emulator build: every case of paf_cases against vm_paf_emit of the same
library byte for byte, text_off, n_lines and n_skipped included; the refusals; the driver's -o x.paf under both emitters. CPU only; the same
cases run on the device in test_gpu_paf.py."""
import numpy as np
import pytest
import paf_cases as P
import sam_device_cases as SD

OWN, SAM, BULK = P.all_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, P.Indexes(VL, ctx)


@pytest.mark.parametrize('case', OWN + SAM + BULK, ids=repr)
def test_device_emitter_matches_host_emitter(env, case):
    VL, ctx, ix = env
    got = P.check_device(VL, ctx, ix.of(case), case)
    if case.name.startswith('bulk_'):
        assert got[2] >= 600 and got[3] >= 7


def test_sam_call_between_paf_calls_is_unchanged(env):
    """the two emitters share a context's buffers: a SAM call after a PAF call gives the SAM emitter's bytes, and the other way round"""
    VL, ctx, ix = env
    case = BULK[0]
    idx = ix.of(case)
    sam0 = SD.run_device(VL, ctx, idx, case)
    paf0 = P.run_device(VL, ctx, idx, case)
    assert SD.run_device(VL, ctx, idx, case) == sam0 == SD.run_host(VL, ctx, idx, case) and P.run_device(VL, ctx, idx, case) == paf0


def test_reference_with_other_letters_is_unsupported(env):
    VL, ctx, _ = env
    ref = [SD.REF[0][:500] + 'R' + SD.REF[0][501:], SD.REF[1]]
    idx = VL.Index.from_seqs(ctx, SD.NAMES, ref, k=15, w=10)
    case = P.Case('r', [SD.one(np.random.default_rng(1), 'r', [(40, '=')], r_st=480)])
    with pytest.raises(VL.VmxError) as ei:
        P.run_device(VL, ctx, idx, case)
    assert ei.value.code == -7 and 'ACGTN' in str(ei.value) and 'vm_paf_emit' in str(ei.value)
    assert b'\tNM:i:0\tcg:Z:40=\n' in P.run_host(VL, ctx, idx, case)[0]       # the host emitter still serves it


def test_bad_records_are_refused(env):
    VL, ctx, ix = env
    rng = np.random.default_rng(2)
    case = P.Case('x', [SD.one(rng, 'a', [(40, '=')]), SD.one(rng, 'b', [(40, '=')])])
    idx = ix.of(case)
    names, name_off, seqs, seq_off, _, _, raw = SD.pack(VL, case)
    for field, value in (('read_idx', 2), ('read_idx', -1), ('contig', 2), ('contig', -1), ('cigar_len', -1)):
        old = getattr(raw.recs[1], field); setattr(raw.recs[1], field, value)
        with pytest.raises(VL.VmxError) as ei:
            VL.paf_emit_device(ctx, idx, P.opts(VL, {}), names, name_off, seqs, seq_off, raw)
        assert ei.value.code == -1
        setattr(raw.recs[1], field, old)
    raw.recs[0].read_idx = 1; raw.recs[1].read_idx = 0                     # not ordered by read
    for emit in (lambda: VL.paf_emit_device(ctx, idx, P.opts(VL, {}), names, name_off, seqs, seq_off, raw),
                 lambda: VL.paf_emit(ctx.lib, idx, P.opts(VL, {}), names, name_off, seqs, seq_off, raw)):
        with pytest.raises(VL.VmxError) as ei:
            emit()
        assert ei.value.code == -1


@pytest.fixture(scope='module')
def driver_inputs(tmp_path_factory):
    """a two-contig 70 kb reference, 8 reads of ~1.5 kb plus one of random bases, and a 6 kb assembly contig"""
    from vacmap_amd import synth
    d = tmp_path_factory.mktemp('pafdev')
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = d / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, 8, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    reads = [cat[off[i]:off[i + 1]].tobytes().decode() for i in range(8)] + [''.join('ACGT'[i] for i in np.random.default_rng(9).integers(0, 4, 700))]
    fq = d / 'r.fq'
    fq.write_text(''.join('@q%d XC:Z:c%d\n%s\n+\n%s\n' % (i, i, s, 'I' * len(s)) for i, s in enumerate(reads)))
    asm = d / 'asm.fa'
    piece = synth.implant_svs(contigs[0][10000:16000], [('DEL', 3000, 200)])
    asm.write_text('>tig1\n%s\n' % piece.tobytes().decode())
    return d, fa, fq, asm, {'q%d' % i: len(s) for i, s in enumerate(reads)}


def test_driver_writes_paf_under_both_emitters(env, driver_inputs, monkeypatch, capsys):
    """driver.main on the emulator build: -o x.paf under --sam-emitter host and device gives equal files without a header, one line per record line
    of the same run's .sam, each the PAF form of that line; --keep-unmapped and -mode asm too; comment options are refused at the argument check"""
    import paf_codec as PC
    from vacmap_amd import driver
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    d, fa, fq, asm, qlen = driver_inputs
    calls = {'device': 0}
    dev = VL.paf_emit_device

    def counted(*a, **kw):
        calls['device'] += 1
        return dev(*a, **kw)
    monkeypatch.setattr(VL, 'paf_emit_device', counted)
    common = ['-ref', str(fa), '-read', str(fq), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '3', '--inflight', '2', '--eqx', '--MD']
    clen = {'cA': 50000, 'cB': 20000}
    for keep in (['--keep-unmapped'],):                  # (one read of random bases: record lines and an unmapped line in one run)
        out = {}
        for tag, extra in (('host.paf', []), ('device.paf', ['--sam-emitter', 'device']), ('host.sam', [])):
            calls['device'] = 0
            capsys.readouterr()
            assert driver.main(common + keep + extra + ['-o', str(d / tag)]) == 0
            out[tag] = (open(d / tag).read().split('\n')[:-1], calls['device'], capsys.readouterr().err)
        sam = [x for x in out['host.sam'][0] if not x.startswith('@')]
        assert out['host.paf'][0] == out['device.paf'][0] and len(sam) == len(out['host.paf'][0]) >= 8 + len(keep)
        assert out['host.paf'][1] == 0 and out['device.paf'][1] >= 3 and out['host.sam'][1] == 0
        assert [PC.paf_from_sam_line(x, qlen[x.split('\t')[0]], clen) for x in sam] == out['host.paf'][0]
        for x in out['host.paf'][0]:
            PC.parse(x)
        assert any(x.split('\t')[4] == '*' for x in out['host.paf'][0])
        assert ' PAF lines' in out['device.paf'][2] and ' SAM lines' in out['host.sam'][2] and 'host SAM emitter' not in out['device.paf'][2]
    for tag, extra in (('asm_host.paf', []), ('asm_device.paf', ['--sam-emitter', 'device']), ('asm.sam', [])):
        calls['device'] = 0
        assert driver.main(['-ref', str(fa), '-read', str(asm), '-mode', 'asm', '-workdir', str(d / 'wd'), '-t', '2', '--nowriteindex', '-o', str(d / tag)] + extra) == 0
        out[tag] = (open(d / tag).read().split('\n')[:-1], calls['device'])
    sam = [x for x in out['asm.sam'][0] if not x.startswith('@')]
    assert out['asm_host.paf'][0] == out['asm_device.paf'][0] and len(sam) == len(out['asm_host.paf'][0]) >= 1 and out['asm_device.paf'][1] == 1
    assert [PC.paf_from_sam_line(x, 5800, clen) for x in sam] == out['asm_host.paf'][0]
    for bad in (['--copycomments'], ['--bam-tags', 'MM,ML']):
        with pytest.raises(SystemExit) as ei:
            driver.main(common + bad + ['-o', str(d / 'no.paf')])
        assert '.paf' in str(ei.value.code) and bad[0] in str(ei.value.code)
    with pytest.raises(SystemExit) as ei:
        driver.main(common + ['-o', str(d / 'out.txt')])
    assert '.paf' in str(ei.value.code)
