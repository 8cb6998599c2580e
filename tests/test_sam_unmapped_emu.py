"""vm_sam_opts.keep_unmapped on the device emitter (k_sam_unmapped in k_sam.hip, the line-slot layout of vmx_sam_dev.h), on the CPU emulator
build of the kernels: vm_sam_emit_device, with and without comments, against vm_sam_emit of the same library byte for byte (text, text_off,
n_lines, n_skipped), option on and off, and the driver's --keep-unmapped. CPU only; the same cases run on the device in test_gpu_sam_unmapped.py."""
import pytest

import sam_device_cases as SD
import sam_unmapped_cases as UC

CASES = UC.cases()
BULK = UC.bulk_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.mark.parametrize('case', CASES + BULK, ids=repr)
def test_device_emitter_equals_host_emitter(env, case):
    VL, ctx, idx = env
    text, off, nl, ns = UC.check_device(VL, ctx, idx, case)
    assert nl == text.count(b'\n') and text.count(b'\t4\t*\t0\t0\t*\t*\t0\t0\t') == sum(1 for r in case.reads if not UC.emits(r))
    if case.name.startswith(('raise_', 'mdraise_')):
        assert (nl, ns) == (3, 1)
        for k in (0, 2):
            alone = UC.run(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts), device=True)
            assert text[off[k]:off[k + 1]] == alone[0]


def test_a_batch_without_records_still_has_its_lines(env):
    VL, ctx, idx = env
    case = [c for c in CASES if c.name == 'lengths'][0]
    assert sum(len(r.recs) for r in case.reads) == 0
    text, off, nl, ns = UC.run(VL, ctx, idx, case, device=True)
    assert (nl, ns) == (len(case.reads), 0) and text == b''.join(UC.unmapped_line(r, None) for r in case.reads)
    assert UC.run(VL, ctx, idx, case, keep=0, device=True) == (b'', [0] * (len(case.reads) + 1), 0, 0)
    assert UC.run(VL, ctx, idx, [c for c in CASES if c.name == 'nothing'][0], device=True) == (b'', [0], 0, 0)


def test_struct_size_is_unchanged():
    import ctypes as C
    from vacmap_amd import lib as VL
    assert C.sizeof(VL.SamOpts) == 40 and VL.SamOpts.keep_unmapped.offset == 36 and VL.SamOpts(0, 0, 0, 0, 0, 0, None, 0).keep_unmapped == 0


def test_driver_keep_unmapped(env, tmp_path, monkeypatch):
    VL, ctx, _ = env
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, fq, names = UC.driver_inputs(tmp_path, 5, 2, 2, ref_lens=(50000, 20000), mean_len=1200)
    lost = UC.check_driver(tmp_path, fa, fq, names, least=4, t='2', batch='3', bam=False)
    assert set(lost) >= {'rnd0', 'rnd1', 'tiny0', 'tiny1'}


def test_driver_refuses_asm(tmp_path):
    from vacmap_amd import driver
    with pytest.raises(SystemExit) as e:
        driver.main(['-ref', str(tmp_path / 'r.fa'), '-read', str(tmp_path / 'a.fa'), '-mode', 'asm', '--keep-unmapped', '-o', str(tmp_path / 'o.sam')])
    assert '--keep-unmapped' in str(e.value) and '\n' not in str(e.value)
