"""vm_sam_opts.keep_unmapped on the MI355X: the cases of sam_unmapped_cases on the device against the host emitter of the same library (option on
and off, with and without comments), the bulk set also against the emulator build's bytes, and one driver run with --keep-unmapped through both
emitters and the native BAM writers."""
import pytest

import sam_device_cases as SD
import sam_unmapped_cases as UC

pytestmark = pytest.mark.gpu

CASES = UC.cases()
BULK = UC.bulk_cases()


@pytest.fixture(scope='module')
def env():
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    yield VL, ctx, SD.index(ctx)
    ctx.close()


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_gpu_device_emitter_equals_host_emitter(env, case):
    VL, ctx, idx = env
    UC.check_host(VL, ctx, idx, case)
    text, off, nl, ns = UC.check_device(VL, ctx, idx, case)
    assert nl == text.count(b'\n') and text.count(b'\t4\t*\t0\t0\t*\t*\t0\t0\t') == sum(1 for r in case.reads if not UC.emits(r))
    if case.name.startswith(('raise_', 'mdraise_')):
        assert (nl, ns) == (3, 1)
        for k in (0, 2):
            alone = UC.run(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts), device=True)
            assert text[off[k]:off[k + 1]] == alone[0]


@pytest.mark.parametrize('case', BULK, ids=repr)
def test_gpu_bulk_equals_host_emitter_and_emulator(env, case):
    """300 reads, about a third of them unmapped: more line slots than a scan block; the device's bytes are the emulator build's"""
    import emu_lib
    VL, ctx, idx = env
    got = UC.check_device(VL, ctx, idx, case)
    assert got[0].count(b'\t4\t*\t0\t0\t*\t*\t0\t0\t') >= 100 and got[3] >= 7
    ectx = emu_lib.context()
    assert UC.run(VL, ectx, _emu_index(ectx), case, device=True) == got


_EMU_INDEX = []


def _emu_index(ectx):
    if not _EMU_INDEX:
        _EMU_INDEX.append(SD.index(ectx))
    return _EMU_INDEX[0]


def test_gpu_driver_keep_unmapped(tmp_path):
    """a 1.5 Mb reference, 200 synthetic reads with 20 random 500-base reads and 5 twelve-base reads among them"""
    fa, fq, names = UC.driver_inputs(tmp_path, 200, 20, 5)
    lost = UC.check_driver(tmp_path, fa, fq, names, least=10)
    assert len(names) == 225 and len(lost) < 60
