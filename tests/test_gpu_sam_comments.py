"""The comment stage of the device SAM emitter on the MI355X: the cases of sam_comment_cases against vm_sam_emit of the same library and the
Python statement of the rule, the step-edge, duplicate and bulk sets also against the emulator build's bytes, and the driver's
--sam-emitter device-comments with --copycomments and with --bam-tags."""
import pytest
import sam_comment_cases as CC
import sam_device_cases as SD

pytestmark = pytest.mark.gpu

CASES = CC.cases()
BULK = CC.bulk_cases()


@pytest.fixture(scope='module')
def env():
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    yield VL, ctx, SD.index(ctx)
    ctx.close()


_EMU = []


def _emu():
    if not _EMU:
        import emu_lib
        ectx = emu_lib.context()
        _EMU.extend([ectx, SD.index(ectx)])
    return _EMU


@pytest.mark.parametrize('case', CASES, ids=repr)
def test_gpu_case_matches_host_emitter_and_rule(env, case):
    VL, ctx, idx = env
    got = CC.check(VL, ctx, idx, case)
    if case.name.startswith('skip_'):
        assert got[3] == 1 and got[1][1] == got[1][2] and got[2] == 2
        for k in (0, 2):
            alone = CC.run_device(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts))
            assert got[0][got[1][k]:got[1][k + 1]] == alone[0] and alone[0].count(b'\tXG:i:') == 1
    if case.name in ('lengths', 'duplicates', 'mixed'):
        assert CC.check(VL, ctx, idx, case, lead=7) == got
        ectx, eidx = _emu()
        assert CC.run_device(VL, ectx, eidx, case) == got


@pytest.mark.parametrize('case', BULK, ids=repr)
def test_gpu_bulk_matches_host_emitter_and_emulator(env, case):
    """120 commented reads in one call: more waves than a workgroup; the device's bytes are the emulator build's"""
    VL, ctx, idx = env
    got = CC.check(VL, ctx, idx, case)
    assert got[2] >= 200 and got[3] >= 2 and got[0].count(b'\tXC:Z:c') >= 200
    ectx, eidx = _emu()
    assert CC.run_device(VL, ectx, eidx, case) == got


def test_gpu_without_comments_the_call_is_the_old_one(env):
    VL, ctx, idx = env
    for name in ('lengths', 'records_hard'):
        case = [c for c in CASES if c.name == name][0]
        none = CC.run_device(VL, ctx, idx, case, with_comments=False)
        assert none == SD.run_device(VL, ctx, idx, case) == CC.run_host(VL, ctx, idx, case, with_comments=False)


def test_gpu_driver_copycomments_on_the_device(tmp_path, monkeypatch, capsys):
    from vacmap_amd import lib as VL
    CC.check_driver_copycomments(VL, tmp_path, monkeypatch, capsys)


def test_gpu_driver_bam_tags_on_the_device(tmp_path, monkeypatch, capsys):
    from vacmap_amd import lib as VL
    CC.check_driver_bam_tags(VL, tmp_path, monkeypatch, capsys)
