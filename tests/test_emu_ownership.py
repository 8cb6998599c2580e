"""Who frees device memory, counted: the emulator build counts its live hipMalloc and hipHostMalloc allocations (tests/emu/hip_emu.h), and a round through every
handle of the library that owns some (tests/ownership_cases.py) must leave none behind. The first round warms what the process keeps for good (a counter
block, if one is on); after the second round both counts are what they were after the first, and in the middle of it they were larger — the counters count.
The shared context of emu_lib stays out of it: it is opened first, so that it is part of both counts alike."""
import pytest

import ownership_cases as OC


@pytest.fixture(scope='module')
def lib():
    import emu_lib
    return emu_lib.context().lib


def live(lib):
    f = lib.L.vmx_emu_live_allocs
    f.argtypes = [__import__('ctypes').c_int]; f.restype = __import__('ctypes').c_longlong
    return f(0), f(1)


def test_two_rounds_leave_what_one_left(lib, golden, tmp_path):
    import vacmap_amd.lib as VL
    first = OC.one_round(VL, lib, golden, str(tmp_path), 'a')
    after_first = live(lib)
    mid = []
    second = OC.one_round(VL, lib, golden, str(tmp_path), 'b', probe=lambda: mid.append(live(lib)))
    after_second = live(lib)
    print('live (device, page-locked): after round one %s, inside round two %s, after round two %s' % (after_first, mid[0], after_second))
    assert after_second == after_first
    assert mid[0][0] > after_first[0] and mid[0][1] > after_first[1]
    assert second == first


def test_error_paths_leave_nothing(lib, tmp_path):
    import vacmap_amd.lib as VL
    OC.error_round(VL, lib, str(tmp_path))
    before = live(lib)
    assert OC.error_round(VL, lib, str(tmp_path)) == [-7, -1]
    assert live(lib) == before
