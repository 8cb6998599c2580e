"""The round of tests/ownership_cases.py — every handle of the library that owns device memory, opened, used and closed, the context last — twice on the
device: every call succeeds, and the second round gives the records, texts and BAM bytes of the first. (What was freed is counted on the emulator build,
test_emu_ownership.py; the device's free memory is no measure here, since other processes allocate on it too.)"""
import pytest

import ownership_cases as OC

pytestmark = pytest.mark.gpu


def test_two_rounds_agree(golden, tmp_path):
    import vacmap_amd.lib as VL
    lib = VL.load()
    first = OC.one_round(VL, lib, golden, str(tmp_path), 'a')
    second = OC.one_round(VL, lib, golden, str(tmp_path), 'b')
    assert first['align'][1] and first['bam'] and first['sorted'] and first['csi']
    assert second == first


def test_error_paths(tmp_path):
    import vacmap_amd.lib as VL
    lib = VL.load()
    assert OC.error_round(VL, lib, str(tmp_path)) == [-7, -1]
    assert OC.error_round(VL, lib, str(tmp_path)) == [-7, -1]
