"""CPU test of the owners of device and page-locked memory (vacmap_amd/csrc/vmx_devbuf.h): DevBuf's head-room rule and parking list, its moves, the views, HostPinned,
and a bundle struct that frees its members by dying. tests/host/devbuf_main.cpp is built with plain g++ against the emulator's allocator under AddressSanitizer and
UBSan and run as a child process; it must end with exit 0 and an empty stderr (LeakSanitizer reports at exit what nobody freed), and every row it prints is checked
here against the rule restated in Python."""
import json, os, subprocess
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GB = 1 << 30


def first_cap(b):
    return b + min(b // 8, GB) + 256


def grown_cap(b):
    return b + min(b // 2, 2 * GB) + 256


@pytest.fixture(scope='module')
def rows(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('devbuf') / 'devbuf')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-DVMX_EMU', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall',
                           '-I', os.path.join(ROOT, 'tests', 'emu'), '-I', os.path.join(ROOT, 'vacmap_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host', 'devbuf_main.cpp'), '-o', exe])      # the static_asserts (no copy, moves, trivial views) are checked here
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()[-2000:]
    out = {}
    for r in json.loads(p.stdout.decode()):
        out.setdefault(r['case'], []).append(r)
    return out


def test_head_room(rows):
    assert [r['bytes'] for r in rows['first']] == [1, 300, 1000, 4096]
    for r in rows['first']:
        assert r['rc'] == 0 and r['cap'] == first_cap(r['bytes']) and r['live'] == 1, r
    assert rows['first_gone'] == [{'case': 'first_gone', 'live': 0, 'parked': 0}]         # a buffer that dies frees its block, and parks nothing
    assert [r['bytes'] for r in rows['grow']] == [594, 1001, 5000] and first_cap(300) == 593   # one byte past the capacity of the first 300 is a growth already
    for r in rows['grow']:
        assert r['rc'] == 0 and r['cap'] == grown_cap(r['bytes']) and r['moved'] == 1, r
        assert r['parked_more'] == 1 and r['live_more'] == 1 and r['parked_bytes'] == first_cap(300), r      # the old block is parked, not freed
    # the caps of the rule, at sizes no test allocates
    assert first_cap(8 * GB) == 9 * GB + 256 and first_cap(16 * GB) == 17 * GB + 256
    assert grown_cap(4 * GB) == 6 * GB + 256 and grown_cap(16 * GB) == 18 * GB + 256
    assert rows['within'] == [{'case': 'within', 'rc': [0, 0], 'same_p': 1, 'same_cap': 1, 'live_more': 0, 'parked': 0}]


def test_parking_list(rows):
    (r,) = rows['park512']
    assert r == {'case': 'park512', 'parked_after_511': 511, 'live_after_511': 512, 'parked_after_512': 0, 'live_after_512': 0}
    (r,) = rows['flush']
    assert r == {'case': 'flush', 'parked_before': 2, 'parked_after': 0, 'bytes_after': 0, 'freed': 2}
    (r,) = rows['stats']                         # every reserve above that allocated: first allocations and growths are counted apart
    assert r['first'] == 4 + 3 + 1 + 512 + 1 + 1 + 2 + 1 + 4 and r['grows'] == 3 + 512 + 2 + 1


def test_moves_and_views(rows):
    assert rows['move_ctor'] == [{'case': 'move_ctor', 'src_empty': 1, 'dst_has': 1, 'live_more': 0}]
    assert rows['move_assign'] == [{'case': 'move_assign', 'src_empty': 1, 'dst_has': 1, 'freed': 1, 'freed_after_self': 1}]
    assert rows['moves_gone'] == [{'case': 'moves_gone', 'live': 0}]
    assert rows['view'] == [{'case': 'view', 'ok': 1, 'freed': 0}]


def test_host_pinned_and_bundle(rows):
    (r,) = rows['pinned']
    assert r['cap'] == [100 + 50 + 4096, 10000 + 5000 + 4096] and r['same_within'] == 1
    assert r['parked'] == 1 and r['live_grown'] == 2 and r['live_after'] == 0 and r['dev_live'] == 0      # parked until the object dies; counted apart from device memory
    (r,) = rows['bundle']
    assert r == {'case': 'bundle', 'live_in': 5, 'host_in': 1, 'live_after': 0, 'host_after': 0}
