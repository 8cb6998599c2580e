"""CPU test of the host's check of the rows given to vm_local_dp_batch (vacmap_amd/csrc/vmx_local_rows.h): the order check and the refusals.
tests/host/local_rows_main.cpp is built with plain g++ under AddressSanitizer and UBSan and run as a child process on batches at every edge of the rule:
exit 0, an empty stderr, and the verdict (code, read, row) the rule gives when restated in Python."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, -1, -7
I32 = 2 ** 31 - 1


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('local_rows') / 'local_rows')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-I', os.path.join(ROOT, 'vacmap_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host', 'local_rows_main.cpp'), '-o', out])
    return out


def verdict(reads, by_start):
    """the rule, restated: reads = [(rows, ng, readlen)] -> (code, read, row): field refusals over the whole batch first, then per read the caller's mistakes"""
    at = 0
    for r, (rows, ng, L) in enumerate(reads):
        for q, _, s, l in rows:
            if not 0 <= l <= 65535 or not -2 ** 31 <= q <= I32 or q + l > I32 or s not in (1, -1):
                return UNSUPPORTED, r, at
            at += 1
    at = 0
    for r, (rows, ng, L) in enumerate(reads):
        if ng < 1 or not 0 <= L <= I32:
            return ARG, r, -1
        prev = None
        for q, _, s, l in rows:
            key = q if by_start else q + l
            if q < 0 or q + l > L or (prev is not None and key < prev):
                return ARG, r, at
            prev = key
            at += 1
    return OK, -1, -1


A, B, C = (3, 50, 1, 15), (30, 80, -1, 15), (60, 110, 1, 15)
BATCHES = {
    'empty batch': [], 'a read without rows': [([], 1, 0), ([A, B], 2, 100)], 'in order': [([A, B, C], 1, 75)], 'ends exactly at its read': [([A, B, C], 1, 75)],
    'one behind its read': [([A, B, C], 1, 74)], 'equal keys': [([A, A, (8, 9, -1, 10)], 1, 40)], 'out of order': [([A, C, B], 1, 200)], 'second read out of order': [([A, B], 1, 200), ([B, A], 1, 200)],
    'by start only': [([(10, 50, 1, 40), (20, 90, 1, 15)], 1, 200)], 'by end only': [([(20, 90, 1, 15), (10, 50, 1, 40)], 1, 200)],
    'l 65535': [([(3, 5, 1, 65535)], 1, 65538)], 'l 65536': [([A, (40, 5, 1, 65536)], 1, 70000)], 'l 0': [([(3, 5, 1, 0)], 1, 10)], 'l -1': [([A, (60, 5, 1, -1)], 1, 100)],
    'q + l = 2^31 - 1': [([(I32 - 15, 5, 1, 15)], 1, I32)], 'q + l = 2^31': [([(I32 - 14, 5, 1, 15)], 1, I32)], 'q = 2^32 + 60': [([A, (2 ** 32 + 60, 5, 1, 15)], 1, I32)],
    'q = -2^31 - 1': [([(-2 ** 31 - 1, 5, 1, 15)], 1, 100)], 'q = -1': [([(-1, 5, 1, 15)], 1, 100)], 's 0': [([A, (40, 5, 0, 15)], 1, 100)], 's 2': [([(40, 5, 2, 15)], 1, 100)],
    's 65537': [([(40, 5, 65537, 15)], 1, 100)], 'no guide': [([A], 0, 100)], 'negative read length': [([], 1, -1)], 'read length 2^31': [([A], 1, 2 ** 31)],
    'a bad field behind a bad order': [([C, A], 1, 100), ([(4, 5, 3, 15)], 1, 100)],
}


@pytest.mark.parametrize('by_start', [0, 1])
def test_rule_on_edge_batches(exe, tmp_path, by_start):
    files, want = [], []
    for i, (name, reads) in enumerate(sorted(BATCHES.items())):
        off = [0]
        for rows, _, _ in reads:
            off.append(off[-1] + len(rows))
        nums = [len(reads), by_start] + off + [ng for _, ng, _ in reads] + [L for _, _, L in reads] + [v for rows, _, _ in reads for row in rows for v in row]
        p = str(tmp_path / ('b%d_%d.txt' % (by_start, i)))
        open(p, 'w').write(' '.join(str(x) for x in nums))
        files.append(p); want.append((name,) + verdict(reads, bool(by_start)))
    r = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    got = [tuple(int(x) for x in ln.split(' ')[:3]) for ln in r.stdout.decode().strip().split('\n')]
    assert [(w[0],) + g for w, g in zip(want, got)] == want
    codes = {w[1] for w in want}
    assert codes == {OK, ARG, UNSUPPORTED}
    assert dict((w[0], w[1]) for w in want)['by end only' if by_start else 'by start only'] == ARG
