"""CPU test of the reference FASTA's line rule (vacmap_amd/csrc/vmx_fasta_rule.h), which the host parser feeds from a plain file or from zlib.
tests/host/fasta_rule_main.cpp is built with plain g++ under AddressSanitizer and UBSan and run as a child process on the edge texts of
fasta_ref_cases, fed in pieces of 1, 7 and 65 536 bytes: exit 0, an empty stderr, and the contigs of the rule restated in Python."""
import os
import subprocess

import pytest

import fasta_ref_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIECES = (1, 7, 65536)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp('fasta_rule') / 'fasta_rule')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-I', os.path.join(ROOT, 'vacmap_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host', 'fasta_rule_main.cpp'), '-o', out])
    return out


def _texts():
    out = {}
    for group in (R.eol_texts(), R.header_texts(), R.letter_texts()):
        out.update(group)
    out['long_line'] = R.long_line_text()
    out['high_bytes'] = b'>c\xe9 1\nAC\xffGT\n\xff\xfe\n'
    return out


@pytest.mark.parametrize('name', sorted(_texts()))
def test_rule_on_edge_texts(exe, tmp_path, name):
    text = _texts()[name]
    p = str(tmp_path / 'in.fa')
    open(p, 'wb').write(text)
    pieces = PIECES if len(text) < 10000 else (4096, 65536)
    r = subprocess.run([exe, p] + [str(x) for x in pieces], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0 and not r.stderr, r.stderr.decode()[-2000:]
    got = {}
    for ln in r.stdout.decode().split('\n'):
        f = ln.split(' ')
        if len(f) == 3:
            got.setdefault(int(f[0]), []).append((bytes.fromhex(f[1]), bytes(c - 32 if 97 <= c <= 122 else c for c in bytes.fromhex(f[2]))))
        elif len(f) == 2:
            got.setdefault(int(f[0]), [])
    want = R.parse(text)
    assert sorted(got) == sorted(pieces)
    for piece in pieces:
        assert got[piece] == want, piece
