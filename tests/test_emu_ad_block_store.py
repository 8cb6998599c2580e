"""CPU tests (no GPU) of the anti-diagonal band fill's block stores: the lane-major traceback layout of vacmap_amd/csrc/vmx_gapfill.h as a plain host program
against a NumPy statement of it, and the band loop of vmx_dp_ad.h (one store per lane, problem and four anti-diagonals) in the emulator build through the
batched path's own entry — cases in ad_block_store_cases.py, the `gpu` twin in test_gpu_ad_block_store.py."""
import json, os, subprocess
import numpy as np
import pytest
import ad_block_store_cases as BS
import kernel_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('ad_layout') / 'ad_layout')
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', '-Wall', '-I', os.path.join(ROOT, 'vacmap_amd', 'csrc'),
                           os.path.join(ROOT, 'tests', 'host', 'ad_layout_main.cpp'), '-o', exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert p.returncode == 0 and not p.stderr, p.stderr.decode()[-2000:]
    return json.loads(p.stdout.decode())


def test_layout_offsets(layout):
    """vmx_ad_tb_off on a grid of (s, l, W) is the formula; a lane's four slots of a block are one aligned run; the map is one-to-one onto the blocks' bytes"""
    AB, S, LN = layout['AB'], layout['S'], layout['L']
    assert AB == 4 and S % AB == 0 and LN == 16
    for W in (1, 2, 4):
        got = np.array(layout['off'][str(W)], dtype=np.int64).reshape(S, LN)
        want = BS.layout_offsets(range(S), range(LN), W, AB)
        assert np.array_equal(got, want), W
        assert sorted(got.ravel().tolist()) == list(range(0, S * LN * W, W)), W               # one-to-one onto the slots of S / AB whole blocks
        first = got[0::AB]                                                                    # each lane's slot on a block's first anti-diagonal
        assert np.all(first % (AB * W) == 0), W
        for k in range(1, AB):
            assert np.array_equal(got[k::AB], first + k * W), (W, k)                          # ... and the next three right behind it
        assert np.all(got // 64 == (first // 64).repeat(AB, axis=0)), W                       # so a block of a lane never leaves its 64-byte line


def test_layout_sizes_and_walk(layout):
    for tl, ql, W, nbytes in layout['bytes']:
        assert nbytes == (tl + ql + 3) // 4 * 4 * 16 * W and nbytes % 64 == 0, (tl, ql, W)
    assert {(r[0] + r[1]) % 4 for r in layout['bytes']} == {0, 1, 2, 3}
    seen = set()
    for tl, ql, ns, i, j, cell, lane_off, step_off, dlo, W in layout['cells']:
        assert W == {1: 1, 2: 2, 3: 4, 4: 4}[ns] and dlo == KC.ad_geom(tl, ql, ns)[1]
        x = (j - i) - dlo; l = x // (2 * ns); k = (x % (2 * ns)) >> 1
        want = int(BS.layout_offsets([i + j - 1], [l], W)[0, 0]) + k
        assert cell == want and lane_off + step_off == want, (tl, ql, ns, i, j)
        assert cell < (tl + ql + 3) // 4 * 4 * 16 * W
        seen.add(ns)
    assert seen == {1, 2, 3, 4}


@pytest.fixture(scope='module')
def emu():
    import emu_lib
    return emu_lib.context()


def test_case_list():
    """the cases hold what they are meant to: every residue of tl + ql mod 4 with odd and even pair counts, tiny problems, one-base sides"""
    for pct in BS.PCTS:
        big, groups = BS.problems(pct)
        tots = [len(t) + len(q) for t, q, _ in big]
        # (the residue fixes the parity of the pair count (n + 1) // 2: even for 0 and 3, odd — the junk pair — for 1 and 2)
        assert {(n % 4, ((n + 1) // 2) % 2) for n in tots} == {(0, 0), (1, 1), (2, 1), (3, 0)}
        assert min(tots) < 4 and max(tots) == BS.LIMIT and 100 <= len(big) <= 400
        assert any(len(t) == 1 for t, q, _ in big) and any(len(q) == 1 for t, q, _ in big)
        assert [len(g) for g in groups] == [2] * 8 + [1, 8]
        assert sorted(sum(map(len, groups[i][1][:2])) - sum(map(len, groups[i][0][:2])) for i in range(8)) == [1, 2, 3, 4, 5, 9, 22, 51]


def test_emu_ad_block_store(emu, oracle, monkeypatch):
    BS.check(emu, oracle, monkeypatch)
