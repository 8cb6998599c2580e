"""Plain gzip inflated in parallel chunks on the MI355X: the cases of test_gzip_input_emu.py on real wavefronts (the match copy reads what
other lanes of the wave stored a moment ago, markers included; the window pass and the marker pass run many workgroups at once), the
device's bytes against the emulator build's, and one 64 MB text at the default chunk size."""
import zlib

import numpy as np
import pytest

import gzip_input_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('chunk', (1024, 4096))
def test_gpu_bytes_equal_zlib(ctx, monkeypatch, chunk):
    G.check_bytes(ctx, monkeypatch, chunk)


def test_gpu_markers(ctx, monkeypatch):
    G.check_markers(ctx, monkeypatch)


def test_gpu_false_candidates_are_dropped(ctx, monkeypatch):
    G.check_false_candidates(ctx, monkeypatch)


def test_gpu_members(ctx, monkeypatch):
    G.check_members(ctx, monkeypatch)


def test_gpu_errors(ctx, monkeypatch):
    G.check_errors(ctx, monkeypatch)


def test_gpu_seeded_edits(ctx, monkeypatch):
    G.check_seeded_edits(ctx, monkeypatch)


def test_gpu_equals_emulator_statistics(ctx, monkeypatch):
    """the search and the link check are deterministic: the device starts, rejects and repeats exactly the chunks the emulator build does"""
    import emu_lib
    from vacmap_amd.lib import gzip_decompress
    ectx = emu_lib.context()
    monkeypatch.setenv('VMX_GZ_CHUNK', '4096')
    z, inner = G.false_candidate_case()
    for data in (z, G.byte_cases()['level6'][0]):
        a, b = {}, {}
        assert gzip_decompress(ctx, data, a) == gzip_decompress(ectx, data, b)
        for k in ('chunks_started', 'candidates_rejected', 'chunks_redone', 'first_chain_bytes'):
            assert a[k] == b[k], (k, a, b)


def test_gpu_64mb_text_at_the_default_chunk(ctx, monkeypatch):
    """64 MB of 15 kb reads, zlib level 1 (a fast writer's file), the default VMX_GZ_CHUNK: the bytes, and hundreds of chunks started"""
    from vacmap_amd.lib import gzip_decompress
    monkeypatch.delenv('VMX_GZ_CHUNK', raising=False)
    rng = np.random.default_rng(64)
    n_reads, L = 2130, 15000
    seqs = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, (n_reads, L))]
    quals = (33 + np.clip(rng.normal(28, 7, (n_reads, L)), 2, 40)).astype(np.uint8)
    rows = np.empty((n_reads, 2 * L + 17), np.uint8)                    # @r<10 digits> \n bases \n+\n qualities \n
    rows[:, :2] = np.frombuffer(b'@r', np.uint8)
    rows[:, 2:12] = (np.arange(n_reads)[:, None] // 10 ** np.arange(9, -1, -1) % 10 + 48).astype(np.uint8)
    rows[:, 12] = 10; rows[:, 13:13 + L] = seqs; rows[:, 13 + L:16 + L] = np.frombuffer(b'\n+\n', np.uint8); rows[:, 16 + L:16 + 2 * L] = quals; rows[:, 16 + 2 * L] = 10
    text = rows.tobytes()
    assert len(text) >= 60 << 20
    z = G.deflate_gz(text, 1)
    st = {}
    got = gzip_decompress(ctx, z, st)
    assert len(got) == len(text) and got == text
    assert st['chunks_started'] - st['candidates_rejected'] >= 100, st


def test_gpu_reader_shapes_equal_fastx(ctx, monkeypatch, tmp_path):
    G.check_reader_shapes(ctx, monkeypatch, tmp_path)


def test_gpu_reader_windows_carry(ctx, monkeypatch, tmp_path):
    G.check_reader_windows(ctx, monkeypatch, tmp_path)


def test_gpu_reader_errors_hand_out_a_prefix(ctx, monkeypatch, tmp_path):
    G.check_reader_errors(ctx, monkeypatch, tmp_path)


def test_gpu_ref_vmx_equals_host_parser(ctx, monkeypatch, tmp_path):
    import vacmap_amd.lib as VL
    G.check_ref_vmx(VL, ctx, monkeypatch, tmp_path)
