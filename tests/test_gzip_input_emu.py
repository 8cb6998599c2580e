"""Plain gzip inflated in parallel chunks (vm_gzip_decompress, lib.gzip_decompress; kernels k_gzip_in.hip) on the CPU emulator build of the
kernels (tests/emu). The comparator is Python's zlib / gzip. The emulator runs a wave's lanes one after the other: test_gpu_gzip_input.py
runs the same cases on real wavefronts."""
import ctypes

import pytest

import gzip_input_cases as G


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.mark.parametrize('chunk', (1024, 4096))
def test_bytes_equal_zlib(ctx, monkeypatch, chunk):
    """levels 1, 6 and 9, Z_FIXED, stored, Z_HUFFMAN_ONLY, Z_RLE, sync and full flushes, b'', one byte, 8 MB of zeros"""
    G.check_bytes(ctx, monkeypatch, chunk)


def test_markers(ctx, monkeypatch):
    """distance 32 768 exactly across chunks; a unit repeated 50 times: markers copied from copies through the window chain"""
    G.check_markers(ctx, monkeypatch)


def test_false_candidates_are_dropped(ctx, monkeypatch):
    """dynamic headers verbatim inside stored blocks: candidates rejected by the link check, the chain decoded again, the bytes right"""
    G.check_false_candidates(ctx, monkeypatch)


def test_members(ctx, monkeypatch):
    """three members (an empty one; FEXTRA, FNAME, FCOMMENT, FHCRC), 64 second-member offsets around chunk edges, 2 000 empty members"""
    G.check_members(ctx, monkeypatch)


def test_errors(ctx, monkeypatch):
    """CRC32, ISIZE, truncation, a bad magic, a bad member behind a good one: both sides raise, the device names what and where"""
    G.check_errors(ctx, monkeypatch)


def test_seeded_edits(ctx, monkeypatch):
    G.check_seeded_edits(ctx, monkeypatch)


def test_default_chunk_and_the_switch_minimum(ctx, monkeypatch):
    """without VMX_GZ_CHUNK the default chunk is used; a value below 1024 is raised to 1024"""
    from vacmap_amd.lib import gzip_decompress
    z, t = G.byte_cases()['level6']
    monkeypatch.delenv('VMX_GZ_CHUNK', raising=False)
    st = {}
    assert gzip_decompress(ctx, z, st) == t and 1 <= st['chunks_started'] <= (len(z) + 32767) // 32768
    monkeypatch.setenv('VMX_GZ_CHUNK', '1')
    st1 = {}
    assert gzip_decompress(ctx, z, st1) == t
    monkeypatch.setenv('VMX_GZ_CHUNK', '1024')
    st2 = {}
    assert gzip_decompress(ctx, z, st2) == t and st1['chunks_started'] == st2['chunks_started']


def test_c_abi_arguments(ctx):
    L = ctx.lib.L
    p = ctypes.c_void_p(); n = ctypes.c_int64()
    assert L.vm_gzip_decompress(None, b'x', 1, ctypes.byref(p), ctypes.byref(n)) == -3
    assert L.vm_gzip_decompress(ctx.h, b'x', 1, None, ctypes.byref(n)) < 0
    assert L.vm_gzip_decompress(ctx.h, b'', 0, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 0
    L.vm_free(p)
    e = G.device_gunzip(ctx, b'\0\0\0\0')[1]
    assert e is not None and 'magic' in str(e)


# ---------------------------------------------------------------- FastqReader(gzip='device')

def test_reader_shapes_equal_fastx(ctx, monkeypatch, tmp_path):
    """LF, CRLF, mixed and the 200 kb read at max_reads 1, 3, 64 and 4096"""
    G.check_reader_shapes(ctx, monkeypatch, tmp_path)


def test_reader_windows_carry(ctx, monkeypatch, tmp_path):
    """VMX_BAM_IN_CHUNK=131072, VMX_BAM_IN_MAXINF=65536: levels 1 and 6 across at least 5 windows, members inside windows, text many times max_inf"""
    G.check_reader_windows(ctx, monkeypatch, tmp_path)


def test_reader_errors_hand_out_a_prefix(ctx, monkeypatch, tmp_path):
    G.check_reader_errors(ctx, monkeypatch, tmp_path)


def test_driver_gzip_inflate_device_equals_host_run(ctx, tmp_path, monkeypatch, capsys):
    """--fastx-reader native --gzip-inflate device on plain-gzip reads gives the host run's SAM body; without --gzip-inflate the stderr
    fallback line is still there"""
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    import test_fastq_input_emu as E
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bg, plain = E._fastq_inputs(tmp_path)
    common = ['-ref', str(fa), '-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd'), '-mode', 'H', '--eqx', '--MD']

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@PG')]
    assert driver.main(common + ['-read', str(plain), '-o', str(tmp_path / 'host.sam')]) == 0
    capsys.readouterr()
    assert driver.main(common + ['-read', str(plain), '-o', str(tmp_path / 'dev.sam'), '--fastx-reader', 'native', '--gzip-inflate', 'device']) == 0
    assert '--fastx-reader native' not in capsys.readouterr().err          # no fallback
    assert driver.main(common + ['-read', str(plain), '-o', str(tmp_path / 'fb.sam'), '--fastx-reader', 'native']) == 0
    err = capsys.readouterr().err
    assert sum(1 for ln in err.split('\n') if '--fastx-reader native' in ln) == 1 and str(plain) in err and 'not BGZF' in err
    a = body(tmp_path / 'host.sam')
    assert a == body(tmp_path / 'dev.sam') == body(tmp_path / 'fb.sam') and sum(1 for x in a if not x.startswith('@')) >= 6


# ---------------------------------------------------------------- Index.from_fasta(reader='native', gzip='device')

def test_ref_vmx_equals_host_parser(ctx, monkeypatch, tmp_path):
    import vacmap_amd.lib as VL
    G.check_ref_vmx(VL, ctx, monkeypatch, tmp_path)


def test_driver_reads_and_reference_plain_gzip_on_the_device(ctx, tmp_path, monkeypatch, capsys):
    """--fastx-reader native --ref-reader native --gzip-inflate device on plain-gzip reads and reference gives the host run's SAM body, through
    vm_index_build_fasta_device_opts and vm_fastq_reader_open_opts"""
    import gzip
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    import test_fastq_input_emu as E
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bg, plain = E._fastq_inputs(tmp_path)
    (tmp_path / 'gzref').mkdir()
    gzref = tmp_path / 'gzref' / 'ref.fa.gz'
    gzref.write_bytes(gzip.compress(fa.read_bytes(), 6))
    common = ['-t', '2', '--nowriteindex', '--batch-reads', '2', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd'), '-mode', 'H', '--eqx', '--MD']
    called = []
    for fn in ('vm_index_build_fasta_device_opts', 'vm_fastq_reader_open_opts'):
        real = getattr(ctx.lib.L, fn)
        monkeypatch.setattr(ctx.lib.L, fn, (lambda real, fn: lambda *a: (called.append(fn), real(*a))[1])(real, fn))

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@PG')]
    assert driver.main(common + ['-ref', str(fa), '-read', str(plain), '-o', str(tmp_path / 'host.sam')]) == 0
    assert called == []
    capsys.readouterr()
    assert driver.main(common + ['-ref', str(gzref), '-read', str(plain), '-o', str(tmp_path / 'dev.sam'), '--fastx-reader', 'native', '--ref-reader', 'native',
                                 '--gzip-inflate', 'device']) == 0
    err = capsys.readouterr().err
    assert '--fastx-reader native' not in err and '--ref-reader native' not in err, err      # no fallback
    assert 'vm_index_build_fasta_device_opts' in called and 'vm_fastq_reader_open_opts' in called, called
    a = body(tmp_path / 'host.sam')
    assert a == body(tmp_path / 'dev.sam') and sum(1 for x in a if not x.startswith('@')) >= 6
