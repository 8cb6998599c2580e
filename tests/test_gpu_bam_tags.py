"""Auxiliary fields of BAM input as comment text on the MI355X: the cases of test_bam_tags_emu.py on the device, and the device's blobs against
the emulator build's. Real wavefronts are what the ballots, the wave scan of the B arrays and the per-lane float conversion run on."""
import pytest

import bam_input_cases as K
import bam_tag_cases as T
import test_bam_tags_emu as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ctx():
    from vacmap_amd.lib import Context
    c = Context(0)
    yield c
    c.close()


def test_gpu_every_type_at_its_edges(ctx, tmp_path):
    E.test_reader_every_type_at_its_edges(ctx, tmp_path)


def test_gpu_selection(ctx, tmp_path):
    E.test_selection(ctx, tmp_path)


def test_gpu_records(ctx, tmp_path, monkeypatch):
    E.test_records(ctx, tmp_path, monkeypatch)


def test_gpu_dropped_fields(ctx, tmp_path):
    E.test_dropped_fields(ctx, tmp_path)


def test_gpu_malformed_aux_fails_the_read(ctx, tmp_path):
    """bounds checks that return an error code: nothing here faults"""
    E.test_malformed_aux_fails_the_read(ctx, tmp_path)


def test_gpu_blobs_equal_the_emulator_builds(ctx, tmp_path):
    import emu_lib
    from vacmap_amd.lib import BamReader
    ectx = emu_lib.context()
    reads = T.reads_with([aux for _, aux in T.edge_records()] + [aux for _, aux, _ in T.dropped_records()])
    p = str(tmp_path / 'both.bam')
    open(p, 'wb').write(T.ubam(reads, block=20000))
    for sel in ('*', ['ML', 'zz', 'fb', 'f3']):
        a, b = BamReader(ctx, p, tags=sel), BamReader(ectx, p, tags=sel)
        try:
            K.same_chunks(K.read_all(a, 7), K.read_all(b, 7))
            assert a.stats()['fields_dropped'] == b.stats()['fields_dropped']
        finally:
            a.close(); b.close()


def test_gpu_driver_end_to_end(ctx, tmp_path, monkeypatch, capsys):
    T.check_driver(ctx, tmp_path, monkeypatch, capsys)
