"""Auxiliary fields of BAM input as comment text (vm_bam_reader_open_tags, lib.BamReader(tags=), driver --bam-tags) on the CPU emulator build of
the kernels. The specification is bam_tag_cases.aux_text; test_gpu_bam_tags.py runs the same cases on the device."""
import numpy as np
import pytest

import bam_input_cases as K
import bam_tag_cases as T


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


# ---------------------------------------------------------------- 1. the specification's pins

def test_spec_pins():
    aux, text = T.every_type_record()
    assert T.aux_text(aux, '*') == (text, 0)
    assert T.aux_text(aux, ['XZ', 'Bf', 'Xc']) == ('Xc:i:-128\tXZ:Z:a b:c\tBf:B:f,1.5,-2,1e+10', 0)
    assert T.aux_text(aux, None) == ('', 0) and T.aux_text(b'', '*') == ('', 0) and T.aux_text(b'xx', None) == ('', 0)
    for bits, want in T.F_EDGES:
        assert T.float_text(bits) == want, hex(bits)
        assert len(want) <= 15 and np.float32(float(want)).view(np.uint32) == bits
    for name, aux in T.malformed_aux().items():
        with pytest.raises(ValueError):
            T.aux_text(aux, '*')
    for name, aux, nd in T.dropped_records():
        assert T.aux_text(aux, '*')[1] == nd, name


def test_driver_read_bam_states_the_rule(tmp_path):
    from vacmap_amd import driver
    reads = T.reads_with([aux for _, aux in T.edge_records() if len(aux) < 30000] + [aux for _, aux, _ in T.dropped_records()])
    p = str(tmp_path / 'd.bam')
    open(p, 'wb').write(T.ubam(reads))
    for sel in ('*', ['zz', 'h1', 'f3', 'ML'], None):
        assert [(r[3] or '').encode('latin-1') for r in driver.read_bam(p, tags=sel)] == T.spec_comments(reads, sel)[0]
    assert all(r[3] is None for r in driver.read_bam(p))
    for aux in T.malformed_aux().values():
        open(p, 'wb').write(T.ubam(T.reads_with([aux])))
        assert len(list(driver.read_bam(p))) == 1
        with pytest.raises(ValueError):
            list(driver.read_bam(p, tags='all'))
    for bad in ('M', 'MMM', 'MM,', ',MM', 'MM,,ML', 'M-', '1M'):
        with pytest.raises(ValueError):
            driver._bam_tag_select(bad)


# ---------------------------------------------------------------- 2. every type at its edges

def test_reader_every_type_at_its_edges(ctx, tmp_path):
    reads = T.reads_with([aux for _, aux in T.edge_records()])
    T.check_against_spec(ctx, tmp_path, reads, '*')
    aux, text = T.every_type_record()
    p = str(tmp_path / 'one.bam')
    open(p, 'wb').write(T.ubam(T.reads_with([aux])))
    assert T.reader_comments(ctx, p, '*')[0] == [text.encode()]
    open(p, 'wb').write(T.ubam(T.reads_with([b''.join(T.fld('e%c' % (65 + k), 'f', ('bits', b)) for k, (b, _) in enumerate(T.F_EDGES))])))
    assert T.reader_comments(ctx, p, '*')[0] == ['\t'.join('e%c:f:%s' % (65 + k, t) for k, (_, t) in enumerate(T.F_EDGES)).encode()]


# ---------------------------------------------------------------- 3. selection

def test_selection(ctx, tmp_path):
    from vacmap_amd import driver
    from vacmap_amd.lib import BamReader, VmxError
    reads = T.reads_with([aux for _, aux in T.edge_records() if len(aux) < 30000])
    p = T.check_against_spec(ctx, tmp_path, reads, ['zz'])
    T.check_against_spec(ctx, tmp_path, reads, ['QQ'])                                      # a tag no record has
    T.check_against_spec(ctx, tmp_path, reads, ['MM'])                                      # duplicated in a record: both are passed through
    T.check_against_spec(ctx, tmp_path, reads, ['bb', 'aa', 'h2', 'Bf'])                    # record order, not list order
    many = ['Q%c' % c for c in 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789'] + ['Y1']
    assert len(many) == 63
    T.check_against_spec(ctx, tmp_path, reads, many + ['bb'])                               # 64 tags: the last of one ballot
    T.check_against_spec(ctx, tmp_path, reads, many + ['Y2', 'bb'])                         # 65: the second ballot
    # none: comments empty, everything else as today
    for tags in (None, '', []):
        rd = BamReader(ctx, p, tags=tags)
        K.same_chunks(K.read_all(rd, 5), list(driver._bam_chunks(p, 5)))
        assert rd.stats()['fields_dropped'] == 0
        rd.close()
    for bad in ('M', 'MMM', 'MM,', ',MM', 'MM,,ML', 'M-', '1M', '**', 'MM ML'):
        with pytest.raises(VmxError) as e:
            BamReader(ctx, p, tags=bad)
        assert e.value.code == T.VM_ERR_ARG


# ---------------------------------------------------------------- 4. records

def test_records(ctx, tmp_path, monkeypatch):
    from vacmap_amd.lib import BamReader
    auxes = [aux for _, aux in T.edge_records() if len(aux) < 30000]
    reads = T.reads_with(auxes + [b''] + auxes[::-1])
    bad = T.malformed_aux()
    reads[3:3] = [('empty1', '', None, 4, auxes[0]), ('empty2', '', None, 4, bad['type']), ('empty3', '', None, 20, bad['nul'])]      # dropped records: aux never looked at
    assert any(r[3] == 16 and r[4] for r in reads)
    T.check_against_spec(ctx, tmp_path, reads, '*', sizes=(1, 3, 4096))
    p = str(tmp_path / 'tags.bam')
    want = T.spec_comments(reads, '*')[0]
    for mb in (1, 3, 4096):                                                                 # max_bases cuts
        assert T.reader_comments(ctx, p, '*', 1000, mb)[0] == want
    import test_bam_input_emu as E
    E._small_windows(monkeypatch)
    T.check_against_spec(ctx, tmp_path, reads, '*', sizes=(3, 4096), block=333, driver_too=False)      # aux regions over members, chunks and windows
    T.check_against_spec(ctx, tmp_path, reads, ['ML', 'zz', 'Bf', 'f3'], sizes=(4096,), block=5000, driver_too=False)


# ---------------------------------------------------------------- 5. dropped fields

def test_dropped_fields(ctx, tmp_path):
    for name, aux, nd in T.dropped_records():
        reads = T.reads_with([T.fld('k1', 'i', 1), aux, T.fld('k2', 'Z', 'after')])
        p = T.check_against_spec(ctx, tmp_path, reads, '*', drops=nd)
        got = T.reader_comments(ctx, p, '*')[0]
        assert got[0] == b'k1:i:1' and got[2] == b'k2:Z:after' and got[1] == T.aux_text(aux, '*')[0].encode() and got[1], name
    name, aux, nd = T.dropped_records()[3]
    T.check_against_spec(ctx, tmp_path, T.reads_with([aux]), ['ab'], drops=0)               # a dropped field nobody asked for is not counted


# ---------------------------------------------------------------- 6. malformed aux data

def test_malformed_aux_fails_the_read(ctx, tmp_path):
    from vacmap_amd.lib import BamReader, VmxError
    for name, aux in T.malformed_aux().items():
        reads = T.reads_with([T.fld('ok', 'i', 1), T.fld('ok', 'i', 2), aux, aux])
        p = str(tmp_path / (name + '.bam'))
        open(p, 'wb').write(T.ubam(reads))
        assert len(T.reader_comments(ctx, p, None)[0]) == 4                                 # the file reads as it always did
        rd = None
        try:
            with pytest.raises(VmxError) as e:
                rd = BamReader(ctx, p, tags=['zz'])                                       # (selected or not, the field chain has to be walked)
                K.read_all(rd, 100)
        finally:
            if rd is not None:
                rd.close()
        assert e.value.code == T.VM_ERR_IO and 'record 3' in str(e.value), (name, str(e.value))


# ---------------------------------------------------------------- 7. the driver

def test_driver_end_to_end(ctx, tmp_path, monkeypatch, capsys):
    T.check_driver(ctx, tmp_path, monkeypatch, capsys)
