"""vm_sam_opts.keep_unmapped on the host emitter (vm_sam_emit), vacmap_amd.sam.unmapped_line and the way of such a line through vm_bam_encode.
The expectation is the cases' own (sam_unmapped_cases: the SAM specification by string formatting). CPU only: the library is the emulator
build, whose host code is the product's."""
import struct

import pytest

import bam_codec as B
import sam_device_cases as SD
import sam_unmapped_cases as UC

CASES = UC.cases()
BULK = UC.bulk_cases()


@pytest.fixture(scope='module')
def env():
    import emu_lib
    from vacmap_amd import lib as VL
    ctx = emu_lib.context()
    return VL, ctx, SD.index(ctx)


@pytest.mark.parametrize('case', CASES + BULK, ids=repr)
def test_host_emitter_writes_the_specified_lines(env, case):
    VL, ctx, idx = env
    text, off, nl, ns = UC.check_host(VL, ctx, idx, case)
    lines = text.split(b'\n')[:-1]
    assert nl == len(lines) and len(off) == len(case.reads) + 1 and off[-1] == len(text)
    for k, r in enumerate(case.reads):                                  # one FLAG 4 line per read that emits no record line, none for the others
        mine = text[off[k]:off[k + 1]].split(b'\n')[:-1]
        assert [x.split(b'\t')[1] == b'4' for x in mine] == ([False] * len(mine) if UC.emits(r) else [True]), (case.name, r.name)
        assert all(x.split(b'\t')[0] == r.name.encode() for x in mine)
    if case.name.startswith(('raise_', 'mdraise_')):                    # the raising read between two good ones: theirs are the bytes they have alone
        assert ns == 1 and nl == 3
        for k in (0, 2):
            alone = UC.run(VL, ctx, idx, SD.Case('alone', [case.reads[k]], **case.opts))
            assert text[off[k]:off[k + 1]] == alone[0] and alone[2:] == (1, 0)


def test_cases_hold_the_shapes_they_name():
    by = {(c.name, r.name): r for c in CASES for r in c.reads}
    assert sorted(len(by['lengths', 'len%d' % n].seq) for n in UC.LENGTHS) == list(UC.LENGTHS)
    assert all(not r.recs for c in CASES if c.name.startswith(('lengths', 'comments', 'one_empty')) for r in c.reads)
    assert {len(r.name) for r in [c for c in CASES if c.name == 'lengths'][0].reads} >= {1, 254}
    assert UC.unmapped_line(by['lengths', 'len0'], None) == b'len0\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n'
    assert UC.unmapped_line(by['lengths', 'len1_short'], 'g').endswith(b'\t0\t0\t' + by['lengths', 'len1_short'].seq.encode() + b'\t*\tRG:Z:g\n')
    r = by['lengths', 'len65']
    assert UC.unmapped_line(r, None) == ('len65\t4\t*\t0\t0\t*\t*\t0\t0\t%s\t%s\n' % (r.seq, r.qual)).encode() and len(r.qual) == 65
    tags = by['comments', 'c_line_tags']
    assert UC.kept_fields(tags.comment, None) == b'\tXK:i:1\tRG:Z:other\tCG:Z:mine' and UC.kept_fields(tags.comment, 'g') == b'\tXK:i:1\tCG:Z:mine'
    assert UC.kept_fields(by['comments', 'c_dup'].comment, None) == b'\tXA:i:1\tXB:Z:b'
    assert UC.kept_fields(by['comments', 'c_tags130'].comment, None).count(b'\t') == 130
    for at in (63, 64, 65):
        assert by['comments', 'c_tab%d' % at].comment[at] == 9
    mixed = [c for c in CASES if c.name == 'mixed_default'][0].reads
    e = [UC.emits(r) for r in mixed]
    assert not e[0] and not e[-1] and e[1] and e[5] and e[2:5] == [False] * 3 and mixed[6].recs and mixed[6].status == -10
    assert sorted(c.name[6:] for c in CASES if c.name.startswith('mixed_')) == sorted(SD.OPTSETS)
    assert all(c.opts['keep_unmapped'] == 1 for c in CASES + BULK) and len(BULK[0].reads) == 300


def test_option_off_is_the_parent_behaviour(env):
    """with the field 0 a read that emits no record line leaves no byte, as before the option existed"""
    VL, ctx, idx = env
    for case in [c for c in CASES if c.name in ('lengths', 'mixed_default', 'raise_M_past_read')] + BULK[:1]:
        text, off, nl, ns = UC.run(VL, ctx, idx, case, keep=0)
        assert b'\t4\t*\t0\t0\t' not in text and nl == text.count(b'\n')
        assert all((off[k + 1] > off[k]) == UC.emits(r) for k, r in enumerate(case.reads))


def test_python_statement_gives_the_same_line():
    from vacmap_amd import sam
    n = 0
    for case in CASES + BULK[:2]:
        rg = case.opts.get('rg')
        for r in case.reads:
            com = getattr(r, 'comment', None)
            got = sam.unmapped_line(r.name, r.seq, r.qual, rg_id=rg, comments=None if com is None else com.decode('latin-1'))
            assert (got + '\n').encode('latin-1') == UC.unmapped_line(r, rg), (case.name, r.name)
            n += 1
    assert n > 600
    assert sam.unmapped_line('q', 'ACGT', None) == 'q\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*'


def _raw_records(bam):
    """(refID, pos, l_read_name, mapq, bin, n_cigar_op, flag, l_seq, next_refID, next_pos, tlen, qualities) of every record, from the bytes"""
    raw = B.bgzf_decompress(bam)
    p = 8 + struct.unpack_from('<i', raw, 4)[0]
    nref = struct.unpack_from('<i', raw, p)[0]; p += 4
    for _ in range(nref):
        p += 8 + struct.unpack_from('<i', raw, p)[0]
    out = []
    while p < len(raw):
        bs = struct.unpack_from('<i', raw, p)[0]
        f = struct.unpack_from('<iiBBHHHiiii', raw, p + 4)
        q0 = p + 4 + 32 + f[2] + 4 * f[5] + (f[7] + 1) // 2
        out.append(f + (raw[q0:q0 + f[7]],))
        p += 4 + bs
    return out


def test_unmapped_lines_through_the_bam_encoder(env, tmp_path):
    """refID -1, pos -1, FLAG 4, MAPQ 0, no CIGAR, the bases, the qualities or 0xff; the optional fields by value"""
    from vacmap_amd.bamout import BamWriter
    VL, ctx, idx = env
    head = ['@HD\tVN:1.6'] + ['@SQ\tSN:%s\tLN:%d' % (n, len(s)) for n, s in zip(SD.NAMES, SD.REF)]
    for name in ('lengths_rg_hard', 'comments', 'mixed_hard_fake_rg'):
        case = [c for c in CASES if c.name == name][0]
        text, off, nl, ns = UC.run(VL, ctx, idx, case)
        path = str(tmp_path / (name + '.bam'))
        w = BamWriter(path, head, lib=ctx.lib)
        w.write(text)
        w.close()
        data = open(path, 'rb').read()
        recs = B.read_bam(data)[2]; raw = _raw_records(data)
        lines = text.decode('latin-1').split('\n')[:-1]
        assert len(recs) == len(raw) == len(lines) == nl
        assert all(B.same_as_sam(d, ln) for d, ln in zip(recs, lines))
        seen = 0
        for k, r in enumerate(case.reads):
            if UC.emits(r):
                continue
            i = text[:off[k]].count(b'\n')
            refid, pos, _, mapq, _, ncig, flag, lseq, nrefid, npos, tlen, qual = raw[i]
            assert (refid, pos, mapq, ncig, flag, nrefid, npos, tlen) == (-1, -1, 0, 0, 4, -1, -1, 0), (name, r.name)
            fields, tags = recs[i]
            has_q = bool(r.qual) and len(r.qual) == len(r.seq)
            assert fields[0] == r.name and fields[9] == (r.seq or '*') and lseq == len(r.seq)
            assert qual == (bytes(ord(c) - 33 for c in r.qual) if has_q else b'\xff' * lseq)
            assert [t[0] for t in tags] == [f[:2] for f in lines[i].split('\t')[11:]]
            seen += 1
        assert seen >= 7
