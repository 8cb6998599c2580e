"""CPU tests (no GPU, no emulator): the constructed cases of local_cases.py for the local re-seeding stage.
  * the generator's self-check: every edge is where it claims to be under spec_ref.local_guides / local_seed / local_raw alone, on either side, and
    every case is N-safe (D1 and text equality give the same rows); the build constants the cases are made for are the headers';
  * spec == the REFERENCE's own rows on every recorded case (tests/golden/local_edges.*, tools/harness/gen_golden_local_edges.py);
  * oracle.local_chain == spec on every case;
  * spec == the reference's raw local anchors of the natural reads of the goldens (V3), which ties the spec to real reads as well.
test_emu_local_edges.py and test_gpu_local_edges.py run the kernels on the same cases."""
import json, os, re, zlib
import numpy as np
import pytest
import local_cases as LC
import spec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_V3 = ['A', 'B', 'C', 'D', 'G', 'J', 'K', 'P']             # the cases check_local_golden runs on the emulator and by default on the GPU; all four modes


def test_build_constants_are_the_headers():
    kh = open(os.path.join(ROOT, 'vacmap_amd', 'csrc', 'vmx_kernels.h')).read()
    band = open(os.path.join(ROOT, 'vacmap_amd', 'csrc', 'k_local_band.hip')).read()
    emu, hw = kh[kh.index('#ifdef VMX_EMU\n#define VMX_LB_QC'):].split('#else', 1)
    hw = hw.split('#define VMX_LB_TABLE_U64', 1)[0]

    def val(text, name):
        return int(re.search(r'#define %s (\d+)' % name, text).group(1))
    for build, text in (('emu', emu), ('gfx950', hw)):
        B = LC.BUILDS[build]
        assert (B['QC'], B['HCAP']) == (val(text, 'VMX_LB_QC'), val(text, 'VMX_LB_HCAP')), build
        assert B['GS'] == val(text, 'VMX_LB_GS'), build
        assert (B['OPEN'], B['PIECES'], B['WIN'], B['HULL_ONE']) == tuple(val(band, 'LB_' + n) for n in ('OPEN', 'PIECES', 'WIN', 'HULL_ONE')), build
    assert '#define VMX_LA_SLOT(len) ((len) / 2 + 4096)' in kh and LC.la_slot(1500) == 4846
    assert 'if (qc <= 16)' in band and '(3 * VMX_LB_HCAP / 4)' in band and 'want < 32 ? 32' in band      # simulate_tile's model of the chunk widths


@pytest.mark.parametrize('build', list(LC.BUILDS))
def test_local_cases_claims(build):
    fams, expects = set(), set()
    for c in LC.constructed(build):
        LC.check_claims(c)
        fams.add(c.family); expects |= {rd.expect for rd in c.reads if rd.expect}
    assert fams == set(LC.FAMILIES) and expects == {'windows', 'open runs', 'hit tile'}


def test_local_spec_is_the_reference_fixture():
    meta = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'local_edges.json')))
    rows = np.load(os.path.join(ROOT, 'tests', 'golden', 'local_edges.npz'))['rows']
    seen = set()
    for build in LC.BUILDS:
        for c in LC.constructed(build):
            if c.family == 'mix' or c.mode == 'asm' or c.label in seen:
                continue
            seen.add(c.label)
            for i, rd in enumerate(c.reads):
                rec = meta.pop('%s|%s' % (c.label, rd.label))
                got = c.rows(i)
                assert len(got) == rec['n'], (c.label, rd.label, len(got), rec['n'])
                if 'crc' in rec:
                    assert zlib.crc32(np.ascontiguousarray(got).tobytes()) == rec['crc'], (c.label, rd.label)
                else:
                    LC.same(got, rows[rec['off']:rec['off'] + rec['n']], c, rd, 'spec against the reference')
    assert not meta, list(meta)[:5]


@pytest.mark.parametrize('build', list(LC.BUILDS))
def test_local_oracle_is_the_spec(oracle, build):
    for c in LC.constructed(build):
        oi = oracle.Index.from_seqs(['c%d' % i for i in range(len(c.contigs))], c.contigs, k=15, w=10)
        prm = oracle.params(c.mode, local_kmersize=c.k)
        for i, rd in enumerate(c.reads):
            raw = oracle.local_chain(oi, rd.seq, rd.paths, prm)['raw'].reshape(-1, 4)
            if len(raw):
                raw = raw[np.argsort(raw[:, 0] + (0 if c.mode in ('R', 'asm') else raw[:, 3]), kind='stable')]
            LC.same(raw, c.rows(i), c, rd, 'oracle against the spec')


@pytest.mark.parametrize('cid', GOLDEN_V3)
def test_local_spec_is_the_golden_v3(golden, cid):
    meta, arrays = golden
    c = meta[cid]
    contigs = [arrays['%s_contig%d' % (cid, i)].tobytes().decode() for i in range(len(c['names']))]
    n = 0
    for ri, r in enumerate(c['reads']):
        key = '%s_r%d' % (cid, ri)
        if 'v3_score' not in r:
            continue
        seq = arrays[key + '_seq'].tobytes().decode()
        rd = seq if r['v2_score'] > 0 else R.revcomp(seq)
        raw = R.local_raw(contigs, rd, [np.array(p, dtype=np.int64) for p in r['v2_paths']], 9, c['mode'])
        assert len(raw) == r['v3_raw_n'], (key, len(raw), r['v3_raw_n'])
        if key + '_v3_raw' in arrays:
            assert np.array_equal(raw, arrays[key + '_v3_raw'].reshape(-1, 4)), key
        else:
            assert zlib.crc32(np.ascontiguousarray(raw).tobytes()) == r['v3_raw_crc'], key
        n += 1
    assert n
