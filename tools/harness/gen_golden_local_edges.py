#!/usr/bin/env python3
"""Record the REFERENCE's raw local anchors on the constructed cases of tests/local_cases.py -> tests/golden/local_edges.{json,npz}.

Per read of every recordable case (the cases of both builds' sizes; not the derived 'mix' case, not -mode asm): the reference's
get_localmap_multi_all_forDP_inv_guide_list of the case's mode (mammap_clrnano.py:28479, mammap_ccs.py, mammap_sensitive.py,
mammap_noprefercloser.py) is called on the read, its reverse complement and its guide paths, with the case's contigs and local_kmersize, and the
array it hands to its local chain DP (the raw local anchors in the DP's input order) is captured. A read without any local anchor makes the
reference raise on the empty array (:28585): recorded as zero rows, told from any other exception by the list the re-seeding function
(..._guide_1) was given, which is then empty. The reference sources are imported in place (refrun + the numba stub) and never copied. Under the
stub an out-of-range index raises where numba would read garbage: such a read has no defined answer, and the recorder refuses to write a fixture
if any read raised otherwise. A case is recorded only if it is N-safe (local_cases.check_claims: D1 and text equality give the same rows).

The inputs are not stored: the generator is seeded, the fixture names the rows by case and read label. Reads with more than DENSE rows (the
tile and capacity families) keep a count and a CRC-32 of the int64 rows, as the V3 goldens do."""
import json, os, sys, zlib
import numpy as np
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
sys.path.insert(0, _ROOT); sys.path.insert(0, _HERE); sys.path.insert(0, os.path.join(_ROOT, 'tests'))
import refrun
import local_cases as LC

GOLD = os.path.join(_ROOT, 'tests', 'golden')
DENSE = 400
LIST = 'get_localmap_multi_all_forDP_inv_guide_list'
ONE = 'get_localmap_multi_all_forDP_inv_guide_1'
LC_DP = ['get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list', 'get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_mismatch',
         'get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_scar']
SKIP = {'H': 40., 'L': 59., 'S': 30., 'R': 30.}


class Captured(Exception):
    pass


def reference_raw(case, i):
    """the rows the reference's L1 + L2 give its local chain DP for read i, or None if it raised for another reason than an empty array"""
    m = refrun.load(case.mode)
    from numba.typed import Dict, List         # (the stub: on the path once the reference is loaded)
    c2s, c2q, off = Dict(), Dict(), 0
    for ci, s in enumerate(case.contigs):
        c2s['c%d' % ci] = off; c2q['c%d' % ci] = s.upper(); off += len(s)
    cap = {}
    orig = {n: getattr(m, n) for n in LC_DP + [ONE] if hasattr(m, n)}

    def dp(one_mapinfo, **kw):                 # the DP itself is not this fixture's subject: stop here
        cap['raw'] = np.array(one_mapinfo, dtype=np.int64).reshape(-1, 4)
        raise Captured()

    def one(*a, **kw):                         # (the list is the third argument, in mode R the first)
        cap['list'] = next(x for x in a if isinstance(x, list))
        return orig[ONE](*a, **kw)
    for n in orig:
        setattr(m, n, one if n == ONE else dp)
    rd = case.reads[i]
    seq = rd.seq.decode().upper()
    try:
        getattr(m, LIST)(List([np.array(p, dtype=np.int64) for p in rd.paths]), seq, LC.R.revcomp(seq), c2s, c2q, kmersize=case.k,
                         skipcost=np.float64(SKIP[case.mode]), maxdiff=30, maxgap=(50 if case.mode == 'L' else 99), shift=1)
    except Captured:
        return cap['raw']
    except IndexError:
        if 'raw' not in cap and 'list' in cap and len(cap['list']) == 0:
            return np.zeros((0, 4), np.int64)
        return None
    finally:
        for n, f in orig.items():
            setattr(m, n, f)
    return None


def recordable():
    """(case, build or None) of every case that goes into the fixture, the build-dependent ones once per build"""
    seen, out = set(), []
    for b in LC.BUILDS:
        for c in LC.constructed(b):
            if c.family == 'mix' or c.mode == 'asm' or c.label in seen:
                continue
            seen.add(c.label); out.append(c)
    return out


def main():
    meta, rows, raised, off = {}, [np.zeros((0, 4), np.int64)], [], 0
    for c in recordable():
        LC.check_claims(c)                     # N-safe, and the edges are where the generator says
        for i, rd in enumerate(c.reads):
            raw = reference_raw(c, i)
            if raw is None:
                raised.append((c.label, rd.label)); continue
            rec = {'n': len(raw)}
            if len(raw) > DENSE:
                rec['crc'] = zlib.crc32(np.ascontiguousarray(raw).tobytes())
            else:
                rec['off'] = off; rows.append(raw); off += len(raw)
            meta['%s|%s' % (c.label, rd.label)] = rec
    assert not raised, 'reads without a defined answer (the reference raised): %r' % raised[:10]
    json.dump(meta, open(os.path.join(GOLD, 'local_edges.json'), 'w'), indent=0, sort_keys=True)
    with open(os.path.join(GOLD, 'local_edges.npz'), 'wb') as f:      # (np.savez_compressed stamps no time: the file is reproducible)
        np.savez_compressed(f, rows=np.concatenate(rows))
    print('%d reads, %d rows -> %d + %d bytes' % (len(meta), off, os.path.getsize(os.path.join(GOLD, 'local_edges.json')),
                                                 os.path.getsize(os.path.join(GOLD, 'local_edges.npz'))))


if __name__ == '__main__':
    main()
