#!/usr/bin/env python3
"""Record the REFERENCE's local chain DPs on the constructed rows of tests/local_dp_cases.py -> tests/golden/local_dp_edges.{json,npz}.

Per recorded set: the live definition of the DP that get_localmap_multi_all_forDP_inv_guide_list would call for the set's mode and guide count —
..._merged_fine_list (:27305), ..._merged_fine_list_mismatch (:28250), mode R: ..._merged_fine_list_scar (mammap_noprefercloser.py:23419) — on the rows in
the DP's input order, with the parameters that function passes: kmersize 9 unless the set says otherwise, maxgap 99 (mode L: 50), the set's skip cost
(mode L's LC-mm: min(skipcost, 40)), large_readgap 30. The `_fast` twins need no call of their own: the reference enters them itself (:27380 / :28333).
Score and path are recorded, the rows next to them (sets of more than DENSE rows keep a CRC-32 of their int64 rows instead: the generator is seeded).
The reference sources are imported in place (refrun + the numba stub) and never copied. Under the stub an out-of-range index raises where numba would
read garbage: such a set has no defined answer, and the recorder refuses to write a fixture if any set raised."""
import json, os, sys, zlib
import numpy as np
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
sys.path.insert(0, _ROOT); sys.path.insert(0, _HERE); sys.path.insert(0, os.path.join(_ROOT, 'tests'))
import refrun
import oracle_lib
import local_dp_cases as D

GOLD = os.path.join(_ROOT, 'tests', 'golden')
DENSE = 400
BASE = 'get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list'
FN = {0: BASE, 1: BASE + '_mismatch', 2: BASE + '_scar'}


def reference_dp(c):
    m = refrun.load(c.mode)
    kw = dict(kmersize=c.k, skipcost=np.float64(c.dp_skip), maxdiff=c.maxdiff, maxgap=c.maxgap)
    if c.variant == 1:
        kw['large_readgap'] = 30
    score, path = getattr(m, FN[c.variant])(np.ascontiguousarray(c.rows), **kw)
    return float(score), np.array([tuple(int(v) for v in a) for a in path], dtype=np.int64).reshape(-1, 4)


def main():
    T = D.oracle_tables(oracle_lib)
    cases = [c for c in D.constructed(T, largest=False) if c.record]
    meta, raised = {}, []
    arr = {'a': [np.zeros((0, 4), np.int64)], 'chain': [np.zeros((0, 4), np.int64)]}
    a_off = c_off = 0
    for c in cases:
        D.check_claims(c, T)                   # the edges are where the generator says
        try:
            score, path = reference_dp(c)
        except (IndexError, ZeroDivisionError) as e:
            raised.append((D.key(c), repr(e))); continue
        rec = {'mode': c.mode, 'ng': c.ng, 'k': c.k, 'maxdiff': c.maxdiff, 'skip': c.skip, 'readlen': c.readlen, 'n': len(c.rows), 'score': score, 'c_off': c_off, 'c_n': len(path)}
        if len(c.rows) > DENSE:
            rec['crc'] = zlib.crc32(np.ascontiguousarray(c.rows).tobytes())
        else:
            rec['a_off'] = a_off; arr['a'].append(c.rows); a_off += len(c.rows)
        arr['chain'].append(path); c_off += len(path)
        meta[D.key(c)] = rec
    assert not raised, 'sets without a defined answer (the reference indexes out of range): %r' % raised[:10]
    json.dump(meta, open(os.path.join(GOLD, 'local_dp_edges.json'), 'w'), indent=0, sort_keys=True)
    with open(os.path.join(GOLD, 'local_dp_edges.npz'), 'wb') as f:      # (np.savez_compressed stamps no time: the file is reproducible)
        np.savez_compressed(f, **{k: np.concatenate(v) for k, v in arr.items()})
    print('%d sets, %d rows stored, %d chain rows -> %d + %d bytes' % (len(meta), a_off, c_off, os.path.getsize(os.path.join(GOLD, 'local_dp_edges.json')),
                                                                      os.path.getsize(os.path.join(GOLD, 'local_dp_edges.npz'))))


if __name__ == '__main__':
    main()
