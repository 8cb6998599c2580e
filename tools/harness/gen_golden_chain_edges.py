#!/usr/bin/env python3
"""Record the REFERENCE's results on the constructed anchor sets of tests/chain_cases.py -> tests/golden/chain_edges.{json,npz}, and with the argument
`linked` tests/golden/chain_edges_linked.{json,npz}: the linked GC-exact / LC of mammap_asm.py (:21686 / :21504) on the sets given to vm_chain_linked, called the way the
reference's loop calls them (:23228-23272), with and without carried state. The state carried between two linked calls is built by chain_cases.py's
restatement of :23250-23272 from the reference's own arrays of the first call; the reference's loop itself is not run.

Per recorded set: the reference's strand flip (:21202), its exact global DP (_d_all :24828; mode R: mammap_noprefercloser.py) or, where the
reference switches (:23570, :23577), its fast one (_d_fast_all :25033) — g_max_index, S, P, S_arg — and decode_hit's MAPQ, score and paths
(:23981; hit2work_1 :23491 runs on the given anchors through an index object whose map() returns them). Inputs are stored next to the outputs.
The reference sources are imported in place and never copied. Under the stub an out-of-range index raises where numba would read garbage:
such a set has no defined answer, and the recorder refuses to write a fixture if any set raised."""
import json, os, sys
import numpy as np
_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(os.path.dirname(_HERE))
sys.path.insert(0, _ROOT); sys.path.insert(0, _HERE); sys.path.insert(0, os.path.join(_ROOT, 'tests'))
import refrun
import chain_cases as CC

GOLD = os.path.join(_ROOT, 'tests', 'golden')
D_ALL = 'get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_d_all'
D_FAST = 'get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_d_fast_all'


class GivenAnchors:
    """index_object of decode_hit: map() returns the constructed rows"""

    def __init__(self, rows, k):
        self.rows, self.k = rows, k

    def map(self, seq, check_num=100, mid_occ=-1):
        return [tuple(int(v) for v in r) for r in self.rows]


def new_arrays():
    """the fixture's arrays, one per kind, concatenated over the sets in the order of recording (offsets in the JSON)"""
    return {'a': [np.zeros((0, 4), np.int64)], 'S': [np.zeros(0, np.float64)], 'P': [np.zeros(0, np.int32)], 'SA': [np.zeros(0, np.int32)], 'paths': [np.zeros((0, 4), np.int64)]}


def record(c, arrays):
    m = refrun.load(c.mode)
    from numba.typed import Dict, List         # (the stub: on the path once the reference is loaded)
    skip = np.float64(CC.SKIP[c.mode])
    rec = {'mode': c.mode, 'label': c.label, 'readlen': c.readlen, 'maxdiff': c.maxdiff, 'n': len(c.anchors)}
    arrays['a'].append(c.anchors)
    if len(c.anchors) > 2:
        flag, fl = m.get_reversed_chain_numpy_rough(c.anchors.copy(), c.readlen)
        fl = np.ascontiguousarray(fl)
        srt = fl[np.argsort(fl[:, 0])]
        fast = len(srt) / c.readlen > 5
        if not fast:
            g, S, P, SA = getattr(m, D_ALL)(srt, kmersize=c.k, skipcost=skip, maxdiff=c.maxdiff, maxgap=CC.MAXGAP)[:4]
            fast = g == -1
        if fast:
            g, S, P, SA = getattr(m, D_FAST)(srt, kmersize=c.k, skipcost=skip, maxdiff=c.maxdiff, maxgap=CC.MAXGAP)[:4]
        rec.update(need_reverse=bool(flag), fast_used=bool(fast), gmax=int(g))
        rec['dp_off'] = sum(len(x) for x in arrays['S'])
        arrays['S'].append(np.asarray(S, dtype=np.float64)); arrays['P'].append(np.asarray(P, dtype=np.int32)); arrays['SA'].append(np.asarray(SA, dtype=np.int32))
    i2c = List(); i2c.append('c')
    c2s = Dict(); c2s['c'] = 0
    try:
        mapq, score, path, factor, rpl = m.decode_hit(GivenAnchors(c.anchors, c.k), i2c, 'A' * c.readlen, c.readlen, c2s, c.k, Dict(), skipcost=(skip, skip),
                                                     maxdiff=(c.maxdiff, c.maxdiff), maxgap=200, check_num=100, c_bias=5000, bin_size=100, overlapprecentage=0.5,
                                                     hastra=False, H=False, mid_occ=-1)
    except UnboundLocalError:          # mode R: `factor` is unbound when two anchors or fewer survive (mammap_noprefercloser.py:24417): the read raises
        assert c.mode == 'R' and len(c.anchors) <= 2
        mapq, score, rpl = 0, 0., []
        rec['raised'] = True
    rec.update(mapq=int(mapq), score=float(score), path_lens=[len(p) for p in rpl])
    rec['a_off'] = sum(len(x) for x in arrays['a'][:-1]); rec['path_off'] = sum(len(x) for x in arrays['paths'])
    arrays['paths'].append(np.array([tuple(int(v) for v in a) for p in rpl for a in p], dtype=np.int64).reshape(-1, 4))
    return rec


LINKED = {0: 'linked_get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_d_all',        # mammap_asm.py:21686
          2: 'linked_get_optimal_chain_sortbyreadpos_forSV_inv_test_merged_fine_list_all'}          # :21504


def reference_linked(rows, which, args, state):
    """the reference's linked DP, called as its loop calls it (mammap_asm.py:23222-23245): an empty state for the first batch"""
    m = refrun.load('asm')
    k, skip, md, mg = args
    if state is None:
        state = (0, 0, np.zeros(0, np.float64), np.zeros(0, np.int32), int(rows[0][0]))
    gms, gmi, pre_S, pre_P, prl = state
    res = getattr(m, LINKED[which])(gms, gmi, np.asarray(pre_S, np.float64), np.asarray(pre_P, np.int32), prl, rows, kmersize=k, skipcost=np.float64(skip), maxdiff=md, maxgap=mg)
    return int(res[0]), np.asarray(res[1], np.float64), np.asarray(res[2], np.int64), np.asarray(res[3], np.int64)


def record_linked(cases):
    meta, arr, off = {}, {'rows': [np.zeros((0, 4), np.int64)], 'S': [np.zeros(0, np.float64)], 'P': [np.zeros(0, np.int32)], 'SA': [np.zeros(0, np.int32)]}, 0
    for c in CC.linked_picks(cases):
        for which in CC.LINKED_ARGS:
            for name, rows, args, state, (g, S, P, SA) in CC.linked_runs(c, which, reference_linked):
                assert g >= 0
                meta['%s|%d|%s' % (CC.key(c), which, name)] = {'off': off, 'n': len(rows), 'g': g}
                arr['rows'].append(rows); arr['S'].append(S); arr['P'].append(P.astype(np.int32)); arr['SA'].append(SA.astype(np.int32))
                off += len(rows)
    json.dump(meta, open(os.path.join(GOLD, 'chain_edges_linked.json'), 'w'), indent=0, sort_keys=True)
    with open(os.path.join(GOLD, 'chain_edges_linked.npz'), 'wb') as f:
        np.savez_compressed(f, **{k: np.concatenate(v) for k, v in arr.items()})
    print('linked: %d calls, %d rows -> %d bytes' % (len(meta), off, os.path.getsize(os.path.join(GOLD, 'chain_edges_linked.npz'))))


def main():
    if 'linked' in sys.argv[1:]:
        return record_linked(CC.constructed())
    cases = [c for c in CC.constructed() if c.record]
    arrays, meta, raised = new_arrays(), {}, []
    for c in cases:
        try:
            meta[CC.key(c)] = record(c, arrays)
        except IndexError as e:
            raised.append((CC.key(c), repr(e)))
    assert not raised, 'sets without a defined answer (the reference indexes out of range): %r' % raised[:10]
    json.dump(meta, open(os.path.join(GOLD, 'chain_edges.json'), 'w'), indent=0, sort_keys=True)
    with open(os.path.join(GOLD, 'chain_edges.npz'), 'wb') as f:      # (np.savez_compressed stamps no time: the file is reproducible)
        np.savez_compressed(f, **{k: np.concatenate(v) for k, v in arrays.items()})
    print('%d sets, %d anchors -> %d + %d bytes' % (len(meta), sum(r['n'] for r in meta.values()), os.path.getsize(os.path.join(GOLD, 'chain_edges.json')),
                                                   os.path.getsize(os.path.join(GOLD, 'chain_edges.npz'))))


if __name__ == '__main__':
    main()
