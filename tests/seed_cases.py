"""Constructed hit sets for map() (k_lookup, k_fill_hits, k_cluster / k_cluster_big / k_cluster_long / k_cluster_gen; the index's default
occurrence cap) and the shared checks.

A seeded, deterministic generator of cases (label, contigs, k, w, reads, list of (check_num, mid_occ), expected routing) placed AT the edges of
VMX-S1's lookup and cluster rules (tests/spec_ref.py: map_read, default_mid_occ) and at the size classes of the cluster kernels.
Shared by test_seed_edges.py (the generator's self-check and the oracle), test_emu_seed_edges.py and test_gpu_seed_edges.py.

The construction: with w = 1 every valid k-mer start is a minimizer. The reference is a run of N (no valid k-mer) with chosen k-mers ("probes":
valid, not their own reverse complement, all distinct up to reverse complement) planted at chosen positions, each with an N on either side;
the index then holds exactly the planted occurrences. A read made of probes separated by N has exactly one minimizer per probe, so its hits
are the ones the generator writes down (Case.intended), to the position. Every family is emitted as it stands and with every read reverse-
complemented (q -> L - q - k, s -> -s), and each family's reference also carries a "ballast" block of probes planted 64 times each, from which two
more reads of the other size classes (320 and 4224 hits; the latter is declined by the first filtered form) ride in every map_batch call.

Expected routing. vmx_seed_stage sends a read by its hit count n to k_cluster (n <= VMX_SORT_LDS; 'small'), to the filtered form k_cluster_big
(n <= 0x3fff; 'big'), or to the LONG filtered form k_cluster_long ('long'); what a filtered form declines goes on to the next one and at last
to the general path k_cluster_gen ('gen'). `path()` states who answers: a filtered form takes a read iff 0 < check_num <= 1024, n is within
its hit limit (0x3fff / 0xffff), the number of candidates (hits with another hit in their own or an adjacent 8192-bp reference bin) is within
its cap, and the check_num-th largest cluster of two or more, if there is one, has fewer than 1023 hits (the size histogram's overflow bin).
ROUTINGS lowers the two hit-count thresholds through the test knobs VMX_CLUSTER_SMALL_MAX / VMX_CLUSTER_HUGE_MIN so that small reads reach
the filtered forms. The emulator tests assert the path with the emulator build's counters; BUILDS holds the constants of either build.

Not covered here: aliasing of filter slots. Two reference bins share a slot only 2^31 bp apart in the filtered form and 2^32 bp apart in the
LONG form (2^28 in the emulator build), which needs a multi-Gb reference and does not fit a test of a few seconds; the filter is a superset
test by design, so aliasing can only add candidates, never lose a cluster. test_gpu_hg38.py runs an index of that size."""
import math
import numpy as np
import spec_ref as R

BIN = 8192                        # reference bases per filter bin
GAP = 5000                        # VMX-S1's cluster cut: a gap of more than this
BIG_MAX_HITS, LONG_MAX_HITS = 0x3fff, 0xffff
CF_MAX_CHECK = 1024               # the filtered forms take 0 < check_num <= 1024
CF_OVERFLOW = 1023                # size histogram: bin 1023 = this size and larger
BUILDS = {'emu': dict(SORT_LDS=4096, SORT_LDS_BIG=8192, CF_CAND=2048, CFB_CAP=8192 - 1024),
          'gfx950': dict(SORT_LDS=4096, SORT_LDS_BIG=16384, CF_CAND=4096, CFB_CAP=16384 - 1024)}
ROUTINGS = {'default': {}, 'big': {'VMX_CLUSTER_SMALL_MAX': '0'}, 'long': {'VMX_CLUSTER_SMALL_MAX': '0', 'VMX_CLUSTER_HUGE_MIN': '0'}}
BALLAST_AT, BALLAST_PROBES, BALLAST_COPIES = 6 * BIN, 70, 64
FIRST = 32 * BIN                  # the families' own placements start here (bins 0 and 1 belong to the filter family)

_RC = str.maketrans('ACGTN', 'TGCAN')


def revcomp(s):
    return s.translate(_RC)[::-1]


def read_of(probes, sep='N'):
    """the read: the probe strings with one `sep` between neighbours; probe i starts at i (k + 1)"""
    return sep.join(probes)


def plant(placements, contig_lens):
    """contigs of N with the strings of `placements` = [(global position, string)] at exactly those positions; every planted string keeps an N
    (or a contig end) on either side and lies inside one contig, so no k-mer other than the planted ones is valid"""
    total = int(sum(contig_lens))
    ref = np.full(total + 2, ord('N'), np.uint8)                              # one guard byte on either side
    ends = np.cumsum(contig_lens); starts = ends - np.asarray(contig_lens)
    for g, s in placements:
        c = int(np.searchsorted(ends, g, 'right'))
        assert 0 <= g and g + len(s) <= ends[c] and g >= starts[c], ('placement leaves its contig', g)
        assert (ref[g:g + len(s) + 2] == ord('N')).all(), ('placements touch', g)
        ref[g + 1:g + 1 + len(s)] = np.frombuffer(s.encode(), np.uint8)
    ref = ref[1:-1]
    return [ref[a:b].tobytes().decode() for a, b in zip(starts, ends)]


class Read:
    def __init__(self, label, seq, elems, params=None):
        self.label, self.seq, self.elems, self.params = label, seq, elems, params       # elems: [(q, probe id, orientation)], None = not stated


class Case:
    def __init__(self, label, contigs, k, w, reads, params, place, claims):
        self.label, self.family, self.contigs, self.k, self.w = label, label.split('/')[0], contigs, k, w
        self.reads, self.params, self.place, self.claims = reads, params, place, claims

    def read(self, label):
        return next(i for i, r in enumerate(self.reads) if r.label == label)

    def intended(self, i, mid_occ):
        """the hit set the generator means read i to have under the cap mid_occ: rows (q, r, s, k) in (r, q, s) order"""
        rows = [(q, g, 1 if o == po else -1, self.k) for q, pid, o in self.reads[i].elems if len(self.place.get(pid, ())) <= mid_occ
                for g, po in self.place.get(pid, ())]
        a = np.array(rows, dtype=np.int64).reshape(-1, 4)
        return a[np.lexsort((a[:, 2], a[:, 0], a[:, 1]))]


class Plan:
    """collects the probes, placements and reads of one case"""

    def __init__(self, label, rng, k=15, w=1, ballast=True, contig_lens=None):
        self.label, self.rng, self.k, self.w, self.contig_lens = label, rng, k, w, contig_lens
        self.probes, self.used, self.place, self.reads, self.claims, self.end = [], set(), {}, [], [], 0
        self.ball = []
        if ballast:
            self.ball = [self.probe() for _ in range(BALLAST_PROBES)]
            for i in range(BALLAST_PROBES * BALLAST_COPIES):
                self.put(self.ball[i % BALLAST_PROBES], BALLAST_AT + (k + 1) * i)
            assert self.end <= FIRST - 4 * BIN

    def probe(self):
        """a random k-mer that is valid, is not its own reverse complement and repeats no earlier probe or its reverse complement"""
        while True:
            s = ''.join('ACGT'[i] for i in self.rng.integers(0, 4, self.k)); rc = revcomp(s)
            if s != rc and s not in self.used and rc not in self.used:
                self.used.add(s); self.probes.append(s)
                return len(self.probes) - 1

    def put(self, pid, gpos, orient=1):
        self.place.setdefault(pid, []).append((int(gpos), orient))
        self.end = max(self.end, int(gpos) + self.k)

    def read(self, label, elems, shuffle=True, params=None):
        """elems: probe ids, or (probe id, -1) for the probe's reverse complement; handed over in shuffled order, so that read order differs
        from reference order"""
        elems = [e if isinstance(e, tuple) else (e, 1) for e in elems]
        if shuffle:
            elems = [elems[i] for i in self.rng.permutation(len(elems))]
        seq = read_of([self.probes[p] if o == 1 else revcomp(self.probes[p]) for p, o in elems])
        self.reads.append(Read(label, seq, [(i * (self.k + 1), p, o) for i, (p, o) in enumerate(elems)], params))

    def raw(self, label, seq):
        self.reads.append(Read(label, seq, []))

    def claim(self, *c):
        self.claims.append(c)

    def case(self, params, rc=True, total=None):
        k = self.k
        reads = list(self.reads)
        if rc:
            for rd in [x for x in self.reads if rc is True or rc(x)]:
                L = len(rd.seq)
                reads.append(Read(rd.label + '/rc', revcomp(rd.seq), [(L - q - k, p, -o) for q, p, o in rd.elems], rd.params))
        if self.ball:
            for n in (5, 66):
                el = [(i * (k + 1), p, 1) for i, p in enumerate(self.ball[:n])]
                reads.append(Read('ballast/%d' % (n * BALLAST_COPIES), read_of([self.probes[p] for _, p, _ in el]), el))
        lens = self.contig_lens or [total or (self.end + 100)]
        contigs = plant([(g, self.probes[p] if o == 1 else revcomp(self.probes[p])) for p, pl in self.place.items() for g, o in pl], lens)
        return Case(self.label, contigs, k, self.w, reads, list(params), self.place, self.claims)


# ------------------------------------------------------------------------------------------------ the spec's view of a case, cached
class Spec:
    def __init__(self, case):
        self.case = case
        self.IH, self.IP = R.index_minimizers(case.contigs, case.k, case.w)
        self._hits, self._rows = {}, {}

    def hits(self, i, mid_occ):
        """every hit of read i in (r, q, s) order"""
        if (i, mid_occ) not in self._hits:
            c = self.case
            h = R.lookup_hits(self.IH, self.IP, c.k, c.w, c.reads[i].seq, mid_occ)
            self._hits[i, mid_occ] = h[np.lexsort((h[:, 2], h[:, 0], h[:, 1]))]
        return self._hits[i, mid_occ]

    def rows(self, i, check_num, mid_occ):
        if (i, check_num, mid_occ) not in self._rows:
            self._rows[i, check_num, mid_occ] = R.cluster_hits(self.hits(i, mid_occ), check_num)
        return self._rows[i, check_num, mid_occ]

    def sizes(self, i, mid_occ):
        """cluster sizes in rank order"""
        r = self.rows(i, 0, mid_occ)[:, 1]
        # (rank order emits cluster after cluster: a new one starts where r steps back or jumps by more than GAP)
        d = np.diff(r)
        return np.diff(np.concatenate([[0], np.nonzero((d > GAP) | (d < 0))[0] + 1, [len(r)]])).tolist() if len(r) else []


_SPECS = {}


def spec_of(case):
    if case.label not in _SPECS:
        _SPECS[case.label] = Spec(case)
    assert _SPECS[case.label].case is case
    return _SPECS[case.label]


# ------------------------------------------------------------------------------------------------ expected routing
def ncand(r):
    """hits with another hit in their own or an adjacent bin"""
    b, cnt = np.unique(np.asarray(r) // BIN, return_counts=True)
    occ = dict(zip(b.tolist(), cnt.tolist()))
    return sum(c for x, c in occ.items() if c >= 2 or x - 1 in occ or x + 1 in occ)


def _filtered_takes(r, check_num, max_hits, cap):
    if not 0 < check_num <= CF_MAX_CHECK or len(r) > max_hits or ncand(r) > cap:
        return False
    r = np.sort(r)
    sz = np.diff(np.concatenate([[0], np.nonzero(np.diff(r) > GAP)[0] + 1, [len(r)]]))
    multi = np.sort(sz[sz >= 2])[::-1]
    return not (len(multi) >= check_num and multi[check_num - 1] >= CF_OVERFLOW)


def path(r, check_num, build, routing):
    """the forms that see a read with hits at reference positions r, in order; the last one answers"""
    B = BUILDS[build]
    n = len(r)
    if n <= (B['SORT_LDS'] if routing == 'default' else 0):
        return ('small',)
    p = ()
    if n <= (0 if routing == 'long' else BIG_MAX_HITS):
        p += ('big',)
        if _filtered_takes(r, check_num, BIG_MAX_HITS, B['CF_CAND']):
            return p
    p += ('long',)
    if _filtered_takes(r, check_num, LONG_MAX_HITS, B['CFB_CAP']):
        return p
    return p + ('gen',)


def counts_of(p):
    """(reads answered, reads declined) the filtered forms count for one read on path p"""
    f = [x for x in p if x in ('big', 'long')]
    return (1, len(f) - 1) if f and p[-1] != 'gen' else (0, len(f))


# ------------------------------------------------------------------------------------------------ families
CUT_PARAMS = [(1, 64), (2, 64), (100, 64), (-1, 64), (2, 1)]


def _cut_groups(P, at, step):
    """the cluster-cut family's groups from global position `at` on, `step` apart; returns the probes of all of them"""
    every = []
    for d in (4999, 5000, 5001, 5002):
        a, b = P.probe(), P.probe()
        P.put(a, at + 137); P.put(b, at + 137 + d); P.read('pair/%d' % d, [b, a], shuffle=False)
        P.claim('sizes', 'pair/%d' % d, 64, [2] if d <= GAP else [1, 1])
        every += [a, b]; at += step
    for name, odd in (('chain/5000', None), ('chain/5001', 7)):
        ch = [P.probe() for _ in range(12)]
        pos = at
        for i, p in enumerate(ch):
            P.put(p, pos); pos += GAP + (1 if i + 1 == odd else 0)
        P.read(name, ch); P.claim('sizes', name, 64, [12] if odd is None else [7, 5])
        every += ch; at += 12 * GAP + step
    a, b = P.probe(), P.probe()                                 # one probe twice in the read: two hits at one r, ordered by q
    P.put(a, at); P.put(b, at + 3000); P.read('same_r', [a, b, a], shuffle=False); P.claim('sizes', 'same_r', 64, [3])
    every += [a, b]; at += step
    a, b = P.probe(), P.probe()                                 # a probe and its reverse complement in the read: one r on both strands
    P.put(a, at); P.put(b, at + GAP, -1); P.read('both_strands', [(a, -1), b, a], shuffle=False); P.claim('sizes', 'both_strands', 64, [3])
    every += [a, b]
    P.read('all', every)
    return every


def cut_cases(rng):
    P = Plan('cut/one_contig', rng)
    _cut_groups(P, FIRST, 8 * BIN)
    out = [P.case(CUT_PARAMS)]
    # the same cut across contig boundaries: global positions run on, so a cluster may span two contigs
    lens = [FIRST + 40000, 60000, 60000, 60000, 60000, 30000, 30000]
    P = Plan('cut/contig_boundary', rng, contig_lens=lens)
    every = []
    edge = lens[0]
    for d in (4999, 5000, 5001, 5002):
        a, b = P.probe(), P.probe()
        P.put(a, edge - 2000); P.put(b, edge - 2000 + d); P.read('pair/%d' % d, [b, a], shuffle=False)
        P.claim('sizes', 'pair/%d' % d, 64, [2] if d <= GAP else [1, 1]); P.claim('spans_contigs', 'pair/%d' % d)
        every += [a, b]; edge += 60000
    a, b = P.probe(), P.probe()                                 # the first and the last k-mer of a contig; the contig after it is all N
    P.put(a, sum(lens[:5])); P.put(b, sum(lens[:6]) - 15)
    P.read('all', every + [a, b])
    out.append(P.case(CUT_PARAMS))
    return out


def bins_cases(rng):
    total = 130 * BIN + 5000                                    # the reference ends inside its last bin
    P = Plan('bins/edges', rng)
    every = []
    m = FIRST // BIN

    def grp(name, pos, sizes, nc):
        nonlocal m
        ps = [P.probe() for _ in pos]
        for p, g in zip(ps, pos):
            P.put(p, g)
        P.read(name, ps[::-1], shuffle=False); P.claim('sizes', name, 64, sizes); P.claim('ncand', name, 64, nc)
        every.extend(ps); m += 8

    grp('straddle', [BIN * m - 1, BIN * m + 4999], [2], 2)
    for d in (5001, 8191, 8192, 8193):                          # adjacent bins, too far for a cluster: candidates, two clusters of one
        grp('adjacent/%d' % d, [BIN * m + 8000, BIN * m + 8000 + d], [1, 1], 2)
    grp('same_bin/near', [BIN * m + 10, BIN * m + 4010], [2], 2)
    grp('same_bin/far', [BIN * m + 10, BIN * m + 8000], [1, 1], 2)
    grp('two_bins_apart', [BIN * m + 8000, BIN * (m + 2) + 10], [1, 1], 0)
    grp('three_bins', [BIN * m + 8000, BIN * m + 13000, BIN * m + 18000], [3], 3)
    grp('bin0_bin1', [0, BIN + 100], [1, 1], 2)
    grp('last_bin', [total - 15 - 6000, total - 15], [1, 1], 2)
    P.claim('last_bin_is_last', 'last_bin')
    P.read('all', every)
    P.claim('ncand', 'all', 64, 2 + 8 + 2 + 2 + 0 + 3 + 2 + 2)
    return [P.case([(1, 64), (3, 64), (5, 64), (12, 64), (100, 64), (-1, 64)], total=total)]


RANK_SIZES = [5, 3, 3, 3, 2, 2, 1, 1, 1, 1]


def rank_cases(rng):
    """clusters of sizes {5, 3, 3, 3, 2, 2, 1, 1, 1, 1}, reference order unlike size order; the singletons alternate between candidate clusters
    of one ('c': 6000 before the next cluster, in its bin) and isolated hits ('i'), so the singleton cut-off meets both kinds on either side"""
    P = Plan('rank/ties', rng)
    layout = ['c', 3, 2, 'i', 5, 3, 'c', 2, 3, 'i']
    m = FIRST // BIN
    every, subset = [], []
    for x in layout:
        if x == 'c':
            p = P.probe(); P.put(p, BIN * m + 1000); every.append(p); subset.append(p)          # the next group starts 6000 on, same bin
            continue
        if x == 'i':
            p = P.probe(); P.put(p, BIN * m + 3000); every.append(p); m += 6
            continue
        ps = [P.probe() for _ in range(x)]
        for j, p in enumerate(ps):
            P.put(p, BIN * m + 7000 + 100 * j)
        every += ps; m += 6
        if x != 5:
            subset += ps
    P.read('all', every); P.read('no_five_no_isolated', subset)
    P.claim('sizes', 'all', 64, RANK_SIZES); P.claim('ncand', 'all', 64, 18 + 2); P.claim('order_differs', 'all', 64)
    P.claim('sizes', 'no_five_no_isolated', 64, [3, 3, 3, 2, 2, 1, 1])
    for cn in (2, 3, 5):
        P.claim('cut_in_tie', 'all', 64, cn)
    for cn in (1, 4, 6):
        P.claim('cut_between_sizes', 'all', 64, cn)
    for cn in (7, 8, 9):
        P.claim('cut_in_singletons', 'all', 64, cn)
    params = [(cn, 64) for cn in list(range(1, 12)) + [50, 1024, 1025, 0, -1]]
    for bld in BUILDS:
        for cn in (1, 6, 7, 11, 1024):
            P.claim('path', 'all', cn, 64, bld, 'big', ('big',)); P.claim('path', 'all', cn, 64, bld, 'long', ('long',))
        for cn in (1025, 0, -1):
            P.claim('path', 'all', cn, 64, bld, 'big', ('big', 'long', 'gen')); P.claim('path', 'all', cn, 64, bld, 'long', ('long', 'gen'))
        P.claim('path', 'all', 3, 64, bld, 'default', ('small',))
    return [P.case(params)]


def overflow_cases(rng):
    """three clusters of 1022, 1023 and 1100 hits (blocks of probes planted over and over, 16 bp apart) beside many small ones. In read 'all' check_num
    1 and 2 put the cut among clusters of 1023 hits and more, which the size histogram cannot tell apart (the filtered forms decline), 3 and 4 just
    below. Read 'two' has the 1023 and the 1022 alone with one cluster of three: 2048 candidates, the emulator build's cap."""
    P = Plan('overflow/1023', rng)
    X, Y = [P.probe() for _ in range(50)], [P.probe() for _ in range(25)]
    at = FIRST
    for size, blk in ((1022, X), (1100, Y), (1023, X)):          # reference order unlike size order
        for i in range(size):
            P.put(blk[i % len(blk)], at + 16 * i)
        at += 16 * size + 3 * BIN
    small = []
    for size in [3] * 6 + [2] * 6 + [1] * 5:
        ps = [P.probe() for _ in range(size)]
        for j, p in enumerate(ps):
            P.put(p, at + 200 * j)
        small += ps; at += 3 * BIN
    P.read('all', X + Y + small); P.read('two', X + small[:3])
    P.claim('sizes', 'all', 200, [1100, 1023, 1022] + [3] * 6 + [2] * 6 + [1] * 5); P.claim('ncand', 'all', 200, 3145 + 30)
    P.claim('sizes', 'two', 200, [1023, 1022, 3]); P.claim('ncand', 'two', 200, 2048)
    for bld, B in BUILDS.items():
        first = ('big',) if 3145 + 30 <= B['CF_CAND'] else ('big', 'long')
        for cn, declined in ((1, True), (2, True), (3, False), (4, False), (30, False)):
            P.claim('path', 'all', cn, 200, bld, 'big', ('big', 'long', 'gen') if declined else first)
            P.claim('path', 'all', cn, 200, bld, 'long', ('long', 'gen') if declined else ('long',))
        P.claim('path', 'all', 1, 200, bld, 'default', ('small',))
        P.claim('path', 'two', 1, 200, bld, 'big', ('big', 'long', 'gen')); P.claim('path', 'two', 1, 200, bld, 'long', ('long', 'gen'))
        P.claim('path', 'two', 2, 200, bld, 'big', ('big',)); P.claim('path', 'two', 2, 200, bld, 'long', ('long',))
    return [P.case([(1, 200), (2, 200), (3, 200), (4, 200), (30, 200), (-1, 200), (3, 64)])]


OCC_COUNTS = [1, 2, 9, 10, 11, 63, 64, 65, 66, 199, 200, 201, 300]
OCC_CAPS = [1, 10, 64, 65, 200, 400]


def occ_cases(rng):
    """probes planted mid_occ - 1, mid_occ and mid_occ + 1 times for mid_occ in {1, 10, 64, 65, 200}; more than 64 and more than 256 occurrences next
    to single ones (k_fill_hits copies a wavefront's hits 64 at a time); reads of 300 minimizers of which only the first or the last has hits
    (k_lookup walks them 256 at a time); reads without any hit, without any k-mer, and the empty read"""
    P = Plan('occ/cap', rng)
    ps = [P.probe() for _ in OCC_COUNTS]
    ones = [P.probe() for _ in range(3)]
    slots = [p for p, c in zip(ps, OCC_COUNTS) for _ in range(c)] + ones
    for i, j in enumerate(rng.permutation(len(slots))):
        P.put(slots[j], FIRST + 48 * i)
    absent = [P.probe() for _ in range(299)]
    P.read('all', [ones[0], ps[12], ones[1], ps[8], ones[2]] + ps[:8] + ps[9:12], shuffle=False)
    P.read('last_of_300', absent + [ps[2]], shuffle=False); P.read('first_of_300', [ps[3]] + absent, shuffle=False)
    P.read('no_hit', absent[:5])
    P.raw('empty', ''); P.raw('shorter_than_k', 'ACGTACGTAC'); P.raw('only_N', 'N' * 40)
    for cap in OCC_CAPS:
        P.claim('nhits', 'all', cap, 3 + sum(c for c in OCC_COUNTS if c <= cap))
    P.claim('nhits', 'last_of_300', 64, 9); P.claim('nhits', 'first_of_300', 64, 10); P.claim('nhits', 'first_of_300', 1, 0)
    for lab in ('no_hit', 'empty', 'shorter_than_k', 'only_N'):
        P.claim('nhits', lab, 400, 0)
    return [P.case([(cn, cap) for cap in OCC_CAPS for cn in (3, -1)])]


def default_cap_cases(rng):
    """references whose distinct-hash count nd and occurrence counts put the quantile index floor((1 - 2e-4) nd) on the largest count (50), on the
    second largest (30, with the 50 above it) and among the single ones (the floor of 10); nd on either side of the step; nd = 1. No ballast here:
    its probes would move the quantile."""
    out = []

    def one(label, counts, cap):
        P = Plan('defcap/' + label, rng, ballast=False)
        ps = [P.probe() for _ in counts]
        slots = [p for p, c in zip(ps, counts) for _ in range(c)]
        for i, j in enumerate(rng.permutation(len(slots))):
            P.put(slots[j], 16 * i)
        P.read('probes', ps[:4]); P.claim('mid_occ', cap); P.claim('nhits', 'probes', -1, sum(c for c in counts[:4] if c <= cap))
        out.append(P.case([(5, -1), (-1, -1), (5, 64)]))

    one('floor', [5, 1, 1, 1] + [1] * 196, 10)
    one('nd1/30', [30], 31)
    one('nd1/3', [3], 10)
    for nd in (4999, 5000, 5001, 5002, 10001):
        kth = min(math.floor((1 - 2e-4) * nd), nd - 1)
        one('nd%d' % nd, [50, 30, 1, 1] + [1] * (nd - 4), {0: 51, 1: 31}.get(nd - 1 - kth, 10))
    return out


def size_cases(rng, build):
    """hit counts at the size classes of the build under test: a block of 1030 probes planted 64 times each in runs 16 bp apart, cut into dense
    clusters of 5 ... 12 runs (320 ... 768 hits) by gaps of 6000; six more probes planted 1, 2, 4, ... 32 times for the remainder; a dozen
    probes planted once, two bins from everything, for isolated hits. A read of the first a block probes has 64 a hits, all candidates."""
    B = BUILDS[build]
    P = Plan('sizes/' + build, rng, ballast=False)
    NB = 1030
    rem = [P.probe() for _ in range(6)]
    blk = [P.probe() for _ in range(NB)]
    at = FIRST
    for b, p in enumerate(rem):                                  # the remainder probes, just before the block (its bin, or the one before)
        for i in range(1 << b):
            P.put(p, at); at += 16
    run_in_group, group = 0, 5
    for p in blk:
        for i in range(64):
            P.put(p, at); at += 16
        run_in_group += 1
        if run_in_group == group:
            at += 6000; run_in_group = 0; group = int(rng.integers(5, 13))
    at = (at // BIN + 3) * BIN
    iso = []
    for _ in range(12):
        p = P.probe(); P.put(p, at + 100); iso.append(p); at += 2 * BIN

    def rd(label, n_dense, n_iso=0, params=None):
        a, r = divmod(n_dense, 64)
        P.read(label, blk[:a] + [rem[b] for b in range(6) if r >> b & 1] + iso[:n_iso], params=params)
        P.claim('nhits', label, 64, n_dense + n_iso)
        if n_dense >= 2:
            P.claim('ncand', label, 64, n_dense)

    few = [(3, 64), (-1, 64)]
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097):
        rd('hits/%d' % n, n)
    rd('cand_cap', B['CF_CAND'], 10); rd('cand_cap+1', B['CF_CAND'] + 1, 10)
    rd('long_cand_cap', B['CFB_CAP'], 10, few); rd('long_cand_cap+1', B['CFB_CAP'] + 1, 10, few)
    for n in sorted({B['SORT_LDS_BIG'] - 1, B['SORT_LDS_BIG'], B['SORT_LDS_BIG'] + 1, BIG_MAX_HITS, BIG_MAX_HITS + 1}):
        rd('hits/%d' % n, n, 0, few)
    rd('hits/65535', 0xffff - 10, 10, few); rd('hits/65536', 0x10000 - 10, 10, few); rd('hits/65801', 65801 - 10, 10, few)
    for rt in ('default', 'big'):
        if rt == 'default' and B['CF_CAND'] + 11 <= B['SORT_LDS']:            # (the emulator build's cap lies below k_cluster's tile)
            P.claim('path', 'cand_cap', 3, 64, build, rt, ('small',)); P.claim('path', 'cand_cap+1', 3, 64, build, rt, ('small',))
        else:
            P.claim('path', 'cand_cap', 3, 64, build, rt, ('big',)); P.claim('path', 'cand_cap+1', 3, 64, build, rt, ('big', 'long'))
        P.claim('path', 'long_cand_cap', 3, 64, build, rt, ('big', 'long')); P.claim('path', 'long_cand_cap+1', 3, 64, build, rt, ('big', 'long', 'gen'))
    P.claim('path', 'long_cand_cap', 3, 64, build, 'long', ('long',)); P.claim('path', 'long_cand_cap+1', 3, 64, build, 'long', ('long', 'gen'))
    P.claim('path', 'hits/4096', 3, 64, build, 'default', ('small',)); P.claim('path', 'hits/4097', 3, 64, build, 'default', ('big', 'long'))
    P.claim('path', 'hits/16383', 3, 64, build, 'default', ('big', 'long', 'gen')); P.claim('path', 'hits/16384', 3, 64, build, 'default', ('long', 'gen'))
    P.claim('path', 'hits/65535', 3, 64, build, 'default', ('long', 'gen')); P.claim('path', 'hits/65536', 3, 64, build, 'default', ('long', 'gen'))
    P.claim('path', 'hits/2048', 3, 64, build, 'big', ('big',)); P.claim('path', 'hits/2048', 3, 64, build, 'long', ('long',))
    return [P.case([(3, 64), (100, 64), (-1, 64)], rc=lambda rd: rd.params is None)]       # (the reads of 7000 hits and more only as they stand)


def kform_cases(rng):
    """k = 17 and k = 28 (the 64-bit sketch) on the cluster-cut groups; w = 10 on a random reference with a repeat, where the hit set is not stated
    and only the spec decides"""
    out = []
    for k in (17, 28):
        P = Plan('kform/k%d' % k, rng, k=k)
        _cut_groups(P, FIRST, 8 * BIN)
        out.append(P.case([(2, 64), (100, 64), (-1, 64)]))
    from kernel_cases import rand_seq, mutate
    unit = rand_seq(rng, 700)
    ref = rand_seq(rng, 9000) + unit + rand_seq(rng, 5600) + unit + rand_seq(rng, 12000) + mutate(rng, unit, 0.03) + rand_seq(rng, 4000)
    reads = [Read('unique', mutate(rng, ref[2000:5000], 0.04), None), Read('repeat', ref[8800:10200], None), Read('repeat/rc', revcomp(ref[8800:10200]), None),
             Read('span', mutate(rng, ref[14000:30000], 0.08), None)]
    out.append(Case('kform/w10', [ref[:20000], ref[20000:]], 15, 10, reads, [(1, -1), (3, -1), (-1, -1), (3, 2), (-1, 1)], {}, []))
    return out


_CASES = {}


def generate():
    """the families that do not depend on the build, made afresh"""
    rng = np.random.default_rng(20240607)
    return cut_cases(rng) + bins_cases(rng) + rank_cases(rng) + overflow_cases(rng) + occ_cases(rng) + default_cap_cases(rng) + kform_cases(rng)


def constructed(build):
    """every case, for the build under test ('emu' or 'gfx950'; only the size-class family depends on it); made once"""
    if build not in _CASES:
        if 'shared' not in _CASES:
            _CASES['shared'] = generate()
        _CASES[build] = _CASES['shared'] + size_cases(np.random.default_rng(20240608), build)
    return _CASES[build]


# ------------------------------------------------------------------------------------------------ shared checks
def reads_for(case, check_num, mid_occ):
    return [i for i, rd in enumerate(case.reads) if rd.params is None or (check_num, mid_occ) in rd.params]


def same(got, exp, case, rd, check_num, mid_occ, what):
    if np.array_equal(got, exp):
        return
    n = min(len(got), len(exp))
    d = np.nonzero((np.asarray(got)[:n] != exp[:n]).any(axis=1))[0]
    at = int(d[0]) if len(d) else n
    raise AssertionError('%s: %s read %s check_num %d mid_occ %d: %d rows against the spec\'s %d; first differing row %d: %s against %s'
                         % (what, case.label, rd.label, check_num, mid_occ, len(got), len(exp), at,
                            got[at].tolist() if at < len(got) else None, exp[at].tolist() if at < len(exp) else None))


def check_claims(case, sp):
    """the generator's self-check: the intended hits are the spec's, and every stated property holds under the spec"""
    mids = sorted({mo for _, mo in case.params})
    for i, rd in enumerate(case.reads):
        if rd.elems is None:
            continue
        for mo in mids:
            cap = mo if mo > 0 else R.default_mid_occ(sp.IH)
            same(sp.hits(i, mo), case.intended(i, cap), case, rd, 0, mo, 'intended hits')
    for c in case.claims:
        kind = c[0]
        if kind == 'mid_occ':
            assert R.default_mid_occ(sp.IH) == c[1], (case.label, c)
            continue
        i = case.read(c[1])
        if kind == 'sizes':
            assert sp.sizes(i, c[2]) == c[3], (case.label, c, sp.sizes(i, c[2]))
        elif kind == 'nhits':
            assert len(sp.hits(i, c[2])) == c[3], (case.label, c, len(sp.hits(i, c[2])))
        elif kind == 'ncand':
            assert ncand(sp.hits(i, c[2])[:, 1]) == c[3], (case.label, c, ncand(sp.hits(i, c[2])[:, 1]))
        elif kind == 'spans_contigs':
            edges = np.cumsum([len(s) for s in case.contigs])
            r = sp.hits(i, 64)[:, 1]
            assert len(r) == 2 and np.searchsorted(edges, r[0], 'right') + 1 == np.searchsorted(edges, r[1], 'right'), (case.label, c)
        elif kind == 'last_bin_is_last':
            assert sp.hits(i, 64)[-1, 1] // BIN == (sum(len(s) for s in case.contigs) - 1) // BIN and sp.hits(i, 64)[-1, 1] + case.k == sum(len(s) for s in case.contigs)
        elif kind == 'order_differs':
            rows = sp.rows(i, 0, c[2])
            assert (np.diff(rows[:, 1]) < 0).any()
        elif kind in ('cut_in_tie', 'cut_between_sizes', 'cut_in_singletons'):
            sz = sp.sizes(i, c[2]); cn = c[3]
            assert {'cut_in_tie': sz[cn - 1] == sz[cn] > 1, 'cut_between_sizes': sz[cn - 1] > sz[cn], 'cut_in_singletons': sz[cn - 1] == sz[cn] == 1}[kind], (case.label, c, sz)
        elif kind == 'path':
            _, _, cn, mo, bld, rt, want = c
            assert path(sp.hits(i, mo)[:, 1], cn, bld, rt) == want, (case.label, c, path(sp.hits(i, mo)[:, 1], cn, bld, rt))
        else:
            raise AssertionError('unknown claim %r' % (c,))


def check_case(ctx, gi, case, sp, build, routing, counter=None, seen=None, params=None):
    """map_batch on every read of the case in ONE call per (check_num, mid_occ) — reads of several size classes side by side, declined and answered —
    against spec_ref.map_read, row for row. With `counter` (the emulator build's count of reads the filtered forms answered / declined) the
    reads go again grouped by expected path, and the counts must be exactly those of the path: every read was answered by the form path() names.
    The caller has set ROUTINGS[routing] in the environment."""
    for cn, mo in (params or case.params):
        idx = reads_for(case, cn, mo)
        got = ctx.map_batch(gi, [case.reads[i].seq for i in idx], check_num=cn, mid_occ=mo)
        for i, g in zip(idx, got):
            same(g, sp.rows(i, cn, mo), case, case.reads[i], cn, mo, '%s routing' % routing)
        if counter is None:
            continue
        groups = {}
        for i in idx:
            groups.setdefault(path(sp.hits(i, mo)[:, 1], cn, build, routing), []).append(i)
        for p, members in groups.items():
            t0, d0 = counter(0), counter(1)
            got = ctx.map_batch(gi, [case.reads[i].seq for i in members], check_num=cn, mid_occ=mo)
            dt, dd = counter(0) - t0, counter(1) - d0
            for i, g in zip(members, got):
                same(g, sp.rows(i, cn, mo), case, case.reads[i], cn, mo, '%s routing, alone with path %s' % (routing, '>'.join(p)))
            want = counts_of(p)
            assert (dt, dd) == (want[0] * len(members), want[1] * len(members)), \
                ('%s: reads %s check_num %d mid_occ %d, %s routing: expected path %s, but the filtered forms answered %d and declined %d of %d reads'
                 % (case.label, [case.reads[i].label for i in members][:6], cn, mo, routing, '>'.join(p), dt, dd, len(members)))
            if seen is not None and not all(case.reads[i].label.startswith('ballast') for i in members):
                seen.add(p[-1])
