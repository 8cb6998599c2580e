"""Constructed inputs for the local re-seeding stage (L1: vmx_local_prep / k_local_prep; L2: k_local_seed_band and the general form k_local_seed)
and the shared check.

A seeded, deterministic generator of cases (label, family, mode, contigs, local_kmersize, reads with their guide paths and the routing
expected of the banded form) placed AT the edges of the rule that spec_ref.local_guides / local_seed / local_raw state, and at the chunk, tile
and list sizes of k_local_seed_band (BUILDS holds the constants of either build). Shared by test_local_edges.py (the generator's self-check,
the oracle, the goldens), test_emu_local_edges.py and test_gpu_local_edges.py.

The construction. Contigs and reads are runs of N with planted PROBES: random ACGT strings whose k-mers are distinct up to reverse complement over
the whole case. A planted copy carries one ACGT flank base on either side, an A in the read and a C or G in the reference (so that a k-mer of Ns and a flank
never matches another probe's, on either strand), and keeps k - 1 Ns to its neighbours: the k-mers that match are exactly the probe's interior ones, whether a k-mer with an N is held never to match (D1) or
compared as text (the reference): check_claims asserts local_seed(d1=True) == local_seed(d1=False) on every case. The hits are therefore the
planted ones to the position, and every edge is stated as a claim (number of accepted hits, the filter clause that accepted, the read
positions hit, the order of rows with equal q + l, ...) that check_claims proves with the spec alone; an edge comes as a pair of reads on
either side of it whose claims differ. A guide is only a list of coordinates: its anchors need not be matches, which is what lets a "comb" of
guide anchors at consecutive read positions (where the accept interval shrinks to 500) cut chosen positions out of a diagonal's hits. Guide read
positions are distinct within a guide: a precondition of the stage (the closest anchors are found by read position; the kernel's slice walk
relies on it). Every read is emitted as it stands and, where the routing does not depend on the position in the read, reverse-complemented
with its paths mirrored (q -> L - q - l, s -> -s, order reversed).

Routing. Under VMX_LSEED_TRACE vmx_local_stage prints how many reads of a call k_local_seed_band handed to k_local_seed and why; check_case
parses that line: the reasons counted must be exactly those the case expects (Rd.expect), and the reads expected to stay are run once more
on their own, where not one may be handed back. Reached on purpose: 'windows' (33 disjoint windows), 'open runs' (33 runs open across one
chunk boundary), 'hit tile' (more hits in 16 read positions than the tile holds).

Hand-back reasons no case reaches, and why they do not fit a test of seconds:
  guide sort  the guide's sort keys exceed the pool sized from the batch's own longest guide: unreachable through vm_local_chain_batch.
  key width   read window of 2^26 positions, or windows + read window beyond the 63-bit hit key: a read or reference of hundreds of Mb.
  intervals   more accept intervals in one chunk than the hit tile has slots (4 per guide segment, HCAP of them): a guide slice is at most GS
              anchors, so at most 4 GS + 8 < HCAP intervals; or one interval of 2^28 positions: a guide jump of 256 Mb.
  pieces      more than 16 disjoint band pieces in one chunk: needs > 16 window-clipped fragments, i.e. a guide slice whose anchors jump between
              more than 16 windows inside one chunk; with GS = 20 (emulator) possible in principle, but every such guide also has > 32 windows
              or anchors closer than LB_SLACK after clipping; left to the natural reads of the goldens.
  log         more (diagonal, chunk) groups than the per-slot pool (>= len / 2 + 8192 records) or than the key's index bits: a read of Mb.
  chunks      8191 chunks: a read window of at least 8191 x 32 positions that stays dense throughout.
  sorts       more anchors of one guide than the pool: falls to the capacity retry first at these sizes.
Not covered either: aliasing of the chunk table's 2^14-bit occupancy map (two k-mers with equal low 14 bits). It is a superset test by design (a
false pass is checked against the exact k-mer in the bucket walk), so aliasing can add candidates, never lose a hit; a chunk of these cases holds
few distinct k-mers (the tile family's repeats have twelve), the goldens' natural reads fill the map. And: a forward and a reverse diagonal with the same
`point` (r - q == -(r + q), possible only for r < q at the very start of the reference) share one cache entry in the reference; the kernels
keep strands apart. No case goes there."""
import re
import numpy as np
import spec_ref as R

# k_local_band.hip / vmx_kernels.h: VMX_LB_QC, VMX_LB_HCAP, VMX_LB_GS (emulator build: the VMX_EMU branch), LB_OPEN, LB_PIECES, LB_WIN, LB_HULL_ONE,
# VMX_LA_SLOT(len). test_local_edges.py reads the two files and asserts these values.
BUILDS = {'emu': dict(QC=128, HCAP=256, GS=20, OPEN=32, PIECES=16, WIN=32, HULL_ONE=16384),
          'gfx950': dict(QC=512, HCAP=512, GS=64, OPEN=32, PIECES=16, WIN=32, HULL_ONE=16384)}
TILE_H = {'emu': dict(once=3, at16=12, fail=20), 'gfx950': dict(once=2, at16=24, fail=36)}    # hits per read position (see tile_cases)


def la_slot(L):
    return L // 2 + 4096


REASONS = ('guide sort', 'windows', 'key width', 'intervals', 'pieces', 'hit tile', 'open runs', 'log', 'chunks', 'sorts')
TRACE_RE = re.compile(r'k_local_seed_band: (\d+) reads, (\d+) handed to k_local_seed \(guide sort (\d+), windows (\d+), key width (\d+), '
                      r'intervals (\d+), pieces (\d+), hit tile (\d+), open runs (\d+), log (\d+), chunks (\d+), sorts (\d+)\)')
GL = 15                           # length of every guide anchor (the stage reads q and r of a guide, and l and s in L1)
REGION = 30000                    # spacing of the regions Plan.region() hands out: further than any window or accept interval reaches
R0 = 20000                        # reference position of read position 0 on the guides' own diagonal, in the one-contig cases


def _kmers(s, k):
    return [s[i:i + k] for i in range(len(s) - k + 1)]


def _canon(s):
    return min(s, R.revcomp(s))


class Probe:
    def __init__(self, rd, rf):
        self.rd, self.rf, self.n = rd, rf, len(rd) - 2        # the read's and the reference's copy, flanks included; n = the read copy's core


class Rd:
    def __init__(self, label, L, paths, expect=None, rc=True):
        self.label, self.paths, self.expect, self.rc = label, [np.array(p, dtype=np.int64).reshape(-1, 4) for p in paths], expect, rc
        self.buf = bytearray(b'N' * L)
        self.gap = 0

    def put(self, q, pr):
        """the probe's read copy with its core at read position q (at q == 0 without the left flank)"""
        s, a = pr.rd, q - 1
        if a < 0:
            s, a = s[1:], 0
        lo, hi = max(a - self.gap, 0), min(a + len(s) + self.gap, len(self.buf))
        assert a + len(s) <= len(self.buf) and self.buf[lo:hi] == b'N' * (hi - lo), ('read placements touch', self.label, q)
        self.buf[a:a + len(s)] = s.encode()

    @property
    def seq(self):
        return bytes(self.buf)


DP_ROWS = 2000
DP_SKIP = {'H': 40., 'L': 59., 'S': 30., 'R': 30.}       # -localpenalty defaults (vacmap:257-296)
_dp_tables = None


def dp_tables():
    """the cost tables tests/golden/tables.json pins (test_oracle_golden.py), as the oracle builds them"""
    global _dp_tables
    if _dp_tables is None:
        import oracle_lib
        _dp_tables = {n: oracle_lib.table(i) for i, n in enumerate(('extra', 'readgap_h', 'readgap_r', 'large_readgap', 'log2cache', 'log2int'))}
    return _dp_tables


def mirrored(rd):
    L = len(rd.buf)
    out = Rd(rd.label + '/rc', L, [[(L - q - l, r, -s, l) for q, r, s, l in p.tolist()[::-1]] for p in rd.paths], rd.expect)
    out.buf = bytearray(R.revcomp(rd.buf.decode()).encode())
    return out


class Case:
    def __init__(self, label, mode, k, contigs, reads, claims):
        self.label, self.family, self.mode, self.k, self.contigs, self.reads, self.claims = label, label.split('/')[0], mode, k, contigs, reads, claims
        self._spec = {}

    def read(self, label):
        return next(i for i, r in enumerate(self.reads) if r.label == label)

    def guides(self, i):
        return R.local_guides(self.reads[i].paths, self.mode)[0]

    def traces(self, i, d1=True):
        """[(rows, trace)] of read i, one per guide that is re-seeded"""
        if (i, d1) not in self._spec:
            self._spec[i, d1] = [R.local_seed(self.contigs, self.reads[i].seq.decode(), g, self.k, self.mode, d1) for g in self.guides(i)]
        return self._spec[i, d1]

    def rows(self, i):
        """spec_ref.local_raw of read i (from the cached per-guide rows)"""
        if ('raw', i) not in self._spec:
            rows = [a for rr, _ in self.traces(i) for a in rr]
            rows.sort(key=(lambda a: a[0]) if self.mode == 'R' else (lambda a: a[0] + a[3]))
            self._spec['raw', i] = np.array(rows, dtype=np.int64).reshape(-1, 4)
        return self._spec['raw', i]

    def hits(self, i):
        return [h for _, t in self.traces(i) for h in t['hits']]

    def dp(self, i):
        """spec_ref.local_dp on the spec's raw rows of read i, with the variant and the parameters get_localmap_multi_all_forDP_inv_guide_list would take
        (None: no rows, -mode asm's own DP, or more than DP_ROWS rows — the plain statement is quadratic in Python)"""
        if ('dp', i) not in self._spec:
            rows, e = self.rows(i), None
            if self.mode != 'asm' and 0 < len(rows) <= DP_ROWS:
                ng = R.local_guides(self.reads[i].paths, self.mode)[1]
                variant = 2 if self.mode == 'R' else (1 if ng > 1 else 0)
                skip = min(DP_SKIP[self.mode], 40.) if (self.mode == 'L' and variant == 1) else DP_SKIP[self.mode]
                e = dict(R.local_dp(rows, variant, self.mode, self.k, skip, 30, 50 if self.mode == 'L' else 99, dp_tables()), variant=variant)
            self._spec['dp', i] = e
        return self._spec['dp', i]


class Plan:
    """collects the probes, the reference and the reads of one case"""

    def __init__(self, label, rng, mode='H', k=9, contig_lens=(70000,)):
        self.label, self.rng, self.mode, self.k = label, rng, mode, k
        self.lens = list(contig_lens)
        self.ends = np.cumsum(self.lens); self.starts = self.ends - np.array(self.lens)
        self.ref = bytearray(b'N' * int(self.ends[-1]))
        self.used, self.reads, self.claims, self.nreg = set(), [], [], 0

    def region(self):
        """a fresh stretch of the first contig, REGION wide: the reference position of read position 0 on the diagonal of a guide of its own"""
        self.nreg += 1
        assert (self.nreg + 1) * REGION <= self.lens[0], 'out of regions'
        return self.nreg * REGION - 10000

    def _rand(self, n):
        return ''.join('ACGT'[i] for i in self.rng.integers(0, 4, n))

    def _rand_distinct(self, n, first=''):
        """n random bases after `first` whose k-mers are new to the case and distinct up to reverse complement (base by base: a long random
        string repeats a 9-mer somewhere)"""
        k = self.k
        while True:
            s, seen = first, {_canon(x) for x in _kmers(first, k)}
            while len(s) < len(first) + n:
                for c in self.rng.permutation(4):
                    t = (s + 'ACGT'[c])[-k:]
                    if len(t) < k or (t != R.revcomp(t) and _canon(t) not in seen and _canon(t) not in self.used):
                        s += 'ACGT'[c]; seen.add(_canon(t))
                        break
                else:
                    break
            if len(s) == len(first) + n:
                return s

    def _other(self, *not_these):
        return [c for c in 'ACGT' if c not in not_these][int(self.rng.integers(0, 4 - len(set(not_these))))]

    def _register(self, rd, rf, common, palindromes=0):
        k = self.k
        ks = _kmers(rd, k) + _kmers(rf, k)
        if sum(1 for x in ks if x == R.revcomp(x)) != palindromes:
            return False
        cs = [_canon(x) for x in ks]
        if len(set(cs)) != len(cs) - common or set(cs) & self.used:
            return False
        self.used |= set(cs)
        return True

    def probe(self, n, mism=(), first=''):
        """a probe of n bases; the reference's copy differs at the positions `mism`; `first`: a prescribed beginning (a k-mer that is its own
        reverse complement). Its k-mers, flanks included, are new to the case and distinct up to reverse complement."""
        k = self.k
        while True:
            core = self._rand_distinct(n - len(first), first)
            cref = list(core)
            for m in mism:
                cref[m] = self._other(core[m])
            rd, rf = 'A' + core + 'A', 'CG'[int(self.rng.integers(0, 2))] + ''.join(cref) + 'CG'[int(self.rng.integers(0, 2))]
            common = sum(1 for i in range(n - k + 1) if not any(i <= m < i + k for m in mism))
            if self._register(rd, rf, common, 2 if first else 0):
                return Probe(rd, rf)

    def tandem(self, p, n_read, n_ref):
        """a tandem repeat of period p: n_read bases of it for the read and n_ref >= n_read for the reference, both from phase 0: read offset o
        matches the reference offsets o + j p"""
        k = self.k
        while True:
            unit = self._rand(p)
            T = unit * (max(n_ref, n_read) // p + 3)
            cyc = [T[i:i + k] for i in range(p)]
            if len({_canon(x) for x in cyc}) != p or any(x == R.revcomp(x) for x in cyc) or {_canon(x) for x in cyc} & self.used:
                continue
            if unit[-1] == 'A' or T[n_read] == 'A':
                continue
            rd, rf = 'A' + T[:n_read] + 'A', self._other('A', 'T', unit[-1]) + T[:n_ref] + self._other('A', 'T', T[n_ref])
            fl = [_canon(x) for x in (rd[:k], rd[-k:], rf[:k], rf[-k:])]
            if len(set(fl)) != 4 or set(fl) & ({_canon(x) for x in cyc} | self.used) or any(x == R.revcomp(x) for x in fl):
                continue
            self.used |= set(fl) | {_canon(x) for x in cyc}
            return Probe(rd, rf)

    def ref_put(self, g, pr, orient=1):
        """the probe's reference copy with its core at global position g (a flank that would leave the contig is dropped); orient -1: reverse-complemented"""
        s = pr.rf if orient == 1 else R.revcomp(pr.rf)
        a = g - 1
        c = int(np.searchsorted(self.ends, g, 'right'))
        if a < self.starts[c]:
            s, a = s[1:], g
        if a + len(s) > self.ends[c]:
            s = s[:-1]
        assert self.starts[c] <= a and a + len(s) <= self.ends[c], ('placement leaves its contig', self.label, g)
        lo, hi = max(a - (self.k - 1), int(self.starts[c])), min(a + len(s) + self.k - 1, int(self.ends[c]))
        assert self.ref[lo:hi] == b'N' * (hi - lo), ('reference placements touch', self.label, g)
        self.ref[a:a + len(s)] = s.encode()

    def read(self, label, L, paths, expect=None, rc=True):
        rd = Rd(label, L, paths, expect, rc and expect is None)
        rd.gap = self.k - 1
        self.reads.append(rd)
        return rd

    def claim(self, *c):
        self.claims.append(c)

    def case(self):
        reads = list(self.reads) + [mirrored(rd) for rd in self.reads if rd.rc]
        for rd in reads:
            for p in rd.paths:
                assert len(set(p[:, 0].tolist())) == len(p) and (np.diff(p[:, 0]) < 0).all(), ('guide read positions: distinct, descending', rd.label)
        contigs = [self.ref[a:b].decode() for a, b in zip(self.starts, self.ends)]
        return Case(self.label, self.mode, self.k, contigs, reads, self.claims)


def diag(qs, base=R0, s=1):
    """a guide on one diagonal: anchors (q, base + q, 1, GL), or (q, base - q, -1, GL), in descending read order"""
    return [(q, base + q if s == 1 else base - q, s, GL) for q in sorted(set(qs), reverse=True)]


# ------------------------------------------------------------------------------------------------ families
def filter_case(rng, mode):
    """one read and one k-mer per edge of the proximity filter (:23231): accepted / rejected, and by which clause"""
    P = Plan('filter/' + mode if mode == 'H' else 'modes/filter/' + mode, rng, mode, contig_lens=(50 * REGION,))
    k = P.k
    look, span = R.LOCAL_SPANS[mode]

    def one(label, L, qs, q, off, accept, why=None):
        """a read of its own region: the guide `qs` on the region's diagonal, one k-mer at read position q and at region + off"""
        b = P.region()
        pr = P.probe(k)
        P.read(label, L, [diag(qs, b)]).put(q, pr); P.ref_put(b + off, pr)
        P.claim('in_table', label, b + off); P.claim('hits', label, 1 if accept else 0)
        if why:
            P.claim('why', label, why)

    A = [500, 6500]                                                # q = 3100: b0 = 2600, b1 = 3400, interval 2000; only |readgap - refgap| < 500 can accept
    one('diff/lo/499', 7000, A, 3100, 500 + 2101, True, (True, False, False)); one('diff/lo/500', 7000, A, 3100, 500 + 2100, False)
    one('diff/hi/499', 7000, A, 3100, 500 + 3099, True, (True, False, False)); one('diff/hi/500', 7000, A, 3100, 500 + 3100, False)
    if look >= 2601 + 500:                                         # (the left side lies outside the narrow modes' window)
        one('diff/left/499', 7000, A, 3100, 500 - 2101, True, (True, False, False)); one('diff/left/500', 7000, A, 3100, 500 - 2100, False)
    B = [1000, 1700, 2500, 4000]                                   # q = 1350: b0 = b1 = 350, interval 1200
    one('ref1/at', 5000, B, 1350, 1000 - 1200, True, (False, True, False)); one('ref1/beyond', 5000, B, 1350, 1000 - 1201, False)
    one('ref2/at', 5000, B, 1350, 1700 + 1200, True, (False, False, True)); one('ref2/beyond', 5000, B, 1350, 1700 + 1201, False)
    one('on_anchor/500', 5000, B, 1700, 1700 + 500, True, (False, True, True)); one('on_anchor/501', 5000, B, 1700, 1700 + 501, False)
    one('before_first/at', 5000, B, 800, 1000 - 900, True, (False, True, True)); one('before_first/beyond', 5000, B, 800, 1000 - 901, False)
    one('after_last/at', 5000, B, 4400, 4000 + 1300, True, (False, True, True)); one('after_last/beyond', 5000, B, 4400, 4000 + 1301, False)
    C = [500, 1999, 3499, 5000]                                    # neighbours 1499, 1500 and 1501 apart: interval 1999, 2000, 2000 (clamped)
    one('clamp/1499/at', 5500, C, 1200, 500 - 1999, True, (False, True, False)); one('clamp/1499/beyond', 5500, C, 1200, 500 - 2000, False)
    one('clamp/1500/at', 5500, C, 2699, 1999 - 2000, True, (False, True, False)); one('clamp/1500/beyond', 5500, C, 2699, 1999 - 2001, False)
    one('clamp/1501/at', 5500, C, 4199, 3499 - 2000, True, (False, True, False)); one('clamp/1501/beyond', 5500, C, 4199, 3499 - 2001, False)
    # one guide segment of 11500 read positions: the hull of its accept intervals passes LB_HULL_ONE = 16384 while the chunks walk along it
    # (11500 + 2000 + (chunk end - 500) + 499): one band interval before, four after
    H = [500, 12000]
    for q in (1500, 8000):
        one('hull/%d/ref2/at' % q, 12600, H, q, 12000 - 2000, True, (False, False, True)); one('hull/%d/ref2/beyond' % q, 12600, H, q, 12000 - 2001, False)
        one('hull/%d/gap' % q, 12600, H, q, 500 + 2001, False)       # inside the hull, between the intervals
    return P.case()


def runs_case(rng, k):
    """the run merge per diagonal (:23232-23344) and the tie order of the stable sort"""
    P = Plan('runs/k%d' % k, rng, 'H', k, contig_lens=(16 * REGION,))
    base = list(range(200, 3801, 400))

    def new(label, qs=base, **kw):
        """a read of 4000 bases with a region of its own: (read, the region's diagonal)"""
        b = P.region()
        return P.read(label, 4000, [diag(qs, b)], **kw), b

    # a diagonal 800 from the guide's is accepted next to a guide anchor (interval >= 893) and rejected ON one (interval 500): k - 1 anchors at
    # consecutive read positions leave hits k apart (the run goes on), k anchors leave them k + 1 apart (it breaks)
    for name, m in (('comb/k', k - 1), ('comb/k+1', k)):
        pr = P.probe(50)
        rd, b = new(name, base + list(range(1000, 1000 + m))); rd.put(980, pr); P.ref_put(b + 980 + 800, pr)
        P.claim('hitq', name, [q for q in range(980, 980 + 50 - k + 1) if not 1000 <= q < 1000 + m])
    P.claim('differ', 'comb/k', 'comb/k+1')
    for n in (19, 20):                                            # l + bonus of 19 and 20
        pr = P.probe(n)
        rd, b = new('split/%d' % n); rd.put(1500, pr); P.ref_put(b + 1550, pr)
        P.claim('rows', 'split/%d' % n, 1 if n == 19 else 2)
    pr = P.probe(30)                                              # a reverse-strand run: r follows the newest hit
    rd, b = new('rev/run'); rd.put(1600, pr); P.ref_put(b + 1660, pr, -1)
    P.claim('rows', 'rev/run', 2); P.claim('strand', 'rev/run', -1)
    # one read k-mer on three diagonals; C is revisited at q = 1000, A at q = 2500, B never: the leftovers (300, ., 1, k) come out C, A, B
    m, x, y = P.probe(k), P.probe(k), P.probe(k)
    rd, R0 = new('revisit'); rd.put(300, m); rd.put(1000, x); rd.put(2500, y)
    for d in (-90, 0, 90):
        P.ref_put(R0 + 300 + d, m)
    P.ref_put(R0 + 1000 + 90, x); P.ref_put(R0 + 2500, y)
    P.claim('rows', 'revisit', 5); P.claim('order', 'revisit', 300 + k, [R0 + 300 + 90, R0 + 300, R0 + 300 - 90])
    # diagonal E appears first (q = 100), F second (q = 200); at q = 3000 one k-mer hits F's position before E's: what is left comes out E, F
    e, f, z = P.probe(k), P.probe(k), P.probe(k)
    rd, R0 = new('leftover'); rd.put(100, e); rd.put(200, f); rd.put(3000, z)
    P.ref_put(R0 + 100 + 80, e); P.ref_put(R0 + 200 - 80, f); P.ref_put(R0 + 3000 + 80, z); P.ref_put(R0 + 3000 - 80, z)
    P.claim('rows', 'leftover', 4); P.claim('order', 'leftover', 3000 + k, [R0 + 3000 + 80, R0 + 3000 - 80])
    w = P.probe(k)                                                # a forward and a reverse hit at one read position: forward first
    rd, R0 = new('both_strands'); rd.put(1800, w); P.ref_put(R0 + 1800 + 70, w); P.ref_put(R0 + 1800 - 70, w, -1)
    P.claim('rows', 'both_strands', 2); P.claim('order', 'both_strands', 1800 + k, [R0 + 1800 + 70, R0 + 1800 - 70])
    pr = P.probe(k + 3)                                           # reverse-strand matches at read positions 0 .. 3: the one at 0 is never looked up
    rd, b = new('rev_at_0', rc=False); rd.put(0, pr); P.ref_put(b + 100, pr, -1)
    P.claim('hitq', 'rev_at_0', [1, 2, 3])
    pr = P.probe(k + 3)                                           # (the same on the forward strand: position 0 is there)
    rd, b = new('fwd_at_0', rc=False); rd.put(0, pr); P.ref_put(b + 100, pr)
    P.claim('hitq', 'fwd_at_0', [0, 1, 2, 3])
    if k % 2 == 0:                                                # a k-mer that is its own reverse complement is skipped
        half = 'ACGTTGCATG'[:k // 2]
        pr = P.probe(k + 6, first=half + R.revcomp(half))
        rd, b = new('palindrome'); rd.put(2200, pr); P.ref_put(b + 2230, pr)
        P.claim('hitq', 'palindrome', list(range(2201, 2207)))
    return P.case()


def chunks_case(rng, build):
    """runs at the chunk boundaries of k_local_seed_band: with sparse hits the chunks are exactly QC wide from readstart = 0"""
    B_ = BUILDS[build]
    QC, GS = B_['QC'], B_['GS']
    P = Plan('chunks/' + build, rng, 'H', contig_lens=(24 * REGION,))
    k = P.k
    L = 6 * QC + 200
    base = list(range(100, L - 50, 300))

    def new(label, qs=base, **kw):
        b = P.region()
        return P.read(label, L, [diag(qs, b)], **kw), b

    B = 3 * QC
    D = 100                                                       # the runs' diagonal: accepted at every read position of the guide's span
    for off in range(-k - 1, 2):                                  # the run's last hit at B + off; the diagonal is hit again k + 1 later (a new run)
        pr = P.probe(46, mism=[30])
        q0 = B + off - (30 - k)
        rd, b = new('end/%+d' % off); rd.put(q0, pr); P.ref_put(b + q0 + D, pr)
        P.claim('hitq', 'end/%+d' % off, list(range(q0, B + off + 1)) + list(range(q0 + 31, q0 + 46 - k + 1)))
    pr = P.probe(30)                                              # ends in the chunk's last k positions, nothing follows
    rd, b = new('end/none'); rd.put(B - 3 - (30 - k), pr); P.ref_put(b + B - 3 - (30 - k) + D, pr)
    pr = P.probe(2 * QC + 40)                                     # spans three chunks
    rd, b = new('span3'); rd.put(B - 20, pr); P.ref_put(b + B - 20 + D, pr)
    pr = P.probe(40)                                              # its first anchor (l = 19) ends exactly at B
    rd, b = new('split_at_boundary'); rd.put(B - 19, pr); P.ref_put(b + B - 19 + D, pr)
    P.claim('has_row', 'split_at_boundary', (B - 19, b + B - 19 + D, 1, 19))
    # hits at B - k - 1, B - k and at B with none between (a comb of k - 1 guide anchors, see runs_case; this diagonal lies 600 from the guide's):
    # the anchor in progress (l = k + 1) goes on across the boundary, from the very first position at which a run may still be open, and
    # stays below 20 (a longer one would be split at B either way); with k anchors the run breaks there
    for name, m in (('comb_at_boundary/k', k - 1), ('comb_at_boundary/k+1', k)):
        pr = P.probe(40)
        rd, b = new(name, [q for q in base if abs(q - B) > 150] + list(range(B - m, B))); rd.put(B - k - 1, pr); P.ref_put(b + B - k - 1 + 600, pr)
        P.claim('hitq', name, [q for q in range(B - k - 1, B - k - 1 + 40 - k + 1) if not B - m <= q < B])
        if m == k - 1:
            P.claim('has_row', name, (B - k - 1, b + B - k - 1 + 600, 1, 19))
    P.claim('differ', 'comb_at_boundary/k', 'comb_at_boundary/k+1')
    for n in (B_['OPEN'], B_['OPEN'] + 1):                        # one read k-mer in the chunk's last k positions on n diagonals: n runs stay open
        pr = P.probe(k)
        rd, b = new('open/%d' % n, expect='open runs' if n > B_['OPEN'] else None, rc=False); rd.put(B - 3, pr)
        for j in range(n):
            P.ref_put(b + B - 3 - 480 + 30 * j, pr)
        P.claim('hits', 'open/%d' % n, n); P.claim('rows', 'open/%d' % n, n)
    step = QC // (GS + 5)                                         # more than GS guide anchors inside one chunk: it is cut at the last staged anchor
    dense = list(range(B + 2, B + QC, step))
    assert len(dense) > GS
    pr = P.probe(QC + 40)
    rd, b = new('gs_cut', base + dense); rd.put(B - 20, pr); P.ref_put(b + B - 20 + D, pr)
    P.claim('hitq', 'gs_cut', list(range(B - 20, B + QC + 20 - k + 1)))
    return P.case()


def simulate_tile(per_q, readstart, readend, B_, carried):
    """the chunk loop's widths on a read with per_q[q] accepted hits: (halvings, smallest width that had to be used) or 'hit tile'; `carried`:
    runs that may be open at a boundary (added to every chunk: the decision must not depend on it, see the claim)"""
    QC, HCAP = B_['QC'], B_['HCAP']
    q0, qc, halvings, least = readstart, QC, 0, QC
    while q0 < readend:
        qb = min(q0 + qc, readend)
        nhit = sum(per_q.get(q, 0) for q in range(q0, qb)) + (carried if per_q.get(q0 - 1, 0) else 0)
        if nhit > HCAP:
            if qc <= 16:
                return 'hit tile'
            qc >>= 1; halvings += 1; least = min(least, qc)
            continue
        want = (qb - q0) * (3 * HCAP // 4) // nhit if nhit > 0 else QC
        want &= ~7
        q0, qc = qb, max(32, min(QC, want))
    return halvings, least


def tile_case(rng, build):
    """tandem repeats: the reference holds h periods (+ k - 1 bases) of a repeat of period 12, the read a region of 2 QC + 100 positions of it that
    starts on a chunk boundary, and every guide anchor points at the block (r = its middle + the anchor's number): every read position of the
    region has exactly h accepted hits, on h diagonals that run for h periods each. h = once overflows the hit tile at the full width and
    fits after one halving; h = at16 fits only at 16 positions; h = fail does not fit at all (handed back: 'hit tile'). After the first dense chunk
    the width follows the density, and h runs cross every boundary that results."""
    B_ = BUILDS[build]
    QC = B_['QC']
    P = Plan('tile/' + build, rng, 'H', contig_lens=(5 * REGION,))
    k, p = P.k, 12
    Lr = 2 * QC + 100
    L = QC + Lr + 300
    for name, h in TILE_H[build].items():
        pr = P.tandem(p, Lr, h * p + k - 1)
        b = P.region()
        g = [(q, b + i, 1, GL) for i, q in enumerate(range(25, L, 50))][::-1]
        P.read(name, L, [g], expect='hit tile' if name == 'fail' else None, rc=name != 'fail').put(QC, pr)
        P.ref_put(b - h * p // 2, pr)
        P.claim('perq', name, QC, QC + Lr - k + 1, h); P.claim('tile', name, build, h)
    return P.case()


def capacity_case(rng):
    """a short repeat read whose local anchors exceed its regular slot of len / 2 + 4096 rows: the 8x retry must answer it"""
    P = Plan('capacity/repeat', rng, 'H')
    L = 1500
    pr = P.tandem(20, 1400, 8000)
    P.read('repeat', L, [diag(range(100, L, 300))], expect='hit tile', rc=False).put(50, pr); P.ref_put(R0 + 50 - 3300, pr)
    P.claim('rows_gt', 'repeat', la_slot(L))
    return P.case()


def windows_case(rng, mode):
    """the reference windows (:23105-23180): cut at >= readgap, single-point windows dropped, clipped at the contig's ends, the retry that cuts at
    contig changes, overlap after widening, the last k-mer of a window"""
    P = Plan('windows/' + mode if mode == 'H' else 'modes/windows/' + mode, rng, mode, contig_lens=(40000, 40000, 40000))
    k = P.k
    look, span = R.LOCAL_SPANS[mode]
    C1, C2 = 40000, 80000
    xs = iter(range(C1 + 12000, C1 + 13400, 40))                  # every read's guide starts 40 further on: no two reads plant at one position

    def mark(rd, q, g, orient=1, n=None):
        pr = P.probe(n or k); rd.put(q, pr); P.ref_put(g, pr, orient)
        return pr

    for d in (4999, 5000):                                        # neighbours readgap - 1 and readgap apart: one window, or two single points (dropped)
        x = next(xs)
        mark(P.read('gap/%d' % d, 1000, [[(600, x + d, 1, GL), (200, x, 1, GL)]]), 210, x + 10)
        P.claim('hits', 'gap/%d' % d, 1 if d < 5000 else 0)
    x = next(xs)
    mark(P.read('single', 1000, [[(200, x, 1, GL)]]), 210, x + 10); P.claim('rows', 'single', 0)
    far = max(look, 5000) + 2000                                  # an isolated anchor's window is dropped: a k-mer next to it is not in the table
    for n in (3, 4):
        x = next(xs)
        g = [(200, x, 1, GL), (300, x + 100, 1, GL), (500, x + 100 + far, 1, GL)] + ([(600, x + 200 + far, 1, GL)] if n == 4 else [])
        mark(P.read('isolated/%d' % n, 1000, [g[::-1]]), 510, x + 110 + far)
        P.claim('hits', 'isolated/%d' % n, 1 if n == 4 else 0)
    # clipped at the contig's start: its first k-mer is in the table, a copy 20 before the start (the contig before) is not
    rd = P.read('clip/start', 1200, [[(800, C1 + 900, 1, GL), (400, C1 + 500, 1, GL)]])
    pr = mark(rd, 5, C1); P.ref_put(C1 - 20, pr)
    P.claim('hits', 'clip/start', 1); P.claim('has_row', 'clip/start', (5, C1, 1, k))
    # ... and at its end: the last k-mer is in, a copy 20 past the end (the next contig) is not
    rd = P.read('clip/end', 1300, [[(600, C2 - 500, 1, GL), (200, C2 - 900, 1, GL)]])
    pr = mark(rd, 1100 - k, C2 - k); P.ref_put(C2 + 20, pr)
    P.claim('hits', 'clip/end', 1); P.claim('has_row', 'clip/end', (1100 - k, C2 - k, 1, k))
    # a guide across two contigs: the first cut gives one window over both (nothing usable), the retry cuts at the contig change
    rd = P.read('two_contigs', 1000, [[(800, C2 + 300, 1, GL), (600, C2 + 100, 1, GL), (400, C2 - 100, 1, GL), (200, C2 - 300, 1, GL)]])
    mark(rd, 250, C2 - 250); mark(rd, 650, C2 + 150); mark(rd, 540, C2 + 40)
    P.claim('hits', 'two_contigs', 3)
    # two windows that overlap after widening (where 5000 < 2 look): a k-mer in the overlap is in the table twice (accepted twice, one row)
    x = next(xs)
    rd = P.read('overlap', 1000, [[(800, x + 5400, 1, GL), (600, x + 5200, 1, GL), (400, x + 200, 1, GL), (200, x, 1, GL)]])
    mark(rd, 410, x + 210)
    P.claim('hits', 'overlap', 2 if 5000 < 2 * look else 1); P.claim('rows', 'overlap', 1)
    # the guide's reference order is the reverse of its read order
    x = next(xs)
    rd = P.read('inversion', 2000, [diag(range(200, 1801, 400), x + 3000, -1)])
    mark(rd, 1000, x + 2000 - (25 - k), -1, 25)
    P.claim('rows', 'inversion', 2); P.claim('strand', 'inversion', -1)
    if span >= 7000:
        # the last k-mer of a window and the one after it, reached by the gap-difference clause from the guide's last anchor. The window ends
        # 7000 after the guide's largest r, the band begins 2000 before its last anchor's: 0 .. 7 between the two puts the window's end at
        # every offset within the band's groups of eight positions (d = -8: the other anchor lies lower, the largest r is the last anchor's own)
        for d in (-8, 1, 2, 3, 4, 5, 6, 7):
            for name, e in (('edge/in/%d' % d, 0), ('edge/out/%d' % d, 1)):
                x = next(xs)
                hi = x + 400 + max(d, 0) + look
                mark(P.read(name, 7500, [[(400, x + 400, 1, GL), (200, x + 400 + d, 1, GL)]]), hi - k + e - x, hi - k + e)
                P.claim('hits', name, 1 - e)
    return P.case()


def many_windows_case(rng):
    """exactly LB_WIN and LB_WIN + 1 disjoint windows: the banded form hands the second one back ('windows'); LB_WIN + 1 of which two touch are
    LB_WIN stretches of the table: kept"""
    W = BUILDS['emu']['WIN']
    assert BUILDS['gfx950']['WIN'] == W
    P = Plan('windows/many', rng, 'H', contig_lens=(16000 * (W + 1) + 24000,))
    k = P.k
    for name, n, touch, o in (('windows/%d' % W, W, False, 10), ('windows/%d' % (W + 1), W + 1, False, 40), ('windows/%d_touching' % (W + 1), W + 1, True, 70)):
        # touching: the second window's first k-mer start is the one after the first window's last (14000 + 40 - (k - 1) on): one stretch of the table
        at = [8000 + 16000 * w if not (touch and w == 1) else 8000 + 14040 - (k - 1) for w in range(n)]
        g = []
        for w in range(n):
            g += [(100 + 80 * w, at[w], 1, GL), (140 + 80 * w, at[w] + 40, 1, GL)]
        rd = P.read(name, 3000, [g[::-1]], expect='windows' if n > W and not touch else None, rc=False)
        for w in (0, 1, n // 2, n - 1):
            pr = P.probe(k); rd.put(100 + 80 * w + o, pr); P.ref_put(at[w] + o, pr)
        P.claim('hits', name, 4); P.claim('nwindows', name, n)
    return P.case()


def prep_case(rng, mode):
    """L1 (vmx_local_prep): multi-path reads at the edges of merge_chain, drop_somechains, the length order and the budget. The primary path lies
    on the diagonal R0 of region 0; every other chain lies in a region of its own, 30000 apart, with a marker k-mer that is hit iff the chain
    is re-seeded (chains next to the primary: a marker the primary's own guide rejects, or one that then comes out twice)."""
    P = Plan('prep/' + mode, rng, mode, contig_lens=(60 * REGION,))
    k = P.k
    L = 4000
    P0 = diag(range(200, 3801, 300))
    pm = P.probe(k); P.ref_put(R0 + 250, pm)                       # the primary's own marker, in every read
    assert P.region() == R0

    def mark(rd, q, g, orient=1):
        pr = P.probe(k); rd.put(q, pr); P.ref_put(g, pr, orient)

    def start(label, paths):
        rd = P.read(label, L, paths); rd.put(250, pm)
        return rd

    if mode == 'asm':
        start('primary_only', [P0]); P.claim('hits', 'primary_only', 1)
        return P.case()
    if mode == 'R':                                                # every path as it is: short ones, other strands
        b1, b2 = P.region(), P.region()
        rd = start('passthrough', [P0, diag([1000, 1030, 1060], b1), diag([1200, 1230, 1260], b2 + 5000, -1)])
        mark(rd, 1010, b1 + 1010); mark(rd, 1210, b2 + 5000 - 1210, -1)
        P.claim('hits', 'passthrough', 3); P.claim('nguides', 'passthrough', 3)
        return P.case()
    # merge_chain: X and Y span 60 read positions each (dropped alone), 260 merged (kept)
    for name, ys, delta, s, merged in (('merge/499', 1200, 499, 1, True), ('merge/500', 1200, 500, 1, False), ('merge/-499', 1200, -499, 1, True),
                                       ('merge/-500', 1200, -500, 1, False), ('merge/strand', 1200, 0, -1, False), ('merge/touch', 1075, 0, 1, True),
                                       ('merge/overlap', 1074, 0, 1, False)):
        b = P.region()
        X = diag([1000, 1030, 1060], b)
        Y = diag([ys, ys + 30, ys + 60], b + delta) if s == 1 else diag([ys, ys + 30, ys + 60], b + 2 * ys, -1)
        q = 1100 if ys == 1200 else 1040
        rd = start(name, [P0, Y, X]); mark(rd, q, b + q)
        P.claim('hits', name, 2 if merged else 1); P.claim('nguides', name, 2 if merged else 1)
    # drop_somechains: the span
    for name, last in (('drop/span99', 1099), ('drop/span100', 1100)):
        b = P.region()
        rd = start(name, [P0, diag([1000, 1050, last], b)]); mark(rd, 1020, b + 1020)
        P.claim('hits', name, 2 if last == 1100 else 1)
    # ... the distance of a chain whose strand disagrees with the primary's: 499 and 500 from the primary's anchor at q = 3800. (These chains lie
    # in the primary's region: each 40 further along the read, so that no two markers meet)
    for i, d in enumerate((499, 500)):
        o = 40 * i
        rz = R0 + 3800 + d
        rd = start('drop/dist%d' % d, [P0, [(2200 + o, rz, -1, GL), (2100 + o, rz + 100, -1, GL), (2000 + o, rz + 200, -1, GL)]])
        mark(rd, 2130 + o, rz + 100 - 30 + 20 * i, -1)
        P.claim('hits', 'drop/dist%d' % d, 2 if d == 500 else 1)
    # ... a strand-majority tie (no primary anchor inside the chain's span: 0 against 0) drops a chain 300 from the primary; with one inside it stays,
    # and its marker, which the primary accepts too, comes out twice
    for name, qs, q in (('drop/tie', [2050, 2110, 2170], 2100), ('drop/majority', [1950, 2010, 2070], 2020)):
        rd = start(name, [P0, diag(qs, R0 + 300)]); mark(rd, q, R0 + 300 + q)
        P.claim('hits', name, 2 if name == 'drop/tie' else 4)        # (the kept chain's guide accepts the primary's marker as well)
    # the budget and the stable length order: chains in regions of their own, given in scrambled order; of equal lengths the later start goes
    lens = {'H': [6, 5, 4, 4, 4], 'L': [5, 4, 4], 'S': [6, 5, 4, 4, 4, 3, 3]}[mode]
    budget = R.LOCAL_BUDGET[mode]
    bases = [P.region() for _ in lens][::-1]                      # (the longer, the higher in the reference)
    chains = [diag([400 + 450 * j + 60 * i for i in range(n)], bases[j]) for j, n in enumerate(lens)]
    order = list(rng.permutation(len(lens)))
    rd = start('budget', [P0] + [chains[j] for j in order])
    for j in range(len(lens)):
        mark(rd, 400 + 450 * j + 10, bases[j] + 400 + 450 * j + 10)
    seeded = len(lens) + 1 if budget is None else budget
    P.claim('hits', 'budget', seeded); P.claim('nguides', 'budget', seeded)
    # equal q + l across guides: one read k-mer between the first two chains, a copy in either's region: the longer chain's row first, the higher r
    pr = P.probe(k); q = 400 + 60 * lens[0] - 40
    rd = start('tie_across_guides', [P0, chains[1], chains[0]]); rd.put(q, pr)
    P.ref_put(bases[0] + q, pr); P.ref_put(bases[1] + q, pr)
    P.claim('hits', 'tie_across_guides', 3); P.claim('order', 'tie_across_guides', q + k, [bases[0] + q, bases[1] + q])
    return P.case()


def mix_case(label, cases):
    """the reads of several cases of one mode and k-mer size in ONE case: the contigs one after another, the guides moved along"""
    mode, k = cases[0].mode, cases[0].k
    contigs, reads, off = [], [], 0
    for c in cases:
        assert (c.mode, c.k) == (mode, k)
        for rd in c.reads:
            m = Rd(c.label + ':' + rd.label, len(rd.buf), [p + np.array([0, off, 0, 0]) for p in rd.paths], rd.expect)
            m.buf = rd.buf
            reads.append(m)
        contigs += c.contigs; off += sum(len(s) for s in c.contigs)
    return Case(label, mode, k, contigs, reads, [])


# ------------------------------------------------------------------------------------------------ the cases, made once
_CASES = {}
MODES = ('L', 'S', 'R')


def generate(build):
    rng = np.random.default_rng(20240901)
    out = [filter_case(rng, 'H')] + [runs_case(rng, k) for k in (9, 10, 11)] + [chunks_case(rng, build), tile_case(rng, build)]
    out += [windows_case(rng, 'H'), many_windows_case(rng), capacity_case(rng)]
    out += [f(rng, m) for m in MODES for f in (filter_case, windows_case)]
    out += [prep_case(rng, m) for m in ('H', 'L', 'S', 'R', 'asm')]
    return out


def constructed(build):
    """every case for the build under test ('emu' or 'gfx950': the chunk and tile families depend on it), made once; 'mix' last"""
    if build not in _CASES:
        cs = generate(build)
        h9 = [c for c in cs if c.mode == 'H' and c.k == 9 and c.label != 'windows/many']
        _CASES[build] = cs + [mix_case('mix/' + build, h9)]
    return _CASES[build]


FAMILIES = ('filter', 'runs', 'chunks', 'tile', 'windows', 'capacity', 'modes', 'prep', 'mix')


# ------------------------------------------------------------------------------------------------ the generator's self-check
def check_claims(case):
    """every stated property holds under the spec alone, and the case is N-safe: D1 and text equality give the same rows"""
    for i, rd in enumerate(case.reads):
        a = [rr for rr, _ in case.traces(i, True)]; b = [rr for rr, _ in case.traces(i, False)]
        assert a == b, ('D1 and text equality differ', case.label, rd.label)
    for c in case.claims:
        kind, i = c[0], case.read(c[1])
        hits, rows = case.hits(i), case.rows(i)
        if kind == 'hits':
            assert len(hits) == c[2], (case.label, c, len(hits))
        elif kind == 'why':
            assert [h[3] for h in hits] == [c[2]], (case.label, c, hits)
        elif kind == 'in_table':
            assert any(lo <= c[2] and c[2] + case.k <= hi for _, t in case.traces(i) for lo, hi in t['windows']), (case.label, c)
        elif kind == 'rows':
            assert len(rows) == c[2], (case.label, c, rows.tolist())
        elif kind == 'rows_gt':
            assert len(rows) > c[2], (case.label, c, len(rows))
        elif kind == 'differ':
            assert not np.array_equal(rows, case.rows(case.read(c[2]))), (case.label, c)
        elif kind == 'hitq':
            assert sorted(h[0] for h in hits) == c[2], (case.label, c, sorted(h[0] for h in hits))
        elif kind == 'perq':
            pq = {}
            for h in hits:
                pq[h[0]] = pq.get(h[0], 0) + 1
            assert pq == {q: c[4] for q in range(c[2], c[3])}, (case.label, c)
        elif kind == 'strand':
            assert len(rows) and (rows[:, 2] == c[2]).all(), (case.label, c, rows.tolist())
        elif kind == 'has_row':
            assert tuple(c[2]) in [tuple(x) for x in rows.tolist()], (case.label, c, rows.tolist())
        elif kind == 'order':
            key = rows[:, 0] if case.mode == 'R' else rows[:, 0] + rows[:, 3]
            want = c[2] - (case.k if case.mode == 'R' else 0)
            assert rows[key == want][:, 1].tolist() == c[3], (case.label, c, rows[key == want].tolist())
        elif kind == 'nguides':
            assert len(case.guides(i)) == c[2], (case.label, c, len(case.guides(i)))
        elif kind == 'nwindows':
            assert [len(t['windows']) for _, t in case.traces(i)] == [c[2]], (case.label, c)
        elif kind == 'tile':
            B_, h = BUILDS[c[2]], c[3]
            pq = case.traces(i)[0][1]['per_q']
            L = len(case.reads[i].buf)
            got = {simulate_tile(pq, 0, L - case.k + 1, B_, carried) for carried in (0, h)}
            assert len(got) == 1, (case.label, c, got)
            got = got.pop()
            want = {'once': got != 'hit tile' and got[1] == B_['QC'] // 2, 'at16': got != 'hit tile' and got[1] == 16, 'fail': got == 'hit tile'}[c[1]]
            assert want, (case.label, c, got)
        else:
            raise AssertionError('unknown claim %r' % (c,))


# ------------------------------------------------------------------------------------------------ the shared check
def same(got, exp, case, rd, what):
    if np.array_equal(got, exp):
        return
    n = min(len(got), len(exp))
    d = np.nonzero((np.asarray(got)[:n] != exp[:n]).any(axis=1))[0]
    at = int(d[0]) if len(d) else n
    raise AssertionError('%s: %s read %s: %d rows against the spec\'s %d; first differing row %d: %s against %s'
                         % (what, case.label, rd.label, len(got), len(exp), at, got[at].tolist() if at < len(got) else None,
                            exp[at].tolist() if at < len(exp) else None))


def parse_trace(text):
    """[(reads, handed back, {reason: count})] of every trace line in `text`"""
    return [(int(m.group(1)), int(m.group(2)), {r: int(v) for r, v in zip(REASONS, m.groups()[2:]) if int(v)}) for m in TRACE_RE.finditer(text)]


def check_case(ctx, index, case, build, band, trace):
    """local_chain_batch on every read of the case in ONE call against spec_ref.local_raw: status 0 and the rows of `raw`, row for row (a read
    without any local anchor has nothing to chain: raw is empty, the status stays 0) — and against spec_ref.local_dp applied to those rows: variant, score
    as bits and the chain (Case.dp: not -mode asm, whose DP is another one, and not the reads of more than DP_ROWS rows). band: VMX_LSEED_BAND as the caller has
    set it in the environment together with VMX_LSEED_TRACE; trace() returns what the process wrote to stderr since the last call. With the
    banded form on, the trace line's hand-backs must be exactly the case's expected ones, and the reads expected to stay, run again on their own,
    must all stay."""
    from vacmap_amd.lib import local_chain_batch
    prm = ctx.lib.params(case.mode, local_kmersize=case.k)

    def run(ids, what):
        trace()
        res = local_chain_batch(ctx, index, prm, [case.reads[i].seq for i in ids], [case.reads[i].paths for i in ids])
        lines = parse_trace(trace())
        for i, g in zip(ids, res):
            exp = case.rows(i)
            assert g['status'] == 0, (what, case.label, case.reads[i].label, g['status'])
            same(g['raw'], exp, case, case.reads[i], what)
            assert len(exp) == 0 or 0 < exp[:, 3].min() and exp[:, 3].max() <= max(19, case.k), (case.label, 'a run is flushed before it reaches 20 (:23240): the 16-bit length field is exact')
            e = case.dp(i)
            if e is not None and not e['switch']:
                assert g['variant'] == e['variant'], (what, case.label, case.reads[i].label, 'variant', g['variant'], e['variant'])
                assert np.float64(g['score']).view(np.uint64) == np.float64(e['score']).view(np.uint64), (what, case.label, case.reads[i].label, 'score', g['score'], e['score'])
                same(g['chain'], e['chain'], case, case.reads[i], what + ', chain')
            elif len(exp) == 0:
                assert len(g['chain']) == 0, (what, case.label, case.reads[i].label, 'a chain without rows')
        return lines

    ids = list(range(len(case.reads)))
    lines = run(ids, 'VMX_LSEED_BAND=%d' % band)
    if not band:
        assert lines == [], lines
        return
    want = {}
    for rd in case.reads:
        if rd.expect:
            want[rd.expect] = want.get(rd.expect, 0) + 1
    assert lines == [(len(ids), sum(want.values()), want)], (case.label, 'hand-backs', lines, want)
    stay = [i for i in ids if not case.reads[i].expect]
    if want and stay:
        lines = run(stay, 'VMX_LSEED_BAND=1, the reads meant for the banded form alone')
        assert lines == [(len(stay), 0, {})], (case.label, 'a read meant for the banded form was handed back', lines)
