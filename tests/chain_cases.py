"""Constructed anchor sets for the global chain DP (k_chain.hip, k_chain_rows.hip, k_chain_fast.hip, k_chain_linked.hip) and the shared checks.

A seeded, deterministic generator of cases (label, mode, readlen, maxdiff, anchors) placed AT the reference loop's rule boundaries
(mammap_clrnano.py:24828-25031, mode R: mammap_noprefercloser.py:23440-23603) and at the kernels' layout thresholds. Shared by the fixture
recorder (tools/harness/gen_golden_chain_edges.py), test_chain_edges.py (oracle), test_emu_chain_edges.py and test_gpu_chain_edges.py.

Every set obeys what map() guarantees (0 <= q, q + l <= readlen, s = +1 / -1) and is handed over in shuffled row order, so that the stable
order of k_flip_sort counts. Sets are built in "DP space" (the orientation the DP sees) with a majority of forward anchors; every family is
emitted as it stands and MIRRORED (q -> readlen - q - l, s -> -s), which the strand flip (:21202) turns back — with the rows reversed, so that
ties at one read position come out in the other order."""
import numpy as np

K = {'H': 15, 'L': 19, 'S': 15, 'R': 15}              # k-mer size of each mode's index (vacmap:257-296)
SKIP = {'H': 40., 'L': 40., 'S': 30., 'R': 30.}      # -globalpenalty defaults; the checks assert that the build's vm_params agree
MAXGAP = 1000                                          # decode_hit :23991
REPEAT_WEIGHT = 20                                     # :24834
NOPRE = -9999999
FAR = 10_000_000                                       # reference distance between unrelated pieces: every table has long saturated by then


class Case:
    def __init__(self, label, mode, readlen, anchors, maxdiff=50, record=True):
        self.label, self.mode, self.readlen, self.maxdiff, self.record = label, mode, int(readlen), int(maxdiff), record
        self.anchors = np.ascontiguousarray(anchors, dtype=np.int64).reshape(-1, 4)
        a = self.anchors
        assert len(a) == 0 or (a[:, 0].min() >= 0 and (a[:, 0] + a[:, 3]).max() <= self.readlen and set(np.unique(a[:, 2])) <= {-1, 1} and a[:, 3].min() > 0), label
        assert len(a) == 0 or a[:, 1].min() >= 0, label

    @property
    def k(self):
        return K[self.mode]


# ------------------------------------------------------------------------------------------------ geometry (DP space)
def run(q0, r0, s, n, l=15, gap=0):
    """n co-linear anchors, read gap = reference gap = `gap` between neighbours: gapcost 0, integer scores l, 2l, ..."""
    st = l + gap
    return [(q0 + t * st, r0 + t * st if s == 1 else r0 - t * st, s, l) for t in range(n)]


def place(aj, s_i, l_i, readgap, refgap):
    """the anchor i behind j for which the reference's gap geometry (:24953-24981) gives exactly (readgap, refgap); readgap < 0 = overlap"""
    qj, rj, sj, lj = aj
    if readgap < 0:
        ov = -readgap
        qi = qj + lj - ov
        bonus = l_i - ov
        assert 0 < ov <= lj and qi >= qj
        if s_i == sj:
            ri = refgap + rj + lj - ov if s_i == 1 else rj - bonus - refgap
        else:
            ri = refgap + rj - ov - 1 if sj == -1 else refgap + 1 + rj + lj - bonus
    else:
        qi = qj + lj + readgap
        if s_i == sj:
            ri = rj + lj + refgap if s_i == 1 else rj - l_i - refgap
        else:
            ri = refgap + rj - 1 if sj == -1 else refgap - l_i + 1 + rj + lj
    return (qi, ri, s_i, l_i)


def geometry(ai, aj):
    """(readgap, refgap, bonus) of :24953-24981, stated again for the generator's self-check (test_chain_edges.py)"""
    readgap = ai[0] - aj[0] - aj[3]
    if readgap < 0:
        bonus = ai[0] + ai[3] - aj[0] - aj[3]; readgap = 0; ov = aj[0] + aj[3] - ai[0]
        if ai[2] == aj[2]:
            refgap = ai[1] + ov - (aj[1] + aj[3]) if ai[2] == 1 else aj[1] - (ai[1] + bonus)
        else:
            refgap = ai[1] + ov - aj[1] + 1 if aj[2] == -1 else ai[1] + bonus - 1 - (aj[1] + aj[3])
    else:
        bonus = ai[3]
        if ai[2] == aj[2]:
            refgap = ai[1] - aj[1] - aj[3] if ai[2] == 1 else aj[1] - ai[1] - ai[3]
        else:
            refgap = ai[1] - aj[1] + 1 if aj[2] == -1 else ai[1] + ai[3] - 1 - aj[1] - aj[3]
    return readgap, refgap, bonus


class Builder:
    """collects the rows of one set; islands are put far apart on the reference and behind each other on the read"""

    def __init__(self, rng, l=15):
        self.rng, self.rows, self.l, self.q, self.isl = rng, [], l, 3, 0

    def base(self, s):
        self.isl += 1
        return 4 * FAR + self.isl * FAR + (0 if s == 1 else FAR // 2)

    def add(self, rows):
        self.rows += [tuple(int(v) for v in r) for r in rows]
        self.q = max(self.q, max(r[0] + r[3] for r in rows))

    def copies(self, q, n, l=None):
        """n more anchors at read position q, each alone on the reference (coverage)"""
        for t in range(n):
            self.rows.append((q, self.base(1) + 977 * t, 1 if t % 3 else -1, l or self.l))

    def pair(self, s_j, s_i, readgap, refgap, cov=1, lead=3, tail=2, l_i=None, gapq=1200):
        """an island: `lead` co-linear anchors on strand s_j, then anchor i at (readgap, refgap) from the last of them, with `cov` anchors at
        i's read position, then `tail` co-linear anchors behind i"""
        l = self.l
        pre = run(self.q + gapq, self.base(s_j), s_j, lead, l)
        ai = place(pre[-1], s_i, l_i or l, readgap, refgap)
        assert geometry(ai, pre[-1])[:2] == (max(readgap, 0), refgap)
        post = run(ai[0] + ai[3] + 2, ai[1] + ai[3] + 2 if s_i == 1 else ai[1] - l - 2, s_i, tail, l) if tail else []
        self.add(pre + [ai] + post)
        self.copies(ai[0], cov - 1)
        return ai

    def ballast(self):
        """forward anchors, each alone, until the forward strand has the majority (no flip in DP space)"""
        neg = sum(1 for r in self.rows if r[2] == -1); pos = len(self.rows) - neg
        used = {r[0] for r in self.rows}
        q = 0
        while pos <= neg:
            while q in used:
                q += 1
            self.rows.append((q, self.base(1), 1, self.l)); used.add(q); pos += 1
        self.q = max(self.q, max(r[0] + r[3] for r in self.rows))

    def cases(self, label, mode, maxdiff=50, pad=None, mirror=True, record=True):
        self.ballast()
        a = np.array(self.rows, dtype=np.int64)
        readlen = int((a[:, 0] + a[:, 3]).max()) + (int(self.rng.integers(0, 40)) if pad is None else pad)
        out = [Case(label, mode, readlen, a[self.rng.permutation(len(a))], maxdiff, record)]
        if mirror:
            m = a.copy(); m[:, 0] = readlen - a[:, 0] - a[:, 3]; m[:, 2] = -a[:, 2]
            out.append(Case(label + '/mirrored', mode, readlen, m[self.rng.permutation(len(m))], maxdiff, record))
        return out


def eff_maxdiff(mode, maxdiff, cov):
    return maxdiff if mode == 'R' else max(maxdiff - min(cov, REPEAT_WEIGHT), 10)


# ------------------------------------------------------------------------------------------------ rule boundaries
def gap_rule_cases(rng, mode):
    """|readgap - refgap| at maxdiff - 1 / 0 / + 1 on both sides, with the coverage at i's position moving maxdiff down to its floor of 10"""
    out = []
    for maxdiff, cov in ((50, 1), (50, 19), (50, 20), (50, 21), (25, 14), (25, 15), (25, 16), (25, 30), (12, 1), (12, 2), (12, 3)):
        md = eff_maxdiff(mode, maxdiff, cov)
        for s in (1, -1):
            b = Builder(rng, K[mode] if mode == 'L' else 15)
            for d in (-1, 0, 1):
                b.pair(s, s, 70, 70 + md + d, cov)
                b.pair(s, s, 70, 70 - md - d, cov)
            out += b.cases('gap/maxdiff%d/cov%d/%s' % (maxdiff, cov, '+-'[s < 0]), mode, maxdiff)
    for s in (1, -1):
        b = Builder(rng)
        for rg in (MAXGAP - 1, MAXGAP, MAXGAP + 1):
            b.pair(s, s, rg, rg); b.pair(s, s, rg, rg + 3); b.pair(s, s, rg, rg - 50 if mode == 'R' else rg - 49)
        for rg, fg in ((0, -1), (0, 0), (1, -1), (1, 0), (5, -1), (5, 0), (0, 1)):
            b.pair(s, s, rg, fg)
        out += b.cases('gap/maxgap_refgap/%s' % '+-'[s < 0], mode)
    return out


def overlap_cases(rng, mode):
    """readgap < 0 in all four strand combinations (:24955-24968): co-linear at maxdiff -1 / 0 / +1, refgap -1 / 0, and far jumps"""
    out = []
    md = eff_maxdiff(mode, 50, 1)
    for s_j in (1, -1):
        for s_i in (1, -1):
            b = Builder(rng)
            for ov in (1, 7, 14, 15):
                for fg in (-1, 0, 2, md - 1, md, md + 1, 400, 30000):
                    b.pair(s_j, s_i, -ov, fg, l_i=15 if ov < 15 else 22)
            out += b.cases('overlap/%s%s' % ('+-'[s_j < 0], '+-'[s_i < 0]), mode)
    return out


def coverage_cases(rng, mode):
    """1, 19, 20, 21, 30 anchors at one read position (saturation at repeat_weight), inside a chain that needs the skip cost and maxdiff there"""
    out = []
    for c in (1, 19, 20, 21, 30):
        b = Builder(rng)
        for s in (1, -1):
            md = eff_maxdiff(mode, 50, c)
            b.pair(s, s, 40, 40 + md, c, lead=8); b.pair(s, s, 40, 40 + md + 1, c, lead=8)
            b.pair(s, s, 10, 3000, c, lead=8)                 # a skip that pays skipcost + coverage and still wins
        out += b.cases('coverage/%d' % c, mode)
    for n in (3, 25):
        rows = [(7, 5 * FAR + 1000 * t, 1 if t % 4 else -1, 15) for t in range(n)]
        b = Builder(rng); b.add(rows)
        out += b.cases('coverage/all_at_one_q/%d' % n, mode, pad=0)
    return out


def tie_cases(rng, mode, windows=(3, 16)):
    out = []
    sizes = sorted({w + d for w in windows for d in (-1, 0, 1, 2)} | {2 * w + d for w in windows for d in (-1, 0, 1)} | {63, 64, 65, 129})
    for n in sizes:                                            # isolated anchors of equal score: every insertion meets equal keys, no scan breaks
        for per_q in (1, 3):
            b = Builder(rng)
            b.add([(5 + 20 * (t // per_q), b.base(1), 1 if t % 5 else -1, 15) for t in range(n)])
            out += b.cases('ties/isolated/%d/per_q%d' % (n, per_q), mode)
    for s in (1, -1):                                          # two predecessors with exactly the same test score
        b = Builder(rng)
        for lead in (8, 9):
            q0 = b.q + 1200
            x = run(q0, b.base(s), s, lead); y = run(q0, b.base(s), s, lead); z = run(q0 + 3, b.base(s), s, lead)
            i = (x[-1][0] + 15 + 30, b.base(s), s, 15)
            b.add(x + y + z + [i] + run(i[0] + 17, i[1] + 17 if s == 1 else i[1] - 17, s, 2))
        out += b.cases('ties/two_predecessors/%s' % '+-'[s < 0], mode)
    for s in (1, -1):                                          # S[j] == max_scores - l_i exactly: the scan stops AT that entry
        b = Builder(rng)
        for lead in (3, 5):
            q0 = b.q + 1200
            x = run(q0, b.base(s), s, lead); y = run(q0 + 1, b.base(s), s, lead); w = run(q0 + 2, b.base(s), s, lead)
            i = place(x[-1], s, 15, 4, 4)
            b.add(x + y + w + [i] + run(i[0] + 20, i[1] + 20 if s == 1 else i[1] - 20, s, 2))
        out += b.cases('ties/break_rule/%s' % '+-'[s < 0], mode)
    return out


def mode_r_cases(rng):
    """the refund of mode R (fixed_penatly + bonus at -1 / 0 / +1, mammap_noprefercloser.py:23557-23570): a skip of 30 into an anchor of
    length l1, then co-linear anchors whose bonus brings fixed_penatly to -1, 0, +1 — in one step, in two, and through an overlap"""
    out = []
    for s in (1, -1):
        b = Builder(rng)
        for l1 in (15, 8):
            need = 30 - l1
            for d in (-1, 0, 1):
                def island(steps):
                    q0 = b.q + 1200
                    x = run(q0, b.base(s), s, 8)
                    cur = (x[-1][0] + 15 + 25, b.base(s), s, l1)
                    rows = x + [cur]
                    for l_i, rg in steps:
                        cur = place(cur, s, l_i, rg, abs(rg)) if rg >= 0 else place(cur, s, l_i, rg, 0)
                        rows.append(cur)
                    rows += run(cur[0] + cur[3] + 1, cur[1] + cur[3] + 1 if s == 1 else cur[1] - 16, s, 3)
                    b.add(rows)
                island([(need + d, 3)])
                island([(5, 0), (need - 5 + d, 2)])
                island([(need + d + 4, -4)])
        out += b.cases('modeR/refund/%s' % '+-'[s < 0], 'R')
    return out


def extra_table_cases(rng, mode):
    """skips whose |readgap - refgap| lands around the ends of the `extra` table's stretches (:15371-15376: gapcost / 100 up to 1000, gapcost / 1000
    on top, 30 + ln(gapcost) / 2 from ~24 900, flat 36.0 from 162 755), past 2^30 and 2^31, and with reference positions above 2^32"""
    out = []
    jumps = [11 if mode == 'R' else 51, 99, 100, 101, 999, 1000, 1001, 9999, 10001, 24000, 24900, 25000, 26000, 162753, 162754, 162755, 162756,
             2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 + 5]
    for s in (1, -1):
        for hi in (0, 1):
            b = Builder(rng)
            b.isl = 900 * hi                                   # reference positions from ~9e9 on: above 2^32
            for g in jumps:
                if s == -1 and g > 2 ** 29 and not hi:
                    continue                                   # (would leave the reference to the left)
                b.pair(s, s, 20, 20 + g, lead=8)
                b.pair(s, -s, 20, g, lead=8)
            out += b.cases('extra/%s/%s' % ('+-'[s < 0], 'r_above_2^32' if hi else 'r_low'), mode)
    return out


def form_cases(rng, mode):
    out = []
    # anchors per base at 5.0 exactly (GC-exact) and just above (GC-fast, :23570)
    for L, extra_n in ((60, 0), (60, 1), (61, 0)):
        n = 5 * 60 + extra_n
        rows = []
        cps = [5 * FAR + 3000 * c for c in range(12)]
        for t in range(n):
            q = t % (60 - 15 + 1)
            c = cps[(t // 46) % 12]
            rows.append((q, c + q + (1 if t % 17 == 0 else 0), 1, 15) if t % 7 else (q, c + 9000 - q, -1, 15))
        a = np.array(rows, dtype=np.int64)
        out.append(Case('form/per_base/%d_over_%d' % (n, L), mode, L, a[rng.permutation(n)]))
        m = a.copy(); m[:, 0] = L - a[:, 0] - 15; m[:, 2] = -a[:, 2]
        out.append(Case('form/per_base/%d_over_%d/mirrored' % (n, L), mode, L, m[rng.permutation(n)]))
    # n = 0 ... 3 (a read of two anchors or fewer is not chained, :23986) and the strand tie neg == pos (no flip)
    for n in (0, 1, 2, 3):
        for s in (1, -1):
            rows = run(4, 5 * FAR, s, n, 15, 2)
            out.append(Case('form/n%d/%s' % (n, '+-'[s < 0]), mode, 80, np.array(rows, dtype=np.int64).reshape(-1, 4)))
    for n in (2, 6):
        a = np.array(run(4, 5 * FAR, 1, n, 15, 2) + run(9, 7 * FAR, -1, n, 15, 2), dtype=np.int64)
        out.append(Case('form/strand_tie/%d' % (2 * n), mode, int((a[:, 0] + a[:, 3]).max()) + 5, a[rng.permutation(len(a))]))
    return out


def bailout_cases(rng, mode):
    """isolated equal anchors never break a scan: opcount / i crosses max_factor = 1000 (:24914) at i = 2002 — a set of 2002 anchors stays in
    GC-exact, 2003 bail out into GC-fast"""
    out = []
    for n in (2002, 2003):
        a = np.array([(2 + t, 5 * FAR + 5000 * t, 1 if t % 9 else -1, 15) for t in range(n)], dtype=np.int64)
        out.append(Case('form/bailout/%d' % n, mode, n + 20, a[rng.permutation(n)]))
    if mode == 'H':
        # GC-fast on a length at the 16-bit edge (k_chain_fast.hip reads vmx_anchor.l through vmx_anchor_len): the bail-out set, a row of l = 32 768 chained
        # co-linearly behind it and a last row far enough out that the scores stay inside the twin's score table (last q + 50). Oracle only.
        n = 2003
        rows = [(2 + t, 5 * FAR + 5000 * t, 1 if t % 9 else -1, 15) for t in range(n)]
        rows += [(2100, 900 * FAR, 1, 15), (2117, 900 * FAR + 17, 1, 32768), (2117 + 32768 + 3, 900 * FAR + 17 + 32768 + 3, 1, 15), (40000, 950 * FAR, 1, 15)]
        a = np.array(rows, dtype=np.int64)
        out.append(Case('form/bailout/l32768', mode, 40040, a[np.random.default_rng(32768).permutation(len(a))], record=False))     # (its own stream: the recorded sets keep theirs)
    return out


def l16_cases(rng, mode):
    """anchor lengths at the 16-bit edge of the device row (vmx_anchor.l): 65 535 is the largest the stage entries accept"""
    out = []
    for l in (32767, 32768, 65535):
        b = Builder(rng, l)
        b.add(run(3, 5 * FAR, 1, 40, l, 0) + run(11, 900 * FAR, -1, 7, l, 5))
        out += b.cases('form/l%d' % l, mode, pad=0)
    return out


# ------------------------------------------------------------------------------------------------ layout boundaries and the random part
def realistic(rng, n, style, l=15):
    """n anchors of one of three styles: 0 co-linear runs with jitter and overlaps, 1 several copies per read position, 2 gaps at maxdiff / maxgap +- 1"""
    rows = []
    q = int(rng.integers(0, 30))
    r = {1: 5 * FAR + int(rng.integers(0, FAR)), -1: 300 * FAR + int(rng.integers(0, FAR))}
    s = 1
    while len(rows) < n:
        u = rng.random()
        if u < 0.04:
            s = -s if rng.random() < 0.5 else s
            r[s] += int(rng.integers(-3000, 30000)) * s
        if style == 2 and u > 0.8:
            rg = int(rng.choice([999, 1000, 1001, 60, 60, 60])); d = int(rng.choice([-51, -50, -49, -40, -39, 39, 40, 41, 49, 50, 51])) if rg == 60 else 0
        else:
            rg = int(rng.integers(-10, 25)); d = int(rng.integers(-2, 3)) if rng.random() < 0.3 else 0
        q = max(q + l + rg, 0)
        r[s] += (l + max(rg, -l + 1) + d) * s
        rows.append((q, max(r[s], 0), s, l))
        if style == 1 and len(rows) < n:
            for c in range(int(rng.integers(0, 4))):
                if len(rows) < n:
                    rows.append((q, 600 * FAR + int(rng.integers(0, 40 * FAR)), int(rng.choice([-1, 1])), l))
        elif rng.random() < 0.15 and len(rows) < n:
            rows.append((max(q - int(rng.integers(0, 9)), 0), 600 * FAR + int(rng.integers(0, 40 * FAR)), int(rng.choice([-1, 1])), l))
    a = np.array(rows[:n], dtype=np.int64)
    readlen = int((a[:, 0] + a[:, 3]).max()) + int(rng.integers(0, 50))
    return readlen, a[rng.permutation(n)]


def layout_sizes(windows=(3, 16), blocks=(16, 64), sort_tile=4096, lds_caps=(384, 512), select_caps=(192, 384, 768, 1536, 3072)):
    """anchor counts around every layout threshold, each -1 / 0 / +1. The defaults are the constants that the GPU build and the emulator build share
    (vmx_kernels.h: VMX_SORT_LDS, VMX_CHAIN_LDS_MAX_SHARED; vmx_align.hip: the LDS buckets and the selection classes; k_chain_rows.hip: the window and
    the register blocks); the recorded fixture depends on them, and test_chain_edges.py fails if the sources state other values"""
    c = set(windows) | set(blocks) | {2 * b for b in blocks} | set(lds_caps) | set(select_caps) | {sort_tile}
    c |= {p for p in (128, 256, 512, 1024, 2048) if p <= sort_tile}
    return sorted({x + d for x in c for d in (-1, 0, 1) if x + d >= 3})


def layout_cases(rng, mode, sizes, record_max=800):
    return [Case('layout/n%d/style%d' % (n, i % 3), mode, *realistic(rng, n, i % 3, K[mode] if mode == 'L' else 15), record=n <= record_max) for i, n in enumerate(sizes)]


def random_cases(rng, mode, count, nmax=900):
    out = []
    for i in range(count):
        n = int(rng.integers(3, 40)) if rng.random() < 0.5 else int(rng.integers(3, nmax + 1))
        out.append(Case('random/%d' % i, mode, *realistic(rng, n, i % 3), maxdiff=int(rng.choice([50, 50, 25, 12])), record=False))
    return out


def constructed(seed=20261, modes=('H', 'L', 'S', 'R'), bailout=True):
    """the constructed part: every rule-boundary family in every mode it applies to, the form switches and the layout sizes"""
    rng = np.random.default_rng(seed)
    out = []
    for mode in modes:
        out += gap_rule_cases(rng, mode) + overlap_cases(rng, mode) + coverage_cases(rng, mode) + tie_cases(rng, mode)
        out += extra_table_cases(rng, mode) + form_cases(rng, mode)
        if mode == 'R':
            out += mode_r_cases(rng)
        if mode in ('H', 'R'):
            out += l16_cases(rng, mode) + layout_cases(rng, mode, layout_sizes())
            if bailout:
                out += bailout_cases(rng, mode)
    labels = [(c.mode, c.label) for c in out]
    assert len(set(labels)) == len(labels)
    return out


def key(c):
    return '%s:%s' % (c.mode, c.label)


# ------------------------------------------------------------------------------------------------ expectations
_fixture = None


def fixture():
    """tests/golden/chain_edges.{json,npz}: what the reference computed on the recorded sets (tools/harness/gen_golden_chain_edges.py)"""
    global _fixture
    if _fixture is None:
        import json, os
        g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
        _fixture = (json.load(open(os.path.join(g, 'chain_edges.json'))), dict(np.load(os.path.join(g, 'chain_edges.npz'))))
    return _fixture


def expected_recorded(c):
    """the reference's result of a recorded case; the stored input must be the generator's"""
    meta, arr = fixture()
    r = meta[key(c)]
    n = r['n']
    assert (r['readlen'], r['maxdiff'], n) == (c.readlen, c.maxdiff, len(c.anchors)) and np.array_equal(arr['a'][r['a_off']:r['a_off'] + n], c.anchors), key(c)
    e = {'mapq': r['mapq'], 'score': r['score'], 'paths': [], 'n': n}
    o = r['path_off']
    for m in r['path_lens']:
        e['paths'].append(arr['paths'][o:o + m].tolist()); o += m
    if n > 2:
        d = r['dp_off']
        e.update(need_reverse=r['need_reverse'], fast_used=r['fast_used'], gmax=r['gmax'], S=arr['S'][d:d + n], P=arr['P'][d:d + n].astype(np.int64), S_arg=arr['SA'][d:d + n].astype(np.int64))
    return e


def expected_oracle(c, O):
    """the same from the CPU oracle, run live — plus the exact DP's opcount, which the reference does not return"""
    n = len(c.anchors)
    prm = O.params(c.mode, global_maxdiff=c.maxdiff)
    assert prm.global_skipcost == SKIP[c.mode]
    e = {'n': n}
    if n > 2:
        flag, fl = O.strand_flip(c.anchors.copy(), c.readlen)
        srt = fl[np.argsort(fl[:, 0], kind='stable')]
        fast = n / c.readlen > 5
        if not fast:
            g, S, P, SA = O.chain_global_raw(srt, c.k, SKIP[c.mode], c.maxdiff, MAXGAP, 0, c.mode)
            e['opcount'] = O.chain_global_opcount(srt, c.k, SKIP[c.mode], c.maxdiff, MAXGAP, c.mode)
            fast = g == -1
        if fast:
            g, S, P, SA = O.chain_global_raw(srt, c.k, SKIP[c.mode], c.maxdiff, MAXGAP, 1, c.mode)
        e.update(need_reverse=bool(flag), fast_used=bool(fast), gmax=int(g), S=S, P=P, S_arg=SA)
    o = O.decode_hit(c.anchors, c.readlen, c.k, prm)
    if o['rc'] == 0:
        e.update(mapq=o['mapq'], score=o['score'], paths=[p.tolist() for p in o['paths']])
    else:                                                      # mode R with two anchors or fewer: the reference raises, the read stays unmapped
        assert c.mode == 'R' and n <= 2
        e.update(mapq=0, score=0., paths=[])
    return e


def same(e, g, what):
    """exact comparison of one read: no tolerance anywhere; S as bit patterns"""
    if e['n'] > 2:
        assert (g['need_reverse'], g['fast_used'], g['gmax']) == (e['need_reverse'], e['fast_used'], e['gmax']), (what, 'need_reverse / fast_used / gmax',
                                                                                                                   g['need_reverse'], g['fast_used'], g['gmax'], e['need_reverse'], e['fast_used'], e['gmax'])
        bad = np.flatnonzero(g['S'].view(np.uint64) != np.asarray(e['S']).view(np.uint64))
        assert len(bad) == 0, (what, 'S', int(bad[0]), float(g['S'][bad[0]]), float(e['S'][bad[0]]))
        bad = np.flatnonzero(g['P'] != e['P'])
        assert len(bad) == 0, (what, 'P', int(bad[0]), int(g['P'][bad[0]]), int(e['P'][bad[0]]))
        bad = np.flatnonzero(g['S_arg'] != e['S_arg'])
        assert len(bad) == 0, (what, 'S_arg', int(bad[0]), int(g['S_arg'][bad[0]]), int(e['S_arg'][bad[0]]))
        if 'opcount' in e and not e['fast_used']:
            assert g['opcount'] == e['opcount'], (what, 'opcount', g['opcount'], e['opcount'])
    else:
        assert g['gmax'] == -1 and not g['paths'], (what, g['gmax'])
    assert (g['mapq'], g['score']) == (e['mapq'], e['score']), (what, 'mapq / score', g['mapq'], g['score'], e['mapq'], e['score'])
    assert [p.tolist() for p in g['paths']] == e['paths'], (what, 'paths')


def batches(cases):
    """cases of one (mode, maxdiff) together, in batches of 1, 2, ... 9, 1, ... reads: wave rows idle, long reads sit beside short ones"""
    groups = {}
    for c in cases:
        groups.setdefault((c.mode, c.maxdiff), []).append(c)
    size = 0
    for (mode, maxdiff), cs in sorted(groups.items()):
        i = 0
        while i < len(cs):
            size = size % 9 + 1
            yield mode, maxdiff, cs[i:i + size]
            i += size


def run_cases(ctx, cases):
    """[(case, result of vm_chain_global_batch(want_raw=1))]"""
    out = []
    for mode, maxdiff, cs in batches(cases):
        prm = ctx.lib.params(mode, global_maxdiff=maxdiff)
        assert prm.global_skipcost == SKIP[mode]
        res = ctx.chain_global_batch(prm, K[mode], [c.anchors for c in cs], [c.readlen for c in cs], want_raw=True)
        out += list(zip(cs, res))
    return out


def check_global(ctx, O, cases, tag=''):
    """every read equals the fixture where it is recorded, and the oracle run live; returns the number of reads compared"""
    for c, g in run_cases(ctx, cases):
        if c.record:
            same(expected_recorded(c), g, (tag, key(c), 'vs the reference fixture'))
        same(expected_oracle(c, O), g, (tag, key(c), 'vs the oracle'))
    return len(cases)


def check_long_beside_short(ctx, O, seed=77):
    """one long read beside three short ones in one wave of the row kernels, the long one in each of the four rows"""
    rng = np.random.default_rng(seed)
    n = 0
    for mode in ('H', 'R'):
        for pos in range(4):
            cs = [Case('short%d' % i, mode, *realistic(rng, 3 + i, i % 3), record=False) for i in range(3)]
            cs.insert(pos, Case('long', mode, *realistic(rng, 1400, pos % 3), record=False))
            res = ctx.chain_global_batch(ctx.lib.params(mode), K[mode], [c.anchors for c in cs], [c.readlen for c in cs], want_raw=True)
            for c, g in zip(cs, res):
                same(expected_oracle(c, O), g, ('long beside short', mode, pos, c.label))
            n += 4
    return n


def check_refusals(ctx, O):
    """vm_chain_global_batch / vm_chain_linked refuse rows that the device's 16 / 32-bit fields cannot carry (VM_ERR_UNSUPPORTED) instead of truncating them;
    the largest accepted length chains like any other, and so do rows that end at the largest accepted position q + l = 2^31 - 1 — through vm_chain_linked,
    which takes no read length and keeps nothing per base (vm_chain_global_batch would need a read of 2 Gb and its per-base tables for them)."""
    from vacmap_amd.lib import VmxError
    UNSUPPORTED = -7
    prm = ctx.lib.params('H')

    def rows(l, q0=3, n=40):
        return np.array(run(q0, 5 * FAR, 1, n, l), dtype=np.int64)
    a = rows(65535)
    g = ctx.chain_global_batch(prm, 15, [a], [int(a[-1, 0]) + 65535], want_raw=True)[0]
    same(expected_oracle(Case('l65535', 'H', int(a[-1, 0]) + 65535, a, record=False), O), g, 'largest accepted length')
    r = ctx.chain_linked(a, 0, 15, 30., 50, 1000)
    eg, eS, eP, eSA = O.chain_linked_raw(a, 0, 15, 30., 50, 1000)
    assert r['gmax'] == eg == 39 and np.array_equal(r['S'].view(np.uint64), eS.view(np.uint64)) and np.array_equal(r['P'], eP)
    top = 2 ** 31 - 1
    for s_ in (1, -1):                                         # co-linear runs, a skip and an overlap whose last anchor ends at q + l = 2^31 - 1
        e = run(top - 15 - 39 * 17, 5 * FAR if s_ == 1 else 9 * FAR, s_, 40, 15, 2)
        e = run(e[0][0] - 3000, 7 * FAR, -s_, 9, 15, 0) + e[:-1] + [place(e[-2], s_, 15 + 2 + 6, -6, 0)]
        e = np.array(sorted(e), dtype=np.int64)
        assert int((e[:, 0] + e[:, 3]).max()) == top and int(e[-1, 0] + e[-1, 3]) == top
        for which, (k_, skip_, md_, mg_) in LINKED_ARGS.items():
            exp = O.chain_linked_raw(e, which, k_, skip_, md_, mg_)
            assert exp[0] == len(e) - 1 and exp[2][-1] == len(e) - 2          # the best chain ends in the last row, reached co-linearly
            _same_linked(ctx.chain_linked(e, which, k_, skip_, md_, mg_), exp, e, skip_, ('q + l = 2^31 - 1', s_, which))
    head = [(3, 50, 1, 15), (30, 80, 1, 15)]
    bad = {'l = 65536': rows(65536), 'l = -1': np.array(head + [(60, 110, 1, -1)]), 'q + l = 2^31': np.array(head + [(2 ** 31 - 15, 2 ** 31, 1, 15)]),
           'q = 2^32 + 60': np.array(head + [(2 ** 32 + 60, 2 ** 33, 1, 15)]), 'q = -2^31 - 1': np.array([(-2 ** 31 - 1, 20, 1, 15)] + head), 's = 65537': np.array(head + [(60, 110, 65537, 15)])}
    for what, b in bad.items():
        b = np.ascontiguousarray(b, dtype=np.int64)
        L = max(int((b[:, 0] + b[:, 3]).max()), 200)
        for call in (lambda: ctx.chain_global_batch(prm, 15, [rows(15), b], [700, L]), lambda: ctx.chain_linked(b, 0, 15, 30., 50, 1000), lambda: ctx.chain_linked(b, 2, 9, 30., 30, 1000)):
            try:
                call()
            except VmxError as e:
                assert e.code == UNSUPPORTED and 'anchor row' in str(e), (what, e.code, str(e))
            else:
                raise AssertionError('%s was accepted' % what)
    # the entries still work after a refusal
    same(expected_oracle(Case('after', 'H', 700, rows(15), record=False), O), ctx.chain_global_batch(prm, 15, [rows(15)], [700], want_raw=True)[0], 'after a refusal')


# ------------------------------------------------------------------------------------------------ the linked DPs of -mode asm
LINKED_ARGS = {0: (15, 30., 50, 1000), 2: (9, 30., 30, 99)}         # (kmersize, skipcost, maxdiff, maxgap) of the reference's calls (mammap_asm.py:23228-23275 / :23328-23373)


def _carry(S, P, SA, rows, skipcost):
    """what mammap_asm.py:23250-23272 carries into the next batch, from the whole arrays: None (`continue`) or (pre_S, pre_P, pre_rows, prereadloc)"""
    g = SA[-1]
    low = S[g] - skipcost - 36 - 20
    sl = len(S) - 1
    while low < S[SA[sl]]:
        sl -= 1
        if sl == 0:
            break
    return S[SA[sl:]] - S[SA[sl]] + 1000, -P[SA[sl:]], rows[SA[sl:]], int(rows[SA[sl:], 0].max())


def _same_linked(r, exp, rows, skipcost, what):
    g, S, P, SA = exp
    assert r['gmax'] == g, (what, 'gmax', r['gmax'], g)
    assert np.array_equal(r['S'].view(np.uint64), S.view(np.uint64)), (what, 'S', np.flatnonzero(r['S'] != S)[:3])
    assert np.array_equal(r['P'], P), (what, 'P', np.flatnonzero(r['P'] != P)[:3])
    assert r['n_hot'] + r['n_cold'] == len(SA) and np.array_equal(r['S_arg_hot'], SA[len(SA) - r['n_hot']:]), (what, 'hot part of S_arg')
    if r['carry_status'] != 0:
        return 0                                               # the device reports that the slice leaves the stored part of the index (VM_READ_UNSUPPORTED): nothing carried
    if P[g] < 0:
        assert r['saved'] == 0, (what, 'saved')
        return 1
    cS, cP, cR, prl = _carry(S, P, SA, rows, skipcost)
    assert r['saved'] == 1 and r['n_carry'] == len(cS), (what, 'carry', r['saved'], r['n_carry'], len(cS))
    assert np.array_equal(r['carry_S'].view(np.uint64), cS.view(np.uint64)) and np.array_equal(r['carry_P'], cP) and np.array_equal(r['carry_rows'], cR), (what, 'carried state')
    assert r['carry_prereadloc'] == prl and r['carry_g_max_scores'] == cS[-1], (what, 'carried scalars')
    return 1


def linked_picks(cases, per_family=6):
    """the sets given to vm_chain_linked: some of every constructed family, taken in DP space (the linked path never flips), and layout sets"""
    picked, seen = [], {}
    for c in cases:
        fam = c.label.split('/')[0]
        if c.mode == 'S' and not c.label.endswith('/mirrored') and len(c.anchors) > 8 and seen.get(fam, 0) < per_family and not c.label.startswith('form/per_base'):
            seen[fam] = seen.get(fam, 0) + 1; picked.append(c)
    picked += [c for c in cases if c.mode == 'S' and c not in picked and c.label in ('ties/two_predecessors/+', 'ties/two_predecessors/-', 'ties/break_rule/+', 'ties/break_rule/-',
                                                                                  'ties/isolated/17/per_q1', 'ties/isolated/65/per_q3', 'form/per_base/300_over_60')]
    # (the winner rule, the break rule, equal keys past the window; the dense set has equal test scores more than 64 candidates apart: one block of a wave-wide scan)
    picked += [c for c in cases if c.mode == 'H' and c.label.startswith('layout/') and 60 <= len(c.anchors) <= 800][::3]
    assert len(picked) > 30 and len(seen) >= 5
    return picked


def linked_runs(c, which, dp):
    """the calls made on one set, as the reference's loop makes them (mammap_asm.py:23228-23272): the whole set as a first batch, its first half as a
    first batch, and the second half behind the state that the first half carries out. dp(rows, which, args, state) -> (g, S, P, S_arg) is the DP
    asked (the reference when recording, the oracle in the tests). Yields (name, rows, args, state, result)"""
    a = c.anchors.copy()
    a[:, 3] = np.minimum(a[:, 3], 60000)
    srt = np.ascontiguousarray(a[np.argsort(a[:, 0], kind='stable')])
    k, skip, md, mg = LINKED_ARGS[which]
    args = (k, skip, min(md, c.maxdiff), mg)
    yield 'whole', srt, args, None, dp(srt, which, args, None)
    h = len(srt) // 2
    res = dp(srt[:h], which, args, None)
    yield 'half', srt[:h], args, None, res
    g1, S1, P1, SA1 = res
    if g1 < 0 or P1[g1] < 0:
        return
    cS, cP, cR, prl = _carry(np.asarray(S1), np.asarray(P1), np.asarray(SA1), srt[:h], skip)
    linked = np.ascontiguousarray(np.concatenate([cR, srt[h:]]))
    state = (float(cS[-1]), len(cS) - 1, cS, cP, prl)
    yield 'linked', linked, args, state, dp(linked, which, args, state)


def oracle_linked(O):
    def dp(rows, which, args, state):
        return O.chain_linked_raw(rows, which, *args, *(state or ()))
    return dp


_linked_fixture = None


def linked_fixture():
    global _linked_fixture
    if _linked_fixture is None:
        import json, os
        g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
        _linked_fixture = (json.load(open(os.path.join(g, 'chain_edges_linked.json'))), dict(np.load(os.path.join(g, 'chain_edges_linked.npz'))))
    return _linked_fixture


def recorded_linked(c, which, name, rows):
    """(g, S, P, S_arg) of the reference for one call of linked_runs, or None if the reference did not make it; the stored rows must be the test's"""
    meta, arr = linked_fixture()
    r = meta.get('%s|%d|%s' % (key(c), which, name))
    if r is None:
        return None
    o, n = r['off'], r['n']
    assert n == len(rows) and np.array_equal(arr['rows'][o:o + n], rows), (key(c), which, name)
    return r['g'], arr['S'][o:o + n], arr['P'][o:o + n].astype(np.int64), arr['SA'][o:o + n].astype(np.int64)


def check_linked(ctx, O, cases):
    """vm_chain_linked (which 0: linked GC-exact, 2: linked LC) with and without carried state: S, P, the hot part of S_arg, g_max_index and the carried
    state against chain_linked_raw, which in turn must equal the reference's recorded arrays"""
    picked = linked_picks(cases)
    n_carry = n_state = 0
    for c in picked:
        for which in LINKED_ARGS:
            for name, rows, args, state, exp in linked_runs(c, which, oracle_linked(O)):
                what = (key(c), which, name)
                ref = recorded_linked(c, which, name, rows)
                assert ref is not None, what
                assert ref[0] == exp[0] and np.array_equal(ref[1].view(np.uint64), exp[1].view(np.uint64)) and np.array_equal(ref[2], exp[2]) and np.array_equal(ref[3], exp[3]), (what, 'oracle vs reference')
                if ctx is not None:
                    n_carry += _same_linked(ctx.chain_linked(rows, which, *args, *(state or ())), exp, rows, args[1], what)
                n_state += name == 'linked'
    assert n_state > len(picked) and (ctx is None or n_carry > n_state), (n_state, n_carry, len(picked))
    return n_state, n_carry


if __name__ == '__main__':
    # a fresh process for the switches that the library reads once (VMX_CHAIN_ROWS=0: the one-wavefront-per-read kernels; VMX_LINK_PLAIN=1: k_chain_linked): `chain_cases.py emu|gpu`
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_lib
    if sys.argv[1] == 'emu':
        import emu_lib
        cx = emu_lib.context()
    else:
        from vacmap_amd.lib import Context
        cx = Context(0)
    rng_ = np.random.default_rng(4300)
    all_ = constructed()
    n_ = check_global(cx, oracle_lib, all_, 'one wavefront per read')
    n_ += check_global(cx, oracle_lib, [c for mode in 'HLSR' for c in random_cases(rng_, mode, 40)], 'one wavefront per read, random')
    n_ += check_long_beside_short(cx, oracle_lib)
    if os.environ.get('VMX_LINK_PLAIN'):                       # the plain form of the linked DP (k_chain_linked.hip), also chosen once per process
        check_linked(cx, oracle_lib, all_); check_refusals(cx, oracle_lib)
    print('chain edges ok: %d reads, VMX_CHAIN_ROWS=%s' % (n_, os.environ.get('VMX_CHAIN_ROWS')))
