"""Constructed anchor rows for the LOCAL chain DPs (L3 LC-exact, L4 LC-mm, L5 their `_fast` twins, mode R's `_scar`: k_chain_rows.hip KIND 2 / 3 / 4,
k_chain_local.hip, k_chain_fast.hip, the routing of vmx_local_dp) and the shared checks of vm_local_dp_batch.

A seeded, deterministic generator of sets (label, mode, guide count, k, maxdiff, skip cost, rows, read length) placed AT the rule boundaries of
mammap_clrnano.py:27305-27528 / :28250-28476 and mammap_noprefercloser.py:23419-23628 and at the kernels' layout thresholds. Rows are built as tagged
islands, far apart on the reference, and then put into the DP's input order (stable by q + l, mode R by q): the entry takes them in that order. Every
family comes as it stands and MIRRORED (q -> L - q - l, s -> -s, sorted again), in every mode its rule exists in, and — outside mode R — once per
variant (one guide chain: LC-exact, two: LC-mm). Each set carries CLAIMS about what spec_ref.local_dp does on it (which row wins through which kind
of step, which counters of the spec's are not zero): check_claims proves them from the spec alone, so a family that no longer reaches its branch
fails on the CPU.

What the DP's input order leaves of some edges, found while building the families:
  * LC-exact / LC-mm see `bonus <= 0` only as bonus == 0 against ROW 0: a candidate is visible once a row with a LARGER read end has advanced the candidate
    space, and rows come in order of read end, so every candidate ends before the current row — except row 0, which is visible from the start to the rows that
    share its read end (overlap/row0_twin). `_scar` (rows by read start, space advanced on read ends) reaches negative bonuses: a long row that starts first
    and ends last.
  * the `_fast` twins' non-terminating `continue` (bonus <= 0 in a bucket of more than five entries) is unreachable for rows in order of read end: bonus <= 0
    needs a visible candidate that ends at or behind the current row; only row 0 can be that, and only before the first advance, when its bucket holds one
    entry. The host's order check (vmx_local_rows.h) is what keeps that loop out of k_chain_local_fast.
  * a row of l >= 32 767 as ROW 0 of a set that switches needs opcount > 1000 (l + 14): a0_cases builds it from 9 301 rows (l = 65 535: 12 751) that all end
    within 15 positions behind row 0 and take it as their predecessor, so that no scan breaks. Held to the oracle alone (spec and reference are quadratic in
    Python). Long rows BEHIND the switch, where the twin (which starts over from row 0) chains them, are in switch/long_row."""
import numpy as np

K = 9
MAXDIFF = 30
SKIP = {'H': 40., 'L': 59., 'S': 30., 'R': 30.}      # -localpenalty defaults (vacmap:257-296); the checks assert that the build's vm_params agree
MAXGAP = {'H': 99, 'L': 50, 'S': 99, 'R': 99}         # what get_localmap_multi_all_forDP_inv_guide_list is called with (:24061)
NOPRE = -9999999
FAR = 10_000_000
RAISED = -10
UNSUPPORTED, ARG = -7, -1
MODES = ('H', 'L', 'S', 'R')
# layout constants the sizes below assume (test_local_dp_edges.py compares them with the sources)
WINDOW, WINDOW_TEST, WAVE_BLOCK, LDS_SHARED, LDS_CAPS, LDS_LARGEST = 16, 3, 64, 512, (512, 768, 1024), 13056
SWITCH_OPS, SWITCH_RATIO = 100000, 1000


def variant_of(mode, ng):
    return 2 if mode == 'R' else (1 if ng > 1 else 0)


def dp_skip(mode, ng, skip):
    """the skip cost the DP is called with: mode L caps LC-mm's at 40 (mammap_ccs.py:28587)"""
    return min(skip, 40.) if (mode == 'L' and ng > 1) else skip


def order(rows, mode):
    """the DP's input order: stable by read end, mode R by read start"""
    a = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    key = a[:, 0] if mode == 'R' else a[:, 0] + a[:, 3]
    return np.argsort(key, kind='stable')


class Set:
    def __init__(self, label, mode, ng, rows, readlen, claims=(), k=K, maxdiff=MAXDIFF, skip=None, record=True, tags=None):
        self.label, self.mode, self.ng, self.k, self.maxdiff, self.record = label, mode, int(ng), int(k), int(maxdiff), record
        self.skip = float(SKIP[mode] if skip is None else skip)
        a = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
        o = order(a, mode)
        self.rows = np.ascontiguousarray(a[o])
        self.readlen = int(readlen)
        self.index = {t: int(np.flatnonzero(o == i)[0]) for t, i in (tags or {}).items()}      # tag -> row index in DP order
        self.claims = list(claims)
        a = self.rows
        assert len(a) == 0 or (a[:, 0].min() >= 0 and (a[:, 0] + a[:, 3]).max() <= self.readlen and set(np.unique(a[:, 2])) <= {-1, 1} and a[:, 3].min() > 0 and a[:, 1].min() >= 0), label
        # (the reference sizes a table by the LAST row's read position + 5000 and indexes it with every row's: keep the recorded sets inside)
        assert len(a) == 0 or not record or a[:, 0].max() < a[-1, 0] + 5000, label

    @property
    def variant(self):
        return variant_of(self.mode, self.ng)

    @property
    def maxgap(self):
        return MAXGAP[self.mode]

    @property
    def dp_skip(self):
        return dp_skip(self.mode, self.ng, self.skip)


def key(c):
    return '%s:%s' % (c.mode, c.label)


# ------------------------------------------------------------------------------------------------ geometry
def run(q0, r0, s, n, l=15, gap=0):
    """n co-linear anchors, read gap = reference gap = `gap`: gap cost 0 and, for gap 0, read-gap cost 0 — scores l, 2 l, ... exactly"""
    st = l + gap
    return [(q0 + t * st, r0 + t * st if s == 1 else r0 - t * st, s, l) for t in range(n)]


def place(aj, s_i, l_i, readgap, refgap):
    """the anchor i behind j for which the gap geometry (:27418-27449) gives exactly (readgap, refgap); readgap < 0: an overlap of -readgap"""
    qj, rj, sj, lj = aj
    if readgap < 0:
        ov = -readgap
        qi = qj + lj - ov
        bonus = qi + l_i - qj - lj
        assert 0 < ov <= lj
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


class Builder:
    """rows of one set as tagged islands: far apart on the reference, behind each other on the read (more than maxgap apart)"""

    def __init__(self, l=15, high=False):
        self.rows, self.tags, self.l, self.q, self.isl, self.claims = [], {}, l, 3, 900 if high else 0, []

    def base(self, s=1):
        self.isl += 1
        return 4 * FAR + self.isl * FAR + (0 if s == 1 else FAR // 2)

    def add(self, rows, tags=None):
        at = len(self.rows)
        self.rows += [tuple(int(v) for v in r) for r in rows]
        for t, i in (tags or {}).items():
            assert t not in self.tags
            self.tags[t] = at + i
        self.q = max(self.q, max(r[0] + r[3] for r in rows))

    def pair(self, tag, s_j, s_i, readgap, refgap, lead=8, tail=2, l_i=None, expect=None, l=None, only=None):
        """an island: `lead` co-linear anchors on strand s_j, anchor i at (readgap, refgap) from the last of them, `tail` co-linear anchors behind i.
        expect: 1 / 2 claims that i's winning step is co-linear / not (and, for 1, that it comes from the lead's last anchor), -1 that i's predecessor is NOT
        the lead's last anchor; only: the variants the claim is made for"""
        l = l or self.l
        pre = run(self.q + 1200, self.base(s_j), s_j, lead, l)
        ai = place(pre[-1], s_i, l_i or l, readgap, refgap)
        from spec_ref import local_gap_geometry
        g = local_gap_geometry(ai, pre[-1])
        assert g[:2] == (max(readgap, 0), refgap), (g, readgap, refgap)
        post = run(ai[0] + ai[3] + 2, ai[1] + ai[3] + 2 if s_i == 1 else ai[1] - l - 2, s_i, tail, l) if tail else []
        self.add(pre + [ai] + post, {tag + '.j': lead - 1, tag + '.i': lead})
        if expect == -1:
            self.claims.append(('notpre', tag + '.i', tag + '.j', only))
        elif expect:
            self.claims.append(('kind', tag + '.i', expect, only))
            if expect == 1:
                self.claims.append(('pre', tag + '.i', tag + '.j', only))
        return ai

    def sets(self, label, modes, variants=(1, 2), mirror=True, pad=7, claims=(), **kw):
        out = []
        a = np.array(self.rows, dtype=np.int64).reshape(-1, 4)
        readlen = int((a[:, 0] + a[:, 3]).max()) + pad
        m = a.copy(); m[:, 0] = readlen - a[:, 0] - a[:, 3]; m[:, 2] = -a[:, 2]
        for mode in modes:
            for ng in ((1,) if mode == 'R' else variants):
                sfx = '' if mode == 'R' else ('/exact' if ng == 1 else '/mm')
                out.append(Set(label + sfx, mode, ng, a, readlen, list(self.claims) + list(claims), tags=self.tags, **kw))
                if mirror:        # the mirrored set is another DP problem (the rows come in the opposite order): it carries the counter claims only
                    out.append(Set(label + sfx + '/mirrored', mode, ng, m, readlen, [c for c in claims if c[0] == 'count_mirrored'], tags=self.tags, **kw))
        return out


# ------------------------------------------------------------------------------------------------ rule boundaries
def colinear_cases():
    out = []
    for maxdiff in (30, 10, 11, 62):
        for s in (1, -1):
            for ov in (0, 4):                                   # plain and overlapping geometry
                b = Builder()
                for d in (-1, 0, 1):
                    for sign in (1, -1):
                        rg = -ov if ov else 40
                        fg = max(rg, 0) + sign * (maxdiff + d)
                        if fg < 0:
                            continue
                        b.pair('md%d%+d%+d' % (maxdiff, d, sign), s, s, rg, fg, expect=1 if d <= 0 else 2, l_i=15 + (6 if ov else 0))
                out += b.sets('colinear/maxdiff%d/%s/%s' % (maxdiff, '+-'[s < 0], 'overlap' if ov else 'plain'), MODES, maxdiff=maxdiff,
                              claims=[('count', 'colinear_wins', 3), ('count', 'noncolinear_wins', 1)] + ([('count', 'overlaps', 1), ('count_mirrored', 'overlaps', 1)] if ov else []))
    for mode in MODES:                                           # readgap at maxgap - 1 / 0 / + 1 (the mode's own maxgap), refgap at -1 / 0
        mg = MAXGAP[mode]
        for s in (1, -1):
            b = Builder()
            for d in (-1, 0, 1):
                # (LC-mm charges 0.5 per base of read gap from 30 on: the skip is the cheaper step there, the claims are for the other two variants)
                b.pair('mg%+d' % d, s, s, mg + d, mg + d, expect=1 if d <= 0 else 2, only=(0, 2))
                b.pair('mg%+d/gap3' % d, s, s, mg + d, mg + d + 3, expect=1 if d <= 0 else 2, only=(0, 2))
            for rg, fg in ((0, -1), (0, 0), (1, -1), (1, 0), (5, -1), (5, 0), (-3, -1), (-3, 0)):
                b.pair('refgap%d/%d' % (rg, fg), s, s, rg, fg, expect=1 if fg >= 0 else -1, l_i=15 if rg >= 0 else 20)     # (refgap -1: the lead's last anchor is out, an earlier one is co-linear)
            out += b.sets('colinear/maxgap_refgap/%s' % '+-'[s < 0], (mode,))
    for s_j in (1, -1):                                          # the eight formulas: four strand pairs, plain and overlapping, near and far
        for s_i in (1, -1):
            b = Builder()
            for rg in (6, -1, -7, -14):
                for fg in (0, 2, MAXDIFF - 1, MAXDIFF, MAXDIFF + 1, 400, 30000):
                    b.pair('f%d/%d' % (rg, fg), s_j, s_i, rg, fg + max(rg, 0) if s_i == s_j else fg, l_i=15 if rg >= 0 else 22,
                           expect=(1 if fg <= MAXDIFF else 2) if s_i == s_j else 2)
            out += b.sets('colinear/strands/%s%s' % ('+-'[s_j < 0], '+-'[s_i < 0]), MODES, claims=[('count', 'overlaps', 10)])
    for s in (1, -1):                                            # gap cost index 10 / 11: 0.5 log2 turns into 2 log2 (H / L / S), stays 0.5 in `_scar`
        b = Builder()
        for g in (9, 10, 11, 12):
            b.pair('g%d' % g, s, s, 20, 20 + g, expect=1); b.pair('g-%d' % g, s, s, 20, 20 - g, expect=1)
        out += b.sets('colinear/gapcost_10_11/%s' % '+-'[s < 0], MODES, claims=[('count', 'gapcost_above10', 4)])
    return out


def overlap_cases():
    out = []
    for s in (1, -1):
        # row 0 and a row inside it that ends where it ends: bonus 0, passed over (taken, the shorter row would score 15 instead of 10)
        b = Builder()
        r0 = (b.q + 20, b.base(s), s, 15)
        tw = place(r0, s, 10, -10, 0)
        b.add([r0, tw] + run(r0[0] + 17, r0[1] + 17 if s == 1 else r0[1] - 17, s, 2), {'row0': 0, 'twin': 1})
        b.claims += [('pre', 'twin', None), ('count', 'bonus_skips', 1)]
        # a chain of consecutive overlaps, each trimmed in the traceback (r moves only on +); one trimmed to length 1
        q0, r0 = b.q + 1200, b.base(s)
        rows = run(q0, r0, s, 3)
        cur = rows[-1]
        for t, (li, ov) in enumerate(((20, 5), (20, 8), (15, 14), (24, 3), (16, 15))):
            cur = place(cur, s, li, -ov, 0)
            rows.append(cur)
        b.add(rows + run(cur[0] + cur[3] + 3, cur[1] + cur[3] + 3 if s == 1 else cur[1] - 18, s, 2), {'last': len(rows) - 1})
        # bonus = +1: the overlapping anchor ends one base behind its predecessor
        x = run(b.q + 1200, b.base(s), s, 4, 30)
        b.add(x + [place(x[-1], s, 16, -15, 0)] + run(x[-1][0] + 40, x[-1][1] + 40 if s == 1 else x[-1][1] - 25, s, 2), {'b1': 4})
        out += b.sets('overlap/chain/%s' % '+-'[s < 0], MODES, claims=[('count', 'trimmed', 5), ('count', 'trimmed_to_1', 1), ('count', 'overlaps', 6), ('kind', 'b1', 1)])
    return out


def scar_cases():
    """mode R only: the refund at fixed_penatly + bonus = -1 / 0 / +1, a debt carried over several co-linear steps, the inherited pair of the LAST update of a
    scan, and rows whose start order differs from their end order (bonus <= 0: passed over, the scan goes on)"""
    out = []
    skip = int(SKIP['R'])
    for s in (1, -1):
        b = Builder()
        for l1 in (15, 8):
            need = skip - l1
            for d in (-1, 0, 1):
                def island(tag, steps):
                    q0 = b.q + 1200
                    x = run(q0, b.base(s), s, 8)
                    cur = (x[-1][0] + 15 + 25, b.base(s), s, l1)             # reached by a skip: owes skip - l1
                    rows = x + [cur]
                    for l_i, rg in steps:
                        cur = place(cur, s, l_i, rg, max(rg, 0))
                        rows.append(cur)
                    n_steps = len(rows)
                    rows += run(cur[0] + cur[3] + 1, cur[1] + cur[3] + 1 if s == 1 else cur[1] - 16, s, 3)
                    b.add(rows, {tag: n_steps - 1})
                island('one%d%+d' % (l1, d), [(need + d, 3)])
                island('two%d%+d' % (l1, d), [(5, 0), (need - 5 + d, 2)])
                island('four%d%+d' % (l1, d), [(2, 0), (2, 1), (1, 0), (need - 5 + d, 2)])
                island('ovl%d%+d' % (l1, d), [(need + d + 4, -4)])
        out += b.sets('scar/refund/%s' % '+-'[s < 0], ('R',), claims=[('count', 'refunds', 12), ('count', 'debts_carried', 12), ('count', 'noncolinear_wins', 12)])
        # the pair comes from the LAST updating candidate: co-linear first (an overlap with a small bonus), then a skip that wins; and a skip first, then a co-linear step
        b = Builder()
        q0 = b.q + 1200
        y = run(q0, b.base(s), s, 4)                               # S = 60 at y[-1]
        c1 = (q0 + 65, b.base(s), s, 60)                           # 60 + 60 - 30 = 90 by a skip; the rows that start inside it do not advance the candidate space
        c2 = place(y[-1], s, 20, 6, 6)                             # starts one base behind c1, co-linear with y[-1]: ~79.7
        i = place(c1, s, 40, -(c1[0] + 60 - c2[0] - 20), 30)       # starts where c2 ends, ends one base behind c1, 30 off c1's diagonal: 90 + 1 - 5.15 co-linearly,
        assert i[0] == c2[0] + 20 and i[0] + 40 == c1[0] + 61       # ~79.7 + 40 - 30 by the skip from c2, which is scanned second and wins
        b.add(y + [c1, c2, i] + run(i[0] + 42, i[1] + 42 if s == 1 else i[1] - 17, s, 3), {'col_then_skip': 6, 'c2': 5})
        b.claims.append(('pre', 'col_then_skip', 'c2'))
        out += b.sets('scar/last_update/col_then_skip/%s' % '+-'[s < 0], ('R',), claims=[('kind', 'col_then_skip', 2), ('count', 'kind_flips', 1)])
        b = Builder()
        x = run(b.q + 1200, b.base(s), s, 6)                       # S = 90: a skip from here gives 90 + 15 - 30 = 75
        y = run(x[0][0] + 2, b.base(s), s, 5)                      # S = 75 at y[-1]; co-linear from here: 75 + 15 - small = ~90
        i = place(y[-1], s, 15, 18, 18)
        b.add(x + y + [i] + run(i[0] + 17, i[1] + 17 if s == 1 else i[1] - 17, s, 3), {'skip_then_col': len(x) + len(y)})
        out += b.sets('scar/last_update/skip_then_col/%s' % '+-'[s < 0], ('R',), claims=[('kind', 'skip_then_col', 1), ('count', 'kind_flips', 1)])
        # a long row that starts first and ends last: the rows inside it do not advance the candidate space, and it is passed over with bonus -1 / 0, taken with + 1
        b = Builder()
        q0, r0 = b.q + 1200, b.base(s)
        lead = run(q0, r0, s, 3)
        long_ = (q0 + 50, b.base(s), s, 100)                       # ends at q0 + 150
        adv = (q0 + 60, b.base(s), s, 120)                         # ends at q0 + 180: advances, `long_` becomes a candidate
        inner = [(q0 + 70 + 3 * t, b.base(s), s, 150 - (70 + 3 * t) + d) for t, d in enumerate((-1, 0, 1))]
        b.add(lead + [long_, adv] + inner + run(q0 + 200, b.base(s), s, 3), {'long': 3, 'in-1': 5, 'in0': 6, 'in+1': 7})
        out += b.sets('scar/start_order/%s' % '+-'[s < 0], ('R',), claims=[('count', 'bonus_skips', 2), ('count', 'held', 3)])
    return out


def tie_cases():
    out = []
    for s in (1, -1):
        # S[j] == max_scores - l_i is still evaluated (strict <); two predecessors of equal test score: the first in scan order — the later row, which sits above
        # its equal in the index — wins
        b = Builder()
        for lead in (3, 5):
            q0 = b.q + 1200
            rx = b.base(s)
            x = run(q0, rx, s, lead)
            y = run(q0, b.base(s), s, lead); w = run(q0, b.base(s), s, lead)
            i = place(x[-1], s, 15, 0, 0)
            b.add(x + y + w + [x[-1], i] + run(i[0] + 20, i[1] + 20 if s == 1 else i[1] - 20, s, 2), {'dup%d' % lead: 3 * lead, 'i%d' % lead: 3 * lead + 1})
            b.claims += [('pre', 'i%d' % lead, 'dup%d' % lead)]
        out += b.sets('ties/break_and_twins/%s' % '+-'[s < 0], MODES, claims=[('count', 'eq_break_evals', 2), ('count', 'tie_tests', 2), ('count', 'breaks', 2)])
    # H higher scores, then a run of E equal ones, then one more equal: it goes above its equals, H entries below the top
    for H in (0, 2, 3, 15, 16, 17):
        for E in (2, 3, 4, 16, 17, 40):
            if (H, E) not in ((0, 2), (0, 40), (2, 3), (3, 4), (15, 16), (16, 17), (17, 2), (16, 40), (2, 17), (3, 16)):
                continue
            b = Builder()
            if H:                                                              # isolated anchors one base longer: above the equals in the index, never a better predecessor
                b.add([(b.q + 2 * t, b.base(1 if t % 4 else -1), 1 if t % 4 else -1, 16) for t in range(H)])
            iso = [(b.q + 5 + 2 * t, b.base(1 if t % 3 else -1), 1 if t % 3 else -1, 15) for t in range(E - 1)]
            b.add(iso)
            dup = (b.q + 3, b.base(1), 1, 15)
            b.add([dup, dup])                                                  # the new equal entry, twice: the follower's predecessor shows their order
            f = place(dup, 1, 15, 0, 0)
            b.add([f, place(f, 1, 15, 2, 2)], {'f': 0})
            b.tags['dup2'] = len(b.rows) - 3
            b.claims.append(('pre', 'f', 'dup2'))
            out += b.sets('ties/equals/H%d_E%d' % (H, E), MODES, claims=[('count', 'insert_among_equals', max(E - 1, 1))] + ([('count', 'below16', 1)] if H >= 16 else []) +
                          ([('count', 'below3', 1)] if H >= 3 else []))
    for n in (2, 3, 4, 15, 16, 17, 18, 40):                       # isolated equal anchors: no scan breaks, every insertion meets equal keys
        b = Builder()
        b.add([(5 + 20 * t, b.base(1 if t % 5 else -1), 1 if t % 5 else -1, 15) for t in range(n)])
        out += b.sets('ties/isolated/%d' % n, MODES, claims=[('count', 'longest_scan', n - 1), ('count', 'insert_among_equals', max(n - 2, 0))])
    return out


def noncolinear_cases(tables):
    """LC-exact's step cost: cross-strand against same-strand steps under local_skipcost 49 / 50 / 51 and the mode defaults, and `extra` at the ends of its stretches"""
    out = []
    for skip in (30., 40., 49., 50., 51., 59.):
        b = Builder()
        for s in (1, -1):
            for g in (300, 5000):
                b.pair('same%d%s' % (g, s), s, s, 20, 20 + g, lead=8, expect=2)
                b.pair('cross%d%s' % (g, s), s, -s, 20, g, lead=8, expect=2)
        out += b.sets('noncolinear/skip%d' % skip, MODES, skip=skip, claims=[('count', 'cross_strand_wins', 4)])
    extra = tables['extra']
    an = 0
    while an < min(20000, len(extra) - 1) and np.float32(min(an * 0.01, 10.0) + an * 0.001) == extra[an]:
        an += 1
    n = len(extra)
    jumps = [MAXDIFF + 1, 99, 100, 101, 999, 1000, 1001, an - 1, an, an + 1, n - 3, n - 2, n - 1, n, n + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 + 5]
    for s in (1, -1):
        for hi in (0, 1):
            b = Builder(high=bool(hi))                              # hi: reference positions from ~9e9 on, above 2^32
            for g in jumps:
                if s == -1 and g > 2 ** 29 and not hi:
                    continue
                b.pair('same%d' % g, s, s, 20, 20 + g, lead=8, expect=2)
                b.pair('cross%d' % g, s, -s, 20, g, lead=8, expect=2)
            out += b.sets('noncolinear/extra/%s/%s' % ('+-'[s < 0], 'r_above_2^32' if hi else 'r_low'), ('H', 'L', 'S'), variants=(1,), claims=[('count', 'extra_saturated', 6)])
    return out


def mm_cases(tables):
    out = []
    n = len(tables['log2cache'])
    for s in (1, -1):
        b = Builder(high=True)
        for g in (n - 2, n - 1, n, n + 1, 2 ** 31 + 3):           # log2cache index at its end
            b.pair('l2c%d' % g, s, s, 20, 20 + g, lead=8, expect=2)
            b.pair('l2cx%d' % g, s, -s, 20, g, lead=8, expect=2)
        for rg in (28, 29, 30, 31):                                # large_readgap: 0.1 log2 turns into 0.5 readgap at 30
            b.pair('lrg%d' % rg, s, s, rg, rg, expect=None)
            b.pair('lrg%d/gap2' % rg, s, s, rg, rg + 2, expect=None)
        out += b.sets('mm/tables/%s' % '+-'[s < 0], ('H', 'L', 'S'), variants=(1, 2), claims=[('count', 'noncolinear_wins', 10)])
    for skip in (39., 40., 41., 59.):                             # mode L's cap of 40 on LC-mm's skip cost
        b = Builder()
        for s in (1, -1):
            b.pair('same%s' % s, s, s, 20, 20 + 700, lead=8, expect=2); b.pair('cross%s' % s, s, -s, 20, 700, lead=8, expect=2)
        out += b.sets('mm/cap40/skip%d' % skip, ('L', 'H'), skip=skip)
    return out


def length_cases():
    """l at the 16-bit edge of the device row: chained co-linearly, trimmed by an overlap (as the earlier and as the later anchor of the pair)"""
    out = []
    for l in (32767, 32768, 65535):
        for s in (1, -1):
            b = Builder()
            q0, r0 = b.q + 20, b.base(s) + (0 if s == 1 else 40 * FAR)
            a0 = run(q0, r0, s, 3)
            big = place(a0[-1], s, l, 2, 2)
            nxt = place(big, s, 15, 3, 3)
            b.add(a0 + [big, nxt] + run(nxt[0] + 17, nxt[1] + 17 if s == 1 else nxt[1] - 17, s, 2), {'big': 3, 'next': 4})
            b.claims += [('pre', 'next', 'big'), ('kind', 'big', 1)]
            q0, r0 = b.q + 1200, b.base(s) + (0 if s == 1 else 40 * FAR)
            a0 = run(q0, r0, s, 3)
            big = place(a0[-1], s, l, -6, 0)                       # the long row is trimmed at its start
            nxt = place(big, s, 30, -9, 0)                         # and overlapped at its end: the next row is trimmed by it
            b.add(a0 + [big, nxt] + run(nxt[0] + 32, nxt[1] + 32 if s == 1 else nxt[1] - 17, s, 2), {'big2': 3, 'next2': 4})
            b.claims += [('pre', 'next2', 'big2')]
            out += b.sets('lengths/l%d/%s' % (l, '+-'[s < 0]), MODES, claims=[('count', 'trimmed', 2)])
    return out


def _group_sizes(target):
    """sizes (c1, c2, c3, c4) of four groups of isolated equal anchors with c2 c1 + c3 (c1 + c2) + c4 (c1 + c2 + c3) == target: row x of group g scans every
    row of the groups before it and nothing breaks (the rows of group 1 behind row 0 scan row 0: c1 - 1 more), so this is opcount when the candidate space advances
    behind group 4; what the first three groups add stays at or below 100 000, so that no earlier advance decides. The smallest total."""
    best = None
    for c1 in range(4, 40):
        for c2 in range(1, 400):
            for c3 in range(1, 400):
                rest = target - (c1 - 1) - c2 * c1 - c3 * (c1 + c2)
                if rest <= 0:
                    break
                if target - rest > SWITCH_OPS:
                    break
                if rest % (c1 + c2 + c3) == 0:
                    c4 = rest // (c1 + c2 + c3)
                    if best is None or c1 + c2 + c3 + c4 < sum(best):
                        best = (c1, c2, c3, c4)
    return best


def switch_cases():
    """the switch to the `_fast` twin: opcount > 100000 and opcount / prereadloc > 1000 where the candidate space advances. A few hundred isolated anchors that end
    within the first 100 read positions; one of them chains co-linearly onto a row of the first group with gap 0, so that every row it scans behind that one has
    S[j] == max_scores - l_i exactly (evaluated, never a break: the count depends on the strict <)."""
    out = []

    def build(label, target, last_end, tail=(), record=True, modes=('H', 'L', 'S'), expect=None, tail_tags=None, claims=(), row0=None):
        sizes = _group_sizes(target)
        rows, tags = [], {}
        isl = [0]

        def base():
            isl[0] += 1
            return 5 * FAR + isl[0] * 20000
        ends = (last_end - 45, last_end - 30, last_end - 15, last_end)
        for g, (c, e) in enumerate(zip(sizes, ends)):
            for t in range(c):
                rows.append((e - 15, base(), 1 if (t + g) % 4 else -1, 15))
        x = rows[sizes[0] - 1]                                      # the last row of group 1 (scanned first among its equals), and the first row of group 2 made its co-linear successor (gap 0)
        rows[sizes[0] - 1] = (x[0], x[1], 1, 15)
        rows[sizes[0]] = (x[0] + 15, x[1] + 15, 1, 15)
        if row0:                                                    # row 0 longer than every score behind it (it ends where group 1 ends: the count stays)
            assert row0 == ends[0]
            rows[0] = (0, base(), 1, row0)
        rows.append((last_end - 15 + 2, base(), 1, 15))            # the row whose larger read end advances the candidate space: the deciding test
        rows += [(last_end + 5 + 3 * t, base(), 1, 15) for t in range(3)]
        rows += run(last_end + 40, base(), 1, 3 if row0 else 4) + run(last_end + 43, base(), -1, 3, 17 if not row0 else 16)       # small buckets of the twin: one entry per integer score
        tags = {t: len(rows) + i for t, i in (tail_tags or {}).items()}
        rows += list(tail)
        a = np.array(rows, dtype=np.int64)
        readlen = int((a[:, 0] + a[:, 3]).max()) + 11
        for mode in modes:
            for ng in (1, 2):
                out.append(Set('%s/%s' % (label, 'exact' if ng == 1 else 'mm'), mode, ng, a, readlen, [('switch_at', target, last_end), ('switch', expect), ('count', 'eq_break_evals', 3)] + list(claims),
                               record=record, tags=tags))
    build('switch/ops100000', 100000, 99, expect=False)
    build('switch/ops100001', 100001, 99, expect=True)
    build('switch/ratio_below', 100999, 101, expect=False, modes=('H',))      # opcount above 100 000, the ratio to prereadloc = 101 just below 1000,
    build('switch/ratio_at', 101000, 101, expect=False, modes=('H',))         # exactly 1000 (not above),
    build('switch/ratio_above', 101001, 101, expect=True, modes=('H',))       # and just above
    # long rows behind the switch: the twin (which starts over from row 0) chains them; their scores stay inside its score table (sized by the last row's q + 50)
    for l in (32767, 32768, 65535):
        q = 70000
        t0 = (q, 900 * FAR, 1, 15)
        big = place(t0, 1, l, 2, 2)
        nxt = place(big, 1, 40, -7, 0)
        far = (big[0] + l + 66000, 950 * FAR, 1, 15)                # the last row: q + 50 above every score
        build('switch/long_row/l%d' % l, 100001, 99, tail=[t0, big, nxt, far], expect=True, modes=('H',))
    # The twins' own rules, on rows behind the switch (the twin starts over from row 0 and chains them). A bucket = the entries of one integer score; more than
    # fast_t = 5 entries are represented by the one whose diagonal key is closest to the row's. K isolated 40-mers make the bucket 40; X among them is the
    # co-linear predecessor of row i, Y lies closer to i's diagonal and is no predecessor worth taking (too far back on the read). K = 5: every entry is tried,
    # X wins. K = 6: Y stands for the bucket, X is never seen. A tie of two keys (Y 3 below, X 3 above i's): the upper one is taken, X wins. int(S): a 40.84
    # counts into bucket 40 (the sixth entry), a 39.84 does not. Claims are made for LC-exact (LC-mm's cheaper skips give the rows other scores); both run.
    def bucket(fill, dx, refgap_x, y=True, frac=None):
        t = [(1000 + 60 * f, 900 * FAR + 3 * f * FAR, 1, 40) for f in range(fill)]
        if frac:                                                    # two co-linear rows, read gap 2: 20 + frac - 0.158...
            t += [(1500, 940 * FAR, 1, 20), (1522, 940 * FAR + 22, 1, frac)]
        X = (2400, 990 * FAR, 1, 40)
        i = place(X, 1, 40, 20, refgap_x)
        diag = i[1] - i[0]
        Y = [(2000, 2000 + diag - dx, 1, 40)] if y else []
        t += Y + [X, i, (i[0] + 300, 995 * FAR, 1, 15)]
        at = len(t) - 3
        return t, {'X': at, 'i': at + 1}
    for name, args, want in (('bucket5', (3, 3, 30), True), ('bucket6', (4, 3, 30), False), ('diagonal_tie', (4, 3, 17), True),
                             ('int_truncation/in', (2, 3, 30, True, 21), False), ('int_truncation/out', (2, 3, 30, True, 20), True), ('int_truncation/none', (3, 3, 30), True)):
        if name == 'int_truncation/none':
            continue
        t, tg = bucket(*args)
        if name.startswith('int_truncation'):                      # (2 fillers + the two-row chain + Y + X: 5 entries of 40, and the fractional one)
            t, tg = bucket(3, 3, 30, True, args[4])
        build('switch/twin/' + name, 100001, 99, tail=t, tail_tags=tg, expect=True, modes=('H',), claims=[('twin_pre' if want else 'twin_notpre', 'i', 'X', (0,))])
    # row 0 outscores everything inserted later: the twin's highest score level never reaches it
    build('switch/twin/row0_highest', 100001, 99, expect=True, modes=('H',), row0=54, claims=[('twin_row0_highest',)])
    # an integer score outside the twin's score table: the reference indexes out of range, the read comes back raised
    build('switch/score_outside_table', 100001, 99, tail=[(300, 900 * FAR, 1, 5000), (320, 950 * FAR, 1, 5010)], expect=True, record=False, modes=('H',))
    return out


# ------------------------------------------------------------------------------------------------ layout sizes and the random part
def realistic(rng, n, style, mode='H'):
    """n rows of one of three styles: 0 sparse co-linear runs with jitter and overlaps, 1 dense repeats (several rows per read position), 2 strand-mixed with gaps at
    maxdiff / maxgap +- 1"""
    rows = []
    q = int(rng.integers(0, 30))
    r = {1: 5 * FAR + int(rng.integers(0, FAR)), -1: 300 * FAR + int(rng.integers(0, FAR))}
    s = 1
    mg = MAXGAP[mode]
    while len(rows) < n:
        l = int(rng.integers(9, 20))
        u = rng.random()
        if u < (0.15 if style == 2 else 0.04):
            s = -s if rng.random() < 0.6 else s
            r[s] += int(rng.integers(-3000, 30000)) * s
        if style == 2 and u > 0.8:
            rg = int(rng.choice([mg - 1, mg, mg + 1, 20, 20, 20])); d = int(rng.choice([-31, -30, -29, -11, -10, 10, 11, 29, 30, 31])) if rg == 20 else 0
        else:
            rg = int(rng.integers(-8, 25)); d = int(rng.integers(-2, 3)) if rng.random() < 0.3 else 0
        q = max(q + l + rg, 0)
        r[s] += (l + max(rg, -l + 1) + d) * s
        rows.append((q, max(r[s], 0), s, l))
        if style == 1 and len(rows) < n:
            for c in range(int(rng.integers(0, 4))):
                if len(rows) < n:
                    rows.append((q + int(rng.integers(0, 3)), 600 * FAR + int(rng.integers(0, 40 * FAR)), int(rng.choice([-1, 1])), int(rng.integers(9, 20))))
    a = np.array(rows[:n], dtype=np.int64).reshape(-1, 4)
    readlen = (int((a[:, 0] + a[:, 3]).max()) if n else 40) + int(rng.integers(0, 50))
    return a, readlen


def layout_sizes(largest=True):
    c = {WINDOW, WINDOW_TEST, 32, WAVE_BLOCK, LDS_SHARED, LDS_CAPS[1]} | ({LDS_LARGEST} if largest else set())
    return sorted({0, 1, 2, 3} | {x + d for x in c for d in (-1, 0, 1)})


def layout_cases(rng, sizes, record_max=1000):
    out = []
    for i, n in enumerate(sizes):
        for mode in ('H', 'R'):
            a, L = realistic(rng, n, i % 3, mode)
            out.append(Set('layout/n%d/style%d' % (n, i % 3), mode, 1 + (i % 2), a, L, record=0 < n <= record_max))
    return out


def random_cases(rng, count, nmax=400):
    out = []
    for mode in MODES:
        for i in range(count):
            n = int(rng.integers(1, 40)) if rng.random() < 0.5 else int(rng.integers(1, nmax + 1))
            a, L = realistic(rng, n, i % 3, mode)
            out.append(Set('random/%d' % i, mode, 1 + int(rng.integers(0, 2)), a, L, maxdiff=int(rng.choice([30, 30, 10, 62])), record=False))
    return out


_constructed = {}


def constructed(tables, largest=True, seed=20262):
    """every rule-boundary family in every mode its rule exists in, the switch and the layout sizes. tables: the cost tables (dict, see spec_ref.local_dp)"""
    if largest in _constructed:
        return _constructed[largest]
    rng = np.random.default_rng(seed)
    out = colinear_cases() + overlap_cases() + scar_cases() + tie_cases() + noncolinear_cases(tables) + mm_cases(tables) + length_cases() + switch_cases()
    out += layout_cases(rng, layout_sizes(largest))
    labels = [key(c) for c in out]
    assert len(set(labels)) == len(labels), [x for x in labels if labels.count(x) > 1][:5]
    _constructed[largest] = out
    return out


FAMILIES = ('colinear', 'overlap', 'scar', 'ties', 'noncolinear', 'mm', 'lengths', 'switch', 'layout')


def oracle_tables(O):
    """the cost tables that tests/golden/tables.json pins by sha256 (test_oracle_golden.py), as the oracle builds them"""
    return {n: O.table(i) for i, n in enumerate(('extra', 'readgap_h', 'readgap_r', 'large_readgap', 'log2cache', 'log2int'))}


# ------------------------------------------------------------------------------------------------ expectations
_spec_cache = {}


SPEC_ROWS = 5000                 # the plain statement is Python: the two largest layout sizes are held to the oracle alone


def expected_spec(c, tables):
    """spec_ref.local_dp on the set (computed once per set and process, never changed); None for a set without rows or of more than SPEC_ROWS rows"""
    k_ = (key(c), c.ng, c.k, c.maxdiff, c.skip, len(c.rows), c.rows.tobytes())        # (labels repeat between the random parts of different tests: the rows are the key)
    if k_ not in _spec_cache:
        import spec_ref
        _spec_cache[k_] = spec_ref.local_dp(c.rows, c.variant, c.mode, c.k, c.dp_skip, c.maxdiff, c.maxgap, tables) if 0 < len(c.rows) <= SPEC_ROWS else None
    return _spec_cache[k_]


def expected_oracle(c, O):
    return O.local_dp(c.rows, c.variant, c.mode, c.k, c.dp_skip, c.maxdiff, c.maxgap) if len(c.rows) else None


def check_claims(c, tables):
    e = expected_spec(c, tables)
    for cl in c.claims:
        if cl[0] in ('kind', 'pre', 'notpre') and len(cl) > 3 and cl[3] is not None and c.variant not in cl[3]:
            continue
        if cl[0].startswith('twin_'):
            continue                                               # (proven with the oracle's twin: check_twin_claims)
        if cl[0] == 'switch':
            assert e['switch'] == cl[1], (key(c), cl, e['switch_at'])
        elif cl[0] == 'switch_at':                                  # the deciding test saw exactly these numbers
            assert (cl[1], cl[2]) in e['tests'], (key(c), cl, e['tests'][-6:])
        elif e['switch']:
            continue
        elif cl[0] == 'kind':
            assert e['kind'][c.index[cl[1]]] == cl[2], (key(c), cl, int(e['kind'][c.index[cl[1]]]))
        elif cl[0] == 'notpre':
            assert e['P'][c.index[cl[1]]] != c.index[cl[2]], (key(c), cl)
        elif cl[0] == 'pre':
            want = NOPRE if cl[2] is None else c.index[cl[2]]
            assert e['P'][c.index[cl[1]]] == want, (key(c), cl, int(e['P'][c.index[cl[1]]]), want)
        elif cl[0] in ('count', 'count_mirrored'):
            assert e['counters'][cl[1]] >= cl[2], (key(c), cl, e['counters'][cl[1]])
        else:
            raise AssertionError('unknown claim %r' % (cl,))


def check_twin_claims(c, O):
    """the claims about a `_fast` twin, which the spec does not restate: proven on the oracle's S / P of the twin"""
    n = 0
    for cl in c.claims:
        if not cl[0].startswith('twin_') or (len(cl) > 3 and c.variant not in cl[3]):
            continue
        o = expected_oracle(c, O)
        assert o['rc'] == 0 and o['fast_used'], (key(c), cl)
        if cl[0] == 'twin_row0_highest':
            assert np.floor(o['S'][1:]).max() < c.rows[0, 3] == o['S'][0] and o['score'] == o['S'][0] and len(o['chain']) == 1, (key(c), cl)
        else:
            got = o['P'][c.index[cl[1]]] == c.index[cl[2]]
            assert got == (cl[0] == 'twin_pre'), (key(c), cl, int(o['P'][c.index[cl[1]]]), c.index[cl[2]])
            b = int(np.floor(o['S'][c.index[cl[2]]]))
            assert b == 40 and int((np.floor(o['S'][:c.index[cl[1]]]) == b).sum()) in (5, 6), (key(c), 'bucket size')
        n += 1
    return n


def a0_cases(lengths=(32768,)):
    """A row of l >= 32 767 as ROW 0 of a set that switches: every other row ends 1 ... 15 behind it (15 groups of m rows, each group one read end) and takes
    row 0 as its predecessor by a skip, so all scores lie within 15 of each other and no scan breaks: a row of group g scans row 0 and the (g - 1) m rows of the
    groups before it, and at the advance into group 15 opcount = 14 m + 91 m^2 > 1000 (l + 14). Oracle only (the plain spec and the reference's Python are quadratic)."""
    out = []
    for l in lengths:
        m = 620 if l <= 32768 else 850
        assert 14 * m + 91 * m * m > SWITCH_RATIO * (l + 14)
        rows = [(0, 5 * FAR, 1, l)]
        for g in range(1, 16):
            rows += [(l + g - 15, 20 * FAR + (g * m + t) * 20000, 1 if t % 4 else -1, 15) for t in range(m)]
        for ng in (1, 2):
            out.append(Set('switch/row0_l%d/%s' % (l, 'exact' if ng == 1 else 'mm'), 'H', ng, rows, l + 15 + 9, [('twin_a0',)], record=False))
    return out


_fixture = None


def fixture():
    global _fixture
    if _fixture is None:
        import json, os
        g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
        _fixture = (json.load(open(os.path.join(g, 'local_dp_edges.json'))), dict(np.load(os.path.join(g, 'local_dp_edges.npz'))))
    return _fixture


def expected_recorded(c):
    """the reference's (score, chain, raised) on a recorded set; the stored input must be the generator's"""
    meta, arr = fixture()
    r = meta[key(c)]
    n = r['n']
    assert (r['readlen'], r['maxdiff'], r['skip'], r['ng'], n) == (c.readlen, c.maxdiff, c.skip, c.ng, len(c.rows)), key(c)
    if 'a_off' in r:
        assert np.array_equal(arr['a'][r['a_off']:r['a_off'] + n], c.rows), key(c)
    else:
        import zlib
        assert r['crc'] == zlib.crc32(np.ascontiguousarray(c.rows).tobytes()), key(c)
    return {'score': np.float64(r['score']), 'chain': arr['chain'][r['c_off']:r['c_off'] + r['c_n']]}


def same_chain(got, exp, what):
    got, exp = np.asarray(got, dtype=np.int64).reshape(-1, 4), np.asarray(exp, dtype=np.int64).reshape(-1, 4)
    assert got.shape == exp.shape and np.array_equal(got, exp), (what, 'chain', got.shape, exp.shape, got[:3].tolist(), exp[:3].tolist())


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def same(c, g, spec, orc, what, rec=None):
    """one read of vm_local_dp_batch against spec, live oracle and (rec) the recorded reference: no tolerance anywhere"""
    what = (what, key(c))
    if len(c.rows) == 0:
        assert g['status'] == 0 and len(g['chain']) == 0 and g['score'] == 0. and g['variant'] == c.variant and not g['fast_used'], (what, g)
        return
    assert g['variant'] == c.variant, (what, 'variant', g['variant'], c.variant)
    assert g['fast_used'] == orc['fast_used'] and (spec is None or orc['fast_used'] == spec['switch']), (what, 'twin used', g['fast_used'], orc['fast_used'], spec and spec['switch'])
    if orc['rc'] != 0:
        assert g['status'] == RAISED and len(g['chain']) == 0, (what, 'a raised read', g['status'])
        return
    assert g['status'] == 0, (what, 'status', g['status'])
    assert bits(g['score']) == bits(orc['score']), (what, 'score vs the oracle', g['score'], orc['score'])
    same_chain(g['chain'], orc['chain'], (what, 'vs the oracle'))
    if spec is not None and not spec['switch']:
        assert bits(g['score']) == bits(spec['score']), (what, 'score vs the spec', g['score'], spec['score'])
        same_chain(g['chain'], spec['chain'], (what, 'vs the spec'))
    if rec is not None:
        assert bits(g['score']) == bits(rec['score']), (what, 'score vs the reference', g['score'], rec['score'])
        same_chain(g['chain'], rec['chain'], (what, 'vs the reference'))
    if g['P'] is not None:
        bad = np.flatnonzero(g['P'] != orc['P'])
        assert len(bad) == 0, (what, 'P', int(bad[0]), int(g['P'][bad[0]]), int(orc['P'][bad[0]]))
    if g['S'] is not None:
        bad = np.flatnonzero(bits(g['S']) != bits(orc['S']))
        assert len(bad) == 0, (what, 'S', int(bad[0]), float(g['S'][bad[0]]), float(orc['S'][bad[0]]))


def batches(cases):
    """sets of one (mode, k, maxdiff, skip) together — LC-exact and LC-mm reads mixed — in batches of 1, 2, ... 9, 1, ... reads"""
    groups = {}
    for c in cases:
        groups.setdefault((c.mode, c.k, c.maxdiff, c.skip), []).append(c)
    size = 0
    for g, cs in sorted(groups.items()):
        i = 0
        while i < len(cs):
            size = size % 9 + 1
            yield g, cs[i:i + size]
            i += size


def run_cases(ctx, cases, device_list=False):
    from vacmap_amd.lib import local_dp_batch
    out = []
    for (mode, k, maxdiff, skip), cs in batches(cases):
        prm = ctx.lib.params(mode, local_kmersize=k, local_maxdiff=maxdiff)
        assert prm.local_skipcost == SKIP[mode]
        prm.local_skipcost = skip
        res = local_dp_batch(ctx, prm, [c.rows for c in cs], [c.ng for c in cs], [c.readlen for c in cs], want_sp=True, device_list=device_list)
        out += list(zip(cs, res))
    return out


def check(ctx, O, tables, cases, tag='', device_list=False, need_s=None, use_spec=True):
    """every read against spec and oracle, and against the fixture where recorded. need_s: True / False asserts that S came back (or did not) for the chained reads"""
    for c, g in run_cases(ctx, cases, device_list):
        rec = expected_recorded(c) if c.record else None
        same(c, g, expected_spec(c, tables) if use_spec else None, expected_oracle(c, O), (tag, 'device list' if device_list else 'host list'), rec)
        if need_s is not None and len(c.rows) and g['status'] == 0 and not g['fast_used']:
            assert (g['S'] is not None) == need_s(c) and g['P'] is not None, (tag, key(c), 'S / P defined', g['S'] is not None)
    return len(cases)


def check_long_beside_short(ctx, O, tables, seed=78, device_list=False):
    """one long read beside three short ones in one wave of the row kernels, the long one in each of the four rows; the variants mixed"""
    rng = np.random.default_rng(seed)
    n = 0
    for mode in ('H', 'R'):
        for pos in range(4):
            cs = [Set('short%d/%d' % (pos, i), mode, 1 + (i + pos) % 2, *realistic(rng, 3 + i, i % 3, mode), record=False) for i in range(3)]
            cs.insert(pos, Set('long%d' % pos, mode, 1 + pos % 2, *realistic(rng, 900, pos % 3, mode), record=False))
            n += check(ctx, O, tables, cs, 'long beside short', device_list)
    return n


def check_refusals(ctx, O, tables):
    """rows the device's fields cannot carry are refused as a whole (VM_ERR_UNSUPPORTED), rows out of order and the other mistakes of a caller are VM_ERR_ARG;
    the largest accepted length chains like any other, and the entry works after a refusal"""
    from vacmap_amd.lib import VmxError, local_dp_batch
    prm = ctx.lib.params('H')
    ok = np.array(run(3, 5 * FAR, 1, 6), dtype=np.int64)
    head = [(3, 50, 1, 15), (30, 80, 1, 15)]

    def call(rows, ng=1, readlen=None, prm_=prm):
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
        L = readlen if readlen is not None else max(int((rows[:, 0] + rows[:, 3]).max()), 200)
        return local_dp_batch(ctx, prm_, [ok, rows], [1, ng], [200, L], want_sp=True)
    big = Set('l65535', 'H', 1, run(3, 5 * FAR, 1, 5, 65535), 3 + 5 * 65535, record=False)
    same(big, call(big.rows)[1], expected_spec(big, tables), expected_oracle(big, O), 'largest accepted length')
    bad = {'l = 65536': (head + [(60, 110, 1, 65536)], UNSUPPORTED), 'l = -1': (head + [(60, 110, 1, -1)], UNSUPPORTED),
           'q + l = 2^31': (head + [(2 ** 31 - 15, 2 ** 31, 1, 15)], UNSUPPORTED), 'q = 2^32 + 60': (head + [(2 ** 32 + 60, 2 ** 33, 1, 15)], UNSUPPORTED),
           'q = -2^31 - 1': ([(-2 ** 31 - 1, 20, 1, 15)] + head, UNSUPPORTED), 's = 0': (head + [(60, 110, 0, 15)], UNSUPPORTED), 's = 2': (head + [(60, 110, 2, 15)], UNSUPPORTED),
           's = 65537': (head + [(60, 110, 65537, 15)], UNSUPPORTED), 'out of order': ([head[1], head[0]], ARG), 'q = -1': ([(-1, 20, 1, 15)] + head, ARG)}
    for what, (b, code) in bad.items():
        try:
            call(b)
        except VmxError as e:
            assert e.code == code and ('anchor row' in str(e)) == (code == UNSUPPORTED), (what, e.code, str(e))
        else:
            raise AssertionError('%s was accepted' % what)
    for what, kw in (('row behind its read', dict(rows=head, readlen=44)), ('no guide', dict(rows=head, ng=0))):
        try:
            call(**kw)
        except VmxError as e:
            assert e.code == ARG, (what, e.code, str(e))
        else:
            raise AssertionError('%s was accepted' % what)
    # mode R takes its rows by read start: a set in order of read end only is refused there, and the other way round
    byend = [(10, 50, 1, 40), (20, 90, 1, 15)]                     # starts 10 < 20, ends 50 > 35
    call(byend, prm_=ctx.lib.params('R'))
    try:
        call(byend)
    except VmxError as e:
        assert e.code == ARG and 'order' in str(e), (e.code, str(e))
    else:
        raise AssertionError('rows out of the order of read ends were accepted')
    after = Set('after', 'H', 2, ok, 200, record=False)
    same(after, call(ok, ng=2)[1], expected_spec(after, tables), expected_oracle(after, O), 'after a refusal')


if __name__ == '__main__':
    # a fresh process for the switches that the library reads once: `local_dp_cases.py emu|gpu` under VMX_CHAIN_ROWS=0 (one wavefront per read), with
    # VMX_LC_LDS_MAX as the caller sets it (0: nothing LDS-resident; 13056: every LDS bucket in use)
    import os, sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import oracle_lib
    if sys.argv[1] == 'emu':
        import emu_lib
        cx = emu_lib.context()
    else:
        from vacmap_amd.lib import Context
        cx = Context(0)
    assert os.environ.get('VMX_CHAIN_ROWS') == '0'
    lds = int(os.environ.get('VMX_LC_LDS_MAX', LDS_SHARED))
    T_ = oracle_tables(oracle_lib)
    all_ = constructed(T_, largest=lds >= LDS_LARGEST)
    caps = [x for x in (512, 768, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 13056) if x <= lds]
    # (fixture and live oracle here; the parent's tests hold the oracle to the spec on the same sets)
    n_ = check(cx, oracle_lib, T_, all_, 'one wavefront per read, VMX_LC_LDS_MAX=%d' % lds, need_s=lambda c: not (caps and len(c.rows) <= caps[-1]), use_spec=False)
    n_ += check(cx, oracle_lib, T_, random_cases(np.random.default_rng(4400), 25), 'one wavefront per read, random', use_spec=False)
    print('local dp edges ok: %d reads, VMX_CHAIN_ROWS=0, VMX_LC_LDS_MAX=%d' % (n_, lds))
