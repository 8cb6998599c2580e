"""TEST-ONLY: plain NumPy references of the primitive specs, written from the spec text (DESIGN.md §2 and the header comments of
oracle/vmo_dp.cc and oracle/vmo_seed.cc), not from any implementation of them. Neither the oracle nor the product is imported here:
these functions judge both. Scores and hashes are int64 / uint64; every DP is the full (or whole banded) matrix, one row at a time.

  levenshtein   VMX-ED     unit-cost edit distance over the 5-letter code alphabet (A C G T, every other byte one code; case ignored)
  dpg_score     VMX-DP-G   optimal global dual-affine score; cigar_score rescores a CIGAR under the same scoring
  dpx           VMX-DP-X   banded anti-diagonal x-drop extension: (score, t_e, q_e)
  sketch        VMX-S1     (w, k) window minimizers with minimap2's published hash64, all ties kept
  map_read      VMX-S1     index lookup under the occurrence cap, hits sorted by (r, q, s), clusters cut at reference gaps > 5000, ranked by
                           (size desc, first r asc), the first check_num emitted; default_mid_occ is the index's own cap
  ksw2_order_cigar         VMX-DP-G with ksw2's published tie order, cell by cell (small problems only)
  local_guides / local_seed / local_raw    L1 / L2: the guide chains and the re-seeded local anchors, from the reference's text
  local_dp                 L3 / L4 / `_scar`: the local chain DPs on rows in their input order, from the reference's text, with branch counters; the cost
                           tables are handed in (the ones tests/golden/tables.json pins)
"""
import re
import numpy as np

NEG = -(1 << 50)                 # minus infinity of the DPs: far below any reachable score, far above int64 overflow

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate('ACGT'):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def codes(s):
    """A C G T (either case) -> 0 1 2 3, any other byte -> 4"""
    b = s.encode() if isinstance(s, str) else bytes(s)
    return _CODE[np.frombuffer(b, np.uint8)] if b else np.zeros(0, np.uint8)


# ------------------------------------------------------------------------------------------------ VMX-ED
def levenshtein(a, b):
    """D(i, j) = min(D(i-1, j) + 1, D(i, j-1) + 1, D(i-1, j-1) + [a_i != b_j]) over codes. The row's left-to-right dependency is a
    prefix minimum: D(i, j) = min_{l <= j} (T(l) + j - l) with T(0) = i and T(l) = min(D(i-1, l) + 1, D(i-1, l-1) + [a_i != b_l])."""
    x, y = codes(a).astype(np.int64), codes(b).astype(np.int64)
    n = len(y)
    J = np.arange(n + 1, dtype=np.int64)
    prev = J.copy()
    for i in range(1, len(x) + 1):
        t = np.empty(n + 1, np.int64)
        t[0] = i
        t[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (y != x[i - 1]))
        prev = np.minimum.accumulate(t - J) + J
    return int(prev[n])


# ------------------------------------------------------------------------------------------------ VMX-DP-G
def _subst(x_i, y, match, mismatch):
    """s(a, b) = match if a == b and a is A/C/G/T, else mismatch (an N never matches, not even an N)"""
    return np.where((y == x_i) & (x_i < 4), match, mismatch).astype(np.int64)


def _row_gap(H, o, e):
    """F(j) = max(H(j-1) - o, F(j-1)) - e along a row, F(0) = -inf: max_{l < j} (H(l) - o - (j - l) e)"""
    J = np.arange(len(H), dtype=np.int64)
    F = np.full(len(H), NEG, np.int64)
    if len(H) > 1:
        F[1:] = np.maximum.accumulate((H + J * e)[:-1]) - o - J[1:] * e
    return np.maximum(F, NEG)


def _close_row(Hv, pieces):
    """H = max(Hv, F_k) where F_k opens from H itself (an insertion run may follow one of the other piece): iterate to the fixed point"""
    H = Hv
    while True:
        Hn = Hv
        for o, e in pieces:
            Hn = np.maximum(Hn, _row_gap(H, o, e))
        if np.array_equal(Hn, H):
            return H
        H = Hn


def dpg_score(t, q, match=2, mismatch=-4, o1=4, e1=2, o2=24, e2=1):
    """VMX-DP-G: max over all global alignments of t (rows, consumed by D) and q (columns, consumed by I) of
    sum s(a, b) - sum over gap runs of the better piece min_k (o_k + L e_k) (E_k / F_k recurrences, H(0,0) = 0)"""
    x, y = codes(t), codes(q)
    pieces = ((o1, e1), (o2, e2))
    Hv = np.full(len(y) + 1, NEG, np.int64)
    Hv[0] = 0
    H = _close_row(Hv, pieces)
    E = [np.full(len(y) + 1, NEG, np.int64) for _ in pieces]
    for i in range(1, len(x) + 1):
        E = [np.maximum(np.maximum(H - o, Ek) - e, NEG) for (o, e), Ek in zip(pieces, E)]
        Hv = np.maximum(E[0], E[1])
        Hv[1:] = np.maximum(Hv[1:], H[:-1] + _subst(x[i - 1], y, match, mismatch))
        H = _close_row(Hv, pieces)
    return int(H[len(y)])


def parse_cigar(cigar):
    ops = re.findall(r'(\d+)([MIDX=])', cigar)
    assert ''.join(n + o for n, o in ops) == cigar, 'malformed CIGAR %r' % cigar
    return [(int(n), o) for n, o in ops]


def cigar_score(cigar, t, q, match=2, mismatch=-4, o1=4, e1=2, o2=24, e2=1):
    """score of the alignment a CIGAR spells, under VMX-DP-G's scoring. It must consume t (M = X D) and q (M = X I) exactly, '=' must
    be a match and 'X' a mismatch; each gap run of L bases costs min(o1 + e1 L, o2 + e2 L). Raises AssertionError otherwise."""
    x, y = codes(t), codes(q)
    i = j = 0
    sc = 0
    for L, op in parse_cigar(cigar):
        assert L > 0, cigar
        if op in 'M=X':
            assert i + L <= len(x) and j + L <= len(y), 'CIGAR runs past a side: %s' % cigar
            eq = (x[i:i + L] == y[j:j + L]) & (x[i:i + L] < 4)
            assert op != '=' or eq.all(), "'=' over a mismatch at t %d" % i
            assert op != 'X' or not eq.any(), "'X' over a match at t %d" % i
            sc += int(eq.sum()) * match + int(L - eq.sum()) * mismatch
            i += L; j += L
        else:
            if op == 'D':
                i += L
            else:
                j += L
            sc -= min(o1 + e1 * L, o2 + e2 * L)
    assert i == len(x) and j == len(y), 'CIGAR consumes (%d, %d) of (%d, %d)' % (i, j, len(x), len(y))
    return sc


def ksw2_order_cigar(t, q, match=2, mis=-4, o1=4, e1=2, o2=24, e2=1):
    """independent pure-Python restatement of VMX-DP-G with the PUBLISHED ksw2 (ksw_extd2, left-aligned) priorities: the source of H is
    the first of diagonal > E1 (deletion, short piece) > F1 (insertion, short piece) > E2 > F2 that is strictly larger than the ones
    before it; a gap state continues iff its extension is strictly better than a new opening. Small inputs only."""
    NEG = -10 ** 9
    tl, ql = len(t), len(q)
    mk = lambda: [[NEG] * (ql + 1) for _ in range(tl + 1)]
    H, E1, E2, F1, F2 = mk(), mk(), mk(), mk(), mk()
    src, x1, x2, y1, y2 = mk(), mk(), mk(), mk(), mk()
    H[0][0] = 0
    for i in range(tl + 1):
        for j in range(ql + 1):
            if i == 0 and j == 0:
                continue
            if i > 0:
                a1, a2 = H[i - 1][j] - o1, H[i - 1][j] - o2
                x1[i][j] = E1[i - 1][j] > a1; x2[i][j] = E2[i - 1][j] > a2
                E1[i][j] = max(a1, E1[i - 1][j]) - e1; E2[i][j] = max(a2, E2[i - 1][j]) - e2
            if j > 0:
                c1, c2 = H[i][j - 1] - o1, H[i][j - 1] - o2
                y1[i][j] = F1[i][j - 1] > c1; y2[i][j] = F2[i][j - 1] > c2
                F1[i][j] = max(c1, F1[i][j - 1]) - e1; F2[i][j] = max(c2, F2[i][j - 1]) - e2
            d = NEG
            if i > 0 and j > 0:
                d = H[i - 1][j - 1] + (match if (t[i - 1] == q[j - 1] and t[i - 1] in 'ACGT') else mis)
            h, sr = d, 0
            for kk, v in ((1, E1[i][j]), (3, F1[i][j]), (2, E2[i][j]), (4, F2[i][j])):       # state codes: 1 E1, 2 E2, 3 F1, 4 F2
                if v > h:
                    h, sr = v, kk
            H[i][j] = h; src[i][j] = sr
    ops = []; i, j, st = tl, ql, 0
    while i > 0 or j > 0:
        if st == 0:
            sr = src[i][j]
            if sr == 0:
                ops.append('M'); i -= 1; j -= 1
            else:
                st = sr
        elif st in (1, 2):
            ext = x1[i][j] if st == 1 else x2[i][j]
            ops.append('D'); i -= 1
            if not ext:
                st = 0
        else:
            ext = y1[i][j] if st == 3 else y2[i][j]
            ops.append('I'); j -= 1
            if not ext:
                st = 0
    ops.reverse()
    out = []; a = 0
    while a < len(ops):
        b = a
        while b < len(ops) and ops[b] == ops[a]:
            b += 1
        out.append('%d%s' % (b - a, ops[a])); a = b
    return ''.join(out), H[tl][ql]


# ------------------------------------------------------------------------------------------------ VMX-DP-X
def dpx(t, q, match=2, mismatch=-4, o=4, e=4, bw=100, zdrop=50):
    """VMX-DP-X on the whole banded matrix: single affine (o, e), cells with |i - j| <= bw (bw < 0: every cell), anchored at H(0,0) = 0,
    cells outside the band are -inf. Then the diagonals d = i + j = 1, 2, ... in order: a cell replaces the best M (start: 0 at (0,0)) iff
    its H > M strictly, cells of a diagonal by ascending i; after diagonal d stop if max(m_d, m_{d-1}) < M - zdrop, m_d the max H on d
    (-inf for a diagonal without in-band cells, m_0 = 0). Returns (M, t_e, q_e)."""
    x, y = codes(t), codes(q)
    tl, ql = len(x), len(y)
    if bw < 0:
        bw = max(tl, ql)
    J = np.arange(ql + 1, dtype=np.int64)
    mdiag = np.full(tl + ql + 1, NEG, np.int64)          # per diagonal: max H and the smallest i that reaches it
    adiag = np.zeros(tl + ql + 1, np.int64)

    def finish_row(i, Hv):
        band = np.abs(J - i) <= bw
        H = np.where(band, _close_row(np.where(band, Hv, NEG), ((o, e),)), NEG)
        upd = band & (H > mdiag[i + J])                  # rows by ascending i: strict '>' keeps the smallest i of a diagonal's max
        mdiag[(i + J)[upd]] = H[upd]; adiag[(i + J)[upd]] = i
        return H

    Hv = np.full(ql + 1, NEG, np.int64)
    Hv[0] = 0
    H = finish_row(0, Hv)
    E = np.full(ql + 1, NEG, np.int64)
    for i in range(1, tl + 1):
        E = np.where(np.abs(J - i) <= bw, np.maximum(np.maximum(H - o, E) - e, NEG), NEG)
        Hv = E.copy()
        Hv[1:] = np.maximum(Hv[1:], H[:-1] + _subst(x[i - 1], y, match, mismatch))
        H = finish_row(i, Hv)
    M, bi, bj, m_prev = 0, 0, 0, 0
    for d in range(1, tl + ql + 1):
        m_d = int(mdiag[d])
        if m_d > M:
            M, bi = m_d, int(adiag[d]); bj = d - bi
        if max(m_d, m_prev) < M - zdrop:
            break
        m_prev = m_d
    return M, bi, bj


# ------------------------------------------------------------------------------------------------ VMX-S1
def hash64(key, mask):
    """minimap2's published hash64 (Thomas Wang's invertible integer mix), every step modulo 2^(2k)"""
    key = np.asarray(key, dtype=np.uint64)
    mask = np.uint64(mask)
    with np.errstate(over='ignore'):
        key = (~key + (key << np.uint64(21))) & mask
        key = key ^ (key >> np.uint64(24))
        key = ((key + (key << np.uint64(3))) + (key << np.uint64(8))) & mask
        key = key ^ (key >> np.uint64(14))
        key = ((key + (key << np.uint64(2))) + (key << np.uint64(4))) & mask
        key = key ^ (key >> np.uint64(28))
        key = (key + (key << np.uint64(31))) & mask
    return key


INF64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def kmer_hashes(seq, k):
    """per k-mer start p in [0, L - k]: (hash of the canonical k-mer, strand = rc < fwd); hash INF64 for a k-mer that holds a non-ACGT
    base or equals its own reverse complement"""
    c = codes(seq)
    P = len(c) - k + 1
    if P <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int8)
    mask = (1 << (2 * k)) - 1
    fwd = np.zeros(P, np.uint64); rc = np.zeros(P, np.uint64)
    c64 = (c & 3).astype(np.uint64)
    for a in range(k):
        fwd = (fwd << np.uint64(2)) | c64[a:a + P]
        rc = rc | ((np.uint64(3) - c64[a:a + P]) << np.uint64(2 * a))
    amb = np.concatenate([[0], np.cumsum(c > 3)])
    valid = (amb[k:k + P] - amb[:P] == 0) & (fwd != rc)
    h = np.where(valid, hash64(np.minimum(fwd, rc), mask), INF64)
    z = np.where(valid & (rc < fwd), 1, 0).astype(np.int8)
    return h, z


def sketch(seq, k, w):
    """VMX-S1: the k-mer start p is a minimizer iff it is valid and some window of w consecutive k-mer starts inside [0, L - k] that
    contains p (one short window of all starts when there are fewer than w) has its minimum hash equal to p's (ties: all kept).
    Returns (hash uint64, pos int32, strand int8) by ascending pos."""
    h, z = kmer_hashes(seq, k)
    P = len(h)
    if P == 0:
        return h, np.zeros(0, np.int32), z
    wl = min(w, P)
    wmin = np.lib.stride_tricks.sliding_window_view(h, wl).min(axis=1)
    # every window holding p has a minimum <= h[p]; p is selected iff the largest of those minima equals h[p]
    pad = np.concatenate([np.zeros(wl - 1, np.uint64), wmin, np.zeros(P - len(wmin), np.uint64)])
    best = np.lib.stride_tricks.sliding_window_view(pad, wl).max(axis=1)
    sel = (h != INF64) & (best == h)
    pos = np.nonzero(sel)[0]
    return h[pos], pos.astype(np.int32), z[pos]


def sketch_brute(seq, k, w):
    """sketch() by enumerating every window (tiny inputs)"""
    h, z = kmer_hashes(seq, k)
    P = len(h)
    wins = [range(a, a + w) for a in range(P - w + 1)] if P >= w else ([range(P)] if P else [])
    keep = set()
    for win in wins:
        m = min(int(h[p]) for p in win)
        keep.update(p for p in win if int(h[p]) == m and h[p] != INF64)
    pos = sorted(keep)
    return h[pos].astype(np.uint64), np.array(pos, np.int32), z[pos].astype(np.int8)


def index_minimizers(seqs, k, w):
    """the index of VMX-S1: every contig's sketch (windows never cross contigs) as (hash, gpos << 1 | strand) pairs, gpos = the contig's
    start in the concatenation of all contigs + p, in ascending (hash, position) order"""
    hs, ps = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)]
    off = 0
    for s in seqs:
        h, p, z = sketch(s, k, w)
        hs.append(h); ps.append(((p.astype(np.uint64) + np.uint64(off)) << np.uint64(1)) | z.astype(np.uint64))
        off += len(s)
    H, Pp = np.concatenate(hs), np.concatenate(ps)
    o = np.lexsort((Pp, H))
    return H[o], Pp[o]


# ------------------------------------------------------------------------------------------------ VMX-S1 map()
CLUSTER_GAP = 5000               # a new cluster starts where r exceeds the previous r by MORE than this
MID_OCC_FLOOR = 10
MID_OCC_TAIL = 2e-4              # the cap sits one above the count at the (1 - 2e-4) quantile of the distinct hashes


def default_mid_occ(index_hashes):
    """the index's own occurrence cap: max(10, counts_sorted[min(floor((1 - 2e-4) nd), nd - 1)] + 1) over the nd distinct hashes"""
    _, counts = np.unique(np.asarray(index_hashes, dtype=np.uint64), return_counts=True)
    nd = len(counts)
    if nd == 0:
        return MID_OCC_FLOOR
    counts = np.sort(counts)
    kth = min(int(np.floor((1.0 - MID_OCC_TAIL) * nd)), nd - 1)
    return max(MID_OCC_FLOOR, int(counts[kth]) + 1)


def lookup_hits(index_hashes, index_positions, k, w, read, mid_occ):
    """every hit of the read, unordered: a read minimizer (hash h, position q, strand z) whose hash occurs c times in the index yields the c
    rows (q, r, s, k), r = the occurrence's global position and s = +1 if its strand equals z, else -1 — if 1 <= c <= mid_occ, none
    otherwise. mid_occ <= 0 stands for the index's default. index_hashes / index_positions as index_minimizers returns them."""
    IH = np.asarray(index_hashes, dtype=np.uint64); IP = np.asarray(index_positions, dtype=np.uint64)
    if mid_occ <= 0:
        mid_occ = default_mid_occ(IH)
    h, p, z = sketch(read, k, w)
    lo = np.searchsorted(IH, h, 'left'); c = np.searchsorted(IH, h, 'right') - lo
    ok = (c >= 1) & (c <= mid_occ)
    lo, c, q, z = lo[ok].astype(np.int64), c[ok].astype(np.int64), p[ok].astype(np.int64), z[ok].astype(np.int64)
    n = int(c.sum())
    owner = np.repeat(np.arange(len(c)), c)                                  # hit -> its read minimizer
    j = np.arange(n, dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)        # ... and the how-manieth occurrence
    pv = IP[lo[owner] + j]
    out = np.empty((n, 4), np.int64)
    out[:, 0] = q[owner]; out[:, 1] = (pv >> np.uint64(1)).astype(np.int64)
    out[:, 2] = np.where((pv & np.uint64(1)).astype(np.int64) == z[owner], 1, -1); out[:, 3] = k
    return out


def cluster_hits(hits, check_num):
    """(n, 4) rows (q, r, s, l) in any order -> the rows map() returns: sorted by (r, q, s); a new cluster starts where r exceeds the previous
    r by more than 5000; clusters ranked by (size descending, first r ascending); the first check_num kept (all if check_num <= 0), emitted
    one after another in rank order, hits in sorted order"""
    hits = np.asarray(hits, dtype=np.int64).reshape(-1, 4)
    n = len(hits)
    if n == 0:
        return hits.copy()
    hits = hits[np.lexsort((hits[:, 2], hits[:, 0], hits[:, 1]))]
    r = hits[:, 1]
    first = np.concatenate([[True], np.diff(r) > CLUSTER_GAP])
    start = np.nonzero(first)[0]
    size = np.diff(np.concatenate([start, [n]]))
    rank = np.lexsort((r[start], -size))
    if check_num > 0:
        rank = rank[:check_num]
    sz = size[rank]
    take = np.repeat(start[rank], sz) + (np.arange(int(sz.sum())) - np.repeat(np.cumsum(sz) - sz, sz))
    return hits[take]


def map_read(index_hashes, index_positions, k, w, read, check_num, mid_occ):
    """VMX-S1 map(): lookup_hits, then cluster_hits"""
    return cluster_hits(lookup_hits(index_hashes, index_positions, k, w, read, mid_occ), check_num)


def cluster_hits_brute(hits, check_num):
    """cluster_hits() with Python lists, one rule per line (tiny inputs)"""
    hs = sorted((int(r), int(q), int(s), int(l)) for q, r, s, l in hits)
    clusters = []
    for h in hs:
        if clusters and h[0] - clusters[-1][-1][0] <= CLUSTER_GAP:
            clusters[-1].append(h)
        else:
            clusters.append([h])
    clusters.sort(key=lambda c: (-len(c), c[0][0]))
    if check_num > 0:
        clusters = clusters[:check_num]
    return np.array([(q, r, s, l) for c in clusters for r, q, s, l in c], dtype=np.int64).reshape(-1, 4)


def map_read_brute(index_hashes, index_positions, k, w, read, check_num, mid_occ):
    """map_read() with a dictionary and loops (tiny inputs)"""
    occ = {}
    for h, pv in zip(index_hashes.tolist(), index_positions.tolist()):
        occ.setdefault(h, []).append(pv)
    if mid_occ <= 0:
        cs = sorted(len(v) for v in occ.values())
        mid_occ = max(10, cs[min(int((1 - 2e-4) * len(cs)), len(cs) - 1)] + 1) if cs else 10
    hits = []
    for h, q, z in zip(*(a.tolist() for a in sketch_brute(read, k, w))):
        pvs = occ.get(h, [])
        if 1 <= len(pvs) <= mid_occ:
            hits += [(q, pv >> 1, 1 if (pv & 1) == z else -1, k) for pv in pvs]
    return cluster_hits_brute(hits, check_num)


# ------------------------------------------------------------------------------------------------ L1 / L2: local re-seeding
LOCAL_SPANS = {'H': (7000, 7000), 'L': (7000, 7000), 'S': (7000, 7000), 'R': (2000, 500), 'asm': (2000, 500)}   # (look span, read span)
LOCAL_BUDGET = {'H': 5, 'L': 3, 'S': None}                                   # guide chains re-seeded per read

_RC = str.maketrans('ACGTN', 'TGCAN')


def revcomp(s):
    return s.translate(_RC)[::-1]


def _rows(a):
    return [tuple(int(v) for v in row) for row in np.asarray(a, dtype=np.int64).reshape(-1, 4)]


def pos2contig(pos, contig2start):
    """the last contig that starts at or before pos"""
    c = 0
    for i, st in enumerate(contig2start):
        if pos < st:
            break
        c = i
    return c


def find_closest(arr, target):
    """findClosest_1: (|arr[i0] - target|, |arr[i1] - target|, i0, i1) of the two neighbours of target in the ascending arr; both the same
    one when target lies on an element, before the first or after the last"""
    n = len(arr)
    if target <= arr[0]:
        return arr[0] - target, arr[0] - target, 0, 0
    if target >= arr[n - 1]:
        return target - arr[n - 1], target - arr[n - 1], n - 1, n - 1
    i, j = 0, n
    while i < j:
        mid = (i + j) // 2
        if arr[mid] == target:
            return 0, 0, mid, mid
        if target < arr[mid]:
            j = mid
        else:
            i = mid + 1
    return abs(arr[j - 1] - target), abs(arr[j] - target), j - 1, j


def local_guides(paths, mode):
    """L1: the guide chains that are re-seeded, in order, from the read's paths (primary first, each (m, 4) rows (q, r, s, l) in descending read
    order). Modes R and asm: the paths as they are. Otherwise merge_chain over paths[1:] (sorted by start; chain j joins chain i when i's end
    anchor ie and j's start anchor js have one strand, ie.q + ie.l <= js.q and |readgap - refgap| < 500), a stable sort by length, drop_somechains
    (a chain goes when its strand majority does not agree with the primary's over its span and it comes within 500 of the primary, or when it
    spans fewer than 100 read bases), a stable sort by length descending, and the budget. Returns (guides, n_total): n_total counts the list
    before the budget."""
    paths = [_rows(p) for p in paths]
    if mode in ('R', 'asm'):
        return paths, len(paths)
    chains = sorted(paths[1:], key=lambda c: c[-1][0])
    iloc = 0
    while iloc < len(chains) - 1:
        jloc = iloc + 1
        while jloc < len(chains):
            ie, js = chains[iloc][0], chains[jloc][-1]
            if ie[0] + ie[3] <= js[0] and ie[2] == js[2]:
                readgap = js[0] - ie[0] - ie[3]
                refgap = js[1] - ie[1] - ie[3] if ie[2] == 1 else ie[1] - js[1] - js[3]
                if abs(readgap - refgap) < 500:
                    chains[iloc] = chains[jloc] + chains[iloc]
                    chains.pop(jloc)
                    continue
            jloc += 1
        iloc += 1
    chains.sort(key=len)
    lst = [paths[0]] + chains
    kept = [lst[0]]
    for chain in lst[1:]:
        sc = [0, 0]; cc = [0, 0]
        distance = None
        cur = 0
        for item in lst[0]:
            if chain[-1][0] <= item[0] <= chain[0][0]:
                sc[0 if item[2] == 1 else 1] += 1
            while chain[cur][0] > item[0]:
                if cur < len(chain) - 1:
                    cur += 1
                else:
                    break
            d = abs(item[1] - chain[cur][1])
            if distance is None or d < distance:
                distance = d
        for item in chain:
            cc[0 if item[2] == 1 else 1] += 1
        keep = (sc[0] > sc[1] and cc[0] > cc[1]) or (sc[0] < sc[1] and cc[0] < cc[1])
        if (not keep and distance < 500) or (chain[0][0] - chain[-1][0]) < 100:
            continue
        kept.append(chain)
    kept.sort(key=lambda c: -len(c))
    budget = LOCAL_BUDGET[mode]
    return (kept if budget is None else kept[:budget]), len(kept)


def local_seed(contigs, read, guide, k, mode, d1=True):
    """L2: the run-merged local anchors of one guide chain, rows (q, r, s, l) in the order they are appended, and a trace
    {'windows': [(lo, hi)] as widened and clipped, 'hits': [(q, strand, refloc, (diff clause, ref1 clause, ref2 clause))] of the accepted hits in
    lookup order, 'per_q': {q: accepted hits}}. The tables _s (k-mers seen once) and _m (more than once) are keyed by the k-mer's text; d1: a
    k-mer with a non-ACGT base enters no table (otherwise only the all-N k-mer is left out, and text equality decides)."""
    look_span, read_span = LOCAL_SPANS[mode]
    contigs = [c.upper() for c in contigs]; read = read.upper()
    contig2start = [0]
    for c in contigs[:-1]:
        contig2start.append(contig2start[-1] + len(c))
    g = _rows(guide)
    readgap = 0
    for pre, now in zip(g, g[1:]):
        readgap = max(readgap, abs(now[0] - pre[0]))
    readgap = max(readgap + 1000, 5000)
    g.sort(key=lambda a: a[1])

    def cut(split_contig):
        se = [(g[0][1], g[0][1])]
        cur = pos2contig(g[0][1], contig2start)
        for item in g[1:]:
            if item[1] - se[-1][1] < readgap and (not split_contig or cur == pos2contig(item[1], contig2start)):
                se[-1] = (se[-1][0], item[1])
            else:
                if se[-1][0] == se[-1][1]:
                    se.pop()
                se.append((item[1], item[1]))
                cur = pos2contig(item[1], contig2start)
        if se[-1][0] == se[-1][1]:
            se.pop()
        return se

    def tables(se):
        _s, _m, multi, windows = {}, {}, [], []
        for min_ref, max_ref in se:
            c = pos2contig(min_ref, contig2start)
            if c != pos2contig(max_ref, contig2start):
                return None
            min_ref -= min(look_span, min_ref - contig2start[c])
            max_ref += look_span
            seq = contigs[c][min_ref - contig2start[c]:max_ref - contig2start[c]]
            windows.append((min_ref, min_ref + len(seq)))
            for iloc in range(0, len(seq) - k + 1):
                kmer = seq[iloc:iloc + k]
                if kmer == 'N' * k or (d1 and kmer.strip('ACGT')):
                    continue
                if kmer not in _s:
                    _s[kmer] = min_ref + iloc
                elif kmer in _m:
                    _m[kmer].append(min_ref + iloc)
                else:
                    _m[kmer] = [_s[kmer], min_ref + iloc]
                    multi.append(kmer)
        for kmer in multi:
            _s.pop(kmer)
        return _s, _m, windows

    t = tables(cut(False))
    if t is None:
        t = tables(cut(True))
        assert t is not None
    _s, _m, windows = t
    g.sort(key=lambda a: a[0])
    assert len({a[0] for a in g}) == len(g), 'guide read positions must be distinct'
    readstart = max(0, g[0][0] - read_span)
    readend = min(len(read) - k + 1, g[-1][0] + read_span)
    readposarr = [a[0] for a in g]
    rc = revcomp(read)
    out, pointdict, pointdict_key = [], {}, []
    trace = {'windows': windows, 'hits': [], 'per_q': {}}

    def on_hit(iloc, refloc, strand):
        point = refloc - iloc if strand == 1 else -(refloc + iloc)
        if point in pointdict:
            c0, c1, c2, c3 = pointdict[point]
            if c0 + c3 >= iloc:
                bonus = iloc - (c0 + c3) + k
                if bonus > 0:
                    keep_r = c1 if strand == 1 else refloc
                    if c3 + bonus < 20:
                        pointdict[point] = (c0, keep_r, strand, c3 + bonus)
                    else:
                        out.append((c0, c1, c2, c3))
                        pointdict[point] = (c0 + c3, c1 + c3 if strand == 1 else refloc, strand, bonus)
            else:
                out.append((c0, c1, c2, c3))
                pointdict[point] = (iloc, refloc, strand, k)
        else:
            pointdict[point] = (iloc, refloc, strand, k)
            pointdict_key.append(point)

    for iloc in range(readstart, readend):
        fwd, rev = read[iloc:iloc + k], rc[-(iloc + k):-iloc]
        if fwd == rev:
            continue
        b0, b1, i0, i1 = find_closest(readposarr, iloc)
        interval = min(b0 + b1 + 500, 2000)
        ref1, ref2 = g[i0][1], g[i1][1]
        rgap = abs(iloc - g[i0][0])
        for kmer, strand in ((fwd, 1), (rev, -1)):
            for refloc in ([_s[kmer]] if kmer in _s else _m.get(kmer, ())):
                why = (abs(rgap - abs(refloc - ref1)) < 500, ref1 - interval <= refloc <= ref1 + interval, ref2 - interval <= refloc <= ref2 + interval)
                if any(why):
                    trace['hits'].append((iloc, strand, refloc, why))
                    trace['per_q'][iloc] = trace['per_q'].get(iloc, 0) + 1
                    on_hit(iloc, refloc, strand)
    for key in pointdict_key:
        out.append(pointdict[key])
    return out, trace


def local_raw(contigs, read, paths, k, mode):
    """the read's raw local anchors: every guide of local_guides re-seeded, the rows concatenated and sorted (stable) by q + l, in mode R by q"""
    rows = []
    for g in local_guides(paths, mode)[0]:
        rows += local_seed(contigs, read, g, k, mode)[0]
    rows.sort(key=(lambda a: a[0]) if mode == 'R' else (lambda a: a[0] + a[3]))
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------ L3 / L4 / `_scar`: the local chain DPs
LOCAL_NOPRE = -9999999
LOCAL_SWITCH_OPS = 100000        # the switch to the `_fast` twin: opcount > 100000 and opcount / prereadloc > 1000, tested where the candidate space advances
LOCAL_SWITCH_RATIO = 1000


def _small_or_equal(S, target, n, point):
    """position of the last score <= target among the n entries of the score-sorted index `point`, -1 if none: the reference's own probe sequence"""
    if target < S[point[0]]:
        return -1
    if target >= S[point[n - 1]]:
        return n - 1
    i, j, mid = 0, n, 0
    while i < j:
        mid = (i + j) // 2
        v = S[point[mid]]
        if target == v:
            if mid < n - 1:
                if S[point[mid + 1]] > target:
                    return mid
                i = mid + 1
            else:
                return mid
        elif target < v:
            if mid > 0 and target >= S[point[mid - 1]]:
                return mid - 1
            j = mid
        else:
            if mid < n - 1 and target < S[point[mid + 1]]:
                return mid
            i = mid + 1
    return mid


def local_gap_geometry(ai, aj):
    """(readgap, refgap, bonus) of the step j -> i, rows (q, r, s, l); bonus <= 0 only where i ends inside j"""
    readgap = ai[0] - aj[0] - aj[3]
    if readgap < 0:
        bonus = ai[0] + ai[3] - aj[0] - aj[3]
        overlap = aj[0] + aj[3] - ai[0]
        readgap = 0
        if ai[2] == aj[2]:
            refgap = ai[1] + overlap - (aj[1] + aj[3]) if ai[2] == 1 else aj[1] - (ai[1] + bonus)
        else:
            refgap = ai[1] + overlap - aj[1] + 1 if aj[2] == -1 else ai[1] + bonus - 1 - (aj[1] + aj[3])
    else:
        bonus = ai[3]
        if ai[2] == aj[2]:
            refgap = ai[1] - aj[1] - aj[3] if ai[2] == 1 else aj[1] - ai[1] - ai[3]
        else:
            refgap = ai[1] - aj[1] + 1 if aj[2] == -1 else ai[1] + ai[3] - 1 - aj[1] - aj[3]
    return readgap, refgap, bonus


def local_dp(rows, variant, mode, k, skipcost, maxdiff, maxgap, tables):
    """The local chain DP on rows (q, r, s, l) in its input order (stable by q + l; `_scar`: by q). variant 0 LC-exact, 1 LC-mm, 2 `_scar`.
    skipcost / maxgap: as the caller of the DP passes them for the mode. tables: dict of the cost tables extra, readgap_h, readgap_r, large_readgap (float32),
    log2cache, log2int (float64) — the ones tests/golden/tables.json pins. Integers are Python integers; scores are IEEE doubles (Python floats are; S is
    stored as numpy.float64) combined in the reference's order: ((S[j] + bonus) - gapcost_list) - readgapcost, (S[j] + bonus) - (skip + table).

    Anchor i looks at the anchors whose read END lies before the read end at which the candidate space last advanced, best score first, and stops at the
    first S[j] < max_scores - l_i (strict; opcount counts that candidate too). A step is co-linear when both anchors have one strand, refgap >= 0,
    readgap <= maxgap and |readgap - refgap| <= maxdiff. An overlap whose bonus is <= 0 is passed over. The first candidate to reach a score keeps it (>).
    New entries enter the score-sorted index above their equals. LC-exact and LC-mm hand the read to their `_fast` twin when, at an advance,
    opcount > 100000 and opcount / prereadloc > 1000: the result then says so and holds nothing else.

    Returns dict: S (float64), P (int64), score, chain (descending read order, overlaps trimmed), opcount, switch (the twin takes the read), tests (the
    (opcount, prereadloc) every advance tested), kind (per row: 0 no predecessor, 1 co-linear step won, 2 non-co-linear step won), and counters."""
    a = [tuple(int(v) for v in r) for r in np.asarray(rows, dtype=np.int64).reshape(-1, 4)]
    n = len(a)
    assert n > 0 and variant in (0, 1, 2)
    scar, mm = variant == 2, variant == 1
    log2int = tables['log2int']
    gapcost_list = [0.0] * (maxdiff + 1)
    for g in range(1, maxdiff + 1):
        gapcost_list[g] = 0.01 * k * g + (0.5 if (g <= 10 or scar) else 2) * float(log2int[g])
    rgc = tables['large_readgap'] if mm else (tables['readgap_r'] if mode == 'R' else tables['readgap_h'])
    extra, log2cache = tables['extra'], tables['log2cache']
    extra_size, l2c_size = len(extra) - 1, len(log2cache) - 1
    skipcost = float(skipcost)
    S = np.empty(n, np.float64); P = np.empty(n, np.int64); kind = np.zeros(n, np.int8)
    S_arg = [0] * n
    fixed = [0.0] * n; prepen = [0.0] * n
    C = dict(colinear_wins=0, noncolinear_wins=0, cross_strand_wins=0, refunds=0, debts_carried=0, bonus_skips=0, longest_scan=0, below16=0, below3=0, insert_among_equals=0,
             eq_break_evals=0, breaks=0, tie_tests=0, scans_past16=0, scans_past3=0, extra_saturated=0, l2c_saturated=0, gapcost_above10=0, overlaps=0, advances=0, held=0,
             late_updates=0, kind_flips=0)
    S[0] = float(a[0][3]); P[0] = LOCAL_NOPRE
    g_max, g_idx = float(a[0][3]), 0
    prereadloc = a[0][0] + a[0][3]
    te, opcount = 1, 0
    out = dict(switch=False, tests=[])
    for i in range(1, n):
        ai = a[i]
        li = float(ai[3])
        max_scores, pre = li, LOCAL_NOPRE
        if prereadloc < ai[0] + ai[3]:
            if not scar:
                out['tests'].append((opcount, prereadloc))
                if opcount > LOCAL_SWITCH_OPS and opcount / prereadloc > LOCAL_SWITCH_RATIO:
                    out.update(switch=True, opcount=opcount, S=None, P=None, score=None, chain=None, kind=None, counters=C)
                    return out
            for kk in range(te, i):
                loc = _small_or_equal(S, S[kk], kk, S_arg) + 1
                C['insert_among_equals'] += loc > 0 and S[S_arg[loc - 1]] == S[kk]
                C['below16'] += kk - loc >= 16
                C['below3'] += kk - loc >= 3
                S_arg[loc + 1:kk + 1] = S_arg[loc:kk]
                S_arg[loc] = kk
            te = i
            prereadloc = ai[0] + ai[3]
            C['advances'] += 1
        else:
            C['held'] += 1
        scanned = updates = 0
        win_kind = 0
        for x in range(te - 1, -1, -1):
            j = S_arg[x]
            opcount += 1
            scanned += 1
            Sj = float(S[j])
            lim = max_scores - li
            if Sj < lim:
                C['breaks'] += 1
                break
            C['eq_break_evals'] += Sj == lim
            aj = a[j]
            readgap, refgap, bonus = local_gap_geometry(ai, aj)
            if ai[0] - aj[0] - aj[3] < 0:
                C['overlaps'] += 1
                if bonus <= 0:
                    C['bonus_skips'] += 1
                    continue
            gapcost = abs(readgap - refgap)
            col = ai[2] == aj[2] and refgap >= 0 and readgap <= maxgap and gapcost <= maxdiff
            nf = npp = 0.0
            if col:
                test = Sj + bonus - gapcost_list[gapcost] - float(rgc[readgap])
                if scar:
                    refund = fixed[j] < 0 and fixed[j] + bonus >= 0
                    if refund:
                        test += prepen[j]
                    if fixed[j] < 0 and fixed[j] + bonus < 0:
                        nf, npp = fixed[j] + bonus, prepen[j]
            elif scar:
                test = Sj + bonus - skipcost
                nf, npp = -skipcost + bonus, skipcost
            elif not mm:
                g = min(gapcost, extra_size)
                pen = (min(50.0, skipcost) if ai[2] != aj[2] else skipcost) + float(extra[g])
                test = Sj + bonus - pen
            else:
                pen = skipcost + float(log2cache[min(l2c_size, gapcost)])
                test = Sj + bonus - pen
            if test > max_scores:
                updates += 1
                C['kind_flips'] += win_kind != 0 and win_kind != (1 if col else 2)
                max_scores, pre, win_kind = test, j, 1 if col else 2
                win = dict(col=col, cross=ai[2] != aj[2], gapcost=gapcost, refund=col and scar and fixed[j] < 0 and fixed[j] + bonus >= 0, debt=col and scar and nf < 0)
                if scar:
                    fixed[i], prepen[i] = nf, npp
            elif test == max_scores and pre != LOCAL_NOPRE:
                C['tie_tests'] += 1
        S[i] = max_scores; P[i] = pre; kind[i] = win_kind
        C['longest_scan'] = max(C['longest_scan'], scanned)
        C['scans_past16'] += scanned > 16
        C['scans_past3'] += scanned > 3
        C['late_updates'] += updates > 1
        if pre != LOCAL_NOPRE:
            C['colinear_wins'] += win['col']
            C['noncolinear_wins'] += not win['col']
            C['cross_strand_wins'] += (not win['col']) and win['cross']
            C['refunds'] += win['refund']
            C['debts_carried'] += win['debt']
            C['gapcost_above10'] += win['col'] and win['gapcost'] > 10
            C['extra_saturated'] += (not win['col']) and variant == 0 and win['gapcost'] >= extra_size
            C['l2c_saturated'] += (not win['col']) and mm and win['gapcost'] >= l2c_size
        if max_scores > g_max:
            g_max, g_idx = max_scores, i
    chain = []
    take = g_idx
    chain.append(a[take])
    preitem = a[take]
    C['trimmed'] = C['trimmed_to_1'] = 0
    while P[take] != LOCAL_NOPRE:
        take = int(P[take])
        now = a[take]
        if preitem[0] < now[0] + now[3]:
            ov = now[0] + now[3] - preitem[0]
            chain[-1] = (preitem[0] + ov, preitem[1] + ov if preitem[2] == 1 else preitem[1], preitem[2], preitem[3] - ov)
            C['trimmed'] += 1
            C['trimmed_to_1'] += preitem[3] - ov == 1
        chain.append(now)
        preitem = now
    out.update(S=S, P=P, score=g_max, chain=np.array(chain, dtype=np.int64).reshape(-1, 4), opcount=opcount, kind=kind, counters={k_: int(v) for k_, v in C.items()})
    return out
