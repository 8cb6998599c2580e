"""CPU tests: the spec references of tests/spec_ref.py against hand-computed answers, brute-force definitions on tiny inputs and each
other — then the ORACLE against the references on random and edge inputs, so that the oracle is no longer its own judge."""
import itertools
from functools import lru_cache
import numpy as np
import pytest
import spec_ref as R
import spec_cases as SC
from kernel_cases import rand_seq, mutate


def _rs(rng, n, alpha):
    return ''.join(alpha[i] for i in rng.integers(0, len(alpha), n))


def _alignments(tl, ql):
    """every op string over M / D / I that consumes tl target and ql query bases"""
    if tl == 0 and ql == 0:
        yield ''
        return
    if tl and ql:
        for s in _alignments(tl - 1, ql - 1):
            yield s + 'M'
    if tl:
        for s in _alignments(tl - 1, ql):
            yield s + 'D'
    if ql:
        for s in _alignments(tl, ql - 1):
            yield s + 'I'


def _rle(ops):
    return ''.join('%d%s' % (len(list(g)), k) for k, g in itertools.groupby(ops))


# ------------------------------------------------------------------------------------------------ VMX-ED
def _lev_brute(a, b):
    x, y = R.codes(a).tolist(), R.codes(b).tolist()

    @lru_cache(None)
    def D(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(D(i - 1, j) + 1, D(i, j - 1) + 1, D(i - 1, j - 1) + (x[i - 1] != y[j - 1]))
    return D(len(x), len(y))


def test_levenshtein():
    assert R.levenshtein('', '') == 0 and R.levenshtein('', 'ACG') == 3 and R.levenshtein('ACGT', '') == 4
    assert R.levenshtein('ACGT', 'AGT') == 1 and R.levenshtein('AC', 'CA') == 2 and R.levenshtein('AAAA', 'TTTT') == 4
    assert R.levenshtein('acgt', 'ACGT') == 0                   # case is ignored
    assert R.levenshtein('NRYN', 'nnnn') == 0                   # every other byte is one code
    assert R.levenshtein('NA', 'AN') == 2
    rng = np.random.default_rng(1)
    for _ in range(300):
        a = _rs(rng, int(rng.integers(0, 9)), 'ACGTN'); b = _rs(rng, int(rng.integers(0, 9)), 'ACGTNacR')
        assert R.levenshtein(a, b) == _lev_brute(a, b) == R.levenshtein(b, a), (a, b)


# ------------------------------------------------------------------------------------------------ VMX-DP-G
def test_cigar_score():
    assert R.cigar_score('2=1X1=', 'ACGT', 'ACTT') == 2 + 2 - 4 + 2
    assert R.cigar_score('4M', 'ACGT', 'ACTT') == 2
    assert R.cigar_score('1M30D1M', 'A' + 'C' * 30 + 'G', 'AG') == 4 - 54 and R.cigar_score('2M3I', 'AC', 'ACGGG') == 4 - 10
    for bad in ('3M', '5M', '2=2=', '1=1X2=', '4X', '1I4M', '4M1D', '2M1X1', 'M4'):
        with pytest.raises(AssertionError):
            R.cigar_score(bad, 'ACGT', 'ACTT')
    with pytest.raises(AssertionError):
        R.cigar_score('1=', 'N', 'N')                          # an N never matches


def test_dpg_score():
    assert R.dpg_score('', '') == 0 and R.dpg_score('A', 'A') == 2 and R.dpg_score('A', 'C') == -4 and R.dpg_score('N', 'N') == -4
    assert R.dpg_score('', 'ACG') == -10 and R.dpg_score('ACGT', '') == -12         # min(4 + 2 L, 24 + L)
    assert R.dpg_score('A' * 30, '') == -54                                         # the second piece: 24 + 30 < 4 + 60
    P, S = 'ACGTTGCAAC', 'GGATCCATGA'
    assert R.dpg_score(P + 'T' * 30 + S, P + S) == 40 - 54 and R.dpg_score(P + S, P + 'T' * 3 + S) == 40 - 10
    rng = np.random.default_rng(2)
    for sc in SC.GAP_SCORES + [(3, -2, 5, 3, 15, 1)]:         # brute force: the best of every alignment, rescored
        for _ in range(25):
            t = _rs(rng, int(rng.integers(0, 5)), 'ACGN'); q = _rs(rng, int(rng.integers(0, 5)), 'ACGN')
            best = max(R.cigar_score(_rle(ops), t, q, *sc) for ops in _alignments(len(t), len(q)))
            assert R.dpg_score(t, q, *sc) == best, (t, q, sc)
    for _ in range(12):                                         # the cell-by-cell ksw2-order DP: same optimum, its CIGAR rescores to it
        t = rand_seq(rng, int(rng.integers(1, 45))); q = mutate(rng, t, 0.25) or 'A'
        for sc in SC.GAP_SCORES:
            cg, s = R.ksw2_order_cigar(t, q, *sc)
            assert s == R.dpg_score(t, q, *sc) == R.cigar_score(cg, t, q, *sc), (t, q, sc)


# ------------------------------------------------------------------------------------------------ VMX-DP-X
def _dpx_brute(t, q, match, mismatch, o, e, bw, zdrops):
    """H(i, j) = the best score of every op string from (0, 0) to (i, j) whose cells all lie in the band; then the diagonal scan"""
    tl, ql = len(t), len(q)
    if bw < 0:
        bw = max(tl, ql)
    x, y = R.codes(t).tolist(), R.codes(q).tolist()
    H = {}
    for i in range(tl + 1):
        for j in range(ql + 1):
            if abs(i - j) > bw:
                continue
            best = None
            for ops in _alignments(i, j):
                a = b = s = 0; ok = True
                for op, g in itertools.groupby(ops):
                    L = len(list(g))
                    if op != 'M':
                        s -= o + e * L
                    for _ in range(L):
                        if op == 'M':
                            s += match if (x[a] == y[b] and x[a] < 4) else mismatch
                        a += op != 'I'; b += op != 'D'
                        ok = ok and abs(a - b) <= bw
                if ok and (best is None or s > best):
                    best = s
            H[i, j] = best
    out = []
    for zdrop in zdrops:
        M, bi, bj, m_prev = 0, 0, 0, 0
        for d in range(1, tl + ql + 1):
            cells = [(i, d - i) for i in range(tl + 1) if (i, d - i) in H]
            m_d = max((H[c] for c in cells), default=R.NEG)
            if m_d > M:
                bi = min(i for i, j in cells if H[i, j] == m_d); M, bj = m_d, d - bi
            if max(m_d, m_prev) < M - zdrop:
                break
            m_prev = m_d
        out.append((M, bi, bj))
    return out


def test_dpx():
    assert R.dpx('ACGTACGTAC', 'ACGTACGTAC') == (20, 10, 10) and R.dpx('', 'ACGT') == (0, 0, 0) and R.dpx('C', 'A') == (0, 0, 0)
    assert R.dpx('ACGT', 'ACGT', bw=0) == (8, 4, 4)                     # bw = 0: the odd (empty) diagonals do not end the scan
    P = 'ACGTTGCAACGGATCCATGA'
    assert R.dpx(P + 'AGG', P + 'CGG') == (40, 20, 20)                  # the later diagonal's equal score does not replace the best
    # 60 - 8 + 7 * 3 at (27, 28) after an insertion = at (28, 27) after a deletion, both on diagonal 55: the smaller i is kept
    assert R.dpx(P + 'ACACACAC', P + 'CACACACA', 3, -2, 6, 2, 100, 10 ** 6) == (73, 27, 28)
    # five mismatches: the deepest max(m_d, m_{d-1}) is 40 - 20, so zdrop 20 crosses to the second P and 19 stops at the first
    assert R.dpx(P + 'TTTTT' + P, P + 'GGGGG' + P, zdrop=19) == (40, 20, 20) and R.dpx(P + 'TTTTT' + P, P + 'GGGGG' + P, zdrop=20) == (60, 45, 45)
    rng = np.random.default_rng(3)
    zdrops = (0, 1, 3, 8, 10 ** 6)
    for p in SC.EXT_SCORES:
        for _ in range(10):
            t = _rs(rng, int(rng.integers(0, 5)), 'ACN'); q = _rs(rng, int(rng.integers(0, 5)), 'ACN')
            for bw in (0, 1, 2, -1):
                assert [R.dpx(t, q, *p, bw, z) for z in zdrops] == _dpx_brute(t, q, *p, bw, zdrops), (t, q, p, bw)


# ------------------------------------------------------------------------------------------------ VMX-S1
def _h64(key, k):
    m = (1 << 2 * k) - 1
    key = (~key + (key << 21)) & m; key ^= key >> 24; key = (key + (key << 3) + (key << 8)) & m; key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & m; key ^= key >> 28
    return (key + (key << 31)) & m


def test_hash64():
    for k in range(1, 8):                                   # invertible: a permutation of the 2k-bit keys
        h = R.hash64(np.arange(4 ** k, dtype=np.uint64), (1 << 2 * k) - 1)
        assert len(np.unique(h)) == 4 ** k and int(h.max()) < 4 ** k
    rng = np.random.default_rng(4)
    for k in (1, 2, 15, 16, 17, 27, 28):
        keys = rng.integers(0, 4 ** k, 200, dtype=np.uint64) if k < 32 else None
        assert [int(v) for v in R.hash64(keys, (1 << 2 * k) - 1)] == [_h64(int(v), k) for v in keys]


def test_kmer_hashes_and_sketch():
    rc = str.maketrans('ACGT', 'TGCA')
    rng = np.random.default_rng(5)
    for k in (1, 2, 3, 5, 15, 16, 28):                      # per position, from the k-mer string itself
        s = rand_seq(rng, 60) + 'N' + rand_seq(rng, 30).lower()
        h, z = R.kmer_hashes(s, k)
        for p in range(len(s) - k + 1):
            f = s[p:p + k].upper(); r = f.translate(rc)[::-1]
            val = lambda u: int(''.join('0123'['ACGT'.index(c)] for c in u), 4)
            if 'N' in f or f == r:
                assert h[p] == R.INF64
            else:
                assert int(h[p]) == _h64(min(val(f), val(r)), k) and int(z[p]) == (val(r) < val(f))
    assert len(R.sketch('ACGT', 4, 1)[0]) == 0 and len(R.sketch('AT' * 5, 2, 3)[0]) == 0          # palindromes are skipped
    assert len(R.sketch('ACG', 4, 5)[0]) == 0
    h, p, z = R.sketch('AAAAAA', 3, 2)
    assert p.tolist() == [0, 1, 2, 3] and len(set(h.tolist())) == 1 and z.tolist() == [0] * 4          # all ties kept
    h2, _, z2 = R.sketch('TTTTTT', 3, 2)
    assert h2.tolist() == h.tolist() and z2.tolist() == [1] * 4
    for k in (1, 2, 3, 5, 15, 16, 17, 27, 28):
        for w in (1, 2, 3, 9, 10, 11, 255):
            for s in SC.sketch_seqs(rng, k, w, long_len=90):
                got, exp = R.sketch(s, k, w), R.sketch_brute(s, k, w)
                assert all(np.array_equal(a, b) for a, b in zip(got, exp)), (k, w, s)


def test_cluster_hits_on_hand_written_sets():
    """VMX-S1's cluster rules on hit sets small enough to rank by eye; rows are (q, r, s, l)"""
    H = lambda *rows: np.array([(q, r, s, 15) for q, r, s in rows], dtype=np.int64).reshape(-1, 4)
    out = lambda hits, cn: [tuple(x[:3]) for x in R.cluster_hits(hits, cn).tolist()]
    # a gap of exactly 5000 stays inside the cluster, 5001 cuts
    assert out(H((7, 10000, 1), (3, 5000, 1)), 0) == [(3, 5000, 1), (7, 10000, 1)] and out(H((7, 10000, 1), (3, 5000, 1)), 1) == [(3, 5000, 1), (7, 10000, 1)]
    assert out(H((7, 10001, 1), (3, 5000, 1)), 1) == [(3, 5000, 1)] and out(H((7, 10001, 1), (3, 5000, 1)), 2) == [(3, 5000, 1), (7, 10001, 1)]
    # a chain of steps of 5000 is one cluster however long it gets
    chain = H(*[(i, 5000 * i, 1) for i in range(6)])
    assert out(chain, 1) == [(i, 5000 * i, 1) for i in range(6)]
    # inside a cluster: r first, then q, then s (-1 before +1)
    tie = H((9, 100, 1), (2, 100, 1), (2, 100, -1), (5, 50, -1))
    assert out(tie, 0) == [(5, 50, -1), (2, 100, -1), (2, 100, 1), (9, 100, 1)]
    # sizes 1, 2, 2, 3 in reference order 2 (at 0), 1 (at 20000), 3 (at 40000), 2 (at 60000): rank = 3, then the twos by first r, then the one
    hits = H((0, 0, 1), (1, 10, 1), (2, 20000, -1), (3, 40000, 1), (4, 40010, 1), (5, 45010, 1), (6, 60000, 1), (7, 60001, -1))
    three = [(3, 40000, 1), (4, 40010, 1), (5, 45010, 1)]; two_a = [(0, 0, 1), (1, 10, 1)]; two_b = [(6, 60000, 1), (7, 60001, -1)]; one = [(2, 20000, -1)]
    assert out(hits, 1) == three and out(hits, 2) == three + two_a and out(hits, 3) == three + two_a + two_b
    assert out(hits, 4) == out(hits, 5) == out(hits, 0) == out(hits, -1) == three + two_a + two_b + one
    assert out(hits[::-1], 3) == three + two_a + two_b                                                  # the order handed in does not matter
    assert R.cluster_hits(np.zeros((0, 4), np.int64), 3).shape == (0, 4)
    rng = np.random.default_rng(6)
    for _ in range(300):
        n = int(rng.integers(0, 14))
        h = np.stack([rng.integers(0, 6, n), rng.choice([0, 1, 4999, 5000, 5001, 5002, 10000, 10001, 15002, 30000, 30001], n), rng.choice([-1, 1], n), np.full(n, 15)], axis=1)
        for cn in (-1, 0, 1, 2, 3, 20):
            assert np.array_equal(R.cluster_hits(h, cn), R.cluster_hits_brute(h, cn)), (h.tolist(), cn)


def test_default_mid_occ_on_hand_written_counts():
    hs = lambda counts: np.repeat(np.arange(len(counts), dtype=np.uint64) * np.uint64(977), counts)
    assert R.default_mid_occ(hs([])) == 10 and R.default_mid_occ(hs([1])) == 10 and R.default_mid_occ(hs([9])) == 10 and R.default_mid_occ(hs([10])) == 11
    assert R.default_mid_occ(hs([30, 1, 1])) == 31                     # nd = 3: floor(0.9998 * 3) = 2, the largest count
    assert R.default_mid_occ(hs([1] * 4998 + [50])) == 51               # nd = 4999: index 4998, the largest
    assert R.default_mid_occ(hs([50, 30] + [1] * 4999)) == 31          # nd = 5001: floor(4999.9998) = 4999 of 0 ... 5000, the second largest
    assert R.default_mid_occ(hs([50, 30] + [1] * 9999)) == 10          # nd = 10001: floor(9998.9998) = 9998 of 0 ... 10000, the third largest


def test_map_read_on_a_hand_written_reference():
    """k = 3, w = 1: ACG (canonical, strand 0), its reverse complement CGT (strand 1) and AAC, each between N"""
    ref = ['NACGNNNNCGTN', 'AACNACG']                      # ACG at 1 and (second contig, offset 12) 16, CGT at 8, AAC at 12
    IH, IP = R.index_minimizers(ref, 3, 1)
    assert sorted((IP >> np.uint64(1)).tolist()) == [1, 8, 12, 16] and R.default_mid_occ(IH) == 10
    rows = lambda read, cn, mo: R.map_read(IH, IP, 3, 1, read, cn, mo).tolist()
    assert rows('ACG', 0, 3) == [[0, 1, 1, 3], [0, 8, -1, 3], [0, 16, 1, 3]]                   # one cluster: every gap <= 5000
    assert rows('ACG', 0, 2) == [] and rows('ACG', 0, -1) == rows('ACG', 0, 3)                  # three occurrences against a cap of 2; -1 = the default (10)
    assert rows('CGTNAAC', 0, 3) == [[0, 1, -1, 3], [0, 8, 1, 3], [4, 12, 1, 3], [0, 16, -1, 3]]
    assert rows('CGTNAAC', 0, 1) == [[4, 12, 1, 3]] and rows('NN', 0, 3) == [] and rows('', 0, 3) == [] and rows('AC', 0, 3) == []
    assert rows('GTT', 1, 1) == [[0, 12, -1, 3]]                                                # the reverse complement of AAC
    rng = np.random.default_rng(7)
    for k, w in ((3, 1), (3, 2), (4, 3), (5, 1)):
        contigs = [_rs(rng, 60, 'ACGTN'), _rs(rng, 25, 'ACGT')]
        ih, ip = R.index_minimizers(contigs, k, w)
        for _ in range(12):
            read = _rs(rng, int(rng.integers(0, 30)), 'ACGTN')
            for cn, mo in ((0, 1), (1, 2), (2, 3), (3, -1), (-1, 50)):
                assert np.array_equal(R.map_read(ih, ip, k, w, read, cn, mo), R.map_read_brute(ih, ip, k, w, read, cn, mo)), (contigs, read, k, w, cn, mo)


# ------------------------------------------------------------------------------------------------ the oracle against the references
def test_oracle_edit_distance_is_spec(oracle):
    qs, ts = SC.edit_distance_pairs(np.random.default_rng(10), (0, 1, 63, 64, 65, 127, 128, 129, 700))
    for q, t in zip(qs, ts):
        assert oracle.edit_distance(q, t) == R.levenshtein(q, t), (len(q), len(t))


def test_oracle_gapfill_is_spec(oracle):
    rng = np.random.default_rng(11)
    for sc in SC.GAP_SCORES:
        for t, q in SC.gapfill_pairs(rng, (60, 160, 161), base=(10, 60)):
            e = R.dpg_score(t, q, *sc)
            for eqx in (False, True):
                cg, s = oracle.k_cigar_global(t, q, *sc, eqx=eqx)
                assert s == e == R.cigar_score(cg, t, q, *sc), (t, q, sc)
            if len(t) * len(q) <= 2500:
                assert oracle.k_cigar_global(t, q, *sc)[0] == R.ksw2_order_cigar(t, q, *sc)[0], (t, q, sc)


def test_oracle_extend_is_spec(oracle):
    rng = np.random.default_rng(12)
    for p in SC.EXT_SCORES:
        for bw in (0, 1, 2, 63, 64, 65, 100, -1):
            for t, q in SC.extend_random(rng, 5, 150):
                for zdrop in (0, 1, 50, 10 ** 6):
                    assert oracle.k_extend(t, q, *p, bw, zdrop) == R.dpx(t, q, *p, bw, zdrop), (t, q, p, bw, zdrop)
        for t, q, bw, zdrop, tag in SC.extend_constructed(rng, p):
            assert oracle.k_extend(t, q, *p, bw, zdrop) == R.dpx(t, q, *p, bw, zdrop), (tag, p)
    rng = np.random.default_rng(13)                            # no band: the case a 496-wide band would get wrong
    a = rand_seq(rng, 1500)
    assert oracle.k_extend(a, a[:50] + rand_seq(rng, 520) + a[50:], 2, -4, 4, 4, -1, 10 ** 6) == (916, 1500, 2020)


def test_oracle_sketch_and_index_are_spec(oracle):
    rng = np.random.default_rng(14)
    for k in (1, 2, 15, 16, 17, 27, 28):
        for w in (1, 2, 9, 10, 11, 255):
            for s in SC.sketch_seqs(rng, k, w, long_len=3000):
                got, exp = oracle.sketch(s, k, w), R.sketch(s, k, w)
                assert all(np.array_equal(a, b) for a, b in zip(got, exp)), (k, w, len(s))
    for k, w in ((1, 1), (15, 10), (19, 10), (28, 255)):
        contigs = [rand_seq(rng, 6000), 'ACGT' * 30 + 'N' * 10 + rand_seq(rng, 300).lower(), rand_seq(rng, max(k - 1, 1)), 'A' * 500 + rand_seq(rng, 900)]
        oi = oracle.Index.from_seqs(['c%d' % i for i in range(len(contigs))], contigs, k=k, w=w)
        got, exp = oi.minimizers(), R.index_minimizers(contigs, k, w)
        assert all(np.array_equal(a, b) for a, b in zip(got, exp)), (k, w)


# ------------------------------------------------------------------------------------------------ L1 / L2: local re-seeding
def _planted(total, at, s):
    return 'N' * at + s + 'N' * (total - at - len(s))


def test_local_find_closest():
    a = [10, 20, 30]
    assert R.find_closest(a, 5) == (5, 5, 0, 0) and R.find_closest(a, 10) == (0, 0, 0, 0) and R.find_closest(a, 35) == (5, 5, 2, 2)
    assert R.find_closest(a, 20) == (0, 0, 1, 1) and R.find_closest(a, 24) == (4, 6, 1, 2) and R.find_closest(a, 11) == (1, 9, 0, 1)
    assert R.find_closest([7], 7) == (0, 0, 0, 0) and R.find_closest([7], 9) == (2, 2, 0, 0)


def test_local_seed_by_hand():
    P = 'ACGTTGCAAGTCC'                                        # 13 bases: five 9-mers
    ref, read = _planted(20000, 10000, P), _planted(300, 100, P)
    guide = [(200, 10100, 1, 15), (50, 9950, 1, 15)]
    rows, tr = R.local_seed([ref], read, guide, 9, 'H')
    assert tr['windows'] == [(2950, 17100)]                   # 9950 - 7000 .. 10100 + 7000
    assert [h[:3] for h in tr['hits']] == [(100 + o, 1, 10000 + o) for o in range(5)] and tr['per_q'] == {100 + o: 1 for o in range(5)}
    assert tr['hits'][0][3] == (True, True, True)             # q = 100: b0 = 50, b1 = 100, interval 650; refloc - ref1 = 50 = the read gap, refloc - ref2 = -100
    assert rows == [(100, 10000, 1, 13)]                      # one run: l = 9, 10, ... 13
    # text equality (the reference): the k-mers of Ns and the probe's ends match too, 92 .. 112; l + bonus reaches 20 at q = 103
    assert R.local_seed([ref], read, guide, 9, 'H', d1=False)[0] == [(92, 9992, 1, 19), (111, 10011, 1, 10)]
    # mode R: reference span 2000, read span 500
    assert R.local_seed([ref], read, guide, 9, 'R')[1]['windows'] == [(7950, 12100)]
    assert R.local_seed([ref], _planted(2000, 1200, P), [(600, 10600, 1, 15), (500, 10500, 1, 15)], 9, 'R')[0] == []      # read window ends at 600 + 500
    assert R.local_seed([ref], _planted(2000, 1095, P), [(600, 9505, 1, 15), (500, 9405, 1, 15)], 9, 'R')[0] == [(1095, 10000, 1, 13)]
    # the reverse strand: r follows the newest hit; no reverse look-up at read position 0
    rows, tr = R.local_seed([ref], _planted(300, 0, R.revcomp(P)), [(150, 10150, 1, 15), (20, 10020, 1, 15)], 9, 'H')
    assert [h[:3] for h in tr['hits']] == [(1, -1, 10003), (2, -1, 10002), (3, -1, 10001), (4, -1, 10000)] and rows == [(1, 10000, -1, 12)]
    # a single-anchor guide, and two anchors readgap apart, have no window: nothing
    assert R.local_seed([ref], read, [(100, 10000, 1, 15)], 9, 'H')[0] == []
    assert R.local_seed([ref], read, [(200, 15000, 1, 15), (100, 10000, 1, 15)], 9, 'H')[0] == []
    assert R.local_seed([ref], read, [(200, 14999, 1, 15), (100, 10000, 1, 15)], 9, 'H')[0] == [(100, 10000, 1, 13)]
    # two copies in the reference: both diagonals, the leftovers in first-appearance order (ascending reference position here)
    ref2 = ref[:10300] + P + ref[10313:]
    assert R.local_seed([ref2], read, guide, 9, 'H')[0] == [(100, 10000, 1, 13), (100, 10300, 1, 13)]
    # a guide across two contigs is cut at the contig change (the retry): with one anchor on either side nothing is left, with two there are two
    # windows, each inside its contig, and the copy at the start of the second contig is found
    two = [ref[:10020], P + ref[10033:]]
    assert R.local_seed(two, read, guide, 9, 'H')[0] == []
    rows, tr = R.local_seed(two, read, [(200, 10100, 1, 15), (150, 10050, 1, 15), (90, 9990, 1, 15), (50, 9950, 1, 15)], 9, 'H')
    assert rows == [(100, 10000, 1, 13), (100, 10020, 1, 13)] and tr['windows'] == [(2950, 10020), (10020, 17100)]


def test_local_guides_and_raw_by_hand():
    P0 = [(q, 1000 + q, 1, 15) for q in range(900, 0, -100)]
    short = [(360, 50360, 1, 15), (330, 50330, 1, 15), (300, 50300, 1, 15)]          # spans 60 read positions: dropped
    longer = [(450, 50450, 1, 15), (375, 50375, 1, 15), (300, 50300, 1, 15)]
    assert R.local_guides([P0, short], 'H') == ([P0], 1) and R.local_guides([P0, short], 'R') == ([P0, short], 2)
    assert R.local_guides([P0, longer], 'H') == ([P0, longer], 2) and R.local_guides([longer, P0], 'H') == ([P0, longer], 2)      # by length, descending
    # two short chains that merge (gap difference 499) are one guide of six anchors; at 500 they stay apart and are dropped
    nxt = [(560, 50560 + 499, 1, 15), (530, 50530 + 499, 1, 15), (500, 50500 + 499, 1, 15)]
    assert R.local_guides([P0, nxt, short], 'H') == ([P0, nxt + short], 2)
    assert R.local_guides([P0, [(q, r + 1, s, l) for q, r, s, l in nxt], short], 'H') == ([P0], 1)
    # the budget: 5 / 3 / all
    many = [[(q, 60000 * (j + 1) + q, 1, 15) for q in (400, 300, 200)] for j in range(6)]
    assert [len(R.local_guides([P0] + many, m)[0]) for m in ('H', 'L', 'S')] == [5, 3, 7] and R.local_guides([P0] + many, 'H')[1] == 7
    # local_raw: the guides' rows in one list, sorted by q + l (stable), in mode R by q
    A, B = 'ACGTTGCAAGTCC', 'TTGACCAGTAC'
    ref = _planted(20000, 10000, A)
    ref = ref[:10090] + B + ref[10101:]
    read = _planted(300, 100, A)
    read = read[:102] + B + read[113:]
    guide = [(200, 10100, 1, 15), (50, 9950, 1, 15)]
    assert R.local_raw([ref], read[:100] + A + read[113:], [guide], 9, 'H').tolist() == [[100, 10000, 1, 13]]
    read2 = _planted(300, 100, A)[:120] + B + 'N' * 169
    assert R.local_raw([ref], read2, [guide], 9, 'H').tolist() == [[100, 10000, 1, 13], [120, 10090, 1, 11]]
    read3 = _planted(300, 104, B)[:130] + A[:9] + 'N' * 161                            # B ends at 115, A's first 9-mer at 139: q + l order is B, A; so is q order
    assert R.local_raw([ref], read3, [guide], 9, 'H').tolist() == [[104, 10090, 1, 11], [130, 10000, 1, 9]]
