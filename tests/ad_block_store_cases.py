"""Cases for the anti-diagonal band fill's block stores (vmx_dp_ad.h: the bytes of four anti-diagonals per lane go out in ONE store, into the lane-major lines of
vmx_gapfill.h), shared by test_emu_ad_block_store.py (emulator build) and test_gpu_ad_block_store.py. Every problem has tl + ql <= 160, the small class of both
builds; the band-width rule is pushed through its four widths with VMX_AD_PCT, as test_emu_gapfill_banded does. What is compared, problem for problem: the CIGAR
of the batched path (vm_k_cigar_batch_banded: band, proof, walk over the band's bytes) with the full-matrix entry's (vm_k_cigar_batch) and the oracle's, the
full-matrix score with the oracle's, and the score the banded CIGAR itself adds up to with both."""
import functools
import re
import numpy as np
import kernel_cases as KC

PCTS = (100, 250, 330, 400)        # VMX_AD_PCT values at which problems of ~70 bases get 1, 2, 3 and 4 diagonal pairs per lane (slots of 1, 2, 4 and 4 bytes)
LIMIT = 160
SCORE = dict(match=2, mismatch=-4, o1=4, e1=2, o2=24, e2=1)


def cigar_score(t, q, cg):
    """what a CIGAR (M or =/X) scores under the gap fill's two-piece affine scoring; it must consume both strings"""
    i = j = s = 0
    for n, op in re.findall(r'(\d+)([MIDX=])', cg):
        n = int(n)
        if op in 'M=X':
            s += sum(SCORE['match'] if (a == b and a != 'N') else SCORE['mismatch'] for a, b in zip(t[i:i + n], q[j:j + n]))
            i += n; j += n
        else:
            s -= min(SCORE['o1'] + n * SCORE['e1'], SCORE['o2'] + n * SCORE['e2'])
            if op == 'D':
                i += n
            else:
                j += n
    assert i == len(t) and j == len(q), (cg, len(t), len(q))
    return s


def light(rng, a, k=2):
    """a with k substitutions: the same length, a path along the main diagonal"""
    a = list(a)
    for p in rng.integers(0, len(a), min(k, len(a))):
        a[p] = 'ACGT'[('ACGT'.index(a[p]) + 1 + int(rng.integers(0, 3))) % 4]
    return ''.join(a)


def sized(rng, tl, ql):
    """(target, query) of exactly these lengths: a shared core with light substitutions, the longer side with one extra run in the middle"""
    n = min(tl, ql)
    core = KC.rand_seq(rng, n)
    other = light(rng, core, 2 if n > 8 else 0)
    extra = KC.rand_seq(rng, abs(tl - ql))
    longer = core[:n // 2] + extra + core[n // 2:]
    return (longer, other) if tl >= ql else (other, longer)


@functools.lru_cache(maxsize=None)
def problems(pct):
    """[(target, query, tag)] for one band-width rule, and the groups that are run as batches of their own (pairs sharing a 16-lane row, a row with X only)"""
    rng = np.random.default_rng(900 + pct)
    out = []
    # the last block of a problem full, or holding 1, 2 or 3 anti-diagonals (tl + ql mod 4), with odd and even pair counts ((tl + ql + 1) // 2): every total at
    # both ends of the small class, square and off by a few bases
    for tot in list(range(2, 22)) + list(range(LIMIT - 43, LIMIT + 1)):
        for d in (0, 3):
            tl = max(1, tot // 2 - d); ql = tot - tl
            t, q = sized(rng, tl, ql)
            out.append((t, q, 'tot%d d%d' % (tot, d)))
    # fewer than four anti-diagonals; one side a single base
    for tl, ql in ((1, 1), (1, 2), (2, 1), (1, 3), (1, 17), (17, 1), (1, 40), (40, 1), (1, 100), (100, 1)):
        t, q = sized(rng, tl, ql)
        out.append((t, q, '%dx%d' % (tl, ql)))
    # gaps on the band's edge lanes: one deletion / insertion as long as the margin g of the band allows, one and two bases less, at the start, the middle and the
    # end of a problem whose flanks are clean (still proven); the walk's gap states read these cells through vmx_tb_cell_off
    L = 70
    ns = max(1, KC.ad_ns(L, L, pct))
    g = KC.ad_geom(L, L, ns)[0]
    for d in sorted(set(x for x in (g - 3, g - 2, g - 1, g) if 1 <= x < L // 2)):
        for pos in (2, L // 2, L - 2 - d):
            a = KC.rand_seq(rng, L)
            out.append((a, a[:pos] + a[pos + d:], 'edge D%d@%d' % (d, pos)))
            out.append((a[:pos] + a[pos + d:], a, 'edge I%d@%d' % (d, pos)))
    # real error rates (the walk leaves the diagonal often)
    for L in (33, 50, 64, 71, 78):
        a = KC.rand_seq(rng, L)
        out.append((a, (KC.mutate(rng, a, 0.10) or 'A')[:LIMIT - L], 'err%d' % L))
    assert all(t and q and len(t) + len(q) <= LIMIT for t, q, _ in out)
    # X and Y of one row: lengths that differ by 1, 2, 3, 4 anti-diagonals and by several blocks — a batch of two is one task whose row 0 holds both; a batch
    # of one is a row with X only
    pairs = []
    for delta in (1, 2, 3, 4, 5, 9, 22, 51):
        tx, qx = sized(rng, 40, 40)
        ty, qy = sized(rng, 40 + delta // 2, 40 + delta - delta // 2)
        pairs.append([(tx, qx, 'pair0 +%d' % delta), (ty, qy, 'pair1 +%d' % delta)])
    pairs.append([(pairs[0][0][0], pairs[0][0][1], 'X only')])
    # eight problems of one width that differ in length: one task, four rows of unequal pairs
    eight = [sized(rng, 30 + 3 * i, 30 + 2 * i) + ('eight%d' % i,) for i in range(8)]
    return out, pairs + [eight]


def packed_order(items):
    """shortest next to longest: the traceback spaces lie back to back in one pool in this order, so a store past the end of a problem's space lands in the
    first block of a much longer or much shorter neighbour"""
    srt = sorted(items, key=lambda x: len(x[0]) + len(x[1]))
    out = []
    while srt:
        out.append(srt.pop(0))
        if srt:
            out.append(srt.pop())
    return out


@functools.lru_cache(maxsize=None)
def expected(O, pct, eqx):
    """the oracle's (cigar, score) for every problem of problems(pct), computed once"""
    big, groups = problems(pct)
    return {(t, q): O.k_cigar_global(t, q, eqx=eqx, **SCORE) for t, q, _ in list(big) + [x for grp in groups for x in grp]}


def check_batch(ctx, O, items, pct, eqx):
    exp = expected(O, pct, eqx)
    ts = [x[0] for x in items]; qs = [x[1] for x in items]
    cg, flag, st = ctx.k_cigar_batch_banded(ts, qs, eqx=eqx)
    cg0, sc0 = ctx.k_cigar_batch(ts, qs, eqx=eqx)
    for i, (t, q, tag) in enumerate(items):
        ecg, esc = exp[(t, q)]
        where = (tag, len(t), len(q), int(flag[i]), pct, eqx)
        assert cg[i] == ecg, where
        assert cg0[i] == ecg and int(sc0[i]) == esc, where
        assert cigar_score(t, q, cg[i]) == esc, where
    return [int(f) for f in flag]


def check(ctx, O, monkeypatch):
    """every case at every band width; returns {ns: problems kept from a band of that width}"""
    kept = {}
    for pct in PCTS:
        monkeypatch.setenv('VMX_AD_PCT', str(pct))
        big, groups = problems(pct)
        flags = check_batch(ctx, O, packed_order(big), pct, eqx=False)
        flags += check_batch(ctx, O, packed_order(big)[::-1], pct, eqx=True)
        for grp in groups:
            flags += check_batch(ctx, O, grp, pct, eqx=False)
        for f in flags:
            if f > 16:
                kept[f - 16] = kept.get(f - 16, 0) + 1
        # the band's bytes are what the walk read for most of them: these problems are proven outright or by a wide margin
        assert sum(1 for f in flags if f > 16) * 10 >= 8 * len(flags), (pct, sum(1 for f in flags if f > 16), len(flags))
    assert set(kept) == {1, 2, 3, 4}, kept      # slot widths 1, 2, 4 and both 4-byte instances
    return kept


def layout_offsets(ss, ls, W, AB=4):
    """byte offset of lane l's slot on anti-diagonal s for W-byte slots (NumPy statement of vmx_ad_tb_off): 64-byte lines of AB anti-diagonals x 16 / W lanes, a
    lane's AB slots side by side"""
    s = np.asarray(ss, dtype=np.int64)[:, None]; l = np.asarray(ls, dtype=np.int64)[None, :]
    wsh = {1: 0, 2: 1, 4: 2}[W]
    lsh = {1: 6, 4: 4, 8: 3}[AB]
    lanes_per_line = 1 << (lsh - wsh)
    return (s // AB) * ((AB * 16) << wsh) + (l // lanes_per_line) * 64 + (l % lanes_per_line) * (AB << wsh) + ((s % AB) << wsh)
