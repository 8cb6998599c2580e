// k_sam.hip — SAM lines on the device: what emit_read() of vmx_sam.hip computes, byte for byte.
//
//   k_sam_count / k_sam_order   records per read (the host scans them into first[]); per read: reassign_mapq, the emitted order (span descending,
//                               the later record first among equals), FLAG and the MAPQ as written. One work-item per read.
//   k_sam_ops                   one wavefront per record, run twice (sizes, then bytes): the raw CIGAR text is tokenised 64 bytes per step, equal
//                               neighbours are merged by a segmented sum that carries from step to step, and every batch of up to 64 merged operators
//                               is handled by the wave at once: merged text, query / reference prefix sums, NM, MD and cs.
//   k_sam_lines                 one wavefront per record line, run twice (sizes, then bytes), with the scan of the line sizes in between. The
//                               read's comment (FASTA / FASTQ comment, uBAM tags as text) is filtered and appended by the same wave (sam_comment).
//   k_sam_unmapped              vm_sam_opts.keep_unmapped only: one wavefront per read, run twice beside k_sam_lines; the FLAG 4 line of a read that
//                               emits no record line, in the read's own line slot, so that one scan lays out both kinds of line in read order.
//
// ORDERING. Lanes hand data to one another through ballots, shuffles and LDS (vmx_wave_lds_fence between an LDS store and another lane's load:
// workgroups are one wavefront). No kernel here loads a global byte that the same launch stored: the merged text, MD and cs that k_sam_lines
// copies were written by an earlier launch of k_sam_ops, the orders by k_sam_order, the offsets by the scans in between.
// BOUNDS. Reads: every query index is checked against the read's length and every reference index against the clamped slice [ta, tb) of the
// contig, as the host's T() / Q() / tslice do (a failed check is the host's Raise and sets the read's flag). Writes: the write pass repeats the
// size pass's arithmetic on the same inputs, and its offsets are the exclusive scans of those sizes.
#include "vmx_sam_dev.h"
#include "k_sam_out.h"

#define SAM_SAT 0x80000000LL            // operator counts saturate here; reaching it is VMX_SAM_E_COUNT

__device__ __forceinline__ long long sam_scan_i64(long long v, int lane) {         // inclusive prefix sum across the wave
    for (int o = 1; o < 64; o <<= 1) { const long long x = __shfl_up(v, (unsigned)o); if (lane >= o) v += x; }
    return v;
}
__device__ __forceinline__ long long sam_get_i64(long long v, int l) { return __shfl(v, l); }
__device__ __forceinline__ void sam_put_u(char* p, unsigned long long u, int nd) { for (int k = nd - 1; k >= 0; --k) { p[k] = (char)('0' + u % 10); u /= 10; } }
__device__ __forceinline__ char sam_lo(char c) { return (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; }
__device__ __forceinline__ char sam_comp(char c) {
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        default: return c;
    }
}
__device__ __forceinline__ char sam_base(uint8_t code) { return (char)((0x4e54474341ull >> (8 * (code < 4 ? code : 4))) & 0xff); }      // "ACGTN"
__device__ __forceinline__ int64_t sam_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ int64_t sam_slice(int64_t a, int64_t n, int64_t len) { const int64_t b = a + n; return (b > len ? len : b) - (a > len ? len : a); }

// the read as the record's strand sees it
struct SamRead { const char* s; int64_t len; bool rev; };
__device__ __forceinline__ char sam_q(const SamRead& R, int64_t i) { return R.rev ? sam_comp(R.s[R.len - 1 - i]) : R.s[i]; }

// ------------------------------------------------------------------------------------------------ records per read, order
__global__ void __launch_bounds__(256) k_sam_count(vmx_sam_in A, vmx_sam_work K) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_recs) return;
    const vm_record& r = A.recs[i];
    if (r.read_idx < 0 || r.read_idx >= A.n_reads || r.contig < 0 || r.contig >= A.nseq || r.cigar_off < 0 || r.cigar_len < 0 || r.cigar_off + r.cigar_len > A.cigars_len ||
        (i > 0 && A.recs[i - 1].read_idx > r.read_idx)) { atomicOr(K.res, (unsigned long long)VMX_SAM_E_RECORD); return; }
    atomicAdd((unsigned long long*)&K.cnt[r.read_idx], 1ull);
}

__global__ void __launch_bounds__(256) k_sam_order(vmx_sam_in A, vmx_sam_work K) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= A.n_reads || (K.res[0] & VMX_SAM_E_RECORD)) return;
    const int64_t f = K.first[r], n = K.first[r + 1] - f;
    if (n <= 0) return;
    const vm_record* R = A.recs + f;
    if (A.markunbalancetra) {                                            // reassign_mapq: the records that stay on the walk keep their MAPQ
        for (int64_t i = 0; i < n; ++i) K.keep[f + i] = 0;
        K.keep[f] = 1;
        int64_t last = 0;
        while (last < n - 1) {
            const int64_t i = last; const vm_record b = R[i];
            bool hit = false; int64_t t = i;
            while (t + 1 < n) {
                ++t; const vm_record& x = R[t];
                if (x.contig != b.contig) continue;
                const int64_t refgap = x.strand == 1 ? x.r_st - b.r_en : b.r_st - x.r_en;
                if ((refgap < 0 ? -refgap : refgap) > 100000) continue;
                if (refgap < 10) { last = t; hit = true; break; }
            }
            if (!hit) last = i + 1;
            K.keep[f + last] = 1;
        }
    }
    for (int64_t i = 0; i < n; ++i) {                                    // rank of record i: longer spans first, the later record first among equals
        const int64_t si = R[i].q_en - R[i].q_st;
        int64_t rank = 0;
        for (int64_t k = 0; k < n; ++k) { const int64_t sk = R[k].q_en - R[k].q_st; rank += (sk > si || (sk == si && k > i)) ? 1 : 0; }
        K.ord[f + rank] = (int32_t)(f + i);
        K.mq[f + rank] = (A.markunbalancetra && !K.keep[f + i]) ? 0 : R[i].mapq;
    }
    const int64_t primary = (A.asm_mode && n > 1 && K.mq[f] == 1 && K.mq[f + 1] != 1) ? 1 : 0;
    for (int64_t j = 0; j < n; ++j) {
        const int v = K.mq[f + j];
        K.flag[f + j] = (j == primary ? 0 : 2048) + (A.recs[K.ord[f + j]].strand == 1 ? 0 : 16);
        K.mq[f + j] = A.asm_mode ? (v != 0 ? 60 : 1) : v;
    }
}

// ------------------------------------------------------------------------------------------------ merged CIGAR, NM, MD, cs
// what a record's walk carries from one batch of merged operators to the next; the same in every lane
struct SamWalk {
    int64_t qp, rp, nm;                          // nm_from_cigar's cursors and sum
    int64_t refloc, readloc, equal; int preop;   // md_cs's
    int64_t cig_pos, md_pos, cs_pos, n_ops;
    bool raised, aborted;
};

// one batch: lane i < cnt holds merged operator i (op, n). R: the read from the walk's position 0; codes: the reference slice, tl bases.
template <bool W>
__device__ __forceinline__ void sam_ops_batch(SamWalk& S, int op, int64_t n, int cnt, int lane, const vmx_sam_in& A, const SamRead& R, int64_t qoff, int64_t ql,
                                              const uint8_t* codes, int64_t tl, bool nm_walk, bool md_quiet, char* cig, char* md, char* cs) {
    const bool act = lane < cnt;
    {   // merged text
        const int nd = act ? sam_ndig((unsigned long long)n) + 1 : 0;
        const int inc = vmx_wave_incl_scan_i32(nd);
        if (W && act) { char* p = cig + S.cig_pos + (inc - nd); sam_put_u(p, (unsigned long long)n, nd - 1); p[nd - 1] = (char)op; }
        S.cig_pos += __shfl(inc, 63);
        S.n_ops += cnt;
    }
    if (nm_walk) {
        const bool q_op = act && (op == 'M' || op == '=' || op == 'X' || op == 'I' || op == 'S');
        const bool r_op = act && (op == 'M' || op == '=' || op == 'X' || op == 'D' || op == 'N');
        const long long qi = sam_scan_i64(q_op ? n : 0, lane), ri = sam_scan_i64(r_op ? n : 0, lane);
        const int64_t myq = S.qp + qi - (q_op ? n : 0), myr = S.rp + ri - (r_op ? n : 0);
        long long d = (act && (op == 'X' || op == 'I' || op == 'D')) ? n : 0;
        const bool isM = act && op == 'M';
        const bool bad = isM && (myq + n > ql || myr + n > tl);
        if (__ballot(bad)) S.raised = true;
        unsigned long long mm = __ballot(isM && !bad);
        while (mm) {                                                     // an M run: 64 columns per step
            const int l = __ffsll((long long)mm) - 1; mm &= mm - 1;
            const int64_t bq = sam_get_i64(myq, l), br = sam_get_i64(myr, l), bn = sam_get_i64(n, l);
            for (int64_t x = lane; x < bn; x += 64) d += (((sam_q(R, qoff + bq + x) ^ sam_base(codes[br + x])) & 0xDF) != 0) ? 1 : 0;
        }
        S.nm += vmx_wave_sum_i64(d);
        S.qp += sam_get_i64(qi, 63); S.rp += sam_get_i64(ri, 63);
    }
    if (!A.md) return;
    const bool isX = op == 'X', isE = op == '=', isD = op == 'D', isI = op == 'I', isSH = op == 'S' || op == 'H';
    const unsigned long long am = __ballot(act && !(isX || isE || isD || isI || isSH));
    const int first_abort = am ? __ffsll((long long)am) - 1 : 64;
    const bool v = act && lane < first_abort && !S.aborted;             // the operators md_cs reaches
    const long long rinc = sam_scan_i64(v && (isX || isE || isD) ? n : 0, lane), qinc = sam_scan_i64(v && (isX || isE || isI) ? n : 0, lane);
    const int64_t refloc = S.refloc + rinc - (v && (isX || isE || isD) ? n : 0), readloc = S.readloc + qinc - (v && (isX || isE || isI) ? n : 0);
    const long long e = v && isE ? n : 0;
    const long long einc = sam_scan_i64(e, lane);
    const unsigned long long rm = __ballot(v && (isX || isD)), rbelow = rm & sam_lt(lane);
    const long long ebase = sam_get_i64(einc, rbelow ? sam_top(rbelow) : 0);
    const int64_t equal = rbelow ? (einc - e) - ebase : S.equal + (einc - e);
    const unsigned long long pm = __ballot(v && (isX || isE || isD)), pbelow = pm & sam_lt(lane);
    const int pv = __shfl(op, pbelow ? sam_top(pbelow) : 0);
    const int preop = pbelow ? pv : S.preop;
    // sizes of this operator's pieces: header (by its lane) and content (cols columns; by its lane when short, by the wave otherwise)
    int64_t cols = 0; int md_h = 0, cs_h = 0; int64_t md_sz = 0, cs_sz = 0; int pre = 0;
    bool xbad = false;
    if (v && isX) {
        cols = n > 0 ? n : 1;
        xbad = refloc + cols > tl || readloc + cols > ql;
        pre = equal > 0 ? sam_ndig((unsigned long long)equal) : (preop == 'D' ? 1 : 0);
        md_h = pre; md_sz = pre + 1 + 2 * (cols - 1); cs_sz = 3 * cols;
    } else if (v && isE) {
        if (A.shortcs) { cs_h = 1 + sam_ndig((unsigned long long)n); cs_sz = cs_h; } else { cols = sam_slice(refloc, n, tl); cs_h = 1; cs_sz = 1 + cols; }
    } else if (v && isD) {
        cols = sam_slice(refloc, n, tl);
        pre = equal > 0 ? sam_ndig((unsigned long long)equal) : (preop == 'X' ? 1 : 0);
        md_h = pre + 1; md_sz = md_h + cols; cs_h = 1; cs_sz = 1 + cols;
    } else if (v && isI) { cols = sam_slice(readloc, n, ql); cs_h = 1; cs_sz = 1 + cols; }
    if (__ballot(xbad)) S.raised = true;
    const long long minc = sam_scan_i64(md_sz, lane), cinc = sam_scan_i64(cs_sz, lane);
    if (W && !md_quiet && !S.raised) {
        char* mp = md + S.md_pos + (minc - md_sz); char* cp = cs + S.cs_pos + (cinc - cs_sz);
        const int64_t ra = refloc > tl ? tl : refloc, qa = readloc > ql ? ql : readloc;      // tslice's clamped start (X never starts past the end here: xbad)
        if (v && (isX || isD)) { if (equal > 0) sam_put_u(mp, (unsigned long long)equal, pre); else if (pre) mp[0] = '0'; }
        if (v && isD) { mp[pre] = '^'; cp[0] = '-'; }
        if (v && isE) { if (A.shortcs) { cp[0] = ':'; sam_put_u(cp + 1, (unsigned long long)n, cs_h - 1); } else cp[0] = '='; }
        if (v && isI) cp[0] = '+';
        const bool wide = cols > 8;
        if (v && !wide && !(isE && A.shortcs)) {
            for (int64_t j = 0; j < cols; ++j) {
                if (isX) { const char t = sam_base(codes[ra + j]); if (j) mp[md_h + 2 * j - 1] = '0'; mp[md_h + 2 * j] = t; cp[3 * j] = '*'; cp[3 * j + 1] = sam_lo(t); cp[3 * j + 2] = sam_lo(sam_q(R, qoff + qa + j)); }
                else if (isD) { const char t = sam_base(codes[ra + j]); mp[md_h + j] = t; cp[1 + j] = sam_lo(t); }
                else if (isE) cp[1 + j] = sam_base(codes[ra + j]);
                else if (isI) cp[1 + j] = sam_lo(sam_q(R, qoff + qa + j));
            }
        }
        unsigned long long wm = __ballot(v && wide && !(isE && A.shortcs));
        while (wm) {                                                     // long pieces: all lanes, 64 columns per step
            const int l = __ffsll((long long)wm) - 1; wm &= wm - 1;
            const int bop = __shfl(op, l), bh = __shfl(md_h, l);
            const int64_t bc = sam_get_i64(cols, l), bra = sam_get_i64(ra, l), bqa = sam_get_i64(qa, l);
            char* bm = md + S.md_pos + sam_get_i64(minc - md_sz, l); char* bcs = cs + S.cs_pos + sam_get_i64(cinc - cs_sz, l);
            for (int64_t j = lane; j < bc; j += 64) {
                if (bop == 'X') { const char t = sam_base(codes[bra + j]); if (j) bm[bh + 2 * j - 1] = '0'; bm[bh + 2 * j] = t; bcs[3 * j] = '*'; bcs[3 * j + 1] = sam_lo(t); bcs[3 * j + 2] = sam_lo(sam_q(R, qoff + bqa + j)); }
                else if (bop == 'D') { const char t = sam_base(codes[bra + j]); bm[bh + j] = t; bcs[1 + j] = sam_lo(t); }
                else if (bop == '=') bcs[1 + j] = sam_base(codes[bra + j]);
                else bcs[1 + j] = sam_lo(sam_q(R, qoff + bqa + j));
            }
        }
    }
    S.md_pos += sam_get_i64(minc, 63); S.cs_pos += sam_get_i64(cinc, 63);
    S.refloc += sam_get_i64(rinc, 63); S.readloc += sam_get_i64(qinc, 63);
    S.equal = rm ? sam_get_i64(einc, 63) - sam_get_i64(einc, sam_top(rm)) : S.equal + sam_get_i64(einc, 63);
    if (pm) S.preop = __shfl(op, sam_top(pm));
    if (am) S.aborted = true;
}

template <bool W>
__device__ __forceinline__ void sam_ops_record(const vmx_sam_in& A, const vmx_sam_work& K, int64_t p, int lane, char* s_txt, int* s_op, long long* s_n) {
    const vm_record rec = A.recs[K.ord[p]];
    const int64_t r = rec.read_idx;
    vmx_sam_rinfo& RI = K.ri[p];
    if (A.status && A.status[r] != 0) { if (!W && lane == 0) { RI = vmx_sam_rinfo{0, 0, 0, 0, 0, 0, 0}; K.tsz[p] = 0; } return; }
    int flags0 = 0;
    if (W) { flags0 = RI.flags; if (flags0 & VMX_SAM_F_RAISED) return; }
    const int64_t qlen = A.seq_off[r + 1] - A.seq_off[r];
    const SamRead R{A.seqs + (A.seq_off[r] - A.seq_base), qlen, rec.strand != 1};
    const int64_t clen = A.coff[rec.contig + 1] - A.coff[rec.contig];
    const int64_t ta = sam_clamp(rec.r_st, clen); int64_t tb = sam_clamp(rec.r_en, clen); if (tb < ta) tb = ta;
    const uint8_t* codes = A.codes + A.coff[rec.contig] + ta; const int64_t tl = tb - ta;
    int64_t qoff = 0, ql = qlen;
    if (A.md) { const int64_t qa = sam_clamp(rec.q_st, qlen); int64_t qb = sam_clamp(rec.q_en, qlen); if (qb < qa) qb = qa; qoff = qa; ql = qb - qa; }
    const bool nm_walk = !A.asm_mode;
    const bool md_quiet = W && (flags0 & VMX_SAM_F_ABORTED);            // both strings are empty: nothing of them is stored
    char* cig = W ? K.scratch + K.toff[p] : nullptr;
    char* md = W ? cig + RI.cig_len : nullptr; char* cs = W ? md + RI.md_len : nullptr;
    SamWalk S{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, false, false};
    const char* text = A.cigars + rec.cigar_off; const int64_t len = rec.cigar_len;
    int cur_op = 0; long long cur_n = 0, carry_num = 0, nm_asm = 0;
    bool count_err = false, flushed = false;
    for (int64_t base = 0;; base += 64) {
        int op = 0; long long n = 0; int nrun = 0;
        if (base < len) {
            const int64_t i = base + lane;
            const int c = i < len ? (int)(unsigned char)text[i] : '0';
            const bool isop = i < len && !(c >= '0' && c <= '9');
            vmx_wave_lds_fence();                                        // (the last step's readers are done with the LDS arrays)
            s_txt[lane] = (char)c;
            vmx_wave_lds_fence();
            const unsigned long long om = __ballot(isop);
            long long num = 0;
            if (isop) {                                                  // the digits between the operator before this one and this one
                const unsigned long long below = om & sam_lt(lane);
                int k = below ? sam_top(below) + 1 : 0;
                num = below ? 0 : carry_num;
                for (; k < lane; ++k) { num = num * 10 + (s_txt[k] - '0'); if (num >= SAM_SAT) num = SAM_SAT; }
            }
            if (__ballot(isop && num >= SAM_SAT)) count_err = true;
            {   // digits behind the step's last operator belong to the next step's first
                const int nvalid = len - base < 64 ? (int)(len - base) : 64;
                int k = om ? sam_top(om) + 1 : 0;
                if (om) carry_num = 0;
                for (; k < nvalid; ++k) { carry_num = carry_num * 10 + (s_txt[k] - '0'); if (carry_num >= SAM_SAT) carry_num = SAM_SAT; }
            }
            const int cnt = __popcll(om);
            if (cnt) {
                if (isop) { const int rank = __popcll(om & sam_lt(lane)); s_op[rank] = c; s_n[rank] = num; }
                vmx_wave_lds_fence();
                const int t_op = lane < cnt ? s_op[lane] : 0; const long long t_n = lane < cnt ? s_n[lane] : 0;
                int prev = __shfl_up(t_op, 1u); if (lane == 0) prev = cur_op;
                const bool head = lane < cnt && t_op != prev;
                nm_asm += vmx_wave_sum_i64(head && (t_op == 'X' || t_op == 'D' || t_op == 'I') ? t_n : 0);
                const unsigned long long hm = __ballot(head), hle = hm & (sam_lt(lane) | (1ull << lane));
                const long long P = sam_scan_i64(t_n, lane);
                const long long pex = sam_get_i64(P - t_n, hle ? sam_top(hle) : 0);
                const long long seg = hle ? P - pex : cur_n + P;         // the run's sum up to this token, what earlier steps carried included
                const bool end = lane + 1 < cnt && ((hm >> (lane + 1)) & 1ull);
                const unsigned long long em = __ballot(end);
                const int carried_done = (cur_op != 0 && (hm & 1ull)) ? 1 : 0;
                vmx_wave_lds_fence();                                    // (every lane has read its token)
                if (carried_done && lane == 0) { s_op[0] = cur_op; s_n[0] = cur_n; }
                if (end) { const int slot = carried_done + __popcll(em & sam_lt(lane)); s_op[slot] = t_op; s_n[slot] = seg; }
                vmx_wave_lds_fence();
                nrun = carried_done + __popcll(em);
                cur_op = __shfl(t_op, cnt - 1); cur_n = sam_get_i64(seg, cnt - 1);
                if (lane < nrun) { op = s_op[lane]; n = s_n[lane]; }
            }
        } else if (!flushed) {
            flushed = true;
            if (cur_op) { nrun = 1; if (lane == 0) { op = cur_op; n = cur_n; } }
        } else break;
        if (nrun) sam_ops_batch<W>(S, op, n, nrun, lane, A, R, qoff, ql, codes, tl, nm_walk, md_quiet, cig, md, cs);
    }
    if (A.md && !S.aborted && S.equal > 0) {                             // the trailing match count of MD
        const int nd = sam_ndig((unsigned long long)S.equal);
        if (W && !md_quiet && !S.raised && lane == 0) sam_put_u(md + S.md_pos, (unsigned long long)S.equal, nd);
        S.md_pos += nd;
    }
    if (W) return;
    if (lane == 0) {
        const bool ab = A.md && S.aborted;
        RI.cig_len = S.cig_pos; RI.md_len = (A.md && !ab) ? S.md_pos : 0; RI.cs_len = (A.md && !ab) ? S.cs_pos : 0; RI.n_ops = S.n_ops;
        RI.nm = A.asm_mode ? nm_asm : S.nm; RI.flags = (S.raised ? VMX_SAM_F_RAISED : 0) | (ab ? VMX_SAM_F_ABORTED : 0); RI.pad = 0;
        K.tsz[p] = S.raised ? 0 : RI.cig_len + RI.md_len + RI.cs_len;
        if (S.raised) atomicOr(&K.rflag[r], 1);
        if (count_err) atomicOr(K.res, (unsigned long long)VMX_SAM_E_COUNT);
    }
}

__global__ void __launch_bounds__(64) k_sam_ops(vmx_sam_in A, vmx_sam_work K, int write) {
    __shared__ char s_txt[64];
    __shared__ int s_op[64];
    __shared__ long long s_n[64];
    const int lane = (int)threadIdx.x;
    const int64_t p = blockIdx.x;
    if (p >= A.n_recs || (K.res[0] & VMX_SAM_E_RECORD)) return;
    if (write) sam_ops_record<true>(A, K, p, lane, s_txt, s_op, s_n);
    else sam_ops_record<false>(A, K, p, lane, s_txt, s_op, s_n);
}

// ------------------------------------------------------------------------------------------------ lines
// (SamOut, the line under construction: k_sam_out.h)

template <bool W> __device__ __forceinline__ void sam_fake_cigar(SamOut<W>& O, const vm_record& y, int64_t qlen, char clip) {
    if (y.q_st > 0) { O.num(y.q_st); O.ch(clip); }
    const int64_t diff = y.q_en - y.q_st - y.r_en + y.r_st;
    if (diff > 0) { O.num(y.r_en - y.r_st); O.ch('M'); O.num(diff); O.ch('I'); }
    else if (diff < 0) { O.num(y.q_en - y.q_st); O.ch('M'); O.num(-diff); O.ch('D'); }
    else { O.num(y.q_en - y.q_st); O.ch('M'); }
    if (qlen - y.q_en > 0) { O.num(qlen - y.q_en); O.ch(clip); }
}

// ---- the read's comment (emit_read()'s rule, mammap_clrnano.py:20686): the tab-separated fields of shape XX:T:value whose tag the line does not
// carry yet. One field at a time, wave-uniform state; inside a field the wave works 64 bytes per step.
// The field that begins at p: e = its end (the next tab, or L), colons = its ':' count (3 = three or more), head = bytes 2 and 4 are ':',
// tag = bytes 0-1 packed, type = byte 3 (the last three mean something only under head). Loads: i < L only; beyond L a lane holds a tab.
__device__ __forceinline__ void sam_field(const char* com, int64_t L, int64_t p, int lane, int64_t& e, int& colons, bool& head, int& tag, int& type) {
    colons = 0;
    for (int64_t base = p;; base += 64) {
        const int64_t i = base + lane;
        const int c = i < L ? (int)(unsigned char)com[i] : '\t';
        const unsigned long long tm = __ballot(c == '\t');
        const unsigned long long cm = __ballot(c == ':') & (tm ? (tm & (0ull - tm)) - 1ull : ~0ull);      // the colons before the field's end
        if (base == p) { head = (cm & 0x14ull) == 0x14ull; tag = __shfl(c, 0) | (__shfl(c, 1) << 8); type = __shfl(c, 3); }
        colons += __popcll(cm); if (colons > 3) colons = 3;
        if (tm) { e = base + (__ffsll((long long)tm) - 1); return; }    // (base + 63 >= L makes tm non-zero: e <= L)
    }
}
__device__ __forceinline__ bool sam_com_type(int t) { return t == 'A' || t == 'i' || t == 'f' || t == 'Z' || t == 'H' || t == 'B'; }
#define SAM_TAG(a, b) ((int)(a) | ((int)(b) << 8))

// A field qualifies by its own bytes and the line's tags; it is kept when no earlier qualifying field of the comment has its tag (only kept
// fields enter the host's `seen`, and the first qualifying field of a tag is always kept). Lane k holds the k-th kept tag, compared by ballot;
// beyond 64 kept tags the fields behind the 64th kept one are walked again (exact for any number of tags).
template <bool W>
__device__ __forceinline__ void sam_comment(SamOut<W>& O, const char* com, int64_t L, bool t_rg, bool t_cg, int lane) {
    int mine = -1, nkept = 0; int64_t p64 = 0;
    for (int64_t p = 0; p <= L;) {
        int64_t e; int colons, tag, type; bool head;
        sam_field(com, L, p, lane, e, colons, head, tag, type);
        const bool fixed = tag == SAM_TAG('S', 'A') || tag == SAM_TAG('N', 'M') || tag == SAM_TAG('M', 'D') || tag == SAM_TAG('c', 's') ||
                           (tag == SAM_TAG('R', 'G') && t_rg) || (tag == SAM_TAG('C', 'G') && t_cg);
        if (head && colons == 2 && sam_com_type(type) && !fixed) {
            bool dup = __ballot(mine == tag) != 0;
            if (!dup && nkept == 64) {
                for (int64_t q = p64; q < p && !dup;) {
                    int64_t e2; int c2, tag2, type2; bool head2;
                    sam_field(com, L, q, lane, e2, c2, head2, tag2, type2);
                    dup = head2 && c2 == 2 && tag2 == tag && sam_com_type(type2);
                    q = e2 + 1;
                }
            }
            if (!dup) {
                if (nkept < 64) { if (lane == nkept) mine = tag; if (++nkept == 64) p64 = e + 1; }
                O.ch('\t'); O.bytes(com + p, e - p);
            }
        }
        p = e + 1;
    }
}

template <bool W>
__device__ __forceinline__ void sam_line(const vmx_sam_in& A, const vmx_sam_work& K, int64_t p, int lane, char* text) {
    const vm_record rec = A.recs[K.ord[p]];
    const int64_t r = rec.read_idx;
    const int64_t sl = vmx_sam_slot(A, p, r);
    if ((A.status && A.status[r] != 0) || K.rflag[r]) { if (!W && lane == 0) K.lsz[sl] = 0; return; }
    const int64_t f = K.first[r], nr = K.first[r + 1] - f;
    const int64_t qlen = A.seq_off[r + 1] - A.seq_off[r];
    const char* seq = A.seqs + (A.seq_off[r] - A.seq_base);
    const int64_t qual_len = (A.quals && A.qual_off) ? A.qual_off[r + 1] - A.qual_off[r] : 0;
    const bool has_qual = qual_len > 0 && qual_len == qlen;
    const char* qual = has_qual ? A.quals + (A.qual_off[r] - A.qual_base) : nullptr;
    const vmx_sam_rinfo ri = K.ri[p];
    const char* cig = K.scratch + K.toff[p];
    const bool cg = 2 * ri.n_ops > 65535 && A.cigar2cg;
    const bool rev = rec.strand != 1;
    const char clip = A.hardclip ? 'H' : 'S';
    SamOut<W> O{W ? text + K.loff[sl] : nullptr, 0, lane};
    O.bytes(A.names + (A.name_off[r] - A.name_base), A.name_off[r + 1] - A.name_off[r]); O.ch('\t');
    O.num(K.flag[p]); O.ch('\t');
    O.bytes(A.cnames + A.cname_off[rec.contig], A.cname_off[rec.contig + 1] - A.cname_off[rec.contig]); O.ch('\t');
    O.num(rec.r_st + 1); O.ch('\t');
    O.num(K.mq[p]); O.ch('\t');
    if (cg) O.ch('*'); else O.bytes(cig, ri.cig_len);
    O.bytes("\t*\t0\t0\t", 7);
    int64_t a = 0, b = qlen;
    if (A.hardclip) { a = sam_clamp(rec.q_st, qlen); b = sam_clamp(rec.q_en, qlen); if (b < a) b = a; }
    if (W) {                                                             // SEQ and QUAL, 64 bytes per step
        char* ps = O.p + O.pos; char* pq = ps + (b - a) + 1;
        for (int64_t x = a + lane; x < b; x += 64) {
            ps[x - a] = rev ? sam_comp(seq[qlen - 1 - x]) : seq[x];
            if (has_qual) pq[x - a] = rev ? qual[qlen - 1 - x] : qual[x];
        }
    }
    O.pos += b - a; O.ch('\t');
    if (has_qual) O.pos += b - a; else O.ch('*');
    if (A.rg) { O.bytes("\tRG:Z:", 6); O.bytes(A.rg, A.rg_len); }
    if (cg) { O.bytes("\tCG:Z:", 6); O.bytes(cig, ri.cig_len); }
    if (nr > 1) {
        O.bytes("\tSA:Z:", 6);
        for (int64_t x = 0; x < nr; ++x) {
            const int64_t px = f + x;
            if (px == p) continue;
            const vm_record y = A.recs[K.ord[px]];
            O.bytes(A.cnames + A.cname_off[y.contig], A.cname_off[y.contig + 1] - A.cname_off[y.contig]); O.ch(',');
            O.num(y.r_st + 1); O.ch(','); O.ch(y.strand == 1 ? '+' : '-'); O.ch(',');
            if (A.fakecigar) sam_fake_cigar<W>(O, y, qlen, clip); else O.bytes(K.scratch + K.toff[px], K.ri[px].cig_len);
            O.ch(','); O.num(K.mq[px]); O.ch(','); O.num(K.ri[px].nm); O.ch(';');
        }
    }
    O.bytes("\tNM:i:", 6); O.num(ri.nm);
    if (A.md) { O.bytes("\tMD:Z:", 6); O.bytes(cig + ri.cig_len, ri.md_len); O.bytes("\tcs:Z:", 6); O.bytes(cig + ri.cig_len + ri.md_len, ri.cs_len); }
    if (A.comments) {
        const int64_t cl = A.com_off[r + 1] - A.com_off[r];
        if (cl > 0) sam_comment<W>(O, A.comments + (A.com_off[r] - A.com_base), cl, A.rg != nullptr, cg, lane);
    }
    O.ch('\n');
    if (!W && lane == 0) K.lsz[sl] = O.pos;
}

__global__ void __launch_bounds__(64) k_sam_lines(vmx_sam_in A, vmx_sam_work K, char* text, int write) {
    const int lane = (int)threadIdx.x;
    const int64_t p = blockIdx.x;
    if (p >= A.n_recs || (K.res[0] & VMX_SAM_E_RECORD)) return;
    if (write) sam_line<true>(A, K, p, lane, text); else sam_line<false>(A, K, p, lane, text);
}

// ---- keep_unmapped: the line of a read that emits no record line (no record, a status other than 0, or a raise: rflag, stored by the size pass
// of k_sam_ops, an earlier launch). One wavefront per read, run twice like k_sam_lines; the line lives in the read's own slot (vmx_sam_dev.h).
// FLAG 4, MAPQ 0, the read whole and in its own orientation whatever hardclip and asm_mode say; RG and the comment as on a record line without CG.

// n bytes of a and (b != nullptr) of b to da and db, 64 bytes of each per step, four steps in flight: the eight loads are issued before the
// first store waits for its byte (few waves run here, one per unmapped read, so a copy is as long as its chain of load latencies)
__device__ __forceinline__ void sam_copy2(char* da, const char* a, char* db, const char* b, int64_t n, int lane) {
    for (int64_t x = lane; x < n; x += 256) {
        char ca[4], cb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { const bool in = x + 64 * k < n; ca[k] = in ? a[x + 64 * k] : 0; cb[k] = (in && b) ? b[x + 64 * k] : 0; }
#pragma unroll
        for (int k = 0; k < 4; ++k) if (x + 64 * k < n) { da[x + 64 * k] = ca[k]; if (b) db[x + 64 * k] = cb[k]; }
    }
}
#define SAM_UNMAPPED_COLS "\t4\t*\t0\t0\t*\t*\t0\t0\t"
template <bool W>
__device__ __forceinline__ void sam_unmapped(const vmx_sam_in& A, const vmx_sam_work& K, int64_t r, int lane, char* text) {
    const int64_t sl = vmx_sam_slot(A, K.first[r + 1], r);
    const bool none = (A.status && A.status[r] != 0) || K.first[r + 1] == K.first[r] || K.rflag[r];
    if (!none) { if (!W && lane == 0) K.lsz[sl] = 0; return; }
    const int64_t qlen = A.seq_off[r + 1] - A.seq_off[r];
    const int64_t qual_len = (A.quals && A.qual_off) ? A.qual_off[r + 1] - A.qual_off[r] : 0;
    const bool has_qual = qual_len > 0 && qual_len == qlen;
    SamOut<W> O{W ? text + K.loff[sl] : nullptr, 0, lane};
    O.bytes(A.names + (A.name_off[r] - A.name_base), A.name_off[r + 1] - A.name_off[r]);
    O.bytes(SAM_UNMAPPED_COLS, (int64_t)sizeof(SAM_UNMAPPED_COLS) - 1);
    if (qlen > 0) {                                                      // SEQ and QUAL, 64 bytes per step
        if (W) sam_copy2(O.p + O.pos, A.seqs + (A.seq_off[r] - A.seq_base), O.p + O.pos + qlen + 1, has_qual ? A.quals + (A.qual_off[r] - A.qual_base) : nullptr, qlen, lane);
        O.pos += qlen;
    } else O.ch('*');
    O.ch('\t');
    if (has_qual) O.pos += qlen; else O.ch('*');
    if (A.rg) { O.bytes("\tRG:Z:", 6); O.bytes(A.rg, A.rg_len); }
    if (A.comments) {
        const int64_t cl = A.com_off[r + 1] - A.com_off[r];
        if (cl > 0) sam_comment<W>(O, A.comments + (A.com_off[r] - A.com_base), cl, A.rg != nullptr, false, lane);
    }
    O.ch('\n');
    if (!W && lane == 0) K.lsz[sl] = O.pos;
}

__global__ void __launch_bounds__(64) k_sam_unmapped(vmx_sam_in A, vmx_sam_work K, char* text, int write) {
    const int lane = (int)threadIdx.x;
    const int64_t r = blockIdx.x;
    if (!A.keep_unmapped || r >= A.n_reads || (K.res[0] & VMX_SAM_E_RECORD)) return;
    if (write) sam_unmapped<true>(A, K, r, lane, text); else sam_unmapped<false>(A, K, r, lane, text);
}

// text_off[r] = where read r's lines begin (text_off[n_reads] = all bytes); lines and skipped reads counted as vm_sam_emit counts them
__global__ void __launch_bounds__(256) k_sam_text_off(vmx_sam_in A, vmx_sam_work K, int64_t* text_off) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > A.n_reads) return;
    if (K.res[0] & VMX_SAM_E_RECORD) { text_off[r] = 0; return; }
    text_off[r] = K.loff[vmx_sam_slot(A, K.first[r], r)];
    if (r == A.n_reads) return;
    const int64_t nr = K.first[r + 1] - K.first[r];
    const bool skipped = (A.status && A.status[r] != 0) || (nr > 0 && K.rflag[r]);
    if (skipped) atomicAdd(&K.res[2], 1ull);
    if (!skipped && nr > 0) atomicAdd(&K.res[1], (unsigned long long)nr);
    else if (A.keep_unmapped) atomicAdd(&K.res[1], 1ull);               // its unmapped line
}

__global__ void __launch_bounds__(256) k_sam_count_other(const char* in, int64_t n, unsigned long long* count) {
    unsigned long long c = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const char u = in[i] & 0xDF;
        c += !(u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'N') ? 1 : 0;
    }
    if (c) atomicAdd(count, c);
}
