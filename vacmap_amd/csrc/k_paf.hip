// k_paf.hip — PAF lines on the device: what emit_read_paf() of vmx_sam.hip computes, byte for byte ("PAF").
//
//   k_paf_lines   one wavefront per line slot, run twice (sizes, then bytes) with the scan of the line sizes in between, in the place k_sam_lines and
//                 k_sam_unmapped take in a SAM call. Blocks [0, n_recs) are record lines, blocks [n_recs, n_recs + n_reads) (keep_unmapped only) the
//                 reads' own slots. Everything else of a call is the SAM emitter's: k_sam_count, k_sam_order, both passes of k_sam_ops, the slot
//                 layout, k_sam_text_off.
//
// What PAF adds per record is read off the merged CIGAR text that the write pass of k_sam_ops stored (an earlier launch): alen, the sum of the
// M = X I D lengths, and the byte range of cg, the text between its leading and its trailing maximal run of S / H operators. The size pass finds
// them (paf_walk) and stores them per emitted position; the write pass loads them (another launch) and repeats the line's arithmetic.
//
// ORDERING. As in k_sam.hip: no load of a byte that the same launch stored. The merged text, MD, cs, rinfo, rflag: k_sam_ops; ord, mq: k_sam_order;
// toff, loff: scans between launches; pinfo: the size pass of this kernel, loaded by its write pass only.
// BOUNDS. Reads of the merged text: indices < cig_len of the record, which is what k_sam_ops wrote at toff[p]; the look-back for an operator's
// count stops at the text's byte 0. cg is [a, b) with 0 <= a < b <= cig_len by construction (both are 1 + the index of an operator byte, and a is taken
// from an operator below the one b is taken from). Writes: the write pass repeats the size pass on the same inputs inside [loff[slot], loff[slot + 1]).
#include "vmx_sam_dev.h"
#include "k_sam_out.h"

// alen and the cg range [a, b) of a merged CIGAR text, 64 bytes per step. The clip runs are found by ballots: `lead` follows the last S / H operator
// as long as no other operator has been met, `end` the last other operator; both are exact for runs of any length, and no lane walks the text alone.
// An operator's count is read by its own lane from the digits before it (merged counts are sums of counts below 2^31: at most 19 digits).
__device__ __forceinline__ void paf_walk(const char* cig, int64_t len, int lane, int64_t& a, int64_t& b, int64_t& alen) {
    int64_t lead = 0, end = 0; bool body = false; unsigned long long al = 0;
    for (int64_t base = 0; base < len; base += 64) {
        const int64_t i = base + lane;
        const int c = i < len ? (int)(unsigned char)cig[i] : '0';
        const bool isop = i < len && !(c >= '0' && c <= '9');
        const bool clip = isop && (c == 'S' || c == 'H');
        const unsigned long long om = __ballot(isop), cm = __ballot(clip), bm = om & ~cm;
        if (!body) {
            const unsigned long long lc = bm ? cm & ((bm & (0ull - bm)) - 1ull) : cm;      // the clips below the step's first other operator
            if (lc) lead = base + sam_top(lc) + 1;
            if (bm) body = true;
        }
        if (bm) end = base + sam_top(bm) + 1;
        if (isop && (c == 'M' || c == '=' || c == 'X' || c == 'I' || c == 'D')) {
            unsigned long long num = 0, mul = 1;
            for (int64_t k = i - 1; k >= 0 && k >= i - 19; --k) {
                const int d = (int)(unsigned char)cig[k];
                if (d < '0' || d > '9') break;
                num += (unsigned long long)(d - '0') * mul; mul *= 10;
            }
            al += num;
        }
    }
    alen = vmx_wave_sum_i64((long long)al);
    a = body ? lead : 0; b = body ? end : 0;
}

#define PAF_UNMAPPED_COLS "\t0\t0\t*\t*\t0\t0\t0\t0\t0\t0\n"

template <bool W>
__device__ __forceinline__ void paf_line(const vmx_sam_in& A, const vmx_sam_work& K, int64_t* pinfo, int64_t p, int lane, char* text) {
    const vm_record rec = A.recs[K.ord[p]];
    const int64_t r = rec.read_idx;
    const int64_t sl = vmx_sam_slot(A, p, r);
    if ((A.status && A.status[r] != 0) || K.rflag[r]) { if (!W && lane == 0) K.lsz[sl] = 0; return; }
    const int64_t qlen = A.seq_off[r + 1] - A.seq_off[r];
    const vmx_sam_rinfo ri = K.ri[p];
    const char* cig = K.scratch + K.toff[p];
    int64_t ca, cb, alen;
    if (W) { ca = pinfo[3 * p]; cb = pinfo[3 * p + 1]; alen = pinfo[3 * p + 2]; }
    else {
        paf_walk(cig, ri.cig_len, lane, ca, cb, alen);
        if (lane == 0) { pinfo[3 * p] = ca; pinfo[3 * p + 1] = cb; pinfo[3 * p + 2] = alen; }
    }
    const bool fwd = rec.strand == 1;
    SamOut<W> O{W ? text + K.loff[sl] : nullptr, 0, lane};
    O.bytes(A.names + (A.name_off[r] - A.name_base), A.name_off[r + 1] - A.name_off[r]); O.ch('\t');
    O.num(qlen); O.ch('\t');
    O.num(fwd ? rec.q_st : qlen - rec.q_en); O.ch('\t');
    O.num(fwd ? rec.q_en : qlen - rec.q_st); O.ch('\t');
    O.ch(fwd ? '+' : '-'); O.ch('\t');
    O.bytes(A.cnames + A.cname_off[rec.contig], A.cname_off[rec.contig + 1] - A.cname_off[rec.contig]); O.ch('\t');
    O.num(A.coff[rec.contig + 1] - A.coff[rec.contig]); O.ch('\t');
    O.num(rec.r_st); O.ch('\t');
    O.num(rec.r_en); O.ch('\t');
    O.num(alen - ri.nm); O.ch('\t');
    O.num(alen); O.ch('\t');
    O.num(K.mq[p]);
    O.bytes("\ttp:A:P\tNM:i:", 13); O.num(ri.nm);
    if (cb > ca) { O.bytes("\tcg:Z:", 6); O.bytes(cig + ca, cb - ca); }
    if (A.md) { O.bytes("\tMD:Z:", 6); O.bytes(cig + ri.cig_len, ri.md_len); O.bytes("\tcs:Z:", 6); O.bytes(cig + ri.cig_len + ri.md_len, ri.cs_len); }
    O.ch('\n');
    if (!W && lane == 0) K.lsz[sl] = O.pos;
}

// keep_unmapped: the line of a read that emits no record line, in the read's own slot (k_sam_unmapped's rule for which reads those are)
template <bool W>
__device__ __forceinline__ void paf_unmapped(const vmx_sam_in& A, const vmx_sam_work& K, int64_t r, int lane, char* text) {
    const int64_t sl = vmx_sam_slot(A, K.first[r + 1], r);
    const bool none = (A.status && A.status[r] != 0) || K.first[r + 1] == K.first[r] || K.rflag[r];
    if (!none) { if (!W && lane == 0) K.lsz[sl] = 0; return; }
    SamOut<W> O{W ? text + K.loff[sl] : nullptr, 0, lane};
    O.bytes(A.names + (A.name_off[r] - A.name_base), A.name_off[r + 1] - A.name_off[r]); O.ch('\t');
    O.num(A.seq_off[r + 1] - A.seq_off[r]);
    O.bytes(PAF_UNMAPPED_COLS, (int64_t)sizeof(PAF_UNMAPPED_COLS) - 1);
    if (!W && lane == 0) K.lsz[sl] = O.pos;
}

__global__ void __launch_bounds__(64) k_paf_lines(vmx_sam_in A, vmx_sam_work K, int64_t* pinfo, char* text, int write) {
    const int lane = (int)threadIdx.x;
    const int64_t p = blockIdx.x;
    if (K.res[0] & VMX_SAM_E_RECORD) return;
    if (p < A.n_recs) { if (write) paf_line<true>(A, K, pinfo, p, lane, text); else paf_line<false>(A, K, pinfo, p, lane, text); return; }
    const int64_t r = p - A.n_recs;
    if (!A.keep_unmapped || r >= A.n_reads) return;
    if (write) paf_unmapped<true>(A, K, r, lane, text); else paf_unmapped<false>(A, K, r, lane, text);
}
