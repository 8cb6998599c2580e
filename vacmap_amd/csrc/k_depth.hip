// k_depth.hip — per-window depth of coverage on the device: what depth_add_read() of vmx_sam.hip and depth_text() of vmx_depth.hip compute, count for
// count and byte for byte (vacmapx.h states the rule at vm_depth_add; DESIGN §7d, "Depth of coverage").
//
//   k_depth_add     one wavefront per emitted record, launched behind the write pass of k_sam_ops (by a stand-alone vm_depth_add_device, or by every
//                   device emit call while an accumulator is attached). The merged CIGAR text is walked 64 bytes per step as paf_walk does: a ballot
//                   of operator bytes, each operator lane reads its count from the digits in front of it, a wave prefix sum of the reference-consuming
//                   lengths gives each operator its reference start, carried from step to step. A covered run (M = X) is clamped to the contig and
//                   split at window boundaries into a head piece (its first window), a tail piece (its last window, when that is another one) and
//                   whole interior windows. Head pieces and tail pieces are each summed per window across the wave by a segmented reduction keyed by
//                   the window index (windows do not decrease along a record), and only the segment heads add. INTERIOR WINDOWS ARE SPREAD OVER THE
//                   WAVE'S LANES (no difference array, so no integrating pass and one table): lane k adds W to the k-th, (k + 64)-th ... of them.
//   k_depth_merge   dst += src (vm_depth_merge into a device accumulator).
//   k_depth_sums    per-contig sums of the counts and their total, one wavefront per slice of a contig's windows.
//   k_depth_lines   the two texts, one lane per line (a window, or a contig / the total), run twice (sizes, then bytes) with the scan in between.
//
// ORDERING. k_depth_add loads the merged text and ri (the write / size pass of k_sam_ops), ord and mq (k_sam_order), rflag (the size pass of k_sam_ops),
// toff (a scan), win_off (uploaded when the accumulator was made): all earlier launches. It loads nothing that the same launch stores: the table is
// touched by 64-bit vector atomic adds only, whose results are not used. k_depth_sums and k_depth_lines load the table in later launches.
// BOUNDS. Text reads: indices i < cig_len of the record, the bytes k_sam_ops wrote at toff[p]; the look-back for an operator's count stops at the
// text's byte 0 (and after 19 digits). Window indices: a covered run is clamped to [0, L_c) first, so a piece's window j = pos div W has
// 0 <= j <= (L_c - 1) div W < ceil(L_c / W) and the table index win_off[c] + j lies in [win_off[c], win_off[c + 1]); a run that is empty after the
// clamp adds nothing. L_c is the index's (A.coff), and the host side refuses an accumulator whose layout was made for another index.
// k_depth_lines: window i of [0, n_win) belongs to the contig c with win_off[c] <= i < win_off[c + 1] (binary search; contigs without windows are
// passed over); the write pass repeats the size pass on the same inputs inside [loff[i], loff[i + 1]).
#include "vmx_depth.h"
#include "k_sam_out.h"

__device__ __forceinline__ long long dep_scan_i64(long long v, int lane) {          // inclusive prefix sum across the wave
    for (int o = 1; o < 64; o <<= 1) { const long long x = __shfl_up(v, (unsigned)o); if (lane >= o) v += x; }
    return v;
}

// counts[key] += the sum of val over each maximal run of active lanes with the same key (keys do not decrease with the lane); one atomic per run
__device__ __forceinline__ void dep_seg_add(unsigned long long* counts, bool act, long long key, long long val, int lane) {
    const unsigned long long am = __ballot(act);
    if (!am) return;
    const unsigned long long below = am & sam_lt(lane);
    const long long pk = __shfl(key, below ? sam_top(below) : 0);
    const bool head = act && (!below || pk != key);
    const unsigned long long hm = __ballot(head);
    const long long v = act ? val : 0;
    const long long P = dep_scan_i64(v, lane);
    const unsigned long long above = (hm >> lane) >> 1;                            // the heads above this lane, bit 0 = lane + 1
    const int endl = above ? lane + (__ffsll((long long)above) - 1) : 63;          // the lane before the next head
    const long long sum = __shfl(P, endl) - (P - v);
    if (head) atomicAdd(&counts[key], (unsigned long long)sum);
}

__global__ void __launch_bounds__(64) k_depth_add(vmx_sam_in A, vmx_sam_work K, vmx_depth_dev D) {
    const int lane = (int)threadIdx.x;
    const int64_t p = blockIdx.x;
    if (p >= A.n_recs || (K.res[0] & VMX_SAM_E_RECORD)) return;
    const vm_record rec = A.recs[K.ord[p]];
    const int64_t r = rec.read_idx;
    if ((A.status && A.status[r] != 0) || K.rflag[r] || K.mq[p] < D.min_mapq) return;
    const int64_t L = A.coff[rec.contig + 1] - A.coff[rec.contig], W = D.window;
    const int64_t wbase = D.win_off[rec.contig];
    const char* cig = K.scratch + K.toff[p];
    const int64_t len = K.ri[p].cig_len;
    int64_t rp = rec.r_st;
    for (int64_t base = 0; base < len; base += 64) {
        const int64_t i = base + lane;
        const int c = i < len ? (int)(unsigned char)cig[i] : '0';
        const bool cov = c == 'M' || c == '=' || c == 'X';
        const bool ref = cov || c == 'D' || c == 'N';
        if (!__ballot(ref)) continue;
        long long n = 0;
        if (ref) {
            unsigned long long num = 0, mul = 1;
            for (int64_t k = i - 1; k >= 0 && k >= i - 19; --k) {
                const int d = (int)(unsigned char)cig[k];
                if (d < '0' || d > '9') break;
                num += (unsigned long long)(d - '0') * mul; mul *= 10;
            }
            n = (long long)num;
        }
        const long long incl = dep_scan_i64(n, lane);
        const int64_t s = rp + (incl - n), e = s + n;
        rp += __shfl(incl, 63);
        const int64_t cs = s < 0 ? 0 : s, ce = e > L ? L : e;
        const bool has = cov && cs < ce;
        if (!__ballot(has)) continue;
        const int64_t w0 = has ? cs / W : 0, w1 = has ? (ce - 1) / W : 0;
        const int64_t hend = (w0 + 1) * W < ce ? (w0 + 1) * W : ce;
        dep_seg_add(D.counts, has, wbase + w0, hend - cs, lane);
        dep_seg_add(D.counts, has && w1 > w0, wbase + w1, ce - w1 * W, lane);
        unsigned long long im = __ballot(has && w1 > w0 + 1);
        while (im) {                                                     // whole interior windows of a long run: all lanes, 64 windows per step
            const int l = __ffsll((long long)im) - 1; im &= im - 1;
            const int64_t a = __shfl((long long)w0, l) + 1, b = __shfl((long long)w1, l);
            for (int64_t w = a + lane; w < b; w += 64) atomicAdd(&D.counts[wbase + w], (unsigned long long)W);
        }
    }
}

__global__ void __launch_bounds__(256) k_depth_merge(unsigned long long* dst, const unsigned long long* src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] += src[i];
}

// sums[c] = the counts of contig c's windows, sums[nseq] = all of them (sums zeroed before the launch). grid (nseq, slices), one wavefront each.
__global__ void __launch_bounds__(64) k_depth_sums(const unsigned long long* counts, const int64_t* win_off, int32_t nseq, unsigned long long* sums) {
    const int lane = (int)threadIdx.x;
    const int64_t c = blockIdx.x;
    if (c >= nseq) return;
    const int64_t a = win_off[c], b = win_off[c + 1];
    long long v = 0;
    for (int64_t i = a + (int64_t)blockIdx.y * 64 + lane; i < b; i += (int64_t)gridDim.y * 64) v += (long long)counts[i];
    v = vmx_wave_sum_i64(v);
    if (lane == 0 && v) { atomicAdd(&sums[c], (unsigned long long)v); atomicAdd(&sums[nseq], (unsigned long long)v); }
}

// a line under construction by one lane
template <bool W> struct DepOut {
    char* p; int64_t pos;
    __device__ __forceinline__ void ch(char c) { if (W) p[pos] = c; ++pos; }
    __device__ __forceinline__ void bytes(const char* s, int64_t n) { if (W) for (int64_t x = 0; x < n; ++x) p[pos + x] = s[x]; pos += n; }
    __device__ __forceinline__ void num(unsigned long long u) {
        const int nd = sam_ndig(u);
        if (W) for (int k = nd - 1; k >= 0; --k) { p[pos + k] = (char)('0' + u % 10); u /= 10; }
        pos += nd;
    }
    __device__ __forceinline__ void mean(unsigned long long count, unsigned long long len) {      // two decimals, half up (the rule's h)
        const unsigned long long h = vmx_depth_hundredths(count, len);
        num(h / 100); ch('.'); ch((char)('0' + (h % 100) / 10)); ch((char)('0' + h % 10));
    }
};

template <bool W>
__device__ __forceinline__ void dep_line(const unsigned long long* counts, const int64_t* win_off, const int64_t* lens, const char* cnames, const int64_t* cname_off, int32_t nseq,
                                         int64_t window, const unsigned long long* sums, int which, int64_t total_len, int64_t i, int64_t* lsz, const int64_t* loff, char* text) {
    DepOut<W> O{W ? text + loff[i] : nullptr, 0};
    if (which == VM_DEPTH_REGIONS) {
        int lo = 0, hi = nseq;                                           // the last c with win_off[c] <= i: its win_off[c + 1] > i, so it has windows
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (win_off[mid] <= i) lo = mid; else hi = mid; }
        const int64_t start = (i - win_off[lo]) * window, end = start + window < lens[lo] ? start + window : lens[lo];
        O.bytes(cnames + cname_off[lo], cname_off[lo + 1] - cname_off[lo]); O.ch('\t');
        O.num((unsigned long long)start); O.ch('\t'); O.num((unsigned long long)end); O.ch('\t');
        O.mean(counts[i], (unsigned long long)(end - start)); O.ch('\n');
    } else {
        const int64_t len = i < nseq ? lens[i] : total_len;
        if (i < nseq) O.bytes(cnames + cname_off[i], cname_off[i + 1] - cname_off[i]); else O.bytes("total", 5);
        O.ch('\t'); O.num((unsigned long long)len); O.ch('\t'); O.num(sums[i]); O.ch('\t');
        O.mean(sums[i], (unsigned long long)len); O.ch('\n');
    }
    if (!W) lsz[i] = O.pos;
}

__global__ void __launch_bounds__(256) k_depth_lines(const unsigned long long* counts, const int64_t* win_off, const int64_t* lens, const char* cnames, const int64_t* cname_off,
                                                     int32_t nseq, int64_t window, const unsigned long long* sums, int which, int64_t total_len, int64_t n_items, int64_t* lsz,
                                                     const int64_t* loff, char* text, int write) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    if (write) dep_line<true>(counts, win_off, lens, cnames, cname_off, nseq, window, sums, which, total_len, i, lsz, loff, text);
    else dep_line<false>(counts, win_off, lens, cnames, cname_off, nseq, window, sums, which, total_len, i, lsz, loff, text);
}
