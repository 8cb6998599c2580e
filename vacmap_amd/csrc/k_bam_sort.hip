// k_bam_sort.hip — coordinate-sorted BAM and its CSI index on the device (driver: --bam-writer native-sort; host side: vmx_bam.hip).
//
// Sorting never compares records: a record's 64-bit key (refID, pos + 1, strand) is read from its encoded bytes, (key, ordinal) pairs
// go through the device radix sort, and k_bam_gather moves the variable-length records into the sorted order. The same gather serves
// a window's run (source = the encoder's output) and the merge (source = the staged ranges of the run files).
// The index kernels work on one entry per record (virtual offsets, bin, interval) that k_bam_index_entries writes after a chunk has been
// compressed. Every reduction is an integer min / max / add or a position-determined write, so the bytes do not depend on wave scheduling.
#include <string.h>
#include "vmx_bam.h"

__device__ __forceinline__ uint32_t bs_ld16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ uint32_t bs_ld32(const uint8_t* p) { return bs_ld16(p) | bs_ld16(p + 2) << 16; }

struct alignas(16) bs_v16 { uint32_t x, y, z, w; };

// ------------------------------------------------------------------------------------------------ keys, run order, gather

// key[i] = uint32(refID) << 32 | uint32(pos + 1) << 1 | reverse strand (refID -1 sorts last); val[i] = i
__global__ void __launch_bounds__(256) k_bam_sort_keys(const uint8_t* rec, const int64_t* roff, int64_t n, uint64_t* key, uint64_t* val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint8_t* r = rec + roff[i];
    const uint32_t ref = bs_ld32(r + 4), pos = bs_ld32(r + 8), flag = bs_ld16(r + 18);
    key[i] = (uint64_t)ref << 32 | (uint64_t)(uint32_t)(pos + 1) << 1 | (flag >> 4 & 1);
    val[i] = (uint64_t)i;
}

// the records of a run in sorted order: size and source offset of output record j (ssz[n] = 0: the scan's total slot)
__global__ void __launch_bounds__(256) k_bam_sort_sizes(const int64_t* roff, const uint64_t* perm, int64_t n, int64_t* ssz, int64_t* so) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    if (j == n) { ssz[j] = 0; return; }
    const int64_t i = (int64_t)perm[j];
    ssz[j] = roff[i + 1] - roff[i];
    so[j] = roff[i];
}

// One wave per record: dst[doff[j] - dbase, doff[j + 1] - dbase) = src[so[j], ...). Bytes up to the destination's 16-byte boundary, then
// 16-byte stores to aligned addresses (the source of a vector is read at whatever alignment it has), then the byte tail.
__global__ void __launch_bounds__(256) k_bam_gather(const uint8_t* src, const int64_t* so, const int64_t* doff, int64_t dbase, uint8_t* dst, int64_t n) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= n) return;
    const int lane = threadIdx.x & 63;
    const int64_t sz = doff[j + 1] - doff[j];
    const uint8_t* s = src + so[j];
    uint8_t* d = dst + (doff[j] - dbase);
    int64_t head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > sz) head = sz;
    if (lane < head) d[lane] = s[lane];
    const int64_t nv = (sz - head) >> 4;
    for (int64_t k = lane; k < nv; k += 64) {
        bs_v16 v;
        memcpy(&v, s + head + (k << 4), 16);
        *(bs_v16*)(d + head + (k << 4)) = v;
    }
    const int64_t t0 = head + (nv << 4);
    if (t0 + lane < sz) d[t0 + lane] = s[t0 + lane];
}

// ------------------------------------------------------------------------------------------------ merge of the runs

// val[i] = run << 40 | index in run, for the concatenated keys of all runs (rstart[r] = first key of run r, rstart[n_runs] = n)
__global__ void __launch_bounds__(256) k_bam_merge_vals(const int64_t* rstart, int32_t n_runs, int64_t n, uint64_t* val) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t lo = 0, hi = n_runs;                                     // the last r with rstart[r] <= i
    while (hi - lo > 1) { const int32_t m = (lo + hi) >> 1; if (rstart[m] <= i) lo = m; else hi = m; }
    val[i] = (uint64_t)lo << VMX_BAM_RUN_SHIFT | (uint64_t)(i - rstart[lo]);
}

// record sizes in the global order. roff_all: the runs' size scans back to back, run r's n_r + 1 entries from rstart[r] + r; gsz[n] = 0
__global__ void __launch_bounds__(256) k_bam_merge_sizes(const uint64_t* gval, const int64_t* roff_all, const int64_t* rstart, int64_t n, int64_t* gsz) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { gsz[i] = 0; return; }
    const int64_t r = (int64_t)(gval[i] >> VMX_BAM_RUN_SHIFT), x = (int64_t)(gval[i] & VMX_BAM_RUN_MASK);
    const int64_t* ro = roff_all + rstart[r] + r;
    gsz[i] = ro[x + 1] - ro[x];
}

// output chunk c = the records that start in bytes [c * chunk_bytes, (c + 1) * chunk_bytes) of the sorted stream: cut[c] = its first record,
// cutoff[c] = that record's byte offset (cut[n_chunks] = n, cutoff[n_chunks] = the stream's length)
__global__ void __launch_bounds__(256) k_bam_merge_cuts(const int64_t* goff, int64_t n, int64_t chunk_bytes, int64_t n_chunks, int64_t* cut, int64_t* cutoff) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_chunks) return;
    int64_t lo = 0, hi = n;                                          // the first i with goff[i] >= c * chunk_bytes
    if (c == n_chunks) lo = n;
    else while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (goff[m] >= c * chunk_bytes) hi = m; else lo = m + 1; }
    cut[c] = lo;
    cutoff[c] = goff[lo];
}

// rmax[c * n_runs + r] = 1 + the largest index of run r in chunk c (0: none). Every run is sorted by the global order, so a chunk takes
// one contiguous range of each run, ending there and starting where the previous chunks ended. rmax is zeroed by the host.
__global__ void __launch_bounds__(256) k_bam_merge_runmax(const uint64_t* gval, const int64_t* cut, int64_t n_chunks, int32_t n_runs, int64_t n,
                                                          unsigned long long* rmax) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int64_t lo = 0, hi = n_chunks;                                   // the last c with cut[c] <= i
    while (hi - lo > 1) { const int64_t m = (lo + hi) >> 1; if (cut[m] <= i) lo = m; else hi = m; }
    const int64_t r = (int64_t)(gval[i] >> VMX_BAM_RUN_SHIFT);
    atomicMax(&rmax[lo * n_runs + r], (unsigned long long)((gval[i] & VMX_BAM_RUN_MASK) + 1));
}

// source offset in the staging buffer of the m records of a chunk: sbase[r] = where run r's range starts in staging - the run offset of the range's first record
__global__ void __launch_bounds__(256) k_bam_merge_src(const uint64_t* gval, int64_t m, const int64_t* roff_all, const int64_t* rstart, const int64_t* sbase, int64_t* so) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t r = (int64_t)(gval[j] >> VMX_BAM_RUN_SHIFT), x = (int64_t)(gval[j] & VMX_BAM_RUN_MASK);
    so[j] = sbase[r] + roff_all[rstart[r] + r + x];
}

// ------------------------------------------------------------------------------------------------ index entries and CSI

__device__ __forceinline__ uint64_t bs_voff(const int64_t* moff, int64_t file_base, int64_t u) {
    return (uint64_t)(file_base + moff[u / VMX_BGZF_BLOCK]) << 16 | (uint64_t)(u % VMX_BGZF_BLOCK);
}

// One wave per record of a compressed chunk (rec: its uncompressed bytes; doff[j] - dbase: record j's offset; moff: the chunk's member
// offsets, n_members + 1 entries; file_base: file offset of the chunk's first member). e_key = uint32(refID) << 32 | bin (all ones
// without a reference), e_end = pos + reference length of the CIGAR as stored (1 when it has none), e_unm = FLAG & 4.
__global__ void __launch_bounds__(256) k_bam_index_entries(const uint8_t* rec, const int64_t* doff, int64_t dbase, int64_t m, const int64_t* moff, int64_t file_base,
                                                           uint64_t* e_key, uint64_t* e_vbeg, uint64_t* e_vend, int32_t* e_beg, uint32_t* e_end, uint32_t* e_unm) {
    const int64_t j = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= m) return;                                              // (a whole wave)
    const int lane = threadIdx.x & 63;
    const int64_t u0 = doff[j] - dbase, u1 = doff[j + 1] - dbase;
    const uint8_t* r = rec + u0;
    const uint32_t nc = bs_ld16(r + 16);
    const uint8_t* cg = r + 36 + r[12];
    uint32_t span = 0;
    for (uint32_t k = lane; k < nc; k += 64) {
        const uint32_t c = bs_ld32(cg + 4 * k), op = c & 15;
        if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += c >> 4;
    }
    for (int d = 32; d; d >>= 1) span += __shfl_xor(span, d);
    if (lane) return;
    const uint32_t ref = bs_ld32(r + 4);
    const int32_t pos = (int32_t)bs_ld32(r + 8);
    e_key[j] = (int32_t)ref < 0 ? ~0ULL : (uint64_t)ref << 32 | bs_ld16(r + 14);
    e_vbeg[j] = bs_voff(moff, file_base, u0);
    e_vend[j] = bs_voff(moff, file_base, u1);
    e_beg[j] = pos;
    e_end[j] = (uint32_t)pos + (span ? span : 1);
    e_unm[j] = bs_ld16(r + 18) >> 2 & 1;
}

__global__ void __launch_bounds__(256) k_csi_iota(uint64_t* v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint64_t)i;
}

// entries sorted by (refID, bin), file order inside: flag[j] = 1 when entry j starts a chunk — a new (refID, bin), or neither adjacent in
// the file to the bin's previous record nor beginning in the BGZF member where that one ends. flag[n] = 0 (the scan's total slot)
__global__ void __launch_bounds__(256) k_csi_flags(const uint64_t* skey, const uint64_t* sidx, const uint64_t* vbeg, const uint64_t* vend, int64_t n, int64_t* flag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > n) return;
    int64_t f = 0;
    if (j < n) {
        f = 1;
        if (j > 0 && skey[j - 1] == skey[j]) {
            const uint64_t b = vbeg[sidx[j]], e = vend[sidx[j - 1]];
            if (b == e || b >> 16 == e >> 16) f = 0;
        }
    }
    flag[j] = f;
}

// chunk k of the index = entries from the k-th flag to the one before the next: (key, vbeg of its first record, vend of its last)
__global__ void __launch_bounds__(256) k_csi_chunks(const uint64_t* skey, const uint64_t* sidx, const uint64_t* vbeg, const uint64_t* vend, const int64_t* flag,
                                                    const int64_t* cpos, int64_t n, uint64_t* ckey, uint64_t* cbeg, uint64_t* cend) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int64_t k = cpos[j] + flag[j] - 1;
    if (flag[j]) { ckey[k] = skey[j]; cbeg[k] = vbeg[sidx[j]]; }
    if (j == n - 1 || flag[j + 1]) cend[k] = vend[sidx[j]];
}

// lin[wbase[ref] + w] = smallest vbeg of the records that reach 16 kb window w of the reference (all ones: none); windows clamped to the table
__global__ void __launch_bounds__(256) k_csi_linear(const uint64_t* e_key, const uint64_t* vbeg, const int32_t* e_beg, const uint32_t* e_end, int64_t n,
                                                    int32_t n_ref, const int64_t* wbase, unsigned long long* lin) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || e_key[i] >> 32 >= (uint64_t)n_ref) return;
    const int64_t ref = (int64_t)(e_key[i] >> 32), nw = wbase[ref + 1] - wbase[ref];
    int64_t w0 = (int64_t)(e_beg[i] < 0 ? 0 : e_beg[i]) >> 14, w1 = ((int64_t)e_end[i] - 1) >> 14;
    if (w1 > nw - 1) w1 = nw - 1;
    if (w0 > w1) w0 = w1;
    if (w0 < 0) return;
    for (int64_t w = w0; w <= w1; ++w) atomicMin(&lin[wbase[ref] + w], (unsigned long long)vbeg[i]);
}

// loffset of a chunk's bin: the linear index at the first window of the bin's span, or at the next window to the right that a record reaches
__global__ void __launch_bounds__(256) k_csi_loffset(const uint64_t* ckey, int64_t nc, int32_t n_ref, const int64_t* wbase, const unsigned long long* lin, uint64_t* cloff) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nc) return;
    if (ckey[k] >> 32 >= (uint64_t)n_ref) { cloff[k] = 0; return; }
    const int64_t ref = (int64_t)(ckey[k] >> 32), bin = (int64_t)(ckey[k] & 0xffffffffu), nw = wbase[ref + 1] - wbase[ref];
    int l = 5;
    while (l > 0 && bin < ((1LL << (3 * l)) - 1) / 7) --l;           // the bin's level: level l starts at (8^l - 1) / 7
    int64_t w = (bin - ((1LL << (3 * l)) - 1) / 7) << (3 * (5 - l));
    uint64_t v = 0;
    for (; w < nw; ++w) if (lin[wbase[ref] + w] != ~0ULL) { v = lin[wbase[ref] + w]; break; }
    cloff[k] = v;
}

// per reference (records are in coordinate order): vbeg of its first record, vend of its last, mapped and unmapped counts; cnt[2 * n_ref] = records without a reference
__global__ void __launch_bounds__(256) k_csi_refstats(const uint64_t* e_key, const uint64_t* vbeg, const uint64_t* vend, const uint32_t* e_unm, int64_t n, int32_t n_ref,
                                                      uint64_t* rbeg, uint64_t* rend, unsigned long long* cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (e_key[i] == ~0ULL) { atomicAdd(&cnt[2 * (int64_t)n_ref], 1ULL); return; }
    const int64_t ref = (int64_t)(e_key[i] >> 32);
    if (ref >= n_ref) return;
    if (i == 0 || e_key[i - 1] >> 32 != e_key[i] >> 32) rbeg[ref] = vbeg[i];
    if (i == n - 1 || e_key[i + 1] >> 32 != e_key[i] >> 32) rend[ref] = vend[i];
    atomicAdd(&cnt[2 * ref + e_unm[i]], 1ULL);
}
