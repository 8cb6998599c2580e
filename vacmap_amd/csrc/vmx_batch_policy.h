// vmx_batch_policy.h — the host's DECISIONS on the batched path (vmx_align.hip, vmx_stage_extend.hip) as pure functions: the extend stage's per-read pool
// geometry, the gap fill's band-width rule, the per-read status, the splice of side batches into a batch's result and the result-size guess. Nothing in here
// touches HIP: the standard library and the public types only, so that a plain C++ compiler builds it alone (tests/host/batch_policy_main.cpp).
#ifndef VMX_BATCH_POLICY_H
#define VMX_BATCH_POLICY_H
#include "../../include/vacmapx.h"
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#ifndef VMX_HD
#if defined(__HIPCC__)
#define VMX_HD __host__ __device__
#else
#define VMX_HD
#endif
#endif

// per-read statuses that never leave align_device, and align_device_once's "run the batch again"
#define VMX_EXT_SHORT_INTERNAL (-9001)   // "an extend-stage pool was too small for this read": run again alone with larger pools
#define VMX_EXT_EXACT_INTERNAL (-9002)   // "this read needs a part of the path that a batch does not run: the later tiers of the divergence filter, or pass 1"
#define VMX_RETRY_BATCH (-9003)          // align_device_once -> align_device: an assumption the batch ran on instead of a host wait did not hold (a pool sized from the context's
                                         // history, the unplanned pass 1): the pools have been grown / the assumption dropped, run the batch again
// the device's per-read codes the status rule looks at (vmx_extend.h, vmx_local.h: vmx_batch.h asserts that they are these)
enum { VMX_POL_EXT_CAPACITY_DEV = -24, VMX_POL_EXT_NEED_EXACT_DEV = -25, VMX_POL_READ_CAPACITY_DEV = -20, VMX_POL_READ_BANDFALL_DEV = -23 };

// ---- pool geometry of the extend stage: what a read with cl local anchors and len bases owns. ONE rule for the waiting path's host loop and k_ext_geometry.
// A pool the test hook names (VMX_TEST_EXT_POOL=<mask>:<div>; bits: 1 segment anchors, 2 segments, 4 record blob, 8 problems per round, 16 problem strings) is divided, never below 1.
VMX_HD inline long long vmx_pool_scaled(int bit, long long x, int ext_mul, int tmask, long long tdiv) {
    const long long y = x * ext_mul;
    return (tmask & bit) ? (y / tdiv > 1 ? y / tdiv : 1) : y;
}
struct vmx_read_geo { long long anchors, segs, blob, full; };      // segment anchors, segments, record text (a multiple of 8), the read's share of cS_full (problem slots, unscaled)
VMX_HD inline vmx_read_geo vmx_read_geometry(long long cl, long long len, int ext_mul, int tmask, long long tdiv) {
    vmx_read_geo g = {0, 0, 0, 0};
    if (cl <= 0) return g;
    g.anchors = vmx_pool_scaled(1, 3 * cl + 8, ext_mul, tmask, tdiv);
    g.segs = vmx_pool_scaled(2, cl + 2, ext_mul, tmask, tdiv);
    g.blob = (vmx_pool_scaled(4, 3 * len + 64 * (cl / 2 + 2) + 56, ext_mul, tmask, tdiv) + 7) & ~7LL;
    g.full = cl + 2;
    return g;
}

// ---- the gap fill's band-width rule (vmx_ad_ns tries a problem in the narrowest band whose margin covers pct % of it): pct follows the reads. One of these per device
// and read mode, shared by the contexts of the process (the table and its mutex: vmx_stage_extend.hip).
struct vmx_ad_rule {
    int pct = 0, floor = 20, hold = 0;
    static int start_pct(int mode) { return mode == VM_MODE_L ? 40 : 90; }
    // what a batch hands the kernels: pct | pct_min << 16
    static int packed(int ad_cur) { return ad_cur | (std::max(20, ad_cur - 25) << 16); }
    // one batch's vote: not_proven of its `problems` gap-fill problems were tried in a band and not proven. ad_cur: the pct the batch ran on.
    void vote(int ad_cur, long long not_proven, long long problems) {
        if (problems < 2000) return;
        if (ad_cur != pct) return;                                   // (a batch that ran on an older value does not vote on the current one)
        const double f = (double)not_proven / (double)problems;
        if (f > 0.03 && pct < 100) { pct = std::min(100, pct + 10); floor = pct; hold = 256; }
        else if (hold > 0) { if (--hold == 0) floor = 20; }
        else if (f < 0.025 && pct > floor) pct = std::max(floor, pct - (f < 0.01 ? 20 : 10));
    }
};

// ---- per-read status of a batch. The overrides apply in this order; a later one wins.
struct vmx_status_in {
    int er_status, er_active, er_redo, er_pass, er_nrec;            // vmx_ext_read
    bool fast_local, do_pass1, force_exact;
    long long test_side_every, r;                                    // VMX_TEST_SIDE_EVERY, the read's index in the batch
    long long gmax, n_anchors; int rmode;                            // the global chain's verdict, the read's anchors, the GC variant (1: mode R)
    int asm_override;                                                // -mode asm: the tie-break step's status, or 0
};
struct vmx_read_outcome { int status; bool unmapped; };
inline vmx_read_outcome vmx_read_status(const vmx_status_in& s) {
    int st = s.er_status == VMX_POL_EXT_CAPACITY_DEV ? VMX_EXT_SHORT_INTERNAL : (s.er_status == VMX_POL_EXT_NEED_EXACT_DEV ? VMX_EXT_EXACT_INTERNAL : s.er_status);
    if (s.fast_local && (s.er_status == VMX_POL_READ_CAPACITY_DEV || s.er_status == VMX_POL_READ_BANDFALL_DEV)) st = VMX_EXT_EXACT_INTERNAL;      // the local stage's retries live on the waiting path
    if (st == 0 && !s.do_pass1 && s.er_active && s.er_redo == 1 && s.er_pass == 1) st = VMX_EXT_EXACT_INTERNAL;      // asks for pass 1, which this batch did not run: again, alone
    if (st == 0 && s.test_side_every > 0 && !s.force_exact && s.r % s.test_side_every == 0) st = VMX_EXT_EXACT_INTERNAL;       // (test hook)
    if (s.gmax == -2 && s.n_anchors > 2) st = VM_READ_RAISED;       // GC-fast: the reference raises on this read (k_chain_fast.hip)
    if (s.gmax == -4) st = VM_READ_UNSUPPORTED;                     // -mode asm: a contig of 500 kb or more inside align_device (vm_align_batch routes those to vmx_asm.hip)
    if (s.asm_override != 0) st = s.asm_override;
    if (s.rmode == 1 && s.n_anchors <= 2) st = VM_READ_RAISED;      // mode R returns an unbound `factor` for <= 2 anchors (mammap_noprefercloser.py:24417)
    return vmx_read_outcome{st, st == 0 && s.er_nrec == 0};
}

// ---- the splice of side batches (reads run again alone) into their batch's result
// what a side batch adds to its batch's statistics: exactly these. (ADVICE r6, 5th finding: n_dp_problems, dp_cells, n_dp_redo and ms_gapfill_* of the side batches are
// dropped, so the per-read DP figures under-count. Adding them changes reported figures and is a change of its own.)
inline void vmx_stats_add_side(vm_batch_stats& st, const vm_batch_stats& st2) {
    st.ms_total += st2.ms_total; for (int i = 0; i < 14; ++i) st.ms_stage[i] += st2.ms_stage[i];
    st.n_host_syncs += st2.n_host_syncs; st.n_ed_tier2 += st2.n_ed_tier2; st.n_ed_full += st2.n_ed_full; st.n_local_anchors += st2.n_local_anchors; st.n_local_general += st2.n_local_general;
}
struct vmx_splice {
    std::vector<vm_record> all; std::string blob;
    // the batch's own result without the records of the reads in `again` (a read that is run again delivers its records from there: the batch's own — none, for
    // every real reason to run a read again — are dropped)
    void begin(const vm_record* recs, int64_t n_recs, const char* cigar_blob, int64_t n, const std::vector<int32_t>& again_reads) {
        std::vector<char> again((size_t)n + 1, 0); for (int32_t r : again_reads) again[(size_t)r] = 1;
        all.clear(); all.reserve((size_t)n_recs);
        for (int64_t i = 0; i < n_recs; ++i) if (!again[(size_t)recs[i].read_idx]) all.push_back(recs[i]);
        int64_t blob_n = 0; for (const vm_record& x : all) blob_n = std::max<int64_t>(blob_n, x.cigar_off + x.cigar_len + 1);
        blob.assign(cigar_blob, (size_t)blob_n);
    }
    // a side batch's records: read j of it is read sub[j] of the batch; its CIGAR text goes behind what is there
    void add_side(const vm_record* r2, int64_t n2, const char* b2, const std::vector<int32_t>& sub) {
        for (int64_t i = 0; i < n2; ++i) { vm_record x = r2[i]; x.read_idx = sub[(size_t)x.read_idx]; x.cigar_off += (int64_t)blob.size(); all.push_back(x); }
        int64_t bl = 0; for (int64_t i = 0; i < n2; ++i) bl = std::max<int64_t>(bl, r2[i].cigar_off + r2[i].cigar_len + 1);
        blob.append(b2, (size_t)bl);
    }
    void finish() { std::stable_sort(all.begin(), all.end(), [](const vm_record& a, const vm_record& b) { return a.read_idx < b.read_idx; }); }      // records stay grouped by read, in read order
    // the batch's counters over the spliced result
    void counters(const std::vector<int32_t>& status, int64_t n, vm_batch_stats& st) const {
        st.n_records = (int64_t)all.size(); st.aligned_bases = 0; st.cigar_bytes = 0; st.n_failed = 0; st.n_unmapped = 0;
        std::vector<char> has((size_t)n + 1, 0);
        for (const vm_record& x : all) { st.aligned_bases += x.q_en - x.q_st; st.cigar_bytes += x.cigar_len; has[(size_t)x.read_idx] = 1; }
        for (int64_t r = 0; r < n; ++r) { if (status[(size_t)r] != 0) st.n_failed++; else if (!has[(size_t)r]) st.n_unmapped++; }
    }
};

// ---- the result copy's size guess: the packed buffers on the device have room for the worst case (cS records, cB CIGAR bytes); the host copies as many records / bytes as the
// context's history suggests for a batch of this size (records are 40 B: a generous guess costs nothing; a short one costs a second wait). No history: nothing is guessed.
struct vmx_res_guess { int64_t nr, nb; };
inline vmx_res_guess vmx_result_guess(double rec_per_read, double blob_per_base, int64_t n, int64_t total_bases, int64_t cS, int64_t cB) {
    vmx_res_guess g = {std::min<int64_t>(cS, (int64_t)(rec_per_read * 2.0 * (double)n) + 256), std::min<int64_t>(cB, (int64_t)(blob_per_base * 1.5 * (double)total_bases) + 65536)};
    if (rec_per_read <= 0.0) { g.nr = 0; g.nb = 0; }
    return g;
}
// the per-context maxima the guess is made from
inline void vmx_result_learn(double& rec_per_read, double& blob_per_base, int64_t nr, int64_t nb, int64_t n, int64_t total_bases) {
    if (n > 0 && total_bases > 0) { rec_per_read = std::max(rec_per_read, (double)nr / (double)n); blob_per_base = std::max(blob_per_base, (double)nb / (double)total_bases); }
}
#endif
