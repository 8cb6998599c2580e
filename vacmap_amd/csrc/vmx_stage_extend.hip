// vmx_stage_extend.hip — E1-E6, the extend stage of a batch (vmx_extend_stage over vmx_batch_run, vmx_batch.h), and one gap-fill chunk (vmx_gapfill_chunk, also the
// stage entry's). Replaces extend_func (/root/reference/src/vacmap/mammap_clrnano.py:19238-19330) for a whole batch: the host sizes pools and launches; every
// problem count stays on the device, and the stage waits for the device once (the gap fill's chunk plan).
#include "vmx_host.h"
#include "vmx_stage.h"
#include "vmx_ext_state.h"
#include "vmx_round.h"
#include <algorithm>
#include <cstdio>
#include <cstring>

using namespace vmx;

__global__ void k_ext_phase(vmx_ext_args A, int phase);
__global__ void k_ed_anchor_bound(vmx_ext_args A, const int32_t* probread, const uint8_t* qpool, const int64_t* qoff, const uint8_t* tpool, const int64_t* toff,
                                  int64_t* ub_out);
__global__ void k_gather(const vmx_pair_desc* desc, const int32_t* n_prob, const int32_t* prob_read, const uint8_t* ocodes, const int64_t* roff,
                         const uint8_t* ref, const int64_t* t_off, const int64_t* q_off, uint8_t* tpool, uint8_t* qpool, int64_t pool_cap, vmx_ext_read* er);
__global__ void k_ext_records(vmx_ext_args A, const vmx_dp_prob* probs, const char* cig_pool, const int32_t* cig_len, const int32_t* cig_q);
__global__ void k_ext_geometry(const int32_t* la_cnt, const int64_t* roff, int n, int mul, int tmask, long long tdiv, long long capA, long long capS, long long capB, int64_t* coff3,
                               int64_t* soff2, int64_t* bloboff, int64_t* tot);

// one gap-fill chunk (vmx_stage.h)
void vmx_gapfill_chunk(vm_ctx* c, vmx_batch_bufs& B, const vm_score& sc, int ad_pct, int eqx, int p0, int64_t pn, const int32_t* n_ptr, int64_t tb_off0,
                       vmx_gf_ctl* ctl, int32_t* redo_list, int64_t redo_cap, hipEvent_t* ke) {
    const vmx_align_knobs knobs = vmx_align_knobs_read();
    const int fill_waves = knobs.now.fill_waves;                      // waves per CU of the fill kernel (tuning knob: VMX_FILL_WAVES)
    const int tr_spread = knobs.once->trace_spread;
    uint8_t* tb_base = B.tb.as<uint8_t>() - tb_off0;           // the problems' absolute traceback offsets index a buffer that holds this chunk only
    vmx_dp_prob* probs = B.dptab.as<vmx_dp_prob>() + p0; int32_t* score = B.dpscore.as<int32_t>() + p0;
    const unsigned Gs = (unsigned)std::max<int64_t>(1, std::min<int64_t>((pn + 1023) / 1024, (int64_t)c->num_cu * 2));
    hipLaunchKernelGGL(k_size_hist, dim3(Gs), dim3(256), 0, c->stream, B.dpsz[0].as<int64_t>() + p0, n_ptr, (int64_t)((1LL << 42) - 1), ctl->scratch);        // (queue keys: vmx_round.h)
    hipLaunchKernelGGL(k_size_scatter, dim3(Gs), dim3(256), 0, c->stream, B.dpsz[0].as<int64_t>() + p0, n_ptr, (const int32_t*)ctl->scratch, ctl->scratch + 257, B.order.as<int32_t>(), ctl->range, ctl->head);
    if (ke) (void)hipEventRecord(ke[0], c->stream);
    {
        vmx_lowprio lp(c);                                    // the long launch at the lowest dispatch priority (vmx_host.h)
        hipLaunchKernelGGL(k_gapfill_fill_ns, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(pn, (int64_t)c->num_cu * fill_waves))), dim3(64), 0, lp.stream(), B.tpool.as<uint8_t>(), B.qpool.as<uint8_t>(),
                           probs, (int)pn, sc.match, sc.mismatch, sc.o1, sc.e1, sc.o2, sc.e2, tb_base, B.bnd.as<int32_t>(), score, B.order.as<int32_t>(), ctl,
                           redo_list, ad_pct, n_ptr, (unsigned long long)redo_cap, 1);
        lp.join();
    }
    // second launch (k_gapfill_redo): the problems whose band was not proven or that were never tried in one (a few per cent). The larger ones go two per wave through a
    // wave-wide band of 256 .. 512 diagonals and are filled in full, one per wave, only where that is not proven either; the others in full, four per wave. Its queue is the
    // list the first launch left; any grid works. ctl->redo_kept / redo_full: problems kept from a wide band / filled in full after all.
    hipLaunchKernelGGL(k_gapfill_redo, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(pn, (int64_t)c->num_cu * 4))), dim3(64), 0, c->stream, B.tpool.as<uint8_t>(), B.qpool.as<uint8_t>(),
                       probs, sc.match, sc.mismatch, sc.o1, sc.e1, sc.o2, sc.e2, tb_base, B.bnd.as<int32_t>(), score, redo_list, ctl, B.tbredo.as<uint8_t>());
    if (ke) (void)hipEventRecord(ke[1], c->stream);
    hipLaunchKernelGGL(k_gapfill_trace, dim3((unsigned)std::max<int64_t>(1, (pn * tr_spread + 63) / 64)), dim3(64), 0, c->stream, B.tpool.as<uint8_t>(), B.qpool.as<uint8_t>(), probs, (int)pn, eqx,
                       tb_base, B.run.as<uint32_t>(), B.cig.as<char>(), B.ciglen.as<int32_t>() + p0, score, B.tbredo.as<uint8_t>(), tr_spread, B.cigq.as<int32_t>() + p0, n_ptr);
    if (ke) (void)hipEventRecord(ke[2], c->stream);
}

static const vm_score gf_score = {2, -4, 4, 2, 24, 1};           // the gap fill's scoring (E5: ext_gather_round's band-width rule, vmx_gapfill_chunk)

// one DP round of the extend stage: descriptors (count on device) -> offsets -> gathered pools. The round's problem count stays on the
// device (B.rcount; every consumer reads it there and launches a grid sized for the hardware, not for the count); it is copied into
// slot `stat_slot` of the batch's counter block, which the host reads once at the end. want_cnt: also return a host copy (one wait) —
// only the gap-fill rounds, whose pools are sized by it, ask for that.
// (The slots' owners are written when the phase kernel allocates them; vmx_alloc_probs never lets the published count pass the capacity.)
static int ext_gather_round(vm_ctx* c, vmx_batch_bufs& B, const vm_index_view& ix, const uint8_t* d_ocodes, const int64_t* d_roff, int cur,
                            int64_t pool_cap, int stat_slot, bool dp, int64_t tb_limit, const int64_t* caps = nullptr, int64_t* plan_out = nullptr, int ad_pct = 0) {
    if (!B.roundpart.p) { VMX_TRY(B.roundpart.reserve(8 * (size_t)VMX_ROUND_PART_WORDS)); VMX_HIP(hipMemsetAsync(B.roundpart.p, 0, 8 * (size_t)VMX_ROUND_PART_WORDS, c->stream)); }
    vmx_round_args R; memset(&R, 0, sizeof R);
    R.desc = B.desc[cur].as<vmx_pair_desc>(); R.n_prob = c->rc_cur;
    R.off[0] = B.toff.as<int64_t>(); R.off[1] = B.qoff.as<int64_t>();
    R.part = B.roundpart.as<int64_t>(); R.stat_out = B.statblk.as<int32_t>() + stat_slot; R.epoch = ++c->round_epoch;
    if (dp) {
        for (int i = 0; i < 4; ++i) R.off[2 + i] = B.dpoff[i].as<int64_t>();
        R.tb_size = B.dpsz[0].as<int64_t>(); R.probs = B.dptab.as<vmx_dp_prob>(); R.plan_out = plan_out; R.tb_limit = tb_limit;
        if (caps) for (int i = 0; i < 4; ++i) R.cap[i] = caps[i];          // unplanned pass: every problem is checked against the pools (k_round.hip)
        R.ad_on = 1; R.ad_match = gf_score.match; R.ad_o1 = gf_score.o1; R.ad_e1 = gf_score.e1; R.ad_o2 = gf_score.o2; R.ad_e2 = gf_score.e2; R.ad_pct = ad_pct;      // the fill's own scoring and band-width rule
        hipLaunchKernelGGL(k_round_prep<true>, dim3(VMX_ROUND_WGS), dim3(256), 0, c->stream, R);
    } else
        hipLaunchKernelGGL(k_round_prep<false>, dim3(VMX_ROUND_WGS), dim3(256), 0, c->stream, R);
    hipLaunchKernelGGL(k_gather, dim3((unsigned)((int64_t)c->num_cu * 8)), dim3(256), 0, c->stream, B.desc[cur].as<vmx_pair_desc>(), c->rc_cur,
                       B.probread.as<int32_t>(), d_ocodes, d_roff, ix.codes, B.toff.as<int64_t>(), B.qoff.as<int64_t>(), B.tpool.as<uint8_t>(), B.qpool.as<uint8_t>(), pool_cap,
                       B.er.as<vmx_ext_read>());
    return 0;
}
static int ext_gather(vmx_batch_run& run, int stat_slot, bool dp, int64_t tb_limit = 0, int64_t* plan_out = nullptr) {
    return ext_gather_round(run.c, run.B, run.ix, run.B.ocodes.as<uint8_t>(), run.d_roff, run.cur, run.pool_cap, stat_slot, dp, tb_limit, nullptr, plan_out, run.ad_pct);
}

// The band-width rule of the gap fill (vmx_ad_ns: the narrowest band whose margin covers pct % of the problem) only decides which problems are TRIED in a band and how wide — the
// proof decides what is kept, so the records do not depend on it. Round 6: pct follows the reads instead of the mode alone. Each context starts at the mode's
// default (90; mode L 40) and steps down (to 20 at the least) by 20 / 10 while fewer than 1 / 2.5 % of a batch's problems are tried in a band and not proven (they go
// to the second launch: in full at ~4x a band attempt when these thresholds were tuned; since round 8 the larger ones through a wave-wide band first, k_gapfill_redo), back up when more than 3 % are, and then holds that floor for 256 batches. HiFi-shape reads settle at 20 (a 270-base
// problem runs on ONE diagonal pair per lane: margin 104 against ~8 points of errors), ONT reads at 80-90 (70 fails 6 %, 55 fails 29 %):
// `profiles/r06_q_band_width_rule_sweep.txt`. VMX_AD_PCT / VMX_AD_PCT_MIN pin the rule (tuning runs). The rule itself: vmx_ad_rule (vmx_batch_policy.h).
static std::mutex ad_m; static vmx_ad_rule ad_tab[16][8];      // per device and read mode, shared by the contexts of the process
static vmx_ad_rule& ad_rule_of(const vmx_batch_run& run) { return ad_tab[run.c->device & 15][run.prm->mode & 7]; }
static void ext_band_rule_read(vmx_batch_run& run) {
    vmx_ad_rule& adr = ad_rule_of(run);
    { std::lock_guard<std::mutex> g(ad_m); if (adr.pct == 0) adr.pct = vmx_ad_pct_env(run.prm->mode) & 0xffff; run.ad_cur = adr.pct; }
    run.ad_pct = run.knobs.now.ad_pinned ? vmx_ad_pct_env(run.prm->mode) : vmx_ad_rule::packed(run.ad_cur);
}
void vmx_band_rule_vote(vmx_batch_run& run, int64_t not_proven) {
    if (run.knobs.now.ad_pinned || run.c->force_exact || run.st.n_dp_problems < 2000) return;
    std::lock_guard<std::mutex> g(ad_m);
    ad_rule_of(run).vote(run.ad_cur, not_proven, run.st.n_dp_problems);
}

// per-read pool geometry from the local anchor count (the chain is never longer than that): host loop on the waiting path, k_ext_geometry inside the pools the context
// already holds on the fast path — one rule, vmx_read_geometry
static int ext_geometry(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t n = run.n;
    const int tmask = run.knobs.now.ext_tmask; const int64_t tdiv = run.knobs.now.ext_tdiv;
    if (!run.fast_local) {
        run.coff3.assign((size_t)n + 1, 0); run.soff2.assign((size_t)n + 1, 0); run.bloboff.assign((size_t)n + 1, 0);
        for (int64_t r = 0; r < n; ++r) {
            const vmx_read_geo g = vmx_read_geometry(run.L.h_la_cnt[r], run.h_roff[r + 1] - run.h_roff[r], c->ext_mul, tmask, tdiv);
            run.coff3[r + 1] = run.coff3[r] + g.anchors; run.soff2[r + 1] = run.soff2[r] + g.segs; run.bloboff[r + 1] = run.bloboff[r] + g.blob; run.cS_full += g.full;
        }
        run.cA = run.coff3[n]; run.cS = run.soff2[n]; run.cB = run.bloboff[n];
        if (!run.preset && c->ext_mul == 1 && tmask == 0) {      // the pools now hold at least this much: what the batches that do not ask may use
            c->geo_cap[0] = std::max<long long>(c->geo_cap[0], run.cA); c->geo_cap[1] = std::max<long long>(c->geo_cap[1], run.cS); c->geo_cap[2] = std::max<long long>(c->geo_cap[2], run.cB);
            c->geo_cap[3] = std::max<long long>(c->geo_cap[3], run.cS_full);
            c->geo_valid = true;
        }
    } else {
        // exactly what the pools already hold (no pool grows on this path: a growth is a hipMalloc of gigabytes with the GPU idle); a batch that needs more has its last
        // reads cut (k_ext_geometry) and run again alone, and this context's next batch takes the waiting path once, which sizes the pools for it
        run.cA = c->geo_cap[0]; run.cS = c->geo_cap[1]; run.cB = c->geo_cap[2]; run.cS_full = c->geo_cap[3];
    }
    VMX_TRY(B.er.reserve(sizeof(vmx_ext_read) * (size_t)(n + 1)));
    if (!run.fast_local) { const vmx_push_req rq[3] = {{&B.coff3, run.coff3.data(), 8 * ((size_t)n + 1)}, {&B.soff2, run.soff2.data(), 8 * ((size_t)n + 1)}, {&B.bloboff, run.bloboff.data(), 8 * ((size_t)n + 1)}}; VMX_TRY(vmx_push_many(c, rq, 3)); }
    else {
        VMX_TRY(B.coff3.reserve(8 * ((size_t)n + 2))); VMX_TRY(B.soff2.reserve(8 * ((size_t)n + 2))); VMX_TRY(B.bloboff.reserve(8 * ((size_t)n + 2))); VMX_TRY(B.geotot.reserve(64));
        hipLaunchKernelGGL(k_ext_geometry, dim3(1), dim3(1024), 0, c->stream, run.L.la_cnt.as<int32_t>(), run.d_roff, (int)n, c->ext_mul, tmask, (long long)tdiv, (long long)run.cA, (long long)run.cS, (long long)run.cB,
                           B.coff3.as<int64_t>(), B.soff2.as<int64_t>(), B.bloboff.as<int64_t>(), B.geotot.as<int64_t>());
    }
    return 0;
}

// the stage's pools, sized by the geometry, and the per-batch counter blocks, cleared once
static int ext_reserve_pools(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t n = run.n, cA = run.cA, cS = run.cS, cB = run.cB;
    VMX_TRY(B.segA.reserve(sizeof(vmx_anchor) * (size_t)(cA + 1))); VMX_TRY(B.segA_s.reserve(sizeof(vmx_anchor) * (size_t)(cA + 1)));
    VMX_TRY(B.st.reserve(4 * (size_t)(cS + 1))); VMX_TRY(B.en.reserve(4 * (size_t)(cS + 1))); VMX_TRY(B.st_s.reserve(4 * (size_t)(cS + 1))); VMX_TRY(B.en_s.reserve(4 * (size_t)(cS + 1)));
    VMX_TRY(B.segprob.reserve(4 * (size_t)(cS + 1))); VMX_TRY(B.dup.reserve(4 * (size_t)(cS + 1)));
    run.round_cap = vmx_pool_scaled(8, run.cS_full + 16, c->ext_mul, run.knobs.now.ext_tmask, run.knobs.now.ext_tdiv);         // one problem per anchor at most in any round
    run.pool_cap = vmx_pool_scaled(16, 6 * run.total_bases + (1 << 20), c->ext_mul, run.knobs.now.ext_tmask, run.knobs.now.ext_tdiv);
    const int64_t round_cap = run.round_cap, pool_cap = run.pool_cap;
    int64_t Lmax_b = 1; for (int64_t r = 0; r < n; ++r) Lmax_b = std::max(Lmax_b, run.h_roff[r + 1] - run.h_roff[r]);
    run.carry_stride = run.preset ? 32768 : 2 * Lmax_b + 32768;      // (ass_extend_func has no divergence filter: a preset chain never reaches the exact kernel, and a ring per
                                                                     //  workgroup sized by a 100 Mb contig asked for 617 GB)
    run.ed_wgs = std::min<int64_t>(c->num_cu, 64);             // workgroups of the exact kernel (x1 long, x2 short patterns): the last tier of the filter, hardly ever
                                                               // reached (0 problems per step on the bench workload), so its carry rings are kept small (0.8 instead of 3.2 GB)        // exact edit-distance kernel: one carry ring per workgroup (1 + 2 per CU), longest text it takes
    VMX_TRY(B.desc[0].reserve(sizeof(vmx_pair_desc) * (size_t)round_cap)); VMX_TRY(B.desc[1].reserve(sizeof(vmx_pair_desc) * (size_t)round_cap));
    VMX_TRY(B.rcount.reserve(256)); VMX_HIP(hipMemsetAsync(B.rcount.p, 0, 256, c->stream)); c->rc_next = 0; c->rc_cur = B.rcount.as<int32_t>(); VMX_TRY(B.oflow.reserve(64)); VMX_TRY(B.probread.reserve(4 * (size_t)round_cap));
    VMX_TRY(B.tl.reserve(8 * (size_t)(round_cap + 1))); VMX_TRY(B.ql.reserve(8 * (size_t)(round_cap + 1))); VMX_TRY(B.toff.reserve(8 * (size_t)(round_cap + 1))); VMX_TRY(B.qoff.reserve(8 * (size_t)(round_cap + 1)));
    VMX_TRY(B.tpool.reserve((size_t)pool_cap + 64)); VMX_TRY(B.qpool.reserve((size_t)pool_cap + 64));
    VMX_TRY(B.edout.reserve(8 * (size_t)(round_cap + 1))); VMX_TRY(B.carry.reserve((size_t)VMX_ED_WAVES * (size_t)run.carry_stride * (size_t)run.ed_wgs * 3 + 64)); VMX_TRY(B.ext3.reserve(12 * (size_t)(round_cap + 1)));
    VMX_TRY(B.rec.reserve(sizeof(vm_record) * (size_t)(cS + 1))); VMX_TRY(B.blob.reserve((size_t)cB + 64)); VMX_TRY(B.reccoff.reserve(8 * (size_t)(cS + 1)));
    VMX_TRY(B.recclen.reserve(4 * (size_t)(cS + 1))); VMX_TRY(B.dupd.reserve((size_t)cB + 64));
    VMX_HIP(hipMemsetAsync(B.oflow.p, 0, 4, c->stream));
    VMX_TRY(B.statblk.reserve(VMX_STAT_BYTES)); VMX_HIP(hipMemsetAsync(B.statblk.p, 0, VMX_STAT_BYTES, c->stream));     // (layout: VMX_STAT_*, vmx_round.h)
    const size_t gfctl_bytes = (size_t)2 * (VMX_MAX_CHUNKS + 1) * sizeof(vmx_gf_ctl);
    VMX_TRY(B.gfctl.reserve(gfctl_bytes)); VMX_HIP(hipMemsetAsync(B.gfctl.p, 0, gfctl_bytes, c->stream));      // the gap fill's per-chunk control blocks and size-order scratch, cleared once
    return 0;
}

static void ext_fill_args(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; vmx_local_bufs& L = run.L; const vm_params* prm = run.prm; const bool preset = run.preset != nullptr;
    vmx_ext_args& A = run.A; memset(&A, 0, sizeof A);
    A.n_reads = (int)run.n; A.nseq = run.ix.nseq; A.local_maxdiff = preset ? 50 : prm->local_maxdiff /* ass_extend_func: large_cost 50, mammap_asm.py:23426 */; A.asm_long = preset ? 1 : 0; A.nodiscard = prm->nodiscard; A.hardclip = prm->hardclip; A.redo_only = 0; A.mode = prm->mode; A.maxdivergence = prm->maxdivergence;
    A.ocodes = B.ocodes.as<uint8_t>(); A.roff = run.d_roff; A.ref = run.ix.codes; A.coff = run.ix.coff;
    A.chain = L.chain.as<vmx_anchor>(); A.chain_len = L.chain_len.as<int32_t>(); A.la_off = L.la_off.as<int64_t>(); A.lstatus = L.status.as<int32_t>();
    A.gscore = run.d_gscore; A.mapq = run.d_mapq; A.er = B.er.as<vmx_ext_read>(); A.coff3 = B.coff3.as<int64_t>(); A.soff = B.soff2.as<int64_t>();
    A.segA = B.segA.as<vmx_anchor>(); A.st = B.st.as<int32_t>(); A.en = B.en.as<int32_t>(); A.segA_snap = B.segA_s.as<vmx_anchor>(); A.st_snap = B.st_s.as<int32_t>(); A.en_snap = B.en_s.as<int32_t>();
    A.seg_prob = B.segprob.as<int32_t>(); A.dup = B.dup.as<int32_t>(); A.round_count = B.rcount.as<int32_t>(); A.round_cap = run.round_cap; A.overflow = B.oflow.as<int32_t>(); A.prob_read = B.probread.as<int32_t>();
    A.ed_out = B.edout.as<int64_t>(); A.ext_te = B.ext3.as<int32_t>(); A.ext_qe = B.ext3.as<int32_t>() + run.round_cap;
    A.rec = B.rec.as<vm_record>(); A.rec_blob = B.blob.as<char>(); A.blob_off = B.bloboff.as<int64_t>(); A.rec_coff = B.reccoff.as<int64_t>(); A.rec_clen = B.recclen.as<int32_t>();
    A.dup_d = B.dupd.as<double>();
    // k_ext_phase / k_ext_records: one lane in `spread` works. Alone, spreading the reads over more waves shortens the batch (a batch of
    // 40-100 kb reads, 1 / 4 / 16 / 64 lanes per read: phases 19.7 / 16.5 / 13.9 / 14.4 ms, records 8.7 / 7.6 / 8.6 / 15.6 ms; batch 130 -> 123 ms);
    // with three batches in flight it does not raise the throughput (34.3 vs 33.7 ms per step), so a shared context keeps one lane per read
    const int ext_env = run.knobs.once->ext_spread, rec_env = run.knobs.once->rec_spread;
    run.ext_spread = ext_env ? ext_env : (c->inflight >= 2 ? 1 : 16); run.rec_spread = rec_env ? rec_env : (c->inflight >= 2 ? 1 : 4);
}

// the stage-trace capture (vm_align_trace): the segment lists as they stand now, with a wait of its own
static void ext_trace_capture(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; vmx_seg_trace* trace = run.trace; const int64_t n = run.n, cA = run.cA, cS = run.cS;
    std::vector<vmx_ext_read> er((size_t)n); std::vector<vmx_anchor> sa((size_t)cA + 1); std::vector<int32_t> st_((size_t)cS + 1), en_((size_t)cS + 1);
    (void)hipMemcpyAsync(er.data(), B.er.p, sizeof(vmx_ext_read) * (size_t)n, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(sa.data(), B.segA.p, sizeof(vmx_anchor) * (size_t)cA, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(st_.data(), B.st.p, 4 * (size_t)cS, hipMemcpyDeviceToHost, c->stream);
    (void)hipMemcpyAsync(en_.data(), B.en.p, 4 * (size_t)cS, hipMemcpyDeviceToHost, c->stream);
    (void)vmx_stream_sync(c);
    trace->off.assign(1, 0);
    for (int64_t r = 0; r < n; ++r) {
        if (er[(size_t)r].active && er[(size_t)r].status == 0)
            for (int sg = 0; sg < er[(size_t)r].nseg; ++sg)
                for (int t = st_[(size_t)(run.soff2[r] + sg)]; t < en_[(size_t)(run.soff2[r] + sg)]; ++t) {
                    const vmx_anchor& a = sa[(size_t)(run.coff3[r] + t)];
                    const int64_t row[5] = {sg, a.q, a.r, a.s, a.l}; trace->rows.insert(trace->rows.end(), row, row + 5);
                }
        trace->off.push_back((int64_t)trace->rows.size() / 5);
    }
}

static void ext_phase(vmx_batch_run& run, int ph) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; vmx_ext_args& A = run.A;
    A.desc = B.desc[run.cur].as<vmx_pair_desc>(); A.desc_prev = B.desc[run.cur ^ 1].as<vmx_pair_desc>();
    c->rc_cur = B.rcount.as<int32_t>() + (c->rc_next++ & 63); A.round_count = c->rc_cur;      // a fresh, already cleared counter per phase (one clearing per batch)
    // the phases that walk every anchor (0 rebuild, 3 snapshot copy, 5 checkpoints) run one wavefront per read; VMX_EXT_WAVE=0: the one-lane form
    const bool wv = run.knobs.once->ext_wave && (ph == 0 || ph == 3 || ph == 5);
    const unsigned gridX = (unsigned)((run.n * run.ext_spread + 63) / 64);
    A.spread = wv ? 64 : run.ext_spread; hipLaunchKernelGGL(k_ext_phase, dim3(wv ? (unsigned)run.n : gridX), dim3(64), 0, c->stream, A, ph);
    if (run.trace && run.trace->stage == ph && !A.redo_only && run.trace->off.empty()) ext_trace_capture(run);
}

// the divergence filter's tiers behind the anchor bound (k_ed_band.hip): four problems per wave in a +-320-row band, one problem per wave in a +-768-row band, and the exact
// unbanded kernel, each only for the problems the tier before could not prove "keep" for
static void ext_filter_later_tiers(vmx_batch_run& run, int64_t cnt) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const vm_params* prm = run.prm;
    int32_t* d_range = B.qrange.as<int32_t>() + VMX_QR_RANGE; int32_t* d_cnt = B.qrange.as<int32_t>() + VMX_QR_CNT;
    int32_t* d_nfull = B.qrange.as<int32_t>() + VMX_QR_NFULL; int32_t* d_n2 = B.qrange.as<int32_t>() + VMX_QR_NT2;
    vmx_size_order_wide(c, B.dpsz[0].as<int64_t>(), c->rc_cur, cnt, (int64_t)VMX_ED_LONG, B.order.as<int32_t>(), d_range, d_cnt, B.szh.as<int32_t>());
    hipLaunchKernelGGL(k_ed_banded4, dim3((unsigned)std::min<int64_t>((cnt + 3) / 4, (int64_t)c->num_cu * 16)), dim3(64), 0, c->stream, B.qpool.as<uint8_t>(), B.qoff.as<int64_t>(),
                       B.tpool.as<uint8_t>(), B.toff.as<int64_t>(), B.order.as<int32_t>(), d_range, d_cnt + 2, B.dpsz[1].as<int64_t>());
    hipLaunchKernelGGL(k_ed_flag, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 1024)), dim3(256), 0, c->stream, B.dpsz[1].as<int64_t>(), B.qoff.as<int64_t>(), B.toff.as<int64_t>(),
                       c->rc_cur, prm->maxdivergence, B.dpsz[0].as<int64_t>(), B.edout.as<int64_t>(), d_n2, 0, (const int32_t*)nullptr, (vmx_ext_read*)nullptr);
    vmx_size_order_wide(c, B.dpsz[0].as<int64_t>(), c->rc_cur, cnt, (int64_t)VMX_ED_LONG, B.order.as<int32_t>(), d_range, d_cnt, B.szh.as<int32_t>());
    hipLaunchKernelGGL(k_ed_banded, dim3((unsigned)std::min<int64_t>(cnt, (int64_t)c->num_cu * 16)), dim3(64), 0, c->stream, B.qpool.as<uint8_t>(), B.qoff.as<int64_t>(),
                       B.tpool.as<uint8_t>(), B.toff.as<int64_t>(), B.order.as<int32_t>(), d_range, d_cnt + 2, B.dpsz[1].as<int64_t>());
    hipLaunchKernelGGL(k_ed_flag, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 1024)), dim3(256), 0, c->stream, B.dpsz[1].as<int64_t>(), B.qoff.as<int64_t>(), B.toff.as<int64_t>(),
                       c->rc_cur, prm->maxdivergence, B.dpsz[0].as<int64_t>(), B.edout.as<int64_t>(), d_nfull, 0, (const int32_t*)nullptr, (vmx_ext_read*)nullptr);
    vmx_size_order_wide(c, B.dpsz[0].as<int64_t>(), c->rc_cur, cnt, (int64_t)VMX_ED_LONG, B.order.as<int32_t>(), d_range, d_cnt, B.szh.as<int32_t>());
    // the exact tier, unconditionally (no read-back of the count: these are side batches of a few reads, or the A/B knob)
    for (int which = 0; which < 2; ++which)
        hipLaunchKernelGGL(k_edit_distance, dim3((unsigned)std::min<int64_t>(cnt, run.ed_wgs * (which == 0 ? 1 : 2))), dim3(which == 0 ? 64 * VMX_ED_WAVES : 256), 0, c->stream,
                           B.qpool.as<uint8_t>(), B.qoff.as<int64_t>(), B.tpool.as<uint8_t>(), B.toff.as<int64_t>(),
                           B.carry.as<int8_t>() + (which ? (size_t)VMX_ED_WAVES * (size_t)run.carry_stride * (size_t)run.ed_wgs : 0), B.order.as<int32_t>(), d_range, d_cnt, which,
                           B.edout.as<int64_t>(), run.carry_stride, B.oflow.as<int32_t>());
}

// divergence filter: edit distance of every segment (:19251)
static int ext_divergence_filter(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t round_cap = run.round_cap;
    VMX_TRY(ext_gather(run, VMX_STAT_ROUND_ED, false));
    const int64_t cnt = round_cap;                           // launch widths only: every kernel below reads the real count on the device
    VMX_TRY(B.order.reserve(4 * (size_t)(2 * round_cap + 64))); VMX_TRY(B.qrange.reserve(VMX_QR_BYTES)); VMX_TRY(B.szh.reserve(4 * 520));
    VMX_TRY(B.dpsz[0].reserve(8 * (size_t)(round_cap + 2))); VMX_TRY(B.dpsz[1].reserve(8 * (size_t)(round_cap + 2)));
    // tier 0 (k_ed_anchor_bound, k_ext.hip): the segment's own anchors cut the pair into independent short pieces whose summed cost
    // bounds the edit distance from above; the later tiers: ext_filter_later_tiers
    (void)hipMemsetAsync(B.qrange.as<int32_t>() + VMX_QR_NFULL, 0, 12, c->stream);      // the three tier counters
    hipLaunchKernelGGL(k_ed_anchor_bound, dim3((unsigned)std::min<int64_t>(cnt, (int64_t)c->num_cu * 16)), dim3(64), 0, c->stream, run.A, B.probread.as<int32_t>(),
                       B.qpool.as<uint8_t>(), B.qoff.as<int64_t>(), B.tpool.as<uint8_t>(), B.toff.as<int64_t>(), B.dpsz[1].as<int64_t>());
    // Round 6: the tiers behind the anchor bound are hardly ever needed (problems left after tier 0 per batch: 0 on ONT and HiFi reads at hg38 size, 0.07 on the
    // vacsim workload), yet every batch paid for them: two size-ordered banded launches, three flag passes, and a host wait to learn whether the exact kernel —
    // whose wide workgroups wait for room on a full GPU even when empty — had anything to do. Now a batch runs tier 0 and ONE flag pass that marks the READ of every
    // problem it could not settle (VMX_EXT_NEED_EXACT_DEV); align_device runs those reads again alone with all tiers (c->force_exact), exact kernel included.
    const bool all_tiers = c->force_exact || run.knobs.once->force_exact;      // (the knob: A/B and tests, every batch runs every tier)
    hipLaunchKernelGGL(k_ed_flag, dim3((unsigned)std::min<int64_t>((cnt + 255) / 256, 1024)), dim3(256), 0, c->stream, B.dpsz[1].as<int64_t>(), B.qoff.as<int64_t>(), B.toff.as<int64_t>(),
                       c->rc_cur, run.prm->maxdivergence, B.dpsz[0].as<int64_t>(), B.edout.as<int64_t>(), B.qrange.as<int32_t>() + VMX_QR_NT1, 1, B.probread.as<int32_t>(), all_tiers ? (vmx_ext_read*)nullptr : B.er.as<vmx_ext_read>());
    if (all_tiers) ext_filter_later_tiers(run, cnt);
    run.cur ^= 1;
    return 0;
}

// x-drop extension of the problems of the current round (their count stays on the device)
static int ext_round(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B;
    VMX_TRY(ext_gather(run, VMX_STAT_ROUND_EXT + run.ext_rounds++, false));
    hipLaunchKernelGGL(k_extend, dim3((unsigned)((int64_t)c->num_cu * 16)), dim3(64), 0, c->stream, B.tpool.as<uint8_t>(), B.toff.as<int64_t>(), B.qpool.as<uint8_t>(),
                       B.qoff.as<int64_t>(), 0, 2, -4, 4, 4, 100, 50, B.ext3.as<int32_t>(), B.ext3.as<int32_t>() + run.round_cap, B.ext3.as<int32_t>() + 2 * run.round_cap, c->rc_cur);
    run.cur ^= 1;
    return 0;
}

// ---- gap fill of one pass (E5). Round 6: ONE host wait per batch in here (the chunk plan of pass 0), none per chunk and none in pass 1.
//  * every chunk has its own control block (struct vmx_gf_ctl, vmx_gapfill.h: queue range and heads, the second launch's list and counters, the size ordering's scratch)
//    in B.gfctl, cleared once per batch: nothing is cleared between chunks, and the host reads all of them with the batch's final results;
//  * the full-matrix traceback space of the problems whose band was not proven (the SECOND launch's pool) is sized from the context's history (largest chunk
//    seen x 1.3, 512 MB to begin with) instead of by a read-back between the two launches; the band pass checks every allocation against the pool and a problem
//    that does not fit is emptied (tl = ql = 0: no fill, empty CIGAR) — the host sees the need at the end, grows the pool and runs the batch again;
//  * pass 1 (the nofilter re-run of a read whose segment filter removed something and whose CIGARs carry paired indels, :24079-24080) is not part of a batch at all:
//    hardly any read asks for it (none of the 150 golden reads, a handful per 100 k synthetic reads), and its eleven launches and one host wait were paid by every batch.
//    A read that asks for it (E.redo) is run again alone by align_device with both passes (c->run_pass1), like the reads that need the later tiers of the divergence filter.
// the chunks of a pass from its plan (run.plan, arrived): chunk q = problems [cuts[q], cuts[q+1]), its control block q of the pass's in B.gfctl
static int ext_gapfill_chunks(vmx_batch_run& run, int pass) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t* plan = run.plan;
    const int cnt = (int)plan[VMX_PLAN_N];
    const int64_t* totals = plan + VMX_PLAN_POOLS;
    if (plan[VMX_PLAN_CHUNKS] < 0) { set_error("gap fill: more traceback chunks than VMX_MAX_CHUNKS"); return VM_ERR_OOM; }
    run.st.n_dp_problems += cnt; run.st.dp_cells += totals[0]; run.st.dp_string_bytes += plan[VMX_PLAN_TBYTES] + plan[VMX_PLAN_QBYTES];
    std::vector<int32_t> cuts; std::vector<int64_t> h_tboff_at;            // traceback offset at every cut
    for (int q = 0; q <= (int)plan[VMX_PLAN_CHUNKS]; ++q) { cuts.push_back((int32_t)plan[VMX_PLAN_CUTS + q]); h_tboff_at.push_back(plan[VMX_PLAN_OFFS + q]); }
    if (cuts.size() < 2) { cuts.assign(2, 0); h_tboff_at.assign(2, 0); }
    int64_t tbmax = 0;
    for (size_t q = 0; q + 1 < cuts.size(); ++q) tbmax = std::max(tbmax, h_tboff_at[q + 1] - h_tboff_at[q]);
    VMX_TRY(B.tb.reserve((size_t)tbmax + 64)); VMX_TRY(B.bnd.reserve(4 * (size_t)(totals[1] + 4))); VMX_TRY(B.run.reserve(4 * (size_t)(totals[2] + 4))); VMX_TRY(B.cig.reserve((size_t)totals[3] + 16));
    if (!cnt) return 0;
    std::vector<int32_t> csz; for (size_t q = 0; q + 1 < cuts.size(); ++q) csz.push_back(cuts[q + 1] - cuts[q]);
    VMX_TRY(vmx_push(c, B.chunkn, csz.data(), csz.size()));
    for (size_t q = 0; q + 1 < cuts.size(); ++q)
        if (!vmx_tb_base_ok(B.tb.p, h_tboff_at[q])) { set_error("gap fill: a chunk's traceback space does not start on a 64-byte line"); return VM_ERR_ARG; }
    for (int q = 0; q + 1 < (int)cuts.size(); ++q) {      // pn = the chunk's size; the kernels read it on the device (B.chunkn)
        vmx_gf_ctl* ctl = B.gfctl.as<vmx_gf_ctl>() + (size_t)(pass * (VMX_MAX_CHUNKS + 1) + q);
        hipEvent_t* ke = q < 8 ? c->gev + (pass ? 24 : 0) + 3 * q : nullptr;      // HIP events around the dominant kernel, on the stream it runs on
        vmx_gapfill_chunk(c, B, gf_score, run.ad_pct, run.prm->eqx, cuts[q], cuts[q + 1] - cuts[q], B.chunkn.as<int32_t>() + q, h_tboff_at[q], ctl, B.order.as<int32_t>() + run.round_cap + 32, run.gf_redo_cap, ke);
        if (ke) c->n_gev[pass] = q + 1;
        run.gf_chunks[pass] = q + 1;
    }
    return 0;
}
static int ext_gapfill(vmx_batch_run& run, int redo_only) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t round_cap = run.round_cap; const int64_t tb_chunk = run.knobs.once->tb_chunk;
    // per-problem tables are sized for the round's capacity
    for (int i = 0; i < 4; ++i) { VMX_TRY(B.dpsz[i].reserve(8 * (size_t)(round_cap + 2))); VMX_TRY(B.dpoff[i].reserve(8 * (size_t)(round_cap + 2))); }
    VMX_TRY(B.dptab.reserve(sizeof(vmx_dp_prob) * (size_t)(round_cap + 1))); VMX_TRY(B.ciglen.reserve(4 * (size_t)(round_cap + 1))); VMX_TRY(B.cigq.reserve(4 * (size_t)(round_cap + 1))); VMX_TRY(B.dpscore.reserve(4 * (size_t)(round_cap + 1)));
    VMX_TRY(B.order.reserve(4 * (size_t)(2 * round_cap + 64)));
    if (!redo_only) {
        // the second launch's pool, from the context's history
        run.gf_redo_cap = std::max<int64_t>((int64_t)((double)c->redo_need_max * 1.3), std::min<int64_t>((int64_t)512 << 20, std::max<int64_t>(tb_chunk / 8, 1 << 20)));
        if (run.knobs.now.redo_pool_bytes > 0 && c->redo_need_max == 0) run.gf_redo_cap = run.knobs.now.redo_pool_bytes;      // test hook: the first guess of a fresh context
        VMX_TRY(B.tbredo.reserve((size_t)run.gf_redo_cap + 64));
        run.gf_redo_cap = (int64_t)B.tbredo.cap - 64;
    }
    c->n_gev[redo_only ? 1 : 0] = 0;
    // ONE launch: string offsets, the four pool-size scans, the problem table and the chunk plan (at most VMX_TB_CHUNK traceback bytes per chunk), then the gather
    int64_t* d_plan = B.statblk.as<int64_t>() + VMX_STAT_PLAN + (redo_only ? VMX_STAT_PLAN_STRIDE : 0);
    VMX_TRY(ext_gather(run, VMX_STAT_ROUND_GF + redo_only, true, tb_chunk, d_plan));
    // the sizing wait of the batch: problem count, pool totals, chunk cuts
    VMX_TRY(vmx_fetch(c, run.plan, d_plan, (size_t)VMX_PLAN_WORDS));
    VMX_HIP(vmx_stream_sync(c));
    VMX_TRY(ext_gapfill_chunks(run, redo_only));
    run.A.redo_only = redo_only;
    run.A.spread = run.rec_spread;
    hipLaunchKernelGGL(k_ext_records, dim3((unsigned)run.n), dim3(64), 0, c->stream, run.A, B.dptab.as<vmx_dp_prob>(), B.cig.as<char>(), B.ciglen.as<int32_t>(), B.cigq.as<int32_t>());     // one wavefront per read
    run.cur ^= 1;
    return 0;
}

int vmx_extend_stage(vmx_batch_run& run) {
    vm_ctx* c = run.c;
    VMX_TRY(ext_geometry(run));
    VMX_TRY(ext_reserve_pools(run));
    ext_fill_args(run);
    ext_band_rule_read(run);
    // pass 0
    ext_phase(run, 0);
    VMX_TRY(ext_divergence_filter(run));
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_FILTER], c->stream));
    for (int ph = 1; ph <= 4; ++ph) { ext_phase(run, ph); VMX_TRY(ext_round(run)); }
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_EDGE], c->stream));
    ext_phase(run, 5); VMX_TRY(ext_gapfill(run, 0));
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_GAPFILL], c->stream));
    // pass 1: reads whose CIGARs carry paired indels are re-run with nofilter (:24079-24080)
    run.do_pass1 = c->run_pass1 || run.knobs.once->force_pass1;      // (the knob: A/B and tests, every batch runs pass 1 as in rounds 1-5)
    if (run.do_pass1) {
        run.A.redo_only = 1;
        ext_phase(run, 3); ext_phase(run, 4); ext_phase(run, 5); VMX_TRY(ext_gapfill(run, 1));
        run.A.redo_only = 0;
    }
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_PASS1], c->stream));
    return 0;
}
