// vmx_align.hip — the batched path: vm_align_batch / vm_reads_upload / vm_align_resident (include/vacmapx.h).
// Replaces get_readmap_DP_test (/root/reference/src/vacmap/mammap_clrnano.py:24023-24084) for a whole batch of reads: seed -> global
// chain -> local re-seed + chain -> extend, every stage a HIP kernel on the context's stream; the host only sizes buffers
// (a few small device->host reads of totals per batch) and launches. No CPU compute path exists.
// One pass of a batch = align_device_once: stage functions over vmx_batch_run (vmx_batch.h); the extend stage is vmx_stage_extend.hip, the host's
// decisions (pool geometry, band-width rule, statuses, splice of side batches) are vmx_batch_policy.h.
#include "vmx_host.h"
#include "vmx_stage.h"
#include "vmx_select.h"
#include "vmx_ext_state.h"
#include "vmx_round.h"
#include "vmx_batch.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>

using namespace vmx;

__global__ void k_orient(const uint8_t* codes, const int64_t* roff, const double* gscore, int n_reads, uint8_t* ocodes);
__global__ void k_scan_i64(const int64_t* in, int64_t* out, int64_t n, int pow2_round);
__global__ void k_res_sizes(const vmx_ext_read* er, const vm_record* rec, const int64_t* soff, int n_reads, int64_t* recn, int64_t* blobn);
__global__ void k_res_pack(const vmx_ext_read* er, const vm_record* rec, const char* blob, const int64_t* soff, const int64_t* blob_off, int n_reads,
                           const int64_t* rec_o, const int64_t* blob_o, vm_record* out_rec, char* out_blob);

// ---- small utility kernels
__global__ void k_compact_rows(const int64_t* __restrict__ rows, const int64_t* __restrict__ koff, const int64_t* __restrict__ aoff, int n_reads, int64_t* __restrict__ out) {
    for (int r = blockIdx.x; r < n_reads; r += gridDim.x) {
        const int64_t n4 = 4 * (aoff[r + 1] - aoff[r]);
        const int64_t* s = rows + 4 * koff[r]; int64_t* d = out + 4 * aoff[r];
        for (int64_t i = threadIdx.x; i < n4; i += blockDim.x) d[i] = s[i];
    }
}
__global__ void k_i32_to_i64(const int32_t* __restrict__ in, int64_t* __restrict__ out, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = in[i];
}
__global__ void k_readlens(const int64_t* __restrict__ roff, int64_t* __restrict__ lens, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) lens[i] = roff[i + 1] - roff[i];
}

// scalars the host wants are gathered on the device into one block and read back with ONE copy (a hipMemcpyAsync per scalar is a
// runtime copy kernel each: ~100 of them per batch before)
// (gap-fill sizing on the device — pool totals and the cut of the problems into traceback chunks — is the last step of k_round_prep<true>, k_round.hip)
__global__ void k_final_scalars(const int64_t* nr, const int64_t* nb, const int32_t* oflow, const int32_t* edc, const int32_t* rounds, int64_t* __restrict__ out) {
    out[VMX_FIN_NREC] = *nr; out[VMX_FIN_NBLOB] = *nb; out[VMX_FIN_OFLOW] = *oflow; out[VMX_FIN_ED_FULL] = edc[0]; out[VMX_FIN_ED_TIER2] = edc[1]; out[VMX_FIN_ED_TIER1] = edc[2];      // (edc: B.qrange from VMX_QR_NFULL on)
    for (int i = 0; i < VMX_STAT_ROUNDS; ++i) out[VMX_FIN_ROUNDS + i] = rounds[i];
}

struct vm_reads { vm_ctx* ctx; int64_t n; std::vector<int64_t> h_off; DevBuf raw, codes, off; };

vmx_batch_bufs* vmx_ctx_batch_bufs(vm_ctx* c) { if (!c->bbufs) c->bbufs = new vmx_batch_bufs(); return c->bbufs; }

// the one place this file and vmx_stage_extend.hip read the environment (vmx_align_knobs, vmx_batch.h: which knob is latched and which is read per call, and why)
vmx_align_knobs vmx_align_knobs_read() {
    static const vmx_align_knobs::once_t latched = [] {
        const auto num = [](const char* name, int lo, int hi, int dflt) { const char* e = getenv(name); const int v = e ? atoi(e) : dflt; return v >= lo && v <= hi ? v : dflt; };
        const auto off_at_zero = [](const char* name) { const char* e = getenv(name); return !(e && atoi(e) == 0); };
        vmx_align_knobs::once_t k;
        k.select_serial = getenv("VMX_SELECT_SERIAL") != nullptr;
        { const char* e = getenv("VMX_GC_LDS_MAX"); k.gc_lds_max = e ? atoi(e) : -1; }
        k.trace_spread = num("VMX_TRACE_SPREAD", 1, 64, 1); k.ext_spread = num("VMX_EXT_SPREAD", 1, 64, 0); k.rec_spread = num("VMX_REC_SPREAD", 1, 64, 0);
        k.local_sync = getenv("VMX_LOCAL_SYNC") != nullptr; k.seed_arena = off_at_zero("VMX_SEED_ARENA"); k.ext_wave = off_at_zero("VMX_EXT_WAVE");
        { const char* e = getenv("VMX_TB_CHUNK_GB"); const double v = e ? atof(e) : 0.0; k.tb_chunk = v > 0.5 ? (int64_t)(v * (double)(1 << 30)) : (int64_t)VMX_TB_CHUNK; }
        { const char* e = getenv("VMX_MAX_BATCH_BASES"); const long long x = e ? atoll(e) : 0; k.max_batch_bases = x > 0 ? (int64_t)x : (int64_t)VMX_MAX_BATCH_BASES; }
        k.force_exact = getenv("VMX_FORCE_EXACT") != nullptr; k.force_pass1 = getenv("VMX_FORCE_PASS1") != nullptr;
        return k;
    }();
    vmx_align_knobs k; k.once = &latched;
    vmx_align_knobs::call_t& w = k.now;
    w.ext_tmask = 0; w.ext_tdiv = 1;
    if (const char* e = getenv("VMX_TEST_EXT_POOL")) { long long m_ = 0, d_ = 1; if (sscanf(e, "%lld:%lld", &m_, &d_) == 2 && d_ >= 1) { w.ext_tmask = (int)m_; w.ext_tdiv = d_; } }
    { const char* e = getenv("VMX_TEST_REDO_POOL_BYTES"); w.redo_pool_bytes = e ? atoll(e) : 0; }
    { const char* e = getenv("VMX_TEST_SIDE_EVERY"); w.side_every = e ? atoll(e) : 0; }
    { const char* e = getenv("VMX_TEST_OOM_ABOVE_BASES"); w.oom_above_bases = e ? atoll(e) : 0; }
    w.ad_pinned = getenv("VMX_AD_PCT") != nullptr || getenv("VMX_AD_PCT_MIN") != nullptr;
    w.fill_waves = 16; if (const char* e = getenv("VMX_FILL_WAVES")) { const int v = atoi(e); if (v >= 1 && v <= 32) w.fill_waves = v; }
    w.dbg_pools = getenv("VMX_DBG_POOLS") != nullptr;
    return k;
}

// k_chain_select by LDS size class: a read claims 17 B of LDS per anchor for its serial peel, so a launch whose reads have at most `cap`
// anchors asks for exactly that (a fixed 52 KB claim kept three waves on a CU — and next to another batch's kernels often none);
// reads beyond the largest class keep everything in HBM. Inside a class the reads with most anchors go first.
int vmx_launch_chain_select(vm_ctx* c, int64_t n, const int64_t* h_aoff, DevBuf& d_list, const vmx_anchor* sorted, const int64_t* d_aoff, const int64_t* d_lens,
                            const double* S, const int32_t* P, const int32_t* SA, const int64_t* gmax, const int32_t* flip, int mode, char* scr, const int64_t* soff,
                            int32_t* d_mapq, double* d_score, int32_t* d_np, int32_t* plen, vmx_anchor* prow) {
    if (n <= 0) return 0;
    constexpr int NC = 6;
    const int caps[NC] = {192, 384, 768, 1536, 3072, 0};
    const bool serial_peel = vmx_align_knobs_read().once->select_serial;      // A/B knob: the one-lane peel of round 3
    std::vector<int32_t> lists[NC];
    for (int64_t r = 0; r < n; ++r) {
        const int64_t m = h_aoff[r + 1] - h_aoff[r];
        int q = NC - 1; for (int i = 0; i < NC - 1; ++i) if (m <= caps[i]) { q = i; break; }
        lists[q].push_back((int32_t)r);
    }
    std::vector<int32_t> rl; size_t off[NC + 1];
    for (int q = 0; q < NC; ++q) {
        std::stable_sort(lists[q].begin(), lists[q].end(), [&h_aoff](int32_t a, int32_t b) { return h_aoff[a + 1] - h_aoff[a] > h_aoff[b + 1] - h_aoff[b]; });
        off[q] = rl.size(); rl.insert(rl.end(), lists[q].begin(), lists[q].end());
    }
    VMX_TRY(vmx_push(c, d_list, rl.data(), rl.size()));
    vmx_fork fk(c);
    for (int q = NC - 1; q >= 0; --q) {                          // the classes with the longest walks first
        const int cnt = (int)lists[q].size(); if (!cnt) continue;
        hipLaunchKernelGGL(k_chain_select, dim3((unsigned)cnt), dim3(64), (size_t)caps[q] * 17 + 64, fk.next(), sorted, d_aoff, serial_peel ? nullptr : d_lens, d_list.as<int32_t>() + off[q], cnt, caps[q],
                           S, P, SA, gmax, flip, mode, scr, soff, d_mapq, d_score, d_np, plen, prow);
    }
    fk.join();
    return 0;
}

// S2 + G1/G2 global chain, G3 GC-fast and the selection (vmx_stage.h)
int vmx_global_stage(vm_ctx* c, vmx_batch_bufs& B, const vm_params* prm, int k, int64_t n, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                     const std::vector<int64_t>& h_aoff, int rmode, int32_t* d_ran) {
    const int64_t tot = h_aoff[n], total_bases = h_roff[n];
    std::vector<int64_t> koff((size_t)n + 1), soff((size_t)n + 1);
    int64_t kt = 0, stt = 0;
    for (int64_t r = 0; r < n; ++r) {
        int64_t m = h_aoff[r + 1] - h_aoff[r]; int64_t N = 1; while (N < m) N <<= 1;
        koff[r] = kt; kt += N; soff[r] = stt; stt += (vmx_select_scratch_bytes(m) + 15) & ~(int64_t)15;
    }
    koff[n] = kt; soff[n] = stt;
    VMX_TRY(B.keys.reserve(8 * (size_t)(kt + 1))); VMX_TRY(vmx_push(c, B.koff, koff.data(), (size_t)n + 1));
    VMX_TRY(B.sorted.reserve(sizeof(vmx_anchor) * (size_t)(tot + 1))); VMX_TRY(B.flip.reserve(4 * (size_t)(n + 1)));
    hipLaunchKernelGGL(k_flip_sort, dim3((unsigned)std::min<int64_t>(n, (int64_t)c->num_cu * 8)), dim3(256), 0, c->stream, B.rows.as<int64_t>(), B.aoff.as<int64_t>(), B.lens.as<int64_t>(),
                       (int)n, B.keys.as<uint64_t>(), B.koff.as<int64_t>(), B.sorted.as<vmx_anchor>(), B.flip.as<int32_t>());
    VMX_TRY(B.S.reserve(8 * (size_t)(tot + 1))); VMX_TRY(B.P.reserve(4 * (size_t)(tot + 1))); VMX_TRY(B.SA.reserve(4 * (size_t)(tot + 1)));
    VMX_TRY(B.cov.reserve((size_t)tot + 16)); VMX_TRY(B.gmax.reserve(8 * (size_t)(n + 1))); VMX_TRY(B.opc.reserve(8 * (size_t)(n + 1)));
    const HostTables& T = host_tables();
    {   // gapcost_list (:24843-24846): 0.01*k*g + 0.5*log2(g), evaluated in double exactly like the reference
        if (prm->global_maxdiff > 62) { set_error("global_maxdiff > 62 unsupported"); return VM_ERR_UNSUPPORTED; }
        std::vector<double> gap(64, 0.0);
        for (int g = 1; g <= prm->global_maxdiff; ++g) gap[g] = (0.01 * k * g + 0.5 * T.log2int[g]);
        VMX_TRY(vmx_push(c, B.gap, gap.data(), 64));
    }
    if (rmode == 1) { VMX_TRY(B.fp.reserve(8 * (size_t)(tot + 1))); VMX_TRY(B.pp.reserve(8 * (size_t)(tot + 1))); }   // fixed_penatly / pre_penatly of mode R's chain
    // LDS buckets by anchor count (25 B per anchor), reads longest-first inside a bucket, one workgroup per read (see vmx_local_stage)
    constexpr int NB = 10;
    const int caps[NB] = {384, 512, 768, 1024, 1536, 2048, 3072, 4096, 8192, 13056};
    std::vector<int32_t> lists[NB + 1];
    std::vector<int64_t> asm_long;
    const int gc_lds_env = vmx_align_knobs_read().once->gc_lds_max;     // VMX_GC_LDS_MAX, see vmx_stage_local.hip
    const int gc_lds_max = gc_lds_env >= 0 ? gc_lds_env : VMX_CHAIN_LDS_MAX_SHARED;
    const bool rows_kernel = vmx_chain_rows_on() && rmode != 2;          // four reads per wavefront (k_chain_rows.hip); -mode asm keeps the one-wave kernel
    for (int64_t r = 0; r < n; ++r) {
        int64_t m = h_aoff[r + 1] - h_aoff[r]; const int64_t L = h_roff[r + 1] - h_roff[r];
        if (m <= 2) continue;                                             // :23986 unmapped
        if (prm->mode == VM_MODE_ASM && L >= 500000) { asm_long.push_back(r); continue; }      // mammap_asm.py:23205: the linked path, not built on the device
        if ((double)m / (double)L > 5.0) continue;                        // fast_enable (:23570): gmax stays -1 -> k_chain_global_fast below
        int bk = NB; for (int q = 0; q < NB; ++q) if (m <= caps[q] && caps[q] <= gc_lds_max) { bk = q; break; }
        if (rows_kernel) bk = NB;                                         // k_chain_global_rows: one list, nothing in LDS
        lists[bk].push_back((int32_t)r);
    }
    {
        std::vector<int32_t> rl; int64_t rl_off[NB + 2];
        for (int q = 0; q <= NB; ++q) {
            std::stable_sort(lists[q].begin(), lists[q].end(), [&h_aoff](int32_t a, int32_t b) { return h_aoff[a + 1] - h_aoff[a] > h_aoff[b + 1] - h_aoff[b]; });
            rl_off[q] = (int64_t)rl.size(); rl.insert(rl.end(), lists[q].begin(), lists[q].end());
        }
        VMX_TRY(vmx_push(c, B.rl, rl.data(), rl.size()));
        VMX_HIP(hipMemsetAsync(B.gmax.p, 0xff, 8 * (size_t)n, c->stream));
        { static const int64_t kUnsupported = -4; for (int64_t r : asm_long) VMX_HIP(hipMemcpyAsync(B.gmax.as<int64_t>() + r, &kUnsupported, 8, hipMemcpyHostToDevice, c->stream)); }
#ifndef VMX_EMU
        VMX_HIP(hipFuncSetAttribute((const void*)k_chain_global, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((size_t)caps[NB - 1] * VMX_GC_BYTES_PER_ANCHOR + 64)));
#endif
        vmx_fork fk(c);                                               // the LDS buckets are independent: run them side by side
        for (int q = NB; q >= 0; --q) {                               // slowest (largest reads) first
            int cnt = (int)lists[q].size(); if (!cnt) continue;
            int cap = q < NB ? caps[q] : 0; size_t shmem = (size_t)cap * VMX_GC_BYTES_PER_ANCHOR + 64;
            if (rows_kernel) {
                hipLaunchKernelGGL((vmx_chain_rows_win3() ? k_chain_global_rows_w3 : k_chain_global_rows), dim3((unsigned)((cnt + 3) / 4)), dim3(64), 0, fk.next(), B.sorted.as<vmx_anchor>(), B.aoff.as<int64_t>(),
                                   B.rl.as<int32_t>() + rl_off[q], cnt, c->tables, B.gap.as<double>(), prm->global_skipcost, prm->global_maxdiff, 1000, B.S.as<double>(),
                                   B.P.as<int32_t>(), B.SA.as<int32_t>(), B.cov.as<uint8_t>(), B.gmax.as<int64_t>(), B.opc.as<int64_t>(), rmode, B.fp.as<double>(), B.pp.as<double>(),
                                   vmx_chain_dbg());
                continue;
            }
            hipLaunchKernelGGL(k_chain_global, dim3((unsigned)cnt), dim3(64), shmem, fk.next(), B.sorted.as<vmx_anchor>(), B.aoff.as<int64_t>(),
                               B.rl.as<int32_t>() + rl_off[q], cnt, cap, c->tables, B.gap.as<double>(), prm->global_skipcost, prm->global_maxdiff, 1000, B.S.as<double>(),
                               B.P.as<int32_t>(), B.SA.as<int32_t>(), B.cov.as<uint8_t>(), B.gmax.as<int64_t>(), B.opc.as<int64_t>(), rmode, B.fp.as<double>(), B.pp.as<double>());
        }
        fk.join();
        vmx_chain_dbg_report(c->stream);
        // G3: reads left at gmax = -1 (more than 5 anchors per base, :23570, or GC-exact's opcount bail-out, :24914) take GC-fast.
        // One wave per read; reads that do not need it return at once.
        VMX_TRY(B.si.reserve(4 * (size_t)(tot + 1))); VMX_TRY(B.tg.reserve(8 * (size_t)(tot + 1))); VMX_TRY(B.cntp.reserve(4 * (size_t)(total_bases + 50 * n + 64)));
        hipLaunchKernelGGL(k_chain_global_fast, dim3((unsigned)n), dim3(64), 0, c->stream, B.sorted.as<vmx_anchor>(), B.aoff.as<int64_t>(), (int)n, d_roff, c->tables,
                           B.gap.as<double>(), prm->global_skipcost, prm->global_maxdiff, 1000, B.S.as<double>(), B.P.as<int32_t>(), B.SA.as<int32_t>(), B.cov.as<uint8_t>(),
                           B.si.as<int32_t>(), B.tg.as<int64_t>(), B.cntp.as<int32_t>(), B.gmax.as<int64_t>(), d_ran, rmode, B.fp.as<double>(), B.pp.as<double>());
    }
    VMX_TRY(B.scr.reserve((size_t)stt + 64)); VMX_TRY(vmx_push(c, B.soff, soff.data(), (size_t)n + 1));
    VMX_TRY(B.res.reserve(16 * (size_t)(n + 2) + 64));
    double* d_gscore; int32_t* d_mapq; int32_t* d_np; vmx_res_ptrs(B, n, &d_gscore, &d_mapq, &d_np);
    VMX_TRY(B.plen.reserve(4 * (size_t)(tot + 1))); VMX_TRY(B.prow.reserve(sizeof(vmx_anchor) * (size_t)(tot + 1)));
    return vmx_launch_chain_select(c, n, h_aoff.data(), B.sellist, B.sorted.as<vmx_anchor>(), B.aoff.as<int64_t>(), B.lens.as<int64_t>(), B.S.as<double>(), B.P.as<int32_t>(), B.SA.as<int32_t>(),
                                   B.gmax.as<int64_t>(), B.flip.as<int32_t>(), prm->mode, B.scr.as<char>(), B.soff.as<int64_t>(), d_mapq, d_gscore, d_np, B.plen.as<int32_t>(), B.prow.as<vmx_anchor>());
}

#define LAUNCH1D(kernel, n, ...) hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(((n) + 255) / 256, 4096))), dim3(256), 0, c->stream, __VA_ARGS__)

int vmx_asm_resolve_ties(vm_ctx* c, const vm_index* mi, int64_t n, const std::vector<int64_t>& h_roff, const std::vector<int64_t>& h_aoff, const uint8_t* d_codes,
                         const vmx_anchor* d_sorted, const double* d_S, const int32_t* d_P, const int32_t* d_SA, const int64_t* d_gmax, const int32_t* d_flip,
                         int32_t* d_mapq, double* d_gscore, int32_t* d_np, int32_t* d_plen, vmx_anchor* d_prow, std::vector<int32_t>& status_override);
int vmx_align_batch_asm_mixed(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const char* seqs, const int64_t* offsets, vm_record** recs, int64_t* n_recs,
                              char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats);
int align_device(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                 vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats, vmx_seg_trace* trace = nullptr, const vmx_preset* preset = nullptr);

static int align_device_once(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                             vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats, vmx_seg_trace* trace, const vmx_preset* preset);
// The pools of the extend stage are sized from bounds that hold by construction for the reference's segment surgery (a chain never has more segments than
// anchors, a round never more problems than anchors, ...) — and where a bound is an estimate (the problem strings of a round: 6 bytes per read base) or a
// construction turns out wrong for some input, THE READ reports it (VMX_EXT_CAPACITY_DEV; round 6: k_gather's string pools mark the owning read as well).
// Round 6: the batch is NOT run again as a whole with every pool x4 — that multiplied ~10 GB of grow-only pools for all 4096 reads because of one
// read, could exhaust the HBM next to the other contexts, and left the pools inflated for the life of the context. The reads that reported it (a handful, if
// any) are run again ALONE as a side batch with their pools x4, x16, ... x1024: a few reads' pools times 1024 still fit inside what the whole batch holds, so
// nothing grows; their records are spliced into the batch's. A read that is still short at x1024 — or whose side batch finds no device memory — is reported as
// VM_READ_CAPACITY; the rest of the batch is unaffected. VMX_TEST_EXT_POOL=<mask>:<div> (tests) divides the pools the mask names (1 segment anchors, 2 segments,
// 4 record blob, 8 problems per round, 16 problem strings) so that each of these ends is exercised.
__global__ void k_side_codes(const uint8_t* __restrict__ codes, const int64_t* __restrict__ roff, const int32_t* __restrict__ pick, const int64_t* __restrict__ soff, int n, uint8_t* __restrict__ out) {
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const int64_t a = roff[pick[j]], len = roff[pick[j] + 1] - a; const uint8_t* s = codes + a; uint8_t* d = out + soff[j];
        for (int64_t i = threadIdx.x; i < len; i += blockDim.x) d[i] = s[i];
    }
}
// align_device_once until it no longer asks to be run again, six times at the most. retries: the runs after the first. Returns VMX_RETRY_BATCH when the sixth still asked.
static int align_device_attempts(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                                 vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status, vm_batch_stats* st, vmx_seg_trace* trace, const vmx_preset* preset, int64_t* retries) {
    int rc = VMX_RETRY_BATCH;
    for (int attempt = 0; attempt < 6 && rc == VMX_RETRY_BATCH; ++attempt) {
        if (attempt) { if (retries) ++*retries; if (trace) { trace->rows.clear(); trace->off.clear(); } }
        rc = align_device_once(c, mi, prm, n, d_codes, d_roff, h_roff, recs, n_recs, cigar_blob, status, st, trace, preset);
    }
    return rc;
}
// what a side batch switches on in the context is switched off again on every way out of align_device
struct vmx_side_mode_guard { vm_ctx* c; ~vmx_side_mode_guard() { c->ext_mul = 1; c->force_exact = false; c->run_pass1 = false; } };

// the reads in `sub` alone, as side batches with everything switched on and the pools x4 ... x1024, until none is short of a pool; their records go into sp, their statuses
// into status. What is left in sub afterwards could not be helped (VM_READ_CAPACITY). retries: side batches run.
static int align_side_batches(vm_ctx* c, const vm_index* mi, const vm_params* prm, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff, const vmx_preset* preset,
                              std::vector<int32_t>& sub, std::vector<int32_t>& status, vmx_splice& sp, vm_batch_stats& st, int64_t& retries) {
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    while (!sub.empty()) {
        bool any_short = false; for (int32_t r : sub) any_short = any_short || status[(size_t)r] == VMX_EXT_SHORT_INTERNAL;
        if (any_short) { if (c->ext_mul >= 1024) break; c->ext_mul *= 4; }       // (reads that only need the filter's later tiers keep the pools as they are)
        c->force_exact = true; c->run_pass1 = true; ++retries;
        if (vmx_align_knobs_read().now.dbg_pools) fprintf(stderr, "[pools] extend stage: %zu read(s) run again alone (pools x%d, every tier of the divergence filter)\n", sub.size(), c->ext_mul);
        const int64_t m = (int64_t)sub.size();
        std::vector<int64_t> s_off((size_t)m + 1, 0); std::vector<vmx_preset> s_pre;
        for (int64_t j = 0; j < m; ++j) { s_off[(size_t)j + 1] = s_off[(size_t)j] + (h_roff[(size_t)sub[(size_t)j] + 1] - h_roff[(size_t)sub[(size_t)j]]); if (preset) s_pre.push_back(preset[sub[(size_t)j]]); }
        int src = 0;
        if ((src = B.side_codes.reserve((size_t)s_off[(size_t)m] + 64)) < 0 || (src = vmx_push(c, B.side_off, s_off.data(), (size_t)m + 1)) < 0 ||
            (src = vmx_push(c, B.sellist, sub.data(), (size_t)m)) < 0) { if (src == VM_ERR_OOM) break; return src; }
        hipLaunchKernelGGL(k_side_codes, dim3((unsigned)std::min<int64_t>(m, (int64_t)c->num_cu * 8)), dim3(256), 0, c->stream, d_codes, d_roff, B.sellist.as<int32_t>(), B.side_off.as<int64_t>(), (int)m,
                           B.side_codes.as<uint8_t>());
        vm_record* r2 = nullptr; int64_t n2 = 0; char* b2 = nullptr; vm_batch_stats st2; std::vector<int32_t> status2((size_t)m + 1, 0);
        src = align_device_attempts(c, mi, prm, m, B.side_codes.as<uint8_t>(), B.side_off.as<int64_t>(), s_off, &r2, &n2, &b2, status2.data(), &st2, nullptr, preset ? s_pre.data() : nullptr, nullptr);
        if (src == VMX_RETRY_BATCH) src = VM_ERR_OOM;
        if (src == VM_ERR_OOM) { free(r2); free(b2); break; }                 // no room for the larger pools: these reads are reported, the batch stands
        if (src < 0) { free(r2); free(b2); return src; }
        std::vector<int32_t> still;
        for (int64_t j = 0; j < m; ++j) { status[(size_t)sub[(size_t)j]] = status2[(size_t)j]; if (status2[(size_t)j] == VMX_EXT_SHORT_INTERNAL) still.push_back(sub[(size_t)j]); }
        sp.add_side(r2, n2, b2, sub);
        free(r2); free(b2);
        vmx_stats_add_side(st, st2);
        sub.swap(still);
    }
    return 0;
}

int align_device(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                 vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats, vmx_seg_trace* trace, const vmx_preset* preset) {
    c->ext_mul = 1;
    vmx_side_mode_guard mode_guard{c};
    std::vector<int32_t> status((size_t)n + 1, 0);
    vm_batch_stats st; memset(&st, 0, sizeof st);
    int64_t batch_retries = 0;
    const int rc = align_device_attempts(c, mi, prm, n, d_codes, d_roff, h_roff, recs, n_recs, cigar_blob, status.data(), &st, trace, preset, &batch_retries);
    if (rc == VMX_RETRY_BATCH) { set_error("the batch was run again five times and its pools still did not hold it"); return VM_ERR_OOM; }
    if (rc < 0) return rc;
    st.n_batch_retries = batch_retries;
    std::vector<int32_t> sub;                                    // reads of the batch that were short of an extend-stage pool, or need what a batch does not run
    for (int64_t r = 0; r < n; ++r) if (status[(size_t)r] == VMX_EXT_SHORT_INTERNAL || status[(size_t)r] == VMX_EXT_EXACT_INTERNAL) sub.push_back((int32_t)r);
    if (!sub.empty()) {
        vmx_splice sp; sp.begin(*recs, *n_recs, *cigar_blob, n, sub);
        free(*recs); free(*cigar_blob); *recs = nullptr; *cigar_blob = nullptr; *n_recs = 0;
        int64_t retries = 0;
        VMX_TRY(align_side_batches(c, mi, prm, d_codes, d_roff, h_roff, preset, sub, status, sp, st, retries));
        for (int32_t r : sub) status[(size_t)r] = VM_READ_CAPACITY;
        sp.finish();
        *recs = (vm_record*)malloc(sizeof(vm_record) * std::max<size_t>(sp.all.size(), 1)); *cigar_blob = (char*)malloc(std::max<size_t>(sp.blob.size(), 1));
        if (!*recs || !*cigar_blob) { free(*recs); free(*cigar_blob); *recs = nullptr; *cigar_blob = nullptr; set_error("out of host memory"); return VM_ERR_OOM; }
        memcpy(*recs, sp.all.data(), sizeof(vm_record) * sp.all.size()); memcpy(*cigar_blob, sp.blob.data(), sp.blob.size());
        *n_recs = (int64_t)sp.all.size();
        st.n_ext_retries = retries; sp.counters(status, n, st);
    }
    if (status_per_read) memcpy(status_per_read, status.data(), 4 * (size_t)n);
    if (stats) *stats = st;
    return VM_OK;
}

// ---- one pass of a batch over the path: state (vmx_batch_run, vmx_batch.h) and stages
vmx_batch_run::vmx_batch_run(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                             const vmx_preset* preset, vmx_seg_trace* trace)
    : c(c), mi(mi), prm(prm), n(n), d_codes(d_codes), d_roff(d_roff), h_roff(h_roff), preset(preset), trace(trace), total_bases(h_roff[(size_t)n]), knobs(vmx_align_knobs_read()),
      B(*vmx_ctx_batch_bufs(c)), L(*vmx_ctx_local_bufs(c)), h_aoff((size_t)n + 1, 0),
      rmode(prm->mode == VM_MODE_R ? 1 : (prm->mode == VM_MODE_ASM ? 2 : 0)) {
    vmx_index_view(mi, &ix);
    memset(&A, 0, sizeof A);
    memset(&st, 0, sizeof st); st.n_reads = n; st.read_bases = total_bases;
    // Round 6: after a context's first batch the LOCAL stage runs without a host wait (vmx_local_stage's fast form) and the extend stage's per-read pool geometry is made
    // on the device (k_ext_geometry) inside pools sized from the context's history — one wait less per batch. A read whose slice does not fit, whose anchors overflow
    // their slot or that the banded seeding kernel hands back is run again alone on the waiting path (side batches, above). VMX_LOCAL_SYNC=1: the waiting path always;
    // VMX_TEST_EXT_POOL (pools of exact size divided) needs the waiting path too.
    fast_local = !preset && !trace && !c->force_exact && !knobs.once->local_sync && vmx_chain_rows_on() && rmode != 2 && c->geo_valid && c->ext_mul == 1 && knobs.now.ext_tmask == 0;
}

// the stages in front of the extension: seed, global chain, local chain
int batch_front(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const vm_params* prm = run.prm; const int64_t n = run.n; vm_batch_stats& st = run.st;
    // ---------------- S1 seed
    std::vector<int64_t> h_koff, h_nhits;
    int64_t* d_seed_rows = nullptr;
    VMX_TRY(vmx_seed_stage(c, run.mi, prm->check_num, prm->mid_occ, n, run.d_codes, run.d_roff, run.total_bases, B.seed, h_koff, h_nhits, run.knobs.once->seed_arena ? &B.tb : nullptr, &d_seed_rows));
    for (int64_t r = 0; r < n; ++r) st.n_hits += h_nhits[r];
    st.n_minimizers = c->last_n_minimizers;
    // compact anchors: aoff = scan(n_anchors)
    VMX_TRY(B.nanc64.reserve(8 * (size_t)(n + 2))); VMX_TRY(B.aoff.reserve(8 * (size_t)(n + 2)));
    LAUNCH1D(k_i32_to_i64, n, B.seed.nanc.as<int32_t>(), B.nanc64.as<int64_t>(), n);
    hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(256), 0, c->stream, B.nanc64.as<int64_t>(), B.aoff.as<int64_t>(), n, 0);
    VMX_TRY(vmx_fetch(c, run.h_aoff.data(), B.aoff.p, (size_t)n + 1));
    VMX_HIP(vmx_stream_sync(c));
    const int64_t tot = run.h_aoff[n];
    st.n_anchors = tot;
    VMX_TRY(B.rows.reserve(32 * (size_t)(tot + 1)));
    hipLaunchKernelGGL(k_compact_rows, dim3((unsigned)std::min<int64_t>(n, (int64_t)c->num_cu * 8)), dim3(128), 0, c->stream, d_seed_rows, B.seed.koff.as<int64_t>(),
                       B.aoff.as<int64_t>(), (int)n, B.rows.as<int64_t>());
    VMX_TRY(B.lens.reserve(8 * (size_t)(n + 1)));
    LAUNCH1D(k_readlens, n, run.d_roff, B.lens.as<int64_t>(), n);
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_SEED], c->stream));

    // ---------------- S2 + G1/G2 global chain, G3, selection
    VMX_TRY(vmx_global_stage(c, B, prm, run.ix.k, n, run.d_roff, run.h_roff, run.h_aoff, run.rmode, nullptr));
    vmx_res_ptrs(B, n, &run.d_gscore, &run.d_mapq, &run.d_np);
    if (prm->mode == VM_MODE_ASM)        // decode_hit's edlib tie-break among equal chains (mammap_asm.py:21302-21326): marked contigs are settled here
        VMX_TRY(vmx_asm_resolve_ties(c, run.mi, n, run.h_roff, run.h_aoff, run.d_codes, B.sorted.as<vmx_anchor>(), B.S.as<double>(), B.P.as<int32_t>(), B.SA.as<int32_t>(), B.gmax.as<int64_t>(),
                                     B.flip.as<int32_t>(), run.d_mapq, run.d_gscore, run.d_np, B.plen.as<int32_t>(), B.prow.as<vmx_anchor>(), run.asm_override));
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_GLOBAL], c->stream));

    // ---------------- orient + L1-L4 local stage
    VMX_TRY(B.ocodes.reserve((size_t)run.total_bases + 64));
    hipLaunchKernelGGL(k_orient, dim3((unsigned)std::min<int64_t>(n, (int64_t)c->num_cu * 8)), dim3(256), 0, c->stream, run.d_codes, run.d_roff, run.d_gscore, (int)n, B.ocodes.as<uint8_t>());
    VMX_TRY(vmx_local_stage(c, run.ix, prm, n, B.ocodes.as<uint8_t>(), run.d_roff, run.h_roff, B.prow.as<vmx_anchor>(), B.plen.as<int32_t>(), run.d_np, B.aoff.as<int64_t>(), run.h_aoff, run.d_gscore, run.L, run.fast_local));
    if (!run.fast_local) for (int64_t r = 0; r < n; ++r) st.n_local_anchors += run.L.h_la_cnt[r];
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_LOCAL], c->stream));
    return 0;
}

// -mode asm, contig of 500 kb and more (vmx_asm.hip): the chain comes from the linked DPs; the extend stage runs on it as
// ass_extend_func does (mammap_asm.py:23423-23460): forward orientation, MAPQ 60
int batch_front_preset(vmx_batch_run& run) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; vmx_local_bufs& L = run.L; const vmx_preset* preset = run.preset; const int64_t n = run.n;
    int64_t tot_chain = 0;
    for (int64_t r = 0; r < n; ++r) { if (preset[r].len < 2) { set_error("preset chain: every contig needs a chain of two anchors or more"); return VM_ERR_ARG; } tot_chain += preset[r].len; }
    VMX_TRY(B.ocodes.reserve((size_t)run.total_bases + 64));
    VMX_HIP(hipMemcpyAsync(B.ocodes.p, run.d_codes, (size_t)run.total_bases, hipMemcpyDeviceToDevice, c->stream));
    VMX_TRY(B.res.reserve(16 * (size_t)(n + 2) + 64));
    vmx_res_ptrs(B, n, &run.d_gscore, &run.d_mapq, &run.d_np);
    std::vector<double> gs((size_t)n, 1.0); std::vector<int32_t> mq((size_t)n, 60), one((size_t)n, 1), zero((size_t)n, 0), len32((size_t)n);
    std::vector<vmx_anchor> chains; chains.reserve((size_t)tot_chain);
    L.h_la_off.assign((size_t)n + 1, 0); L.h_la_cnt.assign((size_t)n, 0);
    for (int64_t r = 0; r < n; ++r) {
        len32[(size_t)r] = (int32_t)preset[r].len; L.h_la_cnt[(size_t)r] = (int32_t)preset[r].len; L.h_la_off[(size_t)r + 1] = L.h_la_off[(size_t)r] + preset[r].len;
        chains.insert(chains.end(), preset[r].chain_desc, preset[r].chain_desc + preset[r].len);
        run.h_aoff[(size_t)r + 1] = run.h_aoff[(size_t)r] + 3;
    }
    VMX_HIP(hipMemcpyAsync(run.d_gscore, gs.data(), 8 * (size_t)n, hipMemcpyHostToDevice, c->stream)); VMX_HIP(hipMemcpyAsync(run.d_mapq, mq.data(), 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VMX_HIP(hipMemcpyAsync(run.d_np, one.data(), 4 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    VMX_TRY(B.gmax.reserve(8 * (size_t)(n + 1))); VMX_HIP(hipMemsetAsync(B.gmax.p, 0, 8 * (size_t)n, c->stream));
    VMX_TRY(vmx_push(c, L.la_off, L.h_la_off.data(), (size_t)n + 1));
    VMX_TRY(vmx_push(c, L.chain, chains.data(), chains.size()));
    VMX_TRY(vmx_push(c, L.chain_len, len32.data(), (size_t)n));
    VMX_TRY(vmx_push(c, L.status, zero.data(), (size_t)n));
    VMX_HIP(vmx_stream_sync(c));                              // the host vectors above are on their way
    for (int e = VMX_EV_SEED; e <= VMX_EV_LOCAL; ++e) VMX_HIP(hipEventRecord(c->ev[e], c->stream));
    return 0;
}

// ---------------- results: pack the records of the batch on the device, then copy exactly those bytes
int batch_results(vmx_batch_run& run, vm_record** recs, char** cigar_blob) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t n = run.n, cS = run.cS, cB = run.cB; vm_batch_stats& st = run.st;
    VMX_TRY(B.dpsz[0].reserve(8 * (size_t)(n + 2))); VMX_TRY(B.dpsz[1].reserve(8 * (size_t)(n + 2))); VMX_TRY(B.dpoff[0].reserve(8 * (size_t)(n + 2))); VMX_TRY(B.dpoff[1].reserve(8 * (size_t)(n + 2)));
    hipLaunchKernelGGL(k_res_sizes, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, B.er.as<vmx_ext_read>(), B.rec.as<vm_record>(), B.soff2.as<int64_t>(), (int)n, B.dpsz[0].as<int64_t>(), B.dpsz[1].as<int64_t>());
    hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(256), 0, c->stream, B.dpsz[0].as<int64_t>(), B.dpoff[0].as<int64_t>(), n, 0);
    hipLaunchKernelGGL(k_scan_i64, dim3(1), dim3(256), 0, c->stream, B.dpsz[1].as<int64_t>(), B.dpoff[1].as<int64_t>(), n, 0);
    hipLaunchKernelGGL(k_final_scalars, dim3(1), dim3(1), 0, c->stream, B.dpoff[0].as<int64_t>() + n, B.dpoff[1].as<int64_t>() + n, B.oflow.as<int32_t>(), B.qrange.as<int32_t>() + VMX_QR_NFULL,
                       B.statblk.as<int32_t>(), B.statblk.as<int64_t>() + VMX_STAT_FIN);
    // ONE wait for the results: the packed buffers on the device have room for the worst case (cS records, cB CIGAR bytes), so the pack
    // kernel runs before the totals are known on the host, and the host copies as many records / bytes as the context's history
    // suggests for a batch of this size (vmx_result_guess). Only when a batch exceeds the guess — the
    // first batch of a context always does — the missing tail costs a second copy and wait (batch_results_tail).
    VMX_TRY(B.totals.reserve(sizeof(vm_record) * (size_t)(cS + 1))); VMX_TRY(B.dupd.reserve((size_t)cB + 64));
    hipLaunchKernelGGL(k_res_pack, dim3((unsigned)std::min<int64_t>(n, (int64_t)c->num_cu * 8)), dim3(64), 0, c->stream, B.er.as<vmx_ext_read>(), B.rec.as<vm_record>(), B.blob.as<char>(),
                       B.soff2.as<int64_t>(), B.bloboff.as<int64_t>(), (int)n, B.dpoff[0].as<int64_t>(), B.dpoff[1].as<int64_t>(), B.totals.as<vm_record>(), B.dupd.as<char>());
    const vmx_res_guess g = vmx_result_guess(c->res_rec_per_read, c->res_blob_per_base, n, run.total_bases, cS, cB);
    run.g_nr = g.nr; run.g_nb = g.nb;
    run.er.resize((size_t)n); run.h_gmax.resize((size_t)n);
    *recs = (vm_record*)malloc(sizeof(vm_record) * (size_t)std::max<int64_t>(g.nr, 1)); *cigar_blob = (char*)malloc((size_t)std::max<int64_t>(g.nb, 1));
    if (!*recs || !*cigar_blob) { set_error("out of host memory"); return VM_ERR_OOM; }
    VMX_TRY(vmx_fetch(c, run.fin, B.statblk.as<int64_t>() + VMX_STAT_FIN, (size_t)VMX_FIN_WORDS));          // record / blob totals, overflow flag, tier counters, per-round problem counts: one copy
    if (run.fast_local) VMX_TRY(vmx_fetch(c, run.geo, B.geotot.p, (size_t)VMX_GEO_WORDS));             // what the geometry kernel found: totals (history), local anchors (statistics)
    run.h_ctl.resize((size_t)2 * (VMX_MAX_CHUNKS + 1));
    VMX_TRY(vmx_fetch(c, run.h_ctl.data(), B.gfctl.p, run.h_ctl.size()));          // the gap fill's per-chunk control blocks (second-launch queue length and pool need)
    VMX_TRY(vmx_fetch(c, run.er.data(), B.er.p, (size_t)n)); VMX_TRY(vmx_fetch(c, run.h_gmax.data(), B.gmax.p, (size_t)n));
    VMX_TRY(vmx_fetch(c, *recs, B.totals.p, (size_t)g.nr)); VMX_TRY(vmx_fetch(c, *cigar_blob, B.dupd.p, (size_t)g.nb));
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_RESULTS], c->stream));
    VMX_HIP(vmx_stream_sync(c));
    VMX_HIP(hipGetLastError());
    const int64_t* fin = run.fin; const int64_t* rounds = fin + VMX_FIN_ROUNDS;
    run.nr = fin[VMX_FIN_NREC]; run.nb = fin[VMX_FIN_NBLOB];
    st.n_segments = rounds[VMX_STAT_ROUND_ED]; st.n_ed_problems = rounds[VMX_STAT_ROUND_ED];
    st.n_ext_problems = rounds[VMX_STAT_ROUND_EXT] + rounds[VMX_STAT_ROUND_EXT + 1] + rounds[VMX_STAT_ROUND_EXT + 2] + rounds[VMX_STAT_ROUND_EXT + 3];
    st.n_ed_full = (int32_t)fin[VMX_FIN_ED_FULL]; st.n_ed_tier2 = (int32_t)fin[VMX_FIN_ED_TIER2]; st.n_ed_tier1 = (int32_t)fin[VMX_FIN_ED_TIER1];
    return 0;
}

// what the batch assumed instead of asking: did it hold?
int batch_check_assumptions(vmx_batch_run& run) {
    vm_ctx* c = run.c; vm_batch_stats& st = run.st; const bool dbg = run.knobs.now.dbg_pools;
    if (run.fast_local) {       // the pools sized from the context's history (k_ext_geometry)
        st.n_local_anchors = run.geo[VMX_GEO_LOCAL];
        if (run.geo[VMX_GEO_CUT] > 0 || run.geo[VMX_GEO_FULL] + 16 > c->geo_cap[3]) c->geo_valid = false;       // this batch outgrew the pools: the next one of this context asks (and grows them)
        if (run.geo[VMX_GEO_CUT] && dbg) fprintf(stderr, "[pools] extend stage: %lld read(s) did not fit the history-sized pools (run again alone)\n", (long long)run.geo[VMX_GEO_CUT]);
    }
    // the gap fill's second-launch pool (ext_gapfill)
    int64_t need_max = 0, ad_failed = 0;
    for (int pass = 0; pass < 2; ++pass)
        for (int q = 0; q < run.gf_chunks[pass]; ++q) {
            const vmx_gf_ctl& ctl = run.h_ctl[(size_t)(pass * (VMX_MAX_CHUNKS + 1) + q)];
            const unsigned long long rb = ctl.redo_bytes;
            st.n_dp_redo += ctl.redo_n; st.n_dp_redo_wide += ctl.redo_kept; st.n_dp_redo_full += ctl.redo_full; st.dp_redo_tb_bytes += (int64_t)rb; st.dp_cells += (int64_t)rb; ad_failed += ctl.n_not_proven;
            need_max = std::max<int64_t>(need_max, (int64_t)rb);
        }
    c->redo_need_max = std::max<long long>(c->redo_need_max, need_max);
    if (need_max > run.gf_redo_cap) {
        if (dbg) fprintf(stderr, "[pools] gap fill: a chunk's second launch needs %.3f GB of traceback space, the pool held %.3f: running the batch again\n", need_max / 1e9, run.gf_redo_cap / 1e9);
        return VMX_RETRY_BATCH;
    }
    vmx_band_rule_vote(run, ad_failed);      // adapt the band-width rule to the rate of band attempts that were not proven
    return 0;
}

int batch_results_tail(vmx_batch_run& run, vm_record** recs, int64_t* n_recs, char** cigar_blob) {
    vm_ctx* c = run.c; vmx_batch_bufs& B = run.B; const int64_t nr = run.nr, nb = run.nb, g_nr = run.g_nr, g_nb = run.g_nb;
    if (run.fin[VMX_FIN_OFLOW]) { set_error("extend stage: a per-batch work pool overflowed"); return VM_ERR_OOM; }
    if (nr > g_nr || nb > g_nb) {                                 // the guess was short: fetch the tails
        if (nr > g_nr) { vm_record* p2 = (vm_record*)realloc(*recs, sizeof(vm_record) * (size_t)nr); if (!p2) { set_error("out of host memory"); return VM_ERR_OOM; } *recs = p2;
                         VMX_TRY(vmx_fetch(c, *recs + g_nr, B.totals.as<vm_record>() + g_nr, (size_t)(nr - g_nr))); }
        if (nb > g_nb) { char* p2 = (char*)realloc(*cigar_blob, (size_t)nb); if (!p2) { set_error("out of host memory"); return VM_ERR_OOM; } *cigar_blob = p2;
                         VMX_TRY(vmx_fetch(c, *cigar_blob + g_nb, B.dupd.as<char>() + g_nb, (size_t)(nb - g_nb))); }
        VMX_HIP(vmx_stream_sync(c));
    }
    vmx_result_learn(c->res_rec_per_read, c->res_blob_per_base, nr, nb, run.n, run.total_bases);
    for (int64_t i = 0; i < nr; ++i) { run.st.aligned_bases += (*recs)[i].q_en - (*recs)[i].q_st; run.st.cigar_bytes += (*recs)[i].cigar_len; }
    *n_recs = nr; run.st.n_records = nr;
    return 0;
}

void batch_read_statuses(vmx_batch_run& run, int32_t* status_per_read) {
    vmx_status_in s;
    s.fast_local = run.fast_local; s.do_pass1 = run.do_pass1; s.force_exact = run.c->force_exact; s.test_side_every = run.knobs.now.side_every; s.rmode = run.rmode;
    for (int64_t r = 0; r < run.n; ++r) {
        const vmx_ext_read& e = run.er[(size_t)r];
        s.er_status = e.status; s.er_active = e.active; s.er_redo = e.redo; s.er_pass = e.pass; s.er_nrec = e.nrec;
        s.r = r; s.gmax = run.h_gmax[(size_t)r]; s.n_anchors = run.h_aoff[(size_t)r + 1] - run.h_aoff[(size_t)r]; s.asm_override = run.asm_override.empty() ? 0 : run.asm_override[(size_t)r];
        const vmx_read_outcome o = vmx_read_status(s);
        if (status_per_read) status_per_read[r] = o.status;
        if (o.status != 0) run.st.n_failed++; else if (o.unmapped) run.st.n_unmapped++;
    }
}

void batch_times(vmx_batch_run& run) {
    vm_ctx* c = run.c; vm_batch_stats& st = run.st; hipEvent_t* ev = c->ev;
    float ms = 0;
    hipEventElapsedTime(&ms, ev[VMX_EV_START], ev[VMX_EV_RESULTS]); st.ms_total = ms;
    for (int i = 1; i < VMX_EV_COUNT; ++i) { hipEventElapsedTime(&ms, ev[i - 1], ev[i]); st.ms_stage[i - 1] = ms; }
    if ((c->kev_set & 1) && hipEventElapsedTime(&ms, c->kev[0], c->kev[1]) == hipSuccess) st.ms_local_seed = ms;
    if ((c->kev_set & 2) && hipEventElapsedTime(&ms, c->kev[2], c->kev[3]) == hipSuccess) st.ms_cluster = ms;
    st.n_host_syncs = c->n_syncs; st.n_local_general = c->n_bandfall;
    // host-side view of the batch (tuning): ms the thread spent inside its waits for the stream, and wall ms of the call up to here — the difference is host
    // work done while this context's stream was EMPTY (sizing, vector work, launches between a wait's return and the next kernel)
    st.ms_stage[VMX_MS_HOST_WAIT] = (float)((c->sync_wait_ns + download_wait_ns()) * 1e-6);
    st.ms_stage[VMX_MS_HOST_WALL] = (float)((std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count() - c->call_t0_ns) * 1e-6);
    for (int pass = 0; pass < 2; ++pass)
        for (int q = 0; q < c->n_gev[pass]; ++q) {
            hipEvent_t* ke = c->gev + 24 * pass + 3 * q;
            if (hipEventElapsedTime(&ms, ke[0], ke[1]) == hipSuccess) st.ms_gapfill_fill += ms;
            if (hipEventElapsedTime(&ms, ke[1], ke[2]) == hipSuccess) st.ms_gapfill_trace += ms;
            st.n_gapfill_launches++;
        }
}

// tuning aid (VMX_DBG_POOLS): which grow-only pools hold the context's HBM (index in declaration order of vmx_batch_bufs / vmx_local_bufs)
static void batch_report_pools(const vmx_batch_run& run) {
    const vmx_batch_bufs& B = run.B; const vmx_local_bufs& L = run.L;
    const DevBuf* bb = (const DevBuf*)&B; size_t tot = 0;
    for (size_t i = 0; i < sizeof(B) / sizeof(DevBuf); ++i) { tot += bb[i].cap; if (bb[i].cap > ((size_t)128 << 20)) fprintf(stderr, "[pools] batch[%zu] %.2f GB\n", i, bb[i].cap / 1e9); }
    fprintf(stderr, "[pools] batch bufs total %.2f GB\n", tot / 1e9);
    const DevBuf* lb = (const DevBuf*)&L; size_t lt = 0; const size_t nl = (size_t)((const char*)&L.la_pool_rows - (const char*)&L) / sizeof(DevBuf);
    for (size_t i = 0; i < nl; ++i) { lt += lb[i].cap; if (lb[i].cap > ((size_t)128 << 20)) fprintf(stderr, "[pools] local[%zu] %.2f GB\n", i, lb[i].cap / 1e9); }
    fprintf(stderr, "[pools] local bufs total %.2f GB\n", lt / 1e9);
    fprintf(stderr, "[pools] process so far: %lld first allocations, %lld re-allocations, %.3f s in hipFree + hipMalloc\n", (long long)vmx::devbuf_stats().first.load(),
            (long long)vmx::devbuf_stats().grows.load(), vmx::devbuf_stats().ns.load() * 1e-9);
}

// every error return hands the caller NULL outputs (callers raise without calling vm_free: ADVICE r3)
struct vmx_out_guard { vm_record** r; char** b; bool keep = false; ~vmx_out_guard() { if (!keep) { free(*r); free(*b); *r = nullptr; *b = nullptr; } } };

static int align_device_once(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                             vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats, vmx_seg_trace* trace, const vmx_preset* preset) {
    *recs = nullptr; *n_recs = 0; *cigar_blob = nullptr;
    vmx_out_guard out_guard{recs, cigar_blob};
    // LIFETIMES: `run` owns every host buffer that a vmx_fetch of this call names as its destination. It is constructed BEFORE fetch_scope, so it is destroyed AFTER it:
    // on every way out the scope first drops the fetch notes (which point into run's buffers), then the buffers die. Keep this order.
    vmx_batch_run run(c, mi, prm, n, d_codes, d_roff, h_roff, preset, trace);
    c->n_syncs = 0; c->n_bandfall = 0; c->kev_set = 0; c->sync_wait_ns = 0; download_wait_ns() = 0;
    vmx_fetch_scope fetch_scope(c);
    c->call_t0_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
    VMX_HIP(hipEventRecord(c->ev[VMX_EV_START], c->stream));
    if (n == 0) { *recs = (vm_record*)malloc(sizeof(vm_record)); *cigar_blob = (char*)malloc(1); if (stats) *stats = run.st; out_guard.keep = true; return VM_OK; }

    VMX_TRY(preset ? batch_front_preset(run) : batch_front(run));
    VMX_TRY(vmx_extend_stage(run));
    VMX_TRY(batch_results(run, recs, cigar_blob));                  // the batch's wait for its results
    VMX_TRY(batch_check_assumptions(run));                          // may ask for the batch to be run again (VMX_RETRY_BATCH) — before anything more is copied
    VMX_TRY(batch_results_tail(run, recs, n_recs, cigar_blob));
    batch_read_statuses(run, status_per_read);
    batch_times(run);
    if (stats) *stats = run.st;
    if (run.knobs.now.dbg_pools) batch_report_pools(run);
    out_guard.keep = true;
    return VM_OK;
}

// One call = at most max_bases bases and VMX_MAX_BATCH_READS reads per pass over the path: a larger one is processed as consecutive sub-batches of the same
// context and its results are concatenated. run_one(a, b, ...) aligns the reads [a, b). A range the device has no memory for (the grow-only pools of
// this and the other contexts, the index and the reads share the HBM) is cut in two and tried again instead of failing the whole call with VM_ERR_OOM —
// down to single reads.
template <class RunOne>
static int align_in_sub_batches(int64_t n, const int64_t* offsets, int64_t max_bases, RunOne run_one, vm_record** recs, int64_t* n_recs, char** cigar_blob, vm_batch_stats* stats) {
    if (n <= VMX_MAX_BATCH_READS && offsets[n] - offsets[0] <= max_bases) {
        const int rc = run_one(0, n, recs, n_recs, cigar_blob, stats);
        if (rc != VM_ERR_OOM || n <= 1) return rc;
        free(*recs); free(*cigar_blob);                          // fall through: the batch is cut into pieces that fit
    }
    *recs = nullptr; *n_recs = 0; *cigar_blob = nullptr;
    std::vector<vm_record> all; std::string blob;
    vm_batch_stats tot; memset(&tot, 0, sizeof tot);
    std::vector<std::pair<int64_t, int64_t>> work;
    for (int64_t a = 0; a < n;) {
        int64_t b = a + 1;                                       // at least one read per sub-batch, whatever its length
        while (b < n && b - a < VMX_MAX_BATCH_READS && offsets[b + 1] - offsets[a] <= max_bases) ++b;
        work.emplace_back(a, b); a = b;
    }
    for (size_t wi = 0; wi < work.size(); ++wi) {
        const int64_t a = work[wi].first, b = work[wi].second;
        vm_record* r = nullptr; int64_t nr = 0; char* cb = nullptr; vm_batch_stats st;
        const int rc = run_one(a, b, &r, &nr, &cb, &st);
        if (rc == VM_ERR_OOM && b - a > 1) {
            free(r); free(cb);
            vmx::devbuf_retired().flush();                       // parked (outgrown) allocations go back to the device first
            const int64_t mid = a + (b - a) / 2;
            work[wi] = std::make_pair(a, mid); work.insert(work.begin() + (std::ptrdiff_t)wi + 1, std::make_pair(mid, b));
            --wi; continue;
        }
        if (rc < 0) { free(r); free(cb); return rc; }
        int64_t bl = 0; for (int64_t i = 0; i < nr; ++i) bl = std::max(bl, r[i].cigar_off + r[i].cigar_len);
        for (int64_t i = 0; i < nr; ++i) { vm_record x = r[i]; x.read_idx += (int32_t)a; x.cigar_off += (int64_t)blob.size(); all.push_back(x); }
        blob.append(cb, (size_t)bl); blob.push_back('\0');
        free(r); free(cb);
        {   // counters and times add up; sizes are per call
            int64_t* d = (int64_t*)&tot; const int64_t* s2 = (const int64_t*)&st;
            for (size_t i = 0; i < offsetof(vm_batch_stats, ms_total) / 8; ++i) d[i] += s2[i];
            tot.ms_total += st.ms_total; for (int i = 0; i < 16; ++i) tot.ms_stage[i] += st.ms_stage[i];
            tot.ms_gapfill_fill += st.ms_gapfill_fill; tot.ms_gapfill_trace += st.ms_gapfill_trace; tot.n_gapfill_launches += st.n_gapfill_launches;
            tot.n_ed_full += st.n_ed_full; tot.n_ed_tier2 += st.n_ed_tier2; tot.n_ed_tier1 += st.n_ed_tier1;
            tot.n_dp_redo += st.n_dp_redo; tot.n_dp_redo_wide += st.n_dp_redo_wide; tot.n_dp_redo_full += st.n_dp_redo_full; tot.dp_redo_tb_bytes += st.dp_redo_tb_bytes; tot.ms_local_seed += st.ms_local_seed; tot.ms_cluster += st.ms_cluster; tot.n_host_syncs += st.n_host_syncs; tot.n_local_general += st.n_local_general; tot.n_ext_retries += st.n_ext_retries; tot.n_batch_retries += st.n_batch_retries;
        }
    }
    *recs = (vm_record*)malloc(sizeof(vm_record) * std::max<size_t>(all.size(), 1)); *cigar_blob = (char*)malloc(std::max<size_t>(blob.size(), 1));
    if (!*recs || !*cigar_blob) { free(*recs); free(*cigar_blob); *recs = nullptr; *cigar_blob = nullptr; set_error("out of host memory"); return VM_ERR_OOM; }
    memcpy(*recs, all.data(), sizeof(vm_record) * all.size()); memcpy(*cigar_blob, blob.data(), blob.size());
    *n_recs = (int64_t)all.size();
    if (stats) *stats = tot;
    return VM_OK;
}
// the bases one pass over the path takes (VMX_MAX_BATCH_BASES). The work pools of a context grow with the pass (~0.85 KB per read base at hg38 size) and never
// shrink, and a scheduler that cuts its batches by read count meets a batch of its longest reads now and then — 4096 reads of 40-100 kb are 160 Mbases
// where the average batch holds 60: every context then keeps pools for 160 Mbases and uses them for 60. With the budget near the AVERAGE batch the
// long-read batch runs as two or three passes of its context and the pools of all contexts are ~2.5 times smaller: more batches in flight fit the HBM.
static int64_t vmx_pass_bases() { return vmx_align_knobs_read().once->max_batch_bases; }

extern "C" {

int vm_reads_upload(vm_ctx* c, int64_t n, const char* seqs, const int64_t* offsets, vm_reads** out) {
    *out = nullptr;
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    VMX_HIP(hipSetDevice(c->device));
    std::unique_ptr<vm_reads> R(new vm_reads()); R->ctx = c; R->n = n; R->h_off.assign(offsets, offsets + n + 1);
    const int64_t tot = offsets[n];
    VMX_TRY(upload(R->raw, seqs, (size_t)tot, c->stream)); VMX_TRY(R->codes.reserve((size_t)tot + 64)); VMX_TRY(upload(R->off, offsets, (size_t)n + 1, c->stream));
    if (tot) LAUNCH1D(k_encode, tot, R->raw.as<char>(), R->codes.as<uint8_t>(), tot);
    VMX_HIP(vmx_stream_sync(c));
    R->raw.release();                  // early: a resident read set keeps its codes and offsets; the ASCII (as large as the codes) makes room for the batch's pools
    *out = R.release();
    return VM_OK;
}
// the same into an existing object (its device buffers are kept and only grow): an uploader that streams batches ahead of the aligning contexts
// cycles a few of these instead of paying a hipMalloc / hipFree pair per batch (hipFree waits for the whole device). No alignment of R may be in flight.
int vm_reads_reupload(vm_ctx* c, vm_reads* R, int64_t n, const char* seqs, const int64_t* offsets) {
    if (!c || !R) { set_error("no context / reads object"); return VM_ERR_NO_CTX; }
    VMX_HIP(hipSetDevice(c->device));
    R->n = n; R->h_off.assign(offsets, offsets + n + 1);
    const int64_t tot = offsets[n];
    VMX_TRY(upload(R->raw, seqs, (size_t)tot, c->stream)); VMX_TRY(R->codes.reserve((size_t)tot + 64)); VMX_TRY(upload(R->off, offsets, (size_t)n + 1, c->stream));
    if (tot) LAUNCH1D(k_encode, tot, R->raw.as<char>(), R->codes.as<uint8_t>(), tot);
    VMX_HIP(vmx_stream_sync(c));
    return VM_OK;
}
void vm_reads_free(vm_reads* R) { delete R; }

int vm_align_resident(vm_ctx* c, const vm_index* mi, const vm_params* prm, const vm_reads* R, vm_record** recs, int64_t* n_recs, char** cigar_blob,
                      int32_t* status_per_read, vm_batch_stats* stats) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    VMX_HIP(hipSetDevice(c->device));
    if (R->n <= VMX_MAX_BATCH_READS && R->h_off[(size_t)R->n] <= vmx_pass_bases())
        return align_device(c, mi, prm, R->n, R->codes.as<uint8_t>(), R->off.as<int64_t>(), R->h_off, recs, n_recs, cigar_blob, status_per_read, stats);
    // more bases than one pass takes: consecutive ranges of the resident reads (their codes stay where they are; a range's offsets are rebased and uploaded)
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    auto run_one = [c, mi, prm, R, status_per_read, &B](int64_t a, int64_t b, vm_record** r, int64_t* nr, char** cb, vm_batch_stats* st) -> int {
        std::vector<int64_t> h((size_t)(b - a) + 1);
        for (int64_t i = a; i <= b; ++i) h[(size_t)(i - a)] = R->h_off[(size_t)i] - R->h_off[(size_t)a];
        VMX_TRY(vmx_push(c, B.off, h.data(), h.size()));
        return align_device(c, mi, prm, b - a, R->codes.as<uint8_t>() + R->h_off[(size_t)a], B.off.as<int64_t>(), h, r, nr, cb, status_per_read ? status_per_read + a : nullptr, st);
    };
    return align_in_sub_batches(R->n, R->h_off.data(), vmx_pass_bases(), run_one, recs, n_recs, cigar_blob, stats);
}

int vm_align_trace(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const char* seqs, const int64_t* offsets, int stage, int64_t** rows, int64_t** row_off) {
    *rows = nullptr; *row_off = nullptr;
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (stage != 0 && stage != 3 && stage != 5) { set_error("vm_align_trace: stage must be 0, 3 or 5"); return VM_ERR_ARG; }
    VMX_HIP(hipSetDevice(c->device));
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    const int64_t tot = offsets[n];
    VMX_TRY(upload(B.raw, seqs, (size_t)tot, c->stream)); VMX_TRY(B.codes.reserve((size_t)tot + 64)); VMX_TRY(upload(B.off, offsets, (size_t)n + 1, c->stream));
    if (tot) LAUNCH1D(k_encode, tot, B.raw.as<char>(), B.codes.as<uint8_t>(), tot);
    std::vector<int64_t> h_off(offsets, offsets + n + 1);
    vmx_seg_trace tr; tr.stage = stage;
    vm_record* recs = nullptr; int64_t nrec = 0; char* blob = nullptr;
    std::vector<int32_t> status((size_t)n + 1);
    const int rc = align_device(c, mi, prm, n, B.codes.as<uint8_t>(), B.off.as<int64_t>(), h_off, &recs, &nrec, &blob, status.data(), nullptr, &tr);
    free(recs); free(blob);
    if (rc < 0) return rc;
    if (tr.off.empty()) tr.off.assign((size_t)n + 1, 0);
    *rows = (int64_t*)malloc(8 * std::max<size_t>(tr.rows.size(), 1)); *row_off = (int64_t*)malloc(8 * tr.off.size());
    memcpy(*rows, tr.rows.data(), 8 * tr.rows.size()); memcpy(*row_off, tr.off.data(), 8 * tr.off.size());
    return VM_OK;
}

static int align_batch_one(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const char* seqs, const int64_t* offsets, vm_record** recs, int64_t* n_recs,
                           char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats) {
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    const int64_t base = offsets[0], tot = offsets[n] - base;
    std::vector<int64_t> h_off((size_t)n + 1);
    for (int64_t i = 0; i <= n; ++i) h_off[(size_t)i] = offsets[i] - base;
    VMX_TRY(vmx_push(c, B.raw, seqs + base, (size_t)tot)); VMX_TRY(B.codes.reserve((size_t)tot + 64)); VMX_TRY(vmx_push(c, B.off, h_off.data(), (size_t)n + 1));
    if (tot) LAUNCH1D(k_encode, tot, B.raw.as<char>(), B.codes.as<uint8_t>(), tot);
    return align_device(c, mi, prm, n, B.codes.as<uint8_t>(), B.off.as<int64_t>(), h_off, recs, n_recs, cigar_blob, status_per_read, stats);
}

// The work pools of a context grow with the batch (≈ 0.85 KB per read base at hg38 size) and never shrink, so one oversized call —
// 100 k long reads in one batch — could exhaust HBM next to the index and the other contexts. A call above VMX_MAX_BATCH_BASES bases or
// VMX_MAX_BATCH_READS reads is therefore processed as consecutive sub-batches of the same context and its results are concatenated;
// callers that size their batches like vacmap_amd.pipeline (4096 reads, ~60 Mbases) never notice.
int vm_align_batch(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const char* seqs, const int64_t* offsets, vm_record** recs, int64_t* n_recs,
                   char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    VMX_HIP(hipSetDevice(c->device));
    if (prm->mode == VM_MODE_ASM)        // contigs of 500 kb and more take the linked path (vmx_asm.hip), one by one
        for (int64_t r = 0; r < n; ++r)
            if (offsets[r + 1] - offsets[r] >= 500000) return vmx_align_batch_asm_mixed(c, mi, prm, n, seqs, offsets, recs, n_recs, cigar_blob, status_per_read, stats);
    // test hook: pretend the device is out of memory for any sub-batch above this many bases (exercises the degradation)
    const int64_t fake_oom = vmx_align_knobs_read().now.oom_above_bases;
    auto run_one = [c, mi, prm, seqs, offsets, status_per_read, fake_oom](int64_t a, int64_t b, vm_record** r, int64_t* nr, char** cb, vm_batch_stats* st) -> int {
        if (fake_oom > 0 && offsets[b] - offsets[a] > fake_oom) { *r = nullptr; *nr = 0; *cb = nullptr; set_error("out of device memory (test hook)"); return VM_ERR_OOM; }
        return align_batch_one(c, mi, prm, b - a, seqs, offsets + a, r, nr, cb, status_per_read ? status_per_read + a : nullptr, st);
    };
    return align_in_sub_batches(n, offsets, vmx_pass_bases(), run_one, recs, n_recs, cigar_blob, stats);
}

}  // extern "C"
