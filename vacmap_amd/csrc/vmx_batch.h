// vmx_batch.h — one batch's pass over the path (align_device_once, vmx_align.hip) as state + stage functions: everything the stages share lives in ONE struct,
// vmx_batch_run, and each stage is a function over it. Included at the end of vmx_stage.h (it uses the buffer bundles declared there).
#ifndef VMX_BATCH_H
#define VMX_BATCH_H
#include "vmx_stage.h"
#include "vmx_ext_state.h"
#include "vmx_local.h"
#include "vmx_round.h"
#include "vmx_batch_policy.h"

static_assert(VMX_POL_EXT_CAPACITY_DEV == VMX_EXT_CAPACITY_DEV && VMX_POL_EXT_NEED_EXACT_DEV == VMX_EXT_NEED_EXACT_DEV && VMX_POL_READ_CAPACITY_DEV == VM_READ_CAPACITY_DEV &&
              VMX_POL_READ_BANDFALL_DEV == VM_READ_BANDFALL_DEV, "vmx_batch_policy.h restates the device's per-read codes");

// diagnostic capture for the stage tests (vm_align_trace): the segment lists of every read as they stand after one phase of the
// extend stage in the first (filtering) pass: rows (segment, q, r, s, l), off[n + 1]
struct vmx_seg_trace { int stage; std::vector<int64_t> rows, off; };

// The environment knobs of vmx_align.hip / vmx_stage_extend.hip, all read by vmx_align_knobs_read() (vmx_align.hip) and nowhere else. Two groups, because WHEN a knob is read
// is part of its meaning: the tuning and A/B knobs are latched when the process first asks and hold for its life (a run is one configuration); the test hooks and the
// knobs of tuning sweeps are read again by every call, because tests set them between two calls of one process.
struct vmx_align_knobs {
    struct once_t {
        bool select_serial;                 // VMX_SELECT_SERIAL: the one-lane peel of k_chain_select
        int gc_lds_max;                     // VMX_GC_LDS_MAX: largest LDS bucket of k_chain_global (-1: not set)
        int trace_spread;                   // VMX_TRACE_SPREAD 1..64 (1): lanes per problem of k_gapfill_trace
        int ext_spread, rec_spread;         // VMX_EXT_SPREAD / VMX_REC_SPREAD 1..64 (0: by the contexts in flight)
        bool local_sync;                    // VMX_LOCAL_SYNC: the waiting path always
        bool seed_arena;                    // VMX_SEED_ARENA=0 switches the seed stage's arena off
        bool ext_wave;                      // VMX_EXT_WAVE=0: the one-lane form of the phases that walk every anchor
        int64_t tb_chunk;                   // VMX_TB_CHUNK_GB (> 0.5): traceback bytes per gap-fill chunk
        int64_t max_batch_bases;            // VMX_MAX_BATCH_BASES: bases one pass over the path takes
        bool force_exact, force_pass1;      // VMX_FORCE_EXACT / VMX_FORCE_PASS1: every batch runs every tier of the divergence filter / pass 1
    };
    struct call_t {
        int ext_tmask; int64_t ext_tdiv;    // VMX_TEST_EXT_POOL=<mask>:<div> (0, 1)
        long long redo_pool_bytes;          // VMX_TEST_REDO_POOL_BYTES: the first guess of a fresh context (0: not set)
        int64_t side_every;                 // VMX_TEST_SIDE_EVERY: every k-th read of a batch is sent through the side batch
        int64_t oom_above_bases;            // VMX_TEST_OOM_ABOVE_BASES: pretend the device has no memory for a larger sub-batch
        bool ad_pinned;                     // VMX_AD_PCT or VMX_AD_PCT_MIN is set: the band-width rule does not adapt (the values: vmx_ad_pct_env)
        int fill_waves;                     // VMX_FILL_WAVES 1..32 (16): waves per CU of the gap fill's first launch
        bool dbg_pools;                     // VMX_DBG_POOLS: report pool events on stderr
    };
    const once_t* once; call_t now;
};
vmx_align_knobs vmx_align_knobs_read();

// the batch's events on the context's stream (vm_ctx.ev), recorded at the END of what they are named after: ms_stage[i] is the time from event i to event i + 1
enum vmx_batch_event { VMX_EV_START = 0, VMX_EV_SEED, VMX_EV_GLOBAL, VMX_EV_LOCAL, VMX_EV_FILTER, VMX_EV_EDGE, VMX_EV_GAPFILL, VMX_EV_PASS1, VMX_EV_RESULTS, VMX_EV_COUNT };
// vm_batch_stats.ms_stage beyond the events: [14] ms the host thread spent inside its waits for the stream, [15] wall ms of the call
enum { VMX_MS_HOST_WAIT = 14, VMX_MS_HOST_WALL = 15 };
static_assert(VMX_EV_COUNT == 9 && VMX_EV_RESULTS - 1 == 7, "ms_stage[0..7] are read by index");

struct vmx_batch_run {
    // ---- the call
    vm_ctx* c; const vm_index* mi; const vm_params* prm; int64_t n; const uint8_t* d_codes; const int64_t* d_roff; const std::vector<int64_t>& h_roff;
    const vmx_preset* preset; vmx_seg_trace* trace;
    vm_index_view ix; int64_t total_bases; vmx_align_knobs knobs;
    vmx_batch_bufs& B; vmx_local_bufs& L;
    // ---- front stages (seed, global chain, local chain — or the preset chains)
    std::vector<int64_t> h_aoff;
    int rmode;                                    // the GC kernels' variant: 0 H / L / S, 1 R, 2 the asm fork
    bool fast_local;                              // no host wait in the local stage, pool geometry on the device (see the constructor)
    double* d_gscore = nullptr; int32_t* d_mapq = nullptr; int32_t* d_np = nullptr;
    std::vector<int32_t> asm_override;            // -mode asm: per-contig status set by the tie-break step
    // ---- extend stage: pool geometry
    std::vector<int64_t> coff3, soff2, bloboff;   // the waiting path's per-read offsets (the fast path makes them on the device)
    int64_t cA = 0, cS = 0, cB = 0, cS_full = 0, round_cap = 0, pool_cap = 0, carry_stride = 0, ed_wgs = 0;
    // ---- extend stage: cursor
    vmx_ext_args A; int cur = 0, ext_rounds = 0, ext_spread = 1, rec_spread = 1; bool do_pass1 = false;
    // ---- gap fill
    int gf_chunks[2] = {0, 0}; int64_t gf_redo_cap = 0; int ad_cur = 0, ad_pct = 0;
    // ---- results
    int64_t nr = 0, nb = 0, g_nr = 0, g_nb = 0;   // records / CIGAR bytes of the batch, and how many of them the first copy asked for
    vm_batch_stats st;
    // ---- EVERY host buffer a vmx_fetch of this call targets (with h_aoff above). vmx_fetch only notes the destination; the bytes arrive at the next wait, and a call that fails in between
    // leaves the notes to its vmx_fetch_scope. The buffers live here so that their lifetime is the struct's: align_device_once constructs the struct before the scope.
    int64_t fin[VMX_FIN_WORDS]; int64_t geo[8] = {0, 0, 0, 0, 0, 0, 0, 0}; int64_t plan[VMX_PLAN_WORDS];
    std::vector<vmx_gf_ctl> h_ctl; std::vector<vmx_ext_read> er; std::vector<int64_t> h_gmax;

    vmx_batch_run(vm_ctx* c, const vm_index* mi, const vm_params* prm, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                  const vmx_preset* preset, vmx_seg_trace* trace);
};

// ---- the stages, in the order align_device_once runs them
int batch_front(vmx_batch_run& run);                      // S1 seed, S2 + G1-G3 global chain and selection, orient + L1-L4 local stage
int batch_front_preset(vmx_batch_run& run);               // -mode asm, contig of 500 kb and more: the chain comes from the caller
int vmx_extend_stage(vmx_batch_run& run);                 // E1-E6 (vmx_stage_extend.hip): pools, divergence filter, edge extension, gap fill (one wait: the chunk plan), records
int batch_results(vmx_batch_run& run, vm_record** recs, char** cigar_blob);      // pack on the device, copy what the context's history suggests, the batch's one wait for its results
int batch_check_assumptions(vmx_batch_run& run);          // what the batch assumed instead of asking: VMX_RETRY_BATCH when the second gap-fill launch's pool was short; geo_valid; the band-rule vote
int batch_results_tail(vmx_batch_run& run, vm_record** recs, int64_t* n_recs, char** cigar_blob);      // the part of the result the guess did not cover (a second wait), result counters
void vmx_band_rule_vote(vmx_batch_run& run, int64_t not_proven);      // vmx_stage_extend.hip: this batch's vote on the gap fill's band-width rule (vmx_ad_rule)
void batch_read_statuses(vmx_batch_run& run, int32_t* status_per_read);
void batch_times(vmx_batch_run& run);
#endif
