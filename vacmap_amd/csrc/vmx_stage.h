// vmx_stage.h — device-buffer bundles and internal stage functions shared by the stage entry points and vm_align_batch.
// The stages of one batch: vmx_seed_stage, vmx_global_stage, vmx_local_stage (below) and, over the batch's state vmx_batch_run (vmx_batch.h, included at the end):
// batch_front / batch_front_preset, vmx_extend_stage (vmx_stage_extend.hip), batch_results, batch_check_assumptions, batch_results_tail, batch_read_statuses, batch_times.
// The host's decisions on that path are pure functions in vmx_batch_policy.h; the environment knobs of the path are vmx_align_knobs (vmx_batch.h).
#ifndef VMX_STAGE_H
#define VMX_STAGE_H
#include "vmx_host.h"

struct vm_index_view {
    const uint8_t* codes; const int64_t* coff; int nseq; int64_t total_len;
    const uint64_t* pos; const vmx_slot* table; int table_bits; int k, w, mid_occ;
};
void vmx_index_view(const vm_index* mi, vm_index_view* v);

// a chain handed to the extend stage instead of the seed / chain stages (host rows, DESCENDING read order like a local chain)
struct vmx_preset { const vmx_anchor* chain_desc; int64_t len; };      // one per read of the call (align_device takes an array of n)

struct vmx_local_bufs {
    vmx::DevBuf sq, dst, rorder, pc2, stg, si, tg, cntp, fp, pp, prep_ws;
    vmx::DevBuf guide_rows, guide_len, ng_used, ng_total, cnt, cur, tpos, hkey, hkey2, dbg, hval, hq, goff, pcnt, gkey, gq, gr, epoch;
    vmx::DevBuf la_rows, la_ekey, la_sorted, la_off, la_cnt, status, gap, rlist, S, P, SA, chain, chain_len, score, variant;
    int64_t la_pool_rows = 0;            // rows of the local-anchor pools (regular slots + overflow area)
    int64_t head_stride = 0;             // entries per slot of k_local_seed's head tables (cnt) as last filled: it depends on local_kmersize
    std::vector<int64_t> h_la_off;
    std::vector<int32_t> h_la_cnt;
};
vmx_local_bufs* vmx_ctx_local_bufs(vm_ctx* c);

// the seed stage's buffers (vmx_seed_stage), named as it names them; rlist: the read lists of the clustering launches
struct vmx_seed_bufs { vmx::DevBuf mzh, mzp, mzc, mst, mcn, mho, nh, koff, keys, ckeys, rows, nanc, rlist; };

// scratch of the stage entry points (vm_edit_distance_batch ... vm_local_chain_batch), grow-only, one set per context. Entries share the members of a
// role: every entry encodes its sequences into `a` (and `b`) and leaves its per-problem results in `out`.
struct vmx_read_set { vmx::DevBuf raw, codes, off; };       // ASCII as uploaded, 2-bit codes (+ 64 bytes), n + 1 offsets
struct vmx_entry_bufs {
    vmx_read_set a, b;                                      // the entry's first / second sequence set (the reads of the seed and chain entries are `a`)
    vmx::DevBuf out;                                        // distances or bounds; (t_e, q_e, score); (score, CIGAR length); minimizers per read; GC-fast's flags
    vmx::DevBuf pool;                                       // the edit distance's carry ring; the full-matrix gap fill's traceback
    vmx::DevBuf sizes, count, order, range;                 // edit distance entries: the device work queue (pattern sizes, their number, order, ranges + counters)
    vmx::DevBuf probs, bnd, run, cig;                       // vm_k_cigar_batch: problem table, boundary / run / CIGAR pools
    vmx::DevBuf hash, pos;                                  // vm_sketch_batch: minimizer columns
    vmx_seed_bufs seed;                                     // vm_map_batch
    vmx::DevBuf rows, plen, npaths, aoff, gscore;           // vm_local_chain_batch: the global paths it is given
};
vmx_entry_bufs* vmx_ctx_entry_bufs(vm_ctx* c);

// the buffers of the batched path (vmx_align.hip), grow-only, one set per context
struct vmx_batch_bufs {
    vmx_seed_bufs seed;
    vmx::DevBuf nanc64, aoff, rows, lens, keys, koff, sorted, flip, S, P, SA, cov, gmax, opc, rl, gap, scr, soff, res, plen, prow, ocodes;
    // extend stage
    vmx::DevBuf er, coff3, soff2, segA, st, en, segA_s, st_s, en_s, segprob, dup, desc[2], rcount, oflow, probread, tl, ql, toff, qoff, tpool, qpool;
    vmx::DevBuf edout, carry, ext3, dpsz[4], dpoff[4], dptab, tb, tbredo, bnd, run, cig, ciglen, dpscore, rec, blob, bloboff, reccoff, recclen, dupd, totals;
    vmx::DevBuf raw, codes, off, order, qrange, si, tg, cntp, fp, pp, chunkn, sellist, cigq, statblk, szh, side_codes, side_off, roundpart, gfctl, geotot;
};
vmx_batch_bufs* vmx_ctx_batch_bufs(vm_ctx* c);

// S2 + G1-G3 + selection: the global chain stage over n reads. Inputs on the device: anchor rows in B.rows (q, r, s, l as int64, read r's from B.aoff[r]),
// B.aoff, the read lengths B.lens and offsets d_roff; h_roff / h_aoff are the host copies of the offsets. rmode: 0 H / L / S, 1 R, 2 -mode asm.
// d_ran (may be null): GC-fast sets it to 1 for the reads it ran. Leaves in B: sorted, flip, S, P, SA, gmax, opc, and the selected paths
// (res: scores, MAPQs, path counts as vmx_res_ptrs lays them out; plen, prow). -mode asm: contigs of 500 kb and more get gmax = -4 and no chain.
int vmx_global_stage(vm_ctx* c, vmx_batch_bufs& B, const vm_params* prm, int k, int64_t n, const int64_t* d_roff, const std::vector<int64_t>& h_roff,
                     const std::vector<int64_t>& h_aoff, int rmode, int32_t* d_ran);
// B.res as the selection fills it: n + 1 scores, then n + 1 MAPQs, then n + 1 path counts
static inline void vmx_res_ptrs(vmx_batch_bufs& B, int64_t n, double** score, int32_t** mapq, int32_t** np) {
    *score = B.res.as<double>(); *mapq = (int32_t*)(*score + n + 1); *np = *mapq + n + 1;
}

// E5 on one chunk of the gap-fill problem table B.dptab: problems [p0, p0 + pn) (pn an upper bound when n_ptr names the count on the device), queue keys
// in B.dpsz[0] (vmx_round_key), traceback space in B.tb from the chunk's first problem on (tb_off0: its traceback offset); the problems the band does not prove
// take their full-matrix space from B.tbredo (redo_cap bytes; one that does not fit is emptied). ctl: the chunk's control block (vmx_gf_ctl, vmx_gapfill.h), zeroed;
// redo_list: room for pn entries. ke: three events (before the fill, after the fill, after the traceback) or null. CIGARs in B.run / B.cig / B.ciglen / B.cigq; B.dpscore carries every problem's layout flag.
void vmx_gapfill_chunk(vm_ctx* c, vmx_batch_bufs& B, const vm_score& sc, int ad_pct, int eqx, int p0, int64_t pn, const int32_t* n_ptr, int64_t tb_off0,
                       vmx_gf_ctl* ctl, int32_t* redo_list, int64_t redo_cap, hipEvent_t* ke);

extern "C" int vmx_seed_stage(vm_ctx* c, const vm_index* mi, int check_num, int mid_occ, int64_t n, const uint8_t* d_codes, const int64_t* d_roff, int64_t total_bases,
                   vmx_seed_bufs& B, std::vector<int64_t>& h_koff, std::vector<int64_t>& h_nhits, vmx::DevBuf* arena = nullptr, int64_t** rows_out = nullptr);
int vmx_local_stage(vm_ctx* c, const vm_index_view& ix, const vm_params* prm, int64_t n, const uint8_t* d_ocodes, const int64_t* d_roff,
                    const std::vector<int64_t>& h_roff, const vmx_anchor* d_path_rows, const int32_t* d_path_len, const int32_t* d_npaths,
                    const int64_t* d_aoff, const std::vector<int64_t>& h_aoff, const double* d_gscore, vmx_local_bufs& L, bool fast = false);
// The second half of vmx_local_stage, L3 - L5: the local chain DPs over the anchors in L (la_sorted / la_off / la_cnt / ng_total / status on the device, la_pool_rows,
// h_la_cnt unless `fast`), with the routing of the product (row kernels or one wavefront per read, LDS buckets, device-built read list when `fast`). Also entered
// by the stage entry vm_local_dp_batch on rows it is given. probe (that entry only; null in the product): what the host knows about the run and no kernel
// stores — d_lc_status gets a copy of the per-read status between the LC launches and L5 (VM_READ_FASTPATH_DEV: the read went on to its `_fast` twin),
// s_in_lds[r] (sized n by the caller) whether read r ran LDS-resident (its S never reached HBM).
struct vmx_local_dp_probe { int32_t* d_lc_status = nullptr; std::vector<uint8_t> s_in_lds; };
int vmx_local_dp(vm_ctx* c, const vm_params* prm, int64_t n, const int64_t* d_roff, const std::vector<int64_t>& h_roff, vmx_local_bufs& L, bool fast,
                 vmx_local_dp_probe* probe = nullptr);
// G1 selection (k_chain_select) over n reads, one launch per LDS size class of the reads' anchor counts (h_aoff), side by side
int vmx_launch_chain_select(vm_ctx* c, int64_t n, const int64_t* h_aoff, vmx::DevBuf& d_list, const vmx_anchor* sorted, const int64_t* d_aoff, const int64_t* d_lens,
                            const double* S, const int32_t* P, const int32_t* SA, const int64_t* gmax, const int32_t* flip, int mode, char* scr, const int64_t* soff,
                            int32_t* d_mapq, double* d_score, int32_t* d_np, int32_t* plen, vmx_anchor* prow);
#include "vmx_batch.h"
#endif
