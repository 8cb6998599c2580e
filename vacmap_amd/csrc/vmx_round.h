// vmx_round.h — arguments of k_round_prep (k_round.hip): one launch per DP round of the extend stage for lengths, offset scans, pool-size scans, problem
// table and traceback chunk plan.
#ifndef VMX_ROUND_H
#define VMX_ROUND_H
#include "vmx_kernels.h"
#include "vmx_extend.h"

#define VMX_MAX_CHUNKS 24
#define VMX_ROUND_WGS 128            // workgroups of k_round_prep (<= 256: one look-back step per thread)
#define VMX_ROUND_PART_WORDS (256 * 8 + 8)      // int64 words of the publication area: 8 per workgroup (sums [0..5], flag [7]) + the finished-workgroups counter

// ---- layouts of the small device blocks the host reads back once per batch (vmx_batch_bufs: statblk, qrange, geotot), shared by the kernels that fill them and the host
// B.statblk, 2048 bytes, cleared once per batch
enum {
    VMX_STAT_BYTES = 2048,
    VMX_STAT_ROUND_ED = 0,          // int32 [0..7]: the rounds' problem counts (k_round_prep's stat_out): the divergence filter's,
    VMX_STAT_ROUND_EXT = 1,         //   the four x-drop rounds' ([1..4]),
    VMX_STAT_ROUND_GF = 6,          //   the gap fill's of pass 0 and ([7]) pass 1
    VMX_STAT_ROUNDS = 8,
    VMX_STAT_FIN = 32,              // int64 [32..45]: the final scalars (k_final_scalars, VMX_FIN_*)
    VMX_STAT_PLAN = 64,             // int64 [64..121]: the chunk plan of pass 0 (k_round_prep<true>, VMX_PLAN_*)
    VMX_STAT_PLAN_STRIDE = 64       // int64 [128..185]: of pass 1
};
// the final scalars
enum { VMX_FIN_NREC = 0, VMX_FIN_NBLOB = 1, VMX_FIN_OFLOW = 2, VMX_FIN_ED_FULL = 3, VMX_FIN_ED_TIER2 = 4, VMX_FIN_ED_TIER1 = 5, VMX_FIN_ROUNDS = 6, VMX_FIN_WORDS = VMX_FIN_ROUNDS + VMX_STAT_ROUNDS };
// a gap-fill round's plan (vmx_round_args.plan_out)
enum { VMX_PLAN_N = 0, VMX_PLAN_POOLS = 1 /* [1..4] traceback, boundary, run, CIGAR totals */, VMX_PLAN_TBYTES = 5, VMX_PLAN_QBYTES = 6, VMX_PLAN_CHUNKS = 7, VMX_PLAN_CUTS = 8,
       VMX_PLAN_OFFS = VMX_PLAN_CUTS + VMX_MAX_CHUNKS + 1, VMX_PLAN_WORDS = VMX_PLAN_CUTS + 2 * (VMX_MAX_CHUNKS + 1) };
// B.qrange (int32): the size ordering's queue range and heads, then the divergence filter's tier counters in k_final_scalars' order
enum { VMX_QR_RANGE = 0, VMX_QR_CNT = 4, VMX_QR_NFULL = 8, VMX_QR_NT2 = 9, VMX_QR_NT1 = 10, VMX_QR_BYTES = 128 };
// B.geotot (int64): what k_ext_geometry found
enum { VMX_GEO_ANCHORS = 0, VMX_GEO_SEGS = 1, VMX_GEO_BLOB = 2, VMX_GEO_FULL = 3, VMX_GEO_LOCAL = 4, VMX_GEO_CUT = 5, VMX_GEO_WORDS = 6 };
static_assert(VMX_STAT_ROUND_ED == 0 && VMX_STAT_ROUND_EXT == 1 && VMX_STAT_ROUND_GF == 6 && VMX_STAT_FIN == 32 && VMX_STAT_PLAN == 64 && VMX_STAT_PLAN + VMX_STAT_PLAN_STRIDE == 128, "statblk layout");
static_assert(VMX_FIN_WORDS == 14 && VMX_FIN_ROUNDS == 6 && 8 * (VMX_STAT_FIN + VMX_FIN_WORDS) <= 8 * VMX_STAT_PLAN, "final scalars end before the plans");
static_assert(VMX_PLAN_WORDS == 58 && VMX_PLAN_WORDS <= VMX_STAT_PLAN_STRIDE && 8 * (VMX_STAT_PLAN + VMX_STAT_PLAN_STRIDE + VMX_PLAN_WORDS) <= VMX_STAT_BYTES, "both plans fit the block");
static_assert(VMX_QR_CNT == 4 && VMX_QR_NFULL == 8 && VMX_QR_NT2 == 9 && VMX_QR_NT1 == 10 && 4 * (VMX_QR_NT1 + 1) <= VMX_QR_BYTES, "qrange layout");
static_assert(VMX_GEO_ANCHORS == 0 && VMX_GEO_SEGS == 1 && VMX_GEO_BLOB == 2 && VMX_GEO_FULL == 3 && VMX_GEO_LOCAL == 4 && VMX_GEO_CUT == 5, "geotot layout");

struct vmx_round_args {
    const vmx_pair_desc* desc; const int32_t* n_prob;
    int64_t* off[6];            // exclusive prefix sums, n + 1 entries each: [0] target string bytes, [1] query string bytes; gap-fill rounds: [2] traceback bytes,
                                // [3] boundary ints, [4] run words, [5] CIGAR bytes
    int64_t* tb_size;           // gap-fill rounds: the problem's QUEUE KEY for the size-order kernels (k_size_hist / k_size_scatter sort by quarter octaves of it, largest first):
                                // [2^42, ..) problems taken one per task (traceback bytes > VMX_HEAD_THRESH), [2^33, 2^42) other problems beyond the small class,
                                // [2^23, 2^33) small-class problems with 4-byte slots (ns 3 / 4), [2^13, 2^23) 2-byte (ns 2), [2^3, 2^13) 1-byte (ns 1), [1, 8) no band; inside a range by size
    vmx_dp_prob* probs;         // gap-fill rounds: the problem table
    int64_t* part;              // VMX_ROUND_PART_WORDS words, zeroed once when allocated
    int32_t* stat_out;          // the round's problem count for the host's statistics block (may be null)
    int64_t* plan_out;          // gap-fill rounds: [0] n, [1..4] pool totals, [5] target bytes, [6] query bytes, [7] number of chunks m (-1: more than VMX_MAX_CHUNKS),
                                // [8 ..] first problem of every chunk (m + 1 entries), then the traceback offsets at those problems (m + 1 entries)
    int64_t tb_limit;           // traceback bytes per chunk
    int64_t cap[4];             // gap-fill rounds, unplanned pass (cap[0] > 0): capacity of the traceback (one chunk) / boundary / run / CIGAR pools in their units; a problem
                                // that would pass one of them is EMPTIED (tl = ql = 0, offsets 0): nothing is filled or traced for it, the host sees the totals and retries
    int ad_on, ad_match, ad_o1, ad_e1, ad_o2, ad_e2, ad_pct;      // gap-fill rounds of the batched path: the band-width rule's inputs (vmx_ad_ns) — a small problem's traceback space
                                // is sized for the slot width of its own band (VMX_AD_W) and its queue key carries that width (below)
    long long epoch;            // launch number of this context (never 0): flags of earlier launches are never mistaken for this one's
};
template <bool DP> __global__ void k_round_prep(vmx_round_args A);

// sizing rule and queue key of a gap-fill problem, shared by k_round_prep and the host-built problem table of vm_k_cigar_batch_banded
// slot width of a small-class problem's own band (0: no band is tried, the problem is filled in full by the second launch out of its pool)
__host__ __device__ __forceinline__ int vmx_round_w(const vmx_round_args& A, long long tl, long long ql) {
    return VMX_AD_W(vmx_ad_ns((int)tl, (int)ql, A.ad_match, A.ad_o1, A.ad_e1, A.ad_o2, A.ad_e2, A.ad_pct & 0xffff, (A.ad_pct >> 16) & 0xffff));
}
// traceback bytes of a problem: a small one's slots are as wide as its own band asks (4 bytes where the caller has no band rule)
__host__ __device__ __forceinline__ long long vmx_round_tb_bytes(const vmx_round_args& A, long long tl, long long ql) {
    return vmx_gf_tb_bytes_batched(tl, ql, (A.ad_on && vmx_gf_small(tl, ql)) ? vmx_round_w(A, tl, ql) : 4);
}
// the queue key (vmx_round_args.tb_size)
__host__ __device__ __forceinline__ long long vmx_round_key(const vmx_round_args& A, long long tl, long long ql) {
    if (tl <= 0 || ql <= 0) return 0;
    if (!VMX_DP16X4_OK(tl, ql)) {
        const long long b = vmx_gf_tb_bytes_full(tl, ql);
        if (b > VMX_HEAD_THRESH) return (b < (1LL << 38) ? b : (1LL << 38)) << 24;
        return b << 23;
    }
    const long long b64 = vmx_gf_key_size_small(tl, ql);                 // (tl + ql) * 64: 2^7 .. 2^16
    if (!A.ad_on) return b64;
    const int w = vmx_round_w(A, tl, ql);
    return w == 4 ? b64 << 16 : (w == 2 ? b64 << 6 : (w == 1 ? b64 >> 4 : (b64 >> 14) + 1));
}
#endif
