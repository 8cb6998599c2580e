// vmx_kernels.h — device-side data types shared by the kernels and the host orchestration.
#ifndef VMX_KERNELS_H
#define VMX_KERNELS_H
#include <stdint.h>

// one DP problem of the gap-fill stage (E5); offsets into the per-batch pools
struct vmx_dp_prob {
    int64_t t_off, q_off;     // into the target / query code pools
    int32_t tl, ql;
    int64_t tb_off;           // traceback bytes (sizes and layouts: vmx_gapfill.h); negative: -tb_off - 1 into the second pool (vmx_tb_ptr)
    int64_t bnd_off;          // int32 units (the three pools' sizes: vmx_gf_pools)
    int64_t run_off;          // uint32 units
    int64_t cig_off;          // bytes
};

// anchor in the layout the chain kernels use (16 B): SURVEY §8(a) row T
struct vmx_anchor {
    int32_t q;     // read position
    int16_t l;     // length
    int16_t s;     // strand +1 / -1
    int64_t r;     // global reference position
};

// The length is an UNSIGNED 16-bit field (0 ... 65535, what the stage entries accept) kept in an int16_t: every reader takes it through this, never as `a.l`
// (a sign-extended 32768 ... 65535 is a negative length, and in k_chain_fast.hip a negative index into S_i_count).
__host__ __device__ __forceinline__ int vmx_anchor_len(const vmx_anchor& a) { return (int)(uint16_t)a.l; }

// hashed minimizer index slot (16 B): open addressing, empty key = ~0
struct vmx_slot { uint64_t key; uint32_t start; uint32_t count; };

// cost tables on the device
struct vmx_tables {
    const float* extra; int32_t extra_n;
    const float* readgap_h; const float* readgap_r; const float* large_readgap;
    const double* log2cache; int32_t log2cache_n;
    const double* log2int;
    int32_t extra_arith_n;   // extra[g] == (float)(min(10, g*0.01) + g*0.001) for every g below this (checked on the host, vmx_capi.hip)
};

// extra[min(g, extra_n-1)] as a double without touching HBM where the table has a closed form: below extra_arith_n the entry is the
// linear part of :15371-15376 (two multiplies; identical to the table by the host's exhaustive check), at or above the last index it
// is the table's final value 36.0; only the logarithmic stretch in between is loaded.
__device__ __forceinline__ double vmx_extra_cost(const vmx_tables& tab, long long g) {
    if (g >= (long long)tab.extra_n - 1) return 36.0;
    if (g < (long long)tab.extra_arith_n) {
        const double dg = (double)(int)g;
        const double a = dg * 0.01;
        return (double)(float)((a < 10.0 ? a : 10.0) + dg * 0.001);
    }
    return (double)tab.extra[g];
}

// ---- gap geometry shared by the chain DPs (GC :24953-24984, LC :27418-27456) ----
// Both geometries without data-dependent branches. With rg = q_i - q_j - l_j, m = min(rg, 0) (the overlap, negated) and d = r_i - r_j the eight
// cases of :24953-24984 collapse to  readgap = rg - m,  bonus = l_i + m,  refgap = +-d + c  with a 32-bit c:
//   s_i = s_j = +1:  d - m - l_j          s_i = +1, s_j = -1:  d - m + 1
//   s_i = s_j = -1: -d - l_i - m          s_i = -1, s_j = +1:  d + l_i + m - 1 - l_j
// and the -mode asm fork's (mammap_asm.py:20660-20688: non_overlap_size = q_i - q_j, no +-1 between opposite strands) to the same two lines for
// equal strands and  d - m  /  d + l_i - m - l_j  for opposite ones. The lanes of a wavefront hold candidates on both strands, with and without
// overlap: as nested ifs the compiler emits an exec-mask region per case; as selects it is a dozen VALU instructions.
template <bool ASMV>
__device__ __forceinline__ void vmx_gap_geometry_sel(int qi, long long ri, int si, int li, int qj, long long rj, int sj, int lj,
                                                     long long& readgap, long long& refgap, long long& bonus) {
    const int rg = qi - qj - lj;                       // read positions and lengths: 32-bit
    const int m = rg < 0 ? rg : 0;
    readgap = (long long)(rg - m);
    bonus = (long long)(li + m);
    const long long d = ri - rj;
    const bool same = si == sj;
    int c; long long t;
    if (si == 1) { c = (same ? -lj : (ASMV ? 0 : 1)) - m; t = d; }
    else { c = same ? -li - m : li - lj + (ASMV ? -m : m - 1); t = same ? -d : d; }
    refgap = t + (long long)c;
}
// arguments of k_local_seed (L2): inputs, per-workgroup-slot scratch pools, outputs
struct vmx_lseed_args {
    const uint8_t* ocodes; const int64_t* roff;            // oriented read codes
    const uint8_t* ref; const int64_t* coff; int32_t nseq;  // reference codes + contig offsets (nseq+1)
    const vmx_anchor* guide_rows; const int32_t* guide_len; const int32_t* n_guides_used; const int64_t* aoff;
    int32_t n_reads, k, look_span, read_span, sort_by_start;
    const int32_t* order; int32_t* queue;                   // read indices longest first + the queue head (zero at launch)
    int64_t la_slot_len;                                    // local-anchor slot of a listed read = la_slot_len * VMX_LA_SLOT(len) rows at la_off[r]
    int32_t* head_pool; int32_t* next_pool;                 // HEAD[head_stride] (epoch-tagged entries) / NEXT[tpos_cap] per slot
    int64_t head_stride;                                    // heads per slot: 4^k, or 2^14 buckets when 14 < 2k <= 18 (k_local_seed)
    int32_t* epoch_pool;                                    // current epoch of every slot's head table (persists across launches)
    int32_t* sq_pool; int32_t* dst_pool;                    // hit_cap ints each
    int64_t* tpos_pool; int64_t tpos_cap;
    unsigned long long* dbg;    // optional phase timers (VMX_DBG=1)
    uint64_t* hkey2_pool;
    uint64_t* hkey_pool; int64_t* hval_pool; int32_t* goff_pool; int64_t hit_cap;
    int32_t* pcnt_pool; int64_t pcnt_cap; int32_t* pc2_pool; int64_t* stg_pool;
    uint64_t* gkey_pool; int32_t* gq_pool; int64_t* gr_pool; int64_t gkey_cap;
    vmx_anchor* la_rows; uint64_t* la_ekey; vmx_anchor* la_sorted; const int64_t* la_off; int32_t* la_cnt; int32_t* status;
    // collect_second_round_anchors (mammap_asm.py:22477-22756; null otherwise): unit r looks up the read positions [r_st[r], r_en[r] - k) of the
    // sequence at ocodes + rd_off[r] (length rd_len[r]: every unit of a contig shares it) and owns la_off[r + 1] - la_off[r] anchor rows
    const int64_t* rd_off; const int64_t* rd_len; const int32_t* r_st; const int32_t* r_en;
};

// k_local_seed_band (k_local_band.hip), one wavefront per read: read positions per chunk, hits per chunk (LDS tile; also the capacity of the
// plan's interval list), guide anchors staged per chunk, log2 of the chunk table's bucket heads, keys of the LDS sort region
// (4 * (heads + 2 * QC + 512) <= 8 * SORTK and HCAP <= SORTK: the table with its occupancy map and the sorted hits live there in turn)
#ifdef VMX_EMU
#define VMX_LB_QC 128               // emulator build: small chunks so that the CPU tests cross many chunk boundaries, cut chunks at the guide slice and overflow the hit tile
#define VMX_LB_HCAP 256
#define VMX_LB_GS 20
#define VMX_LB_NBLOG 8
#define VMX_LB_SORTK 512
#else
#ifndef VMX_LB_QC                    /* (tuning builds override the set: VMX_EXTRA_FLAGS="-DVMX_LB_QC=256 -DVMX_LB_HCAP=256 -DVMX_LB_SORTK=512 -DVMX_LB_NBLOG=8") */
#define VMX_LB_QC 512
#define VMX_LB_HCAP 512
#define VMX_LB_NBLOG 9
#define VMX_LB_SORTK 1024
#endif
#ifndef VMX_LB_GS
#define VMX_LB_GS 64
#endif
#endif
#ifndef VMX_LB_BMLOG
#define VMX_LB_BMLOG 14              /* log2 of the bits of the chunk table's occupancy map */
#endif
#ifndef VMX_LB_WAVES
#define VMX_LB_WAVES 2               /* waves per SIMD the register allocation of k_local_seed_band is held to */
#endif
#define VMX_LB_TABLE_U64 (((1 << VMX_LB_NBLOG) + 2 * VMX_LB_QC + (1 << (VMX_LB_BMLOG - 5))) / 2)          /* heads + entries + occupancy map, in 8-byte units */
#define VMX_LB_REGION_U64 (VMX_LB_SORTK > VMX_LB_TABLE_U64 ? VMX_LB_SORTK : VMX_LB_TABLE_U64)
#define VMX_LB_CQ_BYTES (128 + 2 * VMX_LB_HCAP > 2304 ? 128 + 2 * VMX_LB_HCAP : 2304)     /* candidate queue: one sweep (512 words) + the < 64 left over from the sweep before; later the run walk's marks + one index per hit */
#define VMX_LB_LDS_BYTES (8 * (VMX_LB_REGION_U64 + VMX_LB_HCAP) + VMX_LB_CQ_BYTES)
#define VMX_ED_WAVES 16              // max waves per workgroup of k_edit_distance (passes pipelined across them) = carry ring depth
#define VMX_ED_LONG 16384            // patterns longer than this (> 4 passes) go to the 16-wave launch
#define VMX_EDB_HW 768               // k_ed_banded: half width of the band in rows
#define VMX_EDB_MAXD 512             // k_ed_banded: |m - n| above this is not eligible (goes to the unbanded kernel)
#define VMX_EDB4_HW 320              // k_ed_banded4 (four problems per wave): half width of the band; 2*HW + MAXD + 64 <= 16 blocks
#define VMX_EDB4_MAXD 256            // k_ed_banded4: |m - n| above this goes to k_ed_banded
#ifndef VMX_LSEED_WAVES
#define VMX_LSEED_WAVES 6            // k_local_seed: waves per SIMD the register allocation is held to (80 VGPRs: 3 workgroups of 512 per CU)
#endif
#define VMX_SORT_LDS 4096           // uint64 keys sorted in LDS by vmx_block_sort_u64 (larger sorts run in HBM)
#ifdef VMX_EMU
#define VMX_SORT_LDS_BIG 8192       // emulator build: a small tile so that the CPU tests reach the tiled (multi-tile) sort
#else
#define VMX_SORT_LDS_BIG 16384      // k_cluster_big: keys per LDS tile (128 KB of the 160 KB per CU)
#endif
#define VM_READ_FASTPATH_DEV (-21)   // the reference would switch to a *_fast heuristic that is not built yet
#include "vmx_gapfill.h"      // the gap fill (E5): size classes, band rule, traceback layouts, pool sizes, control block
#define VMX_TB_CHUNK ((int64_t)4 << 30)    // gap fill: traceback bytes held at a time; a batch needing more runs fill + trace chunk by chunk. 4 GB (12 in round 3, 8 earlier
                                          // in round 4): FIVE batches in flight fit at hg38 size (296 of 309 GB) and the step does not notice the extra chunks (VMX_TB_CHUNK_GB: tuning knob)
#ifdef VMX_EMU
#define VMX_MAX_BATCH_BASES 20000          // emulator build: small limits so that the CPU tests split a batch
#define VMX_MAX_BATCH_READS 6
#else
#define VMX_MAX_BATCH_BASES ((int64_t)160 << 20)     // bases per internal sub-batch of vm_align_batch (a pipeline batch is ~60 M)
#define VMX_MAX_BATCH_READS 16384
#endif
#define VMX_LA_SLOT(len) ((len) / 2 + 4096)   // regular local-anchor slot of a read (rows); overflowing reads are re-run with 8x .. 4096x
#define VMX_SELECT_LDS 3072           // k_chain_select: largest LDS size class (17 B per anchor: S, P, S_arg, used flags); see vmx_launch_chain_select
#define VMX_LC_LDS_MAX_DEFAULT 13056   // reads with more local anchors than this run the chain DP on HBM-resident arrays (VMX_LC_LDS_MAX)
#define VMX_GC_LDS_MAX_DEFAULT 13056
#define VMX_CHAIN_LDS_MAX_SHARED 512   // ... what the chain kernels actually use (VMX_LC_LDS_MAX / VMX_GC_LDS_MAX override it): above it S / S_arg stay in HBM, where
                                      // one wave per read leaves room for eight waves per SIMD instead of one — a large LDS claim per wavefront starves the
                                      // kernel itself (alone: 52.5 -> 49.1 ms per batch) and the other batches' kernels of CUs (three in flight: 46.3 -> 42.5)
#define VMX_LC_BYTES_PER_ANCHOR 12   // S8 + SA4 (LDS bytes per anchor in k_chain_local; the anchors themselves are read from HBM in register blocks)
#define VMX_GC_BYTES_PER_ANCHOR 12   // S8 + SA4 (LDS bytes per anchor in k_chain_global; anchors and coverage are read from HBM in register blocks)

#endif
