// vmx_gapfill.h — the data formats of the gap fill (E5), in one place: size classes and band rule, the traceback layouts every fill form writes and
// k_gapfill_trace reads, the traceback / pool sizes of a problem, and the control block through which a chunk's two launches and the host talk.
// Included by vmx_kernels.h. Writers: k_dp.hip (the striped forms), vmx_dp_ad.h (the band forms). Reader: k_gapfill_trace (k_dp.hip).
#ifndef VMX_GAPFILL_H
#define VMX_GAPFILL_H
#include <stddef.h>
#include <stdint.h>

// ------------------------------------------------------------------------------------------------ size classes
#ifdef VMX_EMU
#define VMX_DP16_MAX 420              // emulator build: small switch point so that the CPU tests cover both layouts with small problems
#else
#define VMX_DP16_MAX 6000             // gap fill: problems with tl + ql <= this run two rows per lane in packed int16
#endif
#define VMX_DP16_OK(tl, ql) ((tl) + (ql) <= VMX_DP16_MAX)
// gap fill, small problems: four problems per wavefront, one per 16-lane row, 32-row stripes (two rows per lane), stripe width padded to
// a multiple of 16 steps so that the four rows refill their chunk registers on the same steps
#ifdef VMX_EMU
#define VMX_DP16X4_MAX 160
#else
#define VMX_DP16X4_MAX 1024       // larger problems run one per wavefront: a 700 x 700 problem almost never passes the band proof (its score falls ~0.8 per base
                                  // behind the all-match bound) and its full fill on one 16-lane row was a 5-10 ms tail of the second launch (3072 before)
#endif
#define VMX_DP16X4_OK(tl, ql) ((tl) + (ql) <= VMX_DP16X4_MAX)
#define VMX_X4_W(ql) ((((ql) + 31) + 15) & ~15)
// the small class: a non-empty problem that VMX_DP16X4_OK holds for
template <class I> __host__ __device__ constexpr bool vmx_gf_small(I tl, I ql) { return tl > 0 && ql > 0 && VMX_DP16X4_OK(tl, ql); }

// ------------------------------------------------------------------------------------------------ band rule
// anti-diagonal band form of the small-problem fill (vmx_dp_ad.h): EIGHT problems per wavefront, one per 16-lane DPP row and 16-bit register
// half, each on a fixed band of 32 * ns diagonals d = j - i in [dlo, dlo + 32 ns) (ns = 1 .. VMX_AD_NS_MAX diagonal pairs per lane). dlo is
// even, so that all problems of a wave compute the same diagonal parity on the same step, and the band's margins below min(0, ql - tl) and
// above max(0, ql - tl) are as equal as that allows. vmx_ad_geom returns g: a path that leaves the band holds at least g inserted AND g deleted
// bases (0: the band cannot hold both corners). The result is kept only when vmx_ad_proven (vmx_dp_ad.h) shows every such path is worse.
#define VMX_AD_NS_MAX 4
// nd = the band's width in diagonals (even)
__host__ __device__ static inline int vmx_ad_geom_nd(int tl, int ql, int nd, int* dlo_out) {
    const int dl = ql - tl, lo = dl < 0 ? dl : 0, hi = dl > 0 ? dl : 0;
    const int slack = nd - (hi - lo + 1);
    if (slack < 0) return 0;
    int mb = slack / 2, dlo = lo - mb;
    if (dlo & 1) {
        if (mb + 1 <= slack) { ++mb; --dlo; }
        else if (mb >= 1) { --mb; ++dlo; }
        else return 0;
    }
    *dlo_out = dlo;
    const int ma = slack - mb;
    return (mb < ma ? mb : ma) + 1;
}
__host__ __device__ static inline int vmx_ad_geom(int tl, int ql, int ns, int* dlo_out) { return vmx_ad_geom_nd(tl, ql, 32 * ns, dlo_out); }
// what a path pays at least for leaving a band of margin g: g matches fewer and two gaps of g bases
__host__ __device__ static inline long long vmx_ad_margin(int g, int match, int o1, int e1, int o2, int e2) {
    const long long c1 = o1 + (long long)g * e1, c2 = o2 + (long long)g * e2;
    return (long long)match * g + 2 * (c1 < c2 ? c1 : c2);
}
// band width (diagonal pairs per lane) a problem is tried with: the narrowest whose margin is at least pct % of min(tl, ql) (a 10 %-error
// read loses ~0.7 per base against the all-match bound), the widest one if that still reaches pct_min %, 0 = not worth trying / impossible
// (dpn = diagonals of the band per unit of ns, ns_lo .. ns_hi = the widths the caller has: 32 and 1 .. VMX_AD_NS_MAX for the eight-per-wave form)
__host__ __device__ static inline int vmx_ad_ns_nd(int tl, int ql, int match, int o1, int e1, int o2, int e2, int pct, int pct_min, int dpn, int ns_lo, int ns_hi) {
    if (tl <= 0 || ql <= 0) return 0;
    const int mn = tl < ql ? tl : ql;
    int dlo, g = 0;
    for (int ns = ns_lo; ns <= ns_hi; ++ns) {
        g = vmx_ad_geom_nd(tl, ql, dpn * ns, &dlo);
        if (g >= 1 && (g > mn || vmx_ad_margin(g, match, o1, e1, o2, e2) * 100 >= (long long)pct * mn)) return ns;
    }
    return (g >= 1 && vmx_ad_margin(g, match, o1, e1, o2, e2) * 100 >= (long long)pct_min * mn) ? ns_hi : 0;
}
__host__ __device__ static inline int vmx_ad_ns(int tl, int ql, int match, int o1, int e1, int o2, int e2, int pct, int pct_min) {
    return vmx_ad_ns_nd(tl, ql, match, o1, e1, o2, e2, pct, pct_min, 32, 1, VMX_AD_NS_MAX);
}
#define VMX_AD_PCT_DEFAULT 100
#define VMX_AD_PCT_MIN_DEFAULT 65
// The wave-wide instance of the band form (second launch, k_gapfill_redo: the VMX_REDO_PK class, two problems per wavefront): lane = the lane id, VMX_ADW_DPN * ns
// diagonals, ns = VMX_ADW_NS_MIN .. VMX_AD_NS_MAX (128 diagonals is what the first launch already had). Its rule is a constant of that launch, not the first launch's
// adaptive value: what it does not keep is filled in full on the spot.
#ifdef VMX_EMU
#define VMX_ADW_DPN 36                 /* emulator build: the band is computed 128 ns wide like the product's, but only its lowest 36 ns diagonals are claimed (geometry, g, proof):
                                          with tl + ql <= 160 the full width would hold every problem and the CPU tests would never see one that is not proven, at 32 ns never one
                                          that the first launch's band could not have proven as well */
#else
#define VMX_ADW_DPN 128
#endif
#define VMX_ADW_NS_MIN 2
#define VMX_ADW_PCT 100
#define VMX_ADW_PCT_MIN 65
#ifdef VMX_EMU
#define VMX_REDO_PK(tl, ql) ((tl) > 0 && (ql) > 0 && VMX_DP16X4_OK(tl, ql) && (tl) + (ql) >= 120)
#else
#ifndef VMX_REDO_PK_MIN
#define VMX_REDO_PK_MIN 384            /* redone problems of at least this perimeter run on whole wavefronts (the typical 270 x 270 problem included: the second launch
                                          holds ~3.5 k problems per batch, a quarter of the machine's wave slots — four per wave left it waiting 2.75 ms for 900 waves): two per
                                          wave in the wave-wide band (VMX_ADW_*, above), one per wave in full (vmx_gapfill_fill16) where that band's result is not proven.
                                          Either way in the 128-row layout, flag VMX_PK_FLAG */
#endif
#define VMX_REDO_PK(tl, ql) ((tl) > 0 && (ql) > 0 && VMX_DP16X4_OK(tl, ql) && (tl) + (ql) >= VMX_REDO_PK_MIN)
#endif

// ------------------------------------------------------------------------------------------------ traceback layouts
// One 7-bit byte per cell (VMX-DP-G, k_dp.hip), in one of four layouts. Which one a problem's bytes are in follows from its size class and from the
// word its fill leaves in out_score[p] (B.dpscore in the batched path):
//   0                  the striped layout of the problem's size class (what every fill without a band writes);
//   VMX_PK_FLAG        a small-class problem the second launch ran on the whole wave: the 128-row layout;
//   VMX_AD_FLAG + ns   a small-class problem kept from the first launch's band of 32 ns diagonals: the anti-diagonal layout;
//   a real score       the classes above the small one, and every class in the SCORE form (k_gapfill_fill), which has no band and whose reader passes no
//                      flag. Only a small-class problem's word is ever read as a flag.
#define VMX_AD_FLAG 16
#define VMX_PK_FLAG 1
enum vmx_tb_kind { VMX_TB_ROWS64 = 0, VMX_TB_ROWS128 = 1, VMX_TB_ROWS32 = 2, VMX_TB_AD = 3 };
// the band (diagonal pairs per lane) a flag names: > 0 exactly for the anti-diagonal layout
__host__ __device__ constexpr int vmx_tb_flag_ns(int tl, int ql, int flag) { return (vmx_gf_small(tl, ql) && flag > VMX_AD_FLAG) ? flag - VMX_AD_FLAG : 0; }
__host__ __device__ constexpr int vmx_tb_kind_of(int tl, int ql, int flag) {
    return vmx_gf_small(tl, ql) ? (vmx_tb_flag_ns(tl, ql, flag) ? VMX_TB_AD : flag == VMX_PK_FLAG ? VMX_TB_ROWS128 : VMX_TB_ROWS32)
                                : (tl > 0 && ql > 0 && VMX_DP16_OK(tl, ql)) ? VMX_TB_ROWS128 : VMX_TB_ROWS64;
}

// The striped layouts: stripes of R target rows, a stripe W(ql) steps wide (its anti-diagonals: row r of the stripe is on column j at step (j - 1) + r, so the
// last row needs R - 1 steps of ramp), a step one line of R bytes, byte r the cell of row r. R = 64: one row per lane, int32 cells (vmx_gapfill_fill_one);
// R = 128: two rows per lane of the wave, packed int16 (vmx_gapfill_fill16, and the wave-wide band of vmx_dp_ad.h); R = 32: two rows per lane of a 16-lane
// row (vmx_gapfill_fill16x4), the width padded to a multiple of 16 steps.
template <int RR> struct vmx_tb_stripes {
    static constexpr int R = RR, SH = RR == 32 ? 5 : RR == 64 ? 6 : 7;
    static_assert(RR == 1 << SH, "stripes of 32, 64 or 128 rows");
    template <class I> __host__ __device__ static constexpr I W(I ql) { return RR == 32 ? VMX_X4_W(ql) : ql + (RR - 1); }
    template <class I> __host__ __device__ static constexpr I nstr(I tl) { return (tl + (RR - 1)) >> SH; }      // (tl >= 0)
    // the line a wave (R = 32: a 16-lane row) stores on step `step` of stripe s
    __host__ __device__ __forceinline__ static constexpr size_t step_off(int s, int w, int step) { return ((size_t)s * (size_t)w + (size_t)step) * RR; }
    // ... and in that line the byte of row r of the stripe (a writer's lane stores from its first row on)
    __host__ __device__ __forceinline__ static constexpr size_t row_off(int s, int w, int step, int r) { return step_off(s, w, step) + r; }
    // cell (i, j), 1-based, of a problem whose stripes are w = W(ql) wide
    __host__ __device__ __forceinline__ static constexpr size_t cell_off(int w, int i, int j) {
        const int s = (i - 1) >> SH, r = (i - 1) & (RR - 1);      // (i - 1) / R, (i - 1) % R
        return ((size_t)s * (size_t)w + (size_t)((j - 1) + r)) * RR + r;
    }
    __host__ __device__ static constexpr int64_t bytes(int64_t tl, int64_t ql) { return nstr(tl) * W(ql) * RR; }
};
typedef vmx_tb_stripes<64> vmx_tb_rows64;
typedef vmx_tb_stripes<128> vmx_tb_rows128;
typedef vmx_tb_stripes<32> vmx_tb_rows32;

/* The anti-diagonal layout: one slot of W bytes per lane and anti-diagonal, in 64-byte lines of VMX_AD_AB consecutive anti-diagonals x 64 / (AB W) consecutive
   lanes, LANE-MAJOR inside a line: the AB slots a lane has in a line are one aligned run of AB W bytes (16 for the 4-byte slots), so the band fill keeps the
   bytes of AB steps in registers and writes them with ONE store per lane and problem (vmx_dp_ad.h: 16 / 8 / 4 bytes for W = 4 / 2 / 1) — a wave store covers
   whole lines once instead of a quarter of each of them AB times.
   Why lines of several anti-diagonals at all: with one anti-diagonal per line (rounds 2-3) the traceback walk — nine steps in ten go down a diagonal, two
   anti-diagonals back in the same lane — fetched a new 64-byte sector per step (5.2 GB per step of the pipeline for ~80 MB of bytes used). With AB
   anti-diagonals per line a diagonal stretch reads a line per AB / 2 steps, and the bytes of anti-diagonals s and s - 2 are in the same run.
   The slot is as wide as the band needs — W = 1 byte per lane and anti-diagonal for ns = 1 (one cell per lane and step), 2 for ns = 2, 4 for ns = 3 / 4
   (round 6: a HiFi problem, ns = 1 under the mode-L rule, wrote 64 bytes per anti-diagonal of which 16 were cells). */
#ifndef VMX_AD_AB
#define VMX_AD_AB 4     /* round 6: 4 (8 in rounds 4-5). With the step bound by the fill and the walk a narrow kernel that rides along, the fill's coalescing is worth more than the walk's
                           locality: ONT 15.35 / 15.68 -> 14.96 / 15.16 ms per step, HiFi unchanged (profiles/r06_u_traceback_line_blocking_ab.txt) */
#endif
static_assert(VMX_AD_AB == 4, "the band fill (vmx_dp_ad.h) stores blocks of exactly four anti-diagonals, two step pairs, with one store: AB = 1 or 8 needs another band loop");
#define VMX_AD_W(ns) ((ns) <= 0 ? 0 : ((ns) == 1 ? 1 : ((ns) == 2 ? 2 : 4)))
// byte offset of lane l's slot on anti-diagonal s (0-based: the cells with i + j = s + 1): the block of AB anti-diagonals, the line of the lane in the block,
// the lane's run in the line, the slot in the run. It is the sum of a part of l and a part of s (vmx_tb_ad_lane_off / vmx_tb_ad_step_off). Slot widths are
// powers of two, and the offset is written with the width's log2 (wsh): the fills know it at compile time, the traceback walk holds it in a register, and
// neither depends on the compiler proving a divisor to be a power of two.
#define VMX_AD_LSH 4      /* log2 of the 64 / AB bytes an anti-diagonal has in a line */
static_assert(64 / VMX_AD_AB == 1 << VMX_AD_LSH, "VMX_AD_LSH is log2(64 / VMX_AD_AB)");
__host__ __device__ __forceinline__ constexpr size_t vmx_ad_tb_off_sh(size_t s, size_t l, int wsh) {
    return (s / VMX_AD_AB) * (size_t)((VMX_AD_AB * 16) << wsh) + (l >> (VMX_AD_LSH - wsh)) * 64 + (l & (((size_t)1 << (VMX_AD_LSH - wsh)) - 1)) * (size_t)(VMX_AD_AB << wsh) + ((s % VMX_AD_AB) << wsh);
}
#define VMX_AD_WSH(W) ((W) == 1 ? 0 : (W) == 2 ? 1 : 2)
__host__ __device__ __forceinline__ constexpr size_t vmx_ad_tb_off(size_t s, size_t l, int W) { return vmx_ad_tb_off_sh(s, l, VMX_AD_WSH(W)); }      // W = 1, 2 or 4 bytes
__host__ __device__ constexpr int64_t vmx_ad_tb_bytes(int64_t tl, int64_t ql, int W) { return ((tl + ql + VMX_AD_AB - 1) & ~(int64_t)(VMX_AD_AB - 1)) * 16 * W; }

// The layout of one problem's bytes as k_gapfill_trace walks it: set up once, then one vmx_tb_cell_off per step.
struct vmx_tb_layout {
    int kind;       // vmx_tb_kind: the one thing every access branches on
    int w;          // striped kinds: steps per stripe; VMX_TB_AD: log2 of the bytes of a lane's slot
    int ns, dlo;    // VMX_TB_AD: the band (2 ns diagonals per lane from diagonal dlo on)
};
__host__ __device__ __forceinline__ vmx_tb_layout vmx_tb_layout_of(int tl, int ql, int flag) {
    vmx_tb_layout L;
    L.kind = vmx_tb_kind_of(tl, ql, flag);
    L.ns = 0; L.dlo = 0;
    if (L.kind == VMX_TB_AD) { L.ns = flag - VMX_AD_FLAG; vmx_ad_geom(tl, ql, L.ns, &L.dlo); L.w = VMX_AD_WSH(VMX_AD_W(L.ns)); }
    else L.w = L.kind == VMX_TB_ROWS32 ? vmx_tb_rows32::W(ql) : L.kind == VMX_TB_ROWS128 ? vmx_tb_rows128::W(ql) : vmx_tb_rows64::W(ql);
    return L;
}
// VMX_TB_AD: cell (i, j) is on diagonal x = (j - i) - dlo of the band, in lane x / (2 ns), byte ((x mod 2 ns) >> 1) of the lane's slot on anti-diagonal i + j
__host__ __device__ __forceinline__ constexpr size_t vmx_tb_ad_lane_off(const vmx_tb_layout& L, int i, int j) {      // the part that stays the same down a diagonal
    const int x = (j - i) - L.dlo, l = x / (2 * L.ns), k = (x - 2 * L.ns * l) >> 1;
    return vmx_ad_tb_off_sh(0, l, L.w) + k;
}
__host__ __device__ __forceinline__ constexpr size_t vmx_tb_ad_step_off(const vmx_tb_layout& L, int s) { return vmx_ad_tb_off_sh(s, 0, L.w); }      // the anti-diagonal's part (lane 0's slot)
__host__ __device__ __forceinline__ constexpr size_t vmx_tb_cell_off(const vmx_tb_layout& L, int i, int j) {
    if (L.kind == VMX_TB_AD) { const int x = (j - i) - L.dlo, l = x / (2 * L.ns), k = (x - 2 * L.ns * l) >> 1; return vmx_ad_tb_off_sh(i + j - 1, l, L.w) + k; }
    if (L.kind == VMX_TB_ROWS32) return vmx_tb_rows32::cell_off(L.w, i, j);
    if (L.kind == VMX_TB_ROWS128) return vmx_tb_rows128::cell_off(L.w, i, j);
    return vmx_tb_rows64::cell_off(L.w, i, j);
}

// ------------------------------------------------------------------------------------------------ sizes of a problem
// Traceback bytes. _full: the full-matrix forms (k_gapfill_fill), by size class. _batched: the batched path (k_gapfill_fill_ns), whose small problems get
// the anti-diagonal layout's slots only, w bytes wide (VMX_AD_W of the problem's own band; 4 where the caller has no band rule); the few that have to be filled
// again in full take _redo bytes from a second pool, handed out with an atomic counter when the first launch queues them (vmx_dp_prob.tb_off < 0: offset
// -tb_off - 1 into that pool, vmx_tb_ptr).
__host__ __device__ constexpr int64_t vmx_gf_tb_bytes_full(int64_t tl, int64_t ql) {
    return (tl > 0 && ql > 0) ? (VMX_DP16X4_OK(tl, ql) ? vmx_tb_rows32::bytes(tl, ql) : VMX_DP16_OK(tl, ql) ? vmx_tb_rows128::bytes(tl, ql) : vmx_tb_rows64::bytes(tl, ql)) : 0;
}
__host__ __device__ constexpr int64_t vmx_gf_tb_bytes_batched(int64_t tl, int64_t ql, int w) { return vmx_gf_small(tl, ql) ? vmx_ad_tb_bytes(tl, ql, w) : vmx_gf_tb_bytes_full(tl, ql); }
__host__ __device__ constexpr int64_t vmx_gf_tb_bytes_redo(int64_t tl, int64_t ql) { return VMX_REDO_PK(tl, ql) ? vmx_tb_rows128::bytes(tl, ql) : vmx_tb_rows32::bytes(tl, ql); }
// the size a small-class problem enters the queue key with (vmx_round_key): (tl + ql) * 64, 2^7 .. 2^16 — its bytes with 4-byte slots, whatever its own width
__host__ __device__ constexpr int64_t vmx_gf_key_size_small(int64_t tl, int64_t ql) { return vmx_ad_tb_bytes(tl, ql, 4); }
// (integer arithmetic: a select between the two pool pointers crashes this compiler's optimizer)
__host__ __device__ __forceinline__ uint8_t* vmx_tb_ptr(const uint8_t* tb_pool, const uint8_t* redo_pool, int64_t off) {
    const unsigned long long base = off >= 0 ? (unsigned long long)tb_pool : (unsigned long long)redo_pool;
    return (uint8_t*)(base + (unsigned long long)(off >= 0 ? off : -off - 1));
}
// a chunk's traceback buffer and the offset of its first problem (the prefix sum at the chunk's cut): both multiples of 64, so that with sizes that are
// multiples of 64 (checked below) every problem's space starts on a line — what the band fill's 16-byte stores rely on. The host checks it per chunk.
// (The emulator build's buffers come from malloc: 16 bytes, which is what the stores themselves need.)
#ifdef VMX_EMU
#define VMX_TB_BUF_ALIGN 16
#else
#define VMX_TB_BUF_ALIGN 64
#endif
__host__ __forceinline__ bool vmx_tb_base_ok(const void* buf, int64_t tb_off0) { return ((unsigned long long)buf & (VMX_TB_BUF_ALIGN - 1)) == 0 && (tb_off0 & 63) == 0; }
// the other per-problem pools (vmx_dp_prob): boundary rows (H, E1, E2 of ql + 1 columns), run words of the walk, CIGAR text
struct vmx_gf_pool_sizes { int64_t bnd, run, cig; };      // int32 units, uint32 units, bytes
__host__ __device__ constexpr vmx_gf_pool_sizes vmx_gf_pools(int64_t tl, int64_t ql) { return {3 * (ql + 1), tl + ql + 2, 2 * (tl + ql) + 16}; }
#define VMX_HEAD_THRESH (((int64_t)1 << 18) - 1)   /* traceback bytes above which a gap-fill problem is taken from the queue alone (k_size_order thresh): ~450 x 450 and up */

// ------------------------------------------------------------------------------------------------ control block
// One per chunk (vmx_gapfill_chunk), zeroed by the host once per batch, written by the size-order kernels and the two fill launches, fetched by the host
// with the batch's results. VMX_GF_SLOT ints.
#define VMX_GF_SLOT (32 + 544)
struct vmx_gf_ctl {
    int32_t range[4];                 // k_size_scatter: [0] = entries at the head of the queue that go one per task (key above the threshold), [1] = all queued
    int32_t head[8];                  // first launch's queue heads: [0] eight problems at a time behind the head entries, [1] the head entries one at a time
                                      // (k_size_scatter zeroes [0 .. 3])
    int32_t redo_n;                   // entries of the list the first launch leaves for the second
    int32_t redo_head;                // second launch: head of its four-at-a-time loop
    int32_t redo_pair_head;           // second launch: head of the VMX_REDO_PK loop (two entries at a time)
    int32_t n_not_proven;             // small problems tried in a band and not proven (the host adapts the band-width rule to this rate)
    unsigned long long redo_bytes;    // bytes handed out of the second pool — or asked for: the host grows the pool when this passes its size
    int32_t redo_kept;                // second launch: VMX_REDO_PK problems kept from the wave-wide band
    int32_t redo_full;                //                ... filled in full after all
    int32_t unused[12];
    int32_t scratch[VMX_GF_SLOT - 32];    // k_size_hist / k_size_scatter: 257 class counts, 256 cursors
};
static_assert(sizeof(vmx_gf_ctl) == 4 * VMX_GF_SLOT, "a control block is VMX_GF_SLOT ints");
static_assert(offsetof(vmx_gf_ctl, range) == 4 * 0 && offsetof(vmx_gf_ctl, head) == 4 * 4 && offsetof(vmx_gf_ctl, redo_n) == 4 * 12 && offsetof(vmx_gf_ctl, redo_head) == 4 * 13 &&
              offsetof(vmx_gf_ctl, redo_pair_head) == 4 * 14 && offsetof(vmx_gf_ctl, n_not_proven) == 4 * 15 && offsetof(vmx_gf_ctl, redo_bytes) == 4 * 16 &&
              offsetof(vmx_gf_ctl, redo_kept) == 4 * 18 && offsetof(vmx_gf_ctl, redo_full) == 4 * 19 && offsetof(vmx_gf_ctl, scratch) == 4 * 32,
              "the fields of a fetched control block are where the int indices 0, 4, 12 .. 19 and 32 were");

// ------------------------------------------------------------------------------------------------ build-time checks of the layouts
// (evaluated where VMX_GAPFILL_CHECKS is defined: in k_dp.hip, which holds every writer and the reader — once per build, gfx950 or emulator, not once per includer)
#ifdef VMX_GAPFILL_CHECKS
// every cell of a problem lies inside the problem's bytes and where the writer's (stripe, step, row) addressing puts it — at the stripe and padding edges
template <int RR> constexpr bool vmx_tb_stripes_ok(int tl) {
    typedef vmx_tb_stripes<RR> S;
    const int qls[5] = {1, 15, 16, 17, 33};
    for (int q = 0; q < 5; ++q) {
        const int ql = qls[q], w = S::W(ql);
        const size_t bytes = (size_t)S::bytes(tl, ql);
        for (int i = 1; i <= tl; ++i) {
            const int s = (i - 1) / RR, r = (i - 1) % RR;
            for (int j = 1; j <= ql; ++j) {
                const size_t at = S::cell_off(w, i, j);
                if (!(at < bytes) || at != S::step_off(s, w, (j - 1) + r) + r || at != S::row_off(s, w, (j - 1) + r, r)) return false;
            }
        }
    }
    return true;
}
#define VMX_TB_STRIPES_CHECK(S) \
    static_assert(vmx_tb_stripes_ok<S::R>(1) && vmx_tb_stripes_ok<S::R>(S::R - 1) && vmx_tb_stripes_ok<S::R>(S::R), "striped traceback layout: a cell outside the problem's bytes"); \
    static_assert(vmx_tb_stripes_ok<S::R>(S::R + 1), "striped traceback layout: a cell outside the problem's bytes"); \
    static_assert(vmx_tb_stripes_ok<S::R>(2 * S::R), "striped traceback layout: a cell outside the problem's bytes"); \
    static_assert(vmx_tb_stripes_ok<S::R>(2 * S::R + 1), "striped traceback layout: a cell outside the problem's bytes")
VMX_TB_STRIPES_CHECK(vmx_tb_rows64);
VMX_TB_STRIPES_CHECK(vmx_tb_rows128);
VMX_TB_STRIPES_CHECK(vmx_tb_rows32);
#undef VMX_TB_STRIPES_CHECK
// the anti-diagonal layout, for each slot width, over 16 lanes x the anti-diagonals of a problem ROUNDED UP to whole blocks of AB (the band fill stores whole
// blocks): every slot lies inside the problem's bytes; a lane's AB slots of a block are one run of AB W bytes aligned to its length, in step order; and the map
// is one-to-one on (s, l) — the slots start at multiples of W below bytes = W x (number of slots), so it is enough that no two of them start at the same place
constexpr bool vmx_ad_tb_ok(int W) {
    const int tls[6] = {1, 31, 32, 33, 64, 65}, qls[5] = {1, 15, 16, 17, 33};
    for (int t = 0; t < 6; ++t)
        for (int q = 0; q < 5; ++q) {
            const size_t bytes = (size_t)vmx_ad_tb_bytes(tls[t], qls[q], W);
            const int ns = (tls[t] + qls[q] + VMX_AD_AB - 1) / VMX_AD_AB * VMX_AD_AB;
            if (bytes != (size_t)ns * 16 * (size_t)W) return false;
            bool used[(65 + 33 + VMX_AD_AB) * 16] = {};
            for (int s = 0; s < ns; ++s)
                for (int l = 0; l < 16; ++l) {
                    const size_t at = vmx_ad_tb_off(s, l, W);
                    if (at + W > bytes || at % W || used[at / W]) return false;
                    used[at / W] = true;
                    if (s % VMX_AD_AB == 0 ? at % (size_t)(VMX_AD_AB * W) != 0 : at != vmx_ad_tb_off(s - 1, l, W) + W) return false;
                    if (at != vmx_ad_tb_off(s, 0, W) + vmx_ad_tb_off(0, l, W)) return false;      // a part of the lane plus a part of the anti-diagonal
                }
        }
    return true;
}
static_assert(vmx_ad_tb_ok(1), "anti-diagonal traceback layout, 1-byte slots: not one-to-one into the problem's bytes in aligned runs per lane");
static_assert(vmx_ad_tb_ok(2), "anti-diagonal traceback layout, 2-byte slots: not one-to-one into the problem's bytes in aligned runs per lane");
static_assert(vmx_ad_tb_ok(4), "anti-diagonal traceback layout, 4-byte slots: not one-to-one into the problem's bytes in aligned runs per lane");
// The band fill's 16-byte stores need every problem's traceback space to start at a multiple of 16: the spaces are handed out by a prefix sum over these
// size functions (k_round_prep, vm_k_cigar_batch_banded) from a chunk base that the host checks (vmx_tb_base_ok), so every one of them returns multiples of 64
constexpr bool vmx_tb_sizes_ok() {
    const int ls[28] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5001};      // around every stripe height, padding and class edge
    for (int t = 0; t < 28; ++t)
        for (int q = 0; q < 28; ++q) {
            const int tl = ls[t], ql = ls[q];
            if (vmx_ad_tb_bytes(tl, ql, 1) % 64 || vmx_ad_tb_bytes(tl, ql, 2) % 64 || vmx_ad_tb_bytes(tl, ql, 4) % 64) return false;
            if (vmx_tb_rows32::bytes(tl, ql) % 64 || vmx_tb_rows64::bytes(tl, ql) % 64 || vmx_tb_rows128::bytes(tl, ql) % 64) return false;
            if (vmx_gf_tb_bytes_full(tl, ql) % 64 || vmx_gf_tb_bytes_redo(tl, ql) % 64) return false;
            for (int w = 0; w <= 4; w += (w ? w : 1)) if (vmx_gf_tb_bytes_batched(tl, ql, w) % 64) return false;
        }
    return true;
}
static_assert(vmx_tb_sizes_ok(), "a traceback size that is no multiple of 64 bytes would misalign the next problem's space for the band fill's wide stores");
#endif
#endif
