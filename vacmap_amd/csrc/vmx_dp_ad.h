// vmx_dp_ad.h — E5 gap fill, anti-diagonal band form: EIGHT problems per wavefront (included by k_dp.hip only).
//
// The same dual-affine recurrence and the same 7-bit traceback byte as the striped forms in k_dp.hip (VMX-DP-G), laid out for the
// problems the read path actually produces (tl ~ ql ~ 270, |tl - ql| a few bases): a problem lives in one 16-lane DPP row and one 16-bit
// half of every register (the other half is a second, unrelated problem, so all v_pk_* arithmetic serves two problems), on a FIXED band
// of ND = 32 * NS diagonals d = j - i in [dlo, dlo + ND). Lane l owns the 2 * NS diagonals x = d - dlo in [2 NS l, 2 NS l + 2 NS): the even
// ones ("A" sets, k = 0 .. NS-1) are computed on even anti-diagonals a = i + j, the odd ones ("C" sets) on odd a (dlo is even). A cell
// needs the cell above it (diagonal x + 1) and the cell to its left (diagonal x - 1), both one anti-diagonal back, and its own
// diagonal's previous cell: all of that is in the lane's own registers except one neighbour per step, which comes from the next lane
// (C_{NS-1} takes A_0 of lane l + 1: row_shl:1) or the previous one (A_0 takes C_{NS-1} of lane l - 1: row_shr:1) — three DPP moves per
// step for 2 * NS cells per lane. There are no stripes, no boundary rows in memory and no ramp: a step computes a whole anti-diagonal of
// the band. Rows / columns 0 are not special either: the state starts as -infinity everywhere except H(0,0) = 0, and the recurrence
// itself produces H(0,j) = best gap of j (through F) and H(i,0) (through E) on the way; cells with i < 0 or j < 0 stay near -infinity,
// cells past tl / ql compute garbage that only ever feeds other garbage. Target codes move down the lanes one diagonal pair per two
// steps, query codes move up (one DPP each per step pair), fed at lane 0 / lane 15 from 16-entry chunk registers that rotate one lane
// per use and are refilled with one coalesced load every 16 pairs.
// Traceback bytes: tb[vmx_ad_tb_off(a - 1, l, W) + k] for the cell of anti-diagonal a on diagonal x = 2 NS l + 2 k + (a & 1): W = VMX_AD_W(NS) bytes per lane,
// problem and step (vmx_gapfill.h: 64-byte lines of VMX_AD_AB = 4 anti-diagonals x 64 / (AB W) lanes, a lane's four slots of a line side by side). The band
// loop runs a block of four steps per turn and stores it once: one 16-byte store per lane and problem for the 4-byte slots, 8 for W = 2, 4 for W = 1.
#ifndef VMX_DP_AD_H
#define VMX_DP_AD_H

#ifdef VMX_EMU
__device__ __forceinline__ int vmx_r16_shl1_in(int v, int in) { const int l = vmx_lane(); const int e = __shfl(v, (l & 48) | ((l + 1) & 15)); return (l & 15) == 15 ? in : e; }
__device__ __forceinline__ unsigned vmx_perm(unsigned s0, unsigned s1, unsigned sel) {
    unsigned r = 0;
    for (int b = 0; b < 4; ++b) {
        const unsigned c = (sel >> (8 * b)) & 0xffu;
        const unsigned v = c < 4 ? (s1 >> (8 * c)) & 0xffu : c < 8 ? (s0 >> (8 * (c - 4))) & 0xffu : 0u;
        r |= v << (8 * b);
    }
    return r;
}
#else
__device__ __forceinline__ int vmx_r16_shl1_in(int v, int in) { return __builtin_amdgcn_update_dpp(in, v, 0x101, 0xf, 0xf, false); }   // row_shl:1
__device__ __forceinline__ unsigned vmx_perm(unsigned s0, unsigned s1, unsigned sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
#endif
// the hand-offs of a band that lives in LW lanes: one 16-lane DPP row (row_* moves) or the whole wavefront (wave_* moves, vmx_device.h)
template <int LW> __device__ __forceinline__ int vmx_ad_shl1_in(int v, int in) { if constexpr (LW == 16) return vmx_r16_shl1_in(v, in); else return vmx_shl1_in(v, in); }
template <int LW> __device__ __forceinline__ int vmx_ad_shr1_in(int v, int in) { if constexpr (LW == 16) return vmx_r16_shr1_in(v, in); else return vmx_shr1_in(v, in); }
template <int LW> __device__ __forceinline__ int vmx_ad_rol1(int v) { if constexpr (LW == 16) return vmx_r16_rol1(v); else return vmx_rol1(v); }
template <int LW> __device__ __forceinline__ int vmx_ad_ror1(int v) { if constexpr (LW == 16) return vmx_r16_ror1(v); else return vmx_ror1(v); }

// TAGGED scores: a register half holds 8 * (score + bias) + tag, an unsigned 16-bit value. Every wave-instruction of the two-operand
// 32-bit class (v_add_u32, v_sub_u32, v_and / or / xor) issues in 2.3 cycles on gfx950, everything in the VOP3 / VOP3P / DPP class — all
// packed-int16 arithmetic, v_bfi, v_perm, v_alignbit — in 4.2 (profiles/r04_q_valu_calibration.md). Gap costs and match scores are scaled by
// 8, so subtracting or adding them is a plain 32-bit subtract / add of both halves at once that never touches the tags (and, with every half
// of every result inside [0, 65535], never borrows or carries between the halves: the 32-bit sum of the halves' sums is exact whatever the
// order of the terms). A max is one v_pk_max_u16, and on equal scores the larger tag wins, so the tags encode ksw2's tie order and the
// winner carries its own traceback code:
//   - stored H and every gap-opening candidate H - O carry tag 7; stored E1 / F1 / E2 / F2 carry 6 / 3 / 1 / 0 (VMX_AD_T*). An E or F max of
//     (H - O, E) therefore gives the opening on a tie (as the strict "E > H - O" of the flags always did) and leaves tag 7 when it opened,
//     the E's own tag when it extended: the extension flag is one bit of the result (E1: bit 0, E2: bit 1, F1: bit 2, F2: bit 0 clear).
//   - the h max of (H_diag + score [tag 7], E1, F1, E2, F2) takes the first of diagonal > E1 > F1 > E2 > F2 on a tie, and its tag names
//     the source. One v_and per E / F puts the stored tag back after the max, one v_or per cell the 7 on H.
// The byte is built per pair of cells (vmx_ad_bytes): the low bytes of the halves are gathered with v_perm into the [k.X, k+1.X, k.Y, k+1.Y]
// order the stores want, the source comes out of a v_perm lookup on the h tags, the four flags out of three v_bfi. The match score is
// min(tc ^ qc, PEN) with the codes held << VMX_AD_CSH: 0 on a match, PEN = 8 (match - mismatch) on any mismatch.
// Compiled (gfx950, NS = 4), one step of four cell pairs with its DPP hand-offs and store: 137 VALU = 62 two-cycle + 75 four-cycle,
// ~458 cycles by the table, where the int16 form took 203 = 56 + 147, ~746 (profiles/r07_tagged_fill_ab.md). With the block stores a turn of
// four steps is 628 VALU and 2 stores where four such steps were 656 and 8 (profiles/ad_block_store_ab.md).
//   Range (vmx_ad_bias, vmx_ad_scores_ok): every value a step computes is at most match * (VMX_DP16X4_MAX / 2 + 1) (one match more than the
// best a problem with tl + ql <= VMX_DP16X4_MAX reaches); "-infinity" is VMX_AD_NEGINF and every value, -infinity included, loses at most
// max(e1, e2) per step (E = max(..., E_prev) - e), plus one gap opening or mismatch for the candidates fed to a max. The bias lifts that
// lowest value to 0; the scores fit when the highest one then stays <= 8191. For the gap fill's scoring (2, -4, 4, 2, 24, 1) the values lie
// in [-6170, 1026]: bias 6170, halves in [0, 57575] of the 65535 an unsigned half allows. The same integers as the former int16 form
// (score + 8192) are compared, with the same tie rules, so every traceback byte is the same.
#define VMX_AD_NEGINF (-4096)
#define VMX_AD_CSH 12                                              // codes are held << 12: tc ^ qc is 0 or >= 4096 >= PEN
#define VMX_AD_TE1 6u
#define VMX_AD_TF1 3u
#define VMX_AD_TE2 1u
#define VMX_AD_TF2 0u
__host__ __device__ constexpr long long vmx_ad_imax(long long a, long long b) { return a > b ? a : b; }
__host__ __device__ constexpr long long vmx_ad_imin(long long a, long long b) { return a < b ? a : b; }
__host__ __device__ constexpr long long vmx_ad_bias(int mismatch, int o1, int e1, int o2, int e2) {
    return -((long long)VMX_AD_NEGINF - (long long)(VMX_DP16X4_MAX + 1) * vmx_ad_imax(e1, e2) - vmx_ad_imax(vmx_ad_imax(o1, o2), -(long long)mismatch));
}
// can the anti-diagonal fill run a problem of the small class (tl + ql <= VMX_DP16X4_MAX) with these scores? Besides the range, -infinity
// must stay below every real value of the band (a path along diagonal 0, then one gap), gap costs included.
__host__ __device__ constexpr bool vmx_ad_scores_ok(int match, int mismatch, int o1, int e1, int o2, int e2) {
    return match >= 0 && mismatch <= match && 8LL * (match - mismatch) <= (1 << VMX_AD_CSH) && o1 >= 0 && e1 >= 0 && o2 >= 0 && e2 >= 0 &&
           (long long)match * (VMX_DP16X4_MAX / 2 + 1) + vmx_ad_bias(mismatch, o1, e1, o2, e2) <= 8191 &&
           vmx_ad_imin(mismatch, 0) * (VMX_DP16X4_MAX / 2) - vmx_ad_imin(o1 + (long long)e1 * VMX_DP16X4_MAX, o2 + (long long)e2 * VMX_DP16X4_MAX)
               - vmx_ad_imax(o1, o2) - vmx_ad_imax(e1, e2) > (long long)VMX_AD_NEGINF + vmx_ad_imax(o1, o2);
}
static_assert(vmx_ad_scores_ok(2, -4, 4, 2, 24, 1), "the gap fill's own scoring (vmx_stage_extend.hip: gf_score) must fit the tagged 16-bit domain");
struct vmx_ad_consts { unsigned O1, O2, E1, E2, MATCH, PEN, NH, NE1, NE2, NF1, NF2; };

// one cell (both halves): up = (H, E1, E2) of the cell above, left = (H, F1, F2) of the cell to the left, H = the diagonal predecessor on
// entry and the cell's H on return; tc / qc = target / query codes (<< VMX_AD_CSH). w = {h, e1, e2, f1, f2} before the tags are put back:
// what vmx_ad_bytes reads the traceback byte from.
__device__ __forceinline__ void vmx_ad_cell(const vmx_ad_consts& K, unsigned upH, unsigned upE1, unsigned upE2, unsigned leftH, unsigned leftF1,
                                            unsigned leftF2, unsigned tc, unsigned qc, unsigned& H, unsigned& E1, unsigned& E2, unsigned& F1, unsigned& F2,
                                            unsigned (&w)[5]) {
    const unsigned e1v = vmx_pk_max_u16(upH - K.O1, upE1) - K.E1, e2v = vmx_pk_max_u16(upH - K.O2, upE2) - K.E2;        // tag 7: opened
    const unsigned f1v = vmx_pk_max_u16(leftH - K.O1, leftF1) - K.E1, f2v = vmx_pk_max_u16(leftH - K.O2, leftF2) - K.E2;
    E1 = e1v & ~((7u ^ VMX_AD_TE1) * 0x00010001u); E2 = e2v & ~((7u ^ VMX_AD_TE2) * 0x00010001u);                       // 7 -> the stored tag
    F1 = f1v & ~((7u ^ VMX_AD_TF1) * 0x00010001u); F2 = f2v & ~((7u ^ VMX_AD_TF2) * 0x00010001u);
    const unsigned hd = H + K.MATCH - vmx_pk_min_u16(tc ^ qc, K.PEN);                                                  // tag 7
    const unsigned h = vmx_pk_max_u16(vmx_pk_max_u16(hd, E1), vmx_pk_max_u16(vmx_pk_max_u16(F1, E2), F2));
    H = h | 0x00070007u;
    w[0] = h; w[1] = e1v; w[2] = e2v; w[3] = f1v; w[4] = f2v;
}

// the traceback bytes of cells a and b, [a.X, b.X, a.Y, b.Y] (the order the stores take): bits 0-2 the source (0 diagonal, 1 E1, 2 E2, 3 F1,
// 4 F2), bits 3-6 the extension flags of E1, E2, F1, F2 — the byte the striped forms of k_dp.hip write
__device__ __forceinline__ unsigned vmx_ad_bytes(const unsigned (&a)[5], const unsigned (&b)[5]) {
    constexpr unsigned SEL = 0x06020400u;                                   // low bytes of the halves of a and b
    const unsigned gh = vmx_perm(b[0], a[0], SEL), ge1 = vmx_perm(b[1], a[1], SEL), ge2 = vmx_perm(b[2], a[2], SEL);
    const unsigned gf1 = vmx_perm(b[3], a[3], SEL), gf2 = vmx_perm(b[4], a[4], SEL);
    // source by the h tag: 7 -> 0, 6 (E1) -> 1, 1 (E2) -> 2, 3 (F1) -> 3, 0 (F2) -> 4
    const unsigned src = vmx_perm(0x00010000u, 0x03000204u, gh & 0x07070707u);
    unsigned op = vmx_bfi(0x01010101u, ge1, ge2);                           // "opened" bits: 0 E1, 1 E2 (tag 7, not 6 / 1)
    op = vmx_bfi(0x04040404u, gf1, op);                                     // 2 F1 (7, not 3)
    op = vmx_bfi(0x08080808u, (gf2 << 3) | (gf2 >> 29), op);                // 3 F2 (7, not 0; bit 0 of each byte rotated to bit 3)
    return src | (((op & 0x0f0f0f0fu) ^ 0x0f0f0f0fu) << 3);
}

// the step's stores: w01 = [0.X, 1.X, 0.Y, 1.Y], w23 = [2.X, 3.X, 2.Y, 3.Y]; the byte of a cell the band does not have (k >= NS) is 0
template <int NS>
__device__ __forceinline__ void vmx_ad_pack(const unsigned (&w)[NS][5], unsigned& w01, unsigned& w23) {
    w01 = vmx_ad_bytes(w[0], w[NS > 1 ? 1 : 0]);
    w23 = 0;
    if (NS > 2) w23 = vmx_ad_bytes(w[NS > 2 ? 2 : 0], w[NS > 3 ? 3 : 0]);
    if (NS == 3) w23 &= 0x00ff00ffu;
}

// v[k] by masks, not by a select of array elements (which the compiler turns into a dynamically indexed load and the arrays into memory)
template <int NS>
__device__ __forceinline__ unsigned vmx_ad_pick(const unsigned (&v)[NS], int k) {
    unsigned r = 0;
#pragma unroll
    for (int i = 0; i < NS; ++i) r |= v[i] & (unsigned)-(int)(k == i);
    return r;
}

// X = the problem in the low halves, Y = the one in the high halves of this lane's 16-lane row (tl = 0: idle). Every lane of the wave
// calls it; control flow is wave-uniform. scoreX / scoreY: H(tl, ql) of the band, the same in all lanes of the row.
//   LW = 64 (the second launch, k_gapfill_redo): the band lives in the whole wavefront — lane l = the lane id owns the diagonals
// [2 NS l, 2 NS l + 2 NS) of a band of 128 NS, X and Y are ONE problem each for the whole wave, the hand-offs are wave-wide moves and the chunk
// registers hold 64 codes. The traceback bytes go into the packed two-rows-per-lane layout of vmx_gapfill_fill16 (the space a refilled problem
// owns: vmx_tb_rows128, vmx_gapfill.h), cell (i, j) at (s (ql + 127) + (j - 1) + r) 128 + r with s = (i - 1) >> 7, r = (i - 1) & 127: inside a stripe the NS
// cells of a lane are NS adjacent bytes (k counts them downwards) and an anti-diagonal of the band is one run of 64 NS bytes. Only cells of
// the matrix are stored (one outside it would alias a real cell's address); what the band does not cover stays unwritten — the walk of a
// kept (proven) problem never leaves the band.
// The wave-wide band's store address, strength-reduced by hand (a measured choice): cell (i, j) of anti-diagonal a = i + j, row i = ik + 1, is at
// s * 128 (ql - 2) + 128 (a - 2) + ik in the 128-row layout (129 r + 128 (j - 1) with r = ik - 128 s) — sb * s is a 24-bit multiply, the stripe s < 8.
__host__ __device__ constexpr int vmx_adw_sb(int ql) { return (int)((unsigned)(128 * (ql - 2)) << 8) >> 8; }
__host__ __device__ constexpr int vmx_adw_ab(int a) { return 128 * (a - 2); }
__host__ __device__ constexpr unsigned vmx_adw_off(int sb, int ab, int ik) { return (unsigned)(((ik >> 7) & 7) * sb + (ab + ik)); }
constexpr bool vmx_adw_off_ok(int tl) {
    const int qls[5] = {1, 15, 16, 17, 33};
    for (int q = 0; q < 5; ++q)
        for (int i = 1; i <= tl; ++i)
            for (int j = 1; j <= qls[q]; ++j)
                if (vmx_adw_off(vmx_adw_sb(qls[q]), vmx_adw_ab(i + j), i - 1) != vmx_tb_rows128::cell_off(vmx_tb_rows128::W(qls[q]), i, j)) return false;
    return true;
}
static_assert(vmx_adw_off_ok(1) && vmx_adw_off_ok(127) && vmx_adw_off_ok(128) && vmx_adw_off_ok(129), "vmx_adw_off is cell_off of the 128-row layout");
static_assert(vmx_adw_off_ok(256), "vmx_adw_off is cell_off of the 128-row layout");
static_assert(vmx_adw_off_ok(257), "vmx_adw_off is cell_off of the 128-row layout");

// a value the compiler has to have in a register HERE: left alone it moves the packing of a step's bytes (vmx_ad_bytes) down to the block's store and keeps the
// 5 NS words per step it reads alive across the block's other steps instead of the two words it makes — spills in the NS = 4 loop
#ifdef VMX_EMU
__device__ __forceinline__ void vmx_ad_pin(unsigned&) {}
#else
__device__ __forceinline__ void vmx_ad_pin(unsigned& v) { asm volatile("" : "+v"(v)); }
#endif
// what a lane stores for a block of four steps (W = 2, W = 4): one 8- / 16-byte store through an aligned pointer
struct alignas(8) vmx_u32x2 { unsigned x, y; };
struct alignas(16) vmx_u32x4 { unsigned x, y, z, w; };

template <int NS, int LW = 16>
__device__ __forceinline__ void vmx_gapfill_fill_ad(const uint8_t* __restrict__ TX, const uint8_t* __restrict__ QX, int tlX, int qlX, int dloX, uint8_t* __restrict__ tbX,
                                                   const uint8_t* __restrict__ TY, const uint8_t* __restrict__ QY, int tlY, int qlY, int dloY, uint8_t* __restrict__ tbY,
                                                   int match, int mismatch, int o1, int e1, int o2, int e2, int lane, int& scoreX, int& scoreY) {
    const int l = LW == 16 ? lane & 15 : lane;
    vmx_ad_consts K;
    K.O1 = vmx_pk(8 * o1, 8 * o1); K.O2 = vmx_pk(8 * o2, 8 * o2); K.E1 = vmx_pk(8 * e1, 8 * e1); K.E2 = vmx_pk(8 * e2, 8 * e2);
    K.MATCH = vmx_pk(8 * match, 8 * match); K.PEN = vmx_pk(8 * (match - mismatch), 8 * (match - mismatch));
    const int bias = (int)vmx_ad_bias(mismatch, o1, e1, o2, e2);         // (the caller checked vmx_ad_scores_ok)
    const unsigned neg = 8u * (unsigned)(VMX_AD_NEGINF + bias);
    K.NH = (neg + 7u) * 0x00010001u; K.NE1 = (neg + VMX_AD_TE1) * 0x00010001u; K.NE2 = (neg + VMX_AD_TE2) * 0x00010001u;
    K.NF1 = (neg + VMX_AD_TF1) * 0x00010001u; K.NF2 = (neg + VMX_AD_TF2) * 0x00010001u;
    const int afX = (tlX > 0 && qlX > 0) ? tlX + qlX : 0, afY = (tlY > 0 && qlY > 0) ? tlY + qlY : 0;     // the last anti-diagonal: cell (tl, ql)
    const int total = vmx_uniform_i32(vmx_wave_max_i32(afX > afY ? afX : afY));
    // pair p = 1 ..: the odd step a = 2p - 1 (C sets), then the even step a = 2p (A sets). LW = 16 runs the pairs two at a time, a block of four anti-diagonals
    // whose bytes go out in one store: an odd count gets ONE JUNK PAIR at the end (rather than a flush after the loop: no second copy of the store, and a turn
    // without a branch in it). Its steps lie past every problem's last anti-diagonal, like the steps a shorter problem of the wave always ran: garbage that feeds
    // garbage (the steps stay <= VMX_DP16X4_MAX, a multiple of 4: inside the range the bias is sized for), bytes no walk reads, in space rounded up to whole blocks.
    static_assert(VMX_DP16X4_MAX % 4 == 0, "the junk pair of the 16-lane band must not take the step count past the small class's limit");
    const int npairs = LW == 16 ? (((total + 1) >> 1) + 1) & ~1 : (total + 1) >> 1;
    const int poX = (afX + 1) >> 1, peX = afX >> 1, poY = (afY + 1) >> 1, peY = afY >> 1;     // last pair whose odd / even step stores
    const int hX = dloX >> 1, hY = dloY >> 1;                   // dlo is even
    // set k of lane l in pair p: target row p - 1 - h - NS l - k on the odd step and one more on the even step, query column p + h + NS l + k on both
    auto tcf = [&](const uint8_t* T, int tl, int i) -> int { return ((i >= 1 && i <= tl) ? vmx_tcode(T[i - 1]) : 5) << VMX_AD_CSH; };
    auto qcf = [&](const uint8_t* Q, int ql, int j) -> int { return ((j >= 1 && j <= ql) ? (int)Q[j - 1] : 4) << VMX_AD_CSH; };
    unsigned tcode[NS], qcode[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        tcode[k] = vmx_pk(tcf(TX, tlX, -hX - NS * l - k), tcf(TY, tlY, -hY - NS * l - k));
        qcode[k] = vmx_pk(qcf(QX, qlX, hX + NS * l + k), qcf(QY, qlY, hY + NS * l + k));          // one column back: pair 1 starts with a shift
    }
    unsigned HA[NS], E1A[NS], E2A[NS], F1A[NS], F2A[NS], HC[NS], E1C[NS], E2C[NS], F1C[NS], F2C[NS];
    {
        // H(0,0) = 0 on diagonal 0 (x = -dlo: an A set), -infinity everywhere else
        const int l0X = (-dloX) / (2 * NS), k0X = ((-dloX) % (2 * NS)) >> 1, l0Y = (-dloY) / (2 * NS), k0Y = ((-dloY) % (2 * NS)) >> 1;
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const unsigned m = ((l == l0X && k == k0X) ? 0xffffu : 0u) | ((l == l0Y && k == k0Y) ? 0xffff0000u : 0u);
            HA[k] = vmx_bfi(m, (8u * (unsigned)bias + 7u) * 0x00010001u, K.NH);
            E1A[k] = K.NE1; E2A[k] = K.NE2; F1A[k] = K.NF1; F2A[k] = K.NF2;
            HC[k] = K.NH; E1C[k] = K.NE1; E2C[k] = K.NE2; F1C[k] = K.NF1; F2C[k] = K.NF2;
        }
    }
    // where H(tl, ql) lives: diagonal x = (ql - tl) - dlo
    const int xfX = (qlX - tlX) - dloX, xfY = (qlY - tlY) - dloY;
    const int lfX = xfX / (2 * NS), kfX = (xfX % (2 * NS)) >> 1, lfY = xfY / (2 * NS), kfY = (xfY % (2 * NS)) >> 1;
    int finX = 0, finY = 0;
    constexpr int W = VMX_AD_W(NS);                           // bytes of the lane's slot: as many as the lane has cells per step (round 6; 4 before, whatever NS)
    constexpr int PB = LW == 16 ? VMX_AD_AB / 2 : 1;          // step pairs per turn of the band loop: LW = 16 runs a block of the traceback layout per turn (below)
    static_assert(LW != 16 || PB == 2, "the 16-lane band stores blocks of four anti-diagonals");
    uint8_t* const pX = LW == 16 ? tbX + vmx_ad_tb_off(0, l, W) : tbX;       // the lane's run of anti-diagonals 0 .. 3; the block's part of the offset is added per store
    uint8_t* const pY = LW == 16 ? tbY + vmx_ad_tb_off(0, l, W) : tbY;
    // LW = 16: the words of the FOUR steps of a block (two pairs: the anti-diagonals s = 2p - 2 .. 2p + 1 of an odd p, one line block of the layout) stay in
    // registers and go out as one store of 4 W bytes per lane and problem: bw[t] = {w01, w23} of the block's step t. The problem's space starts on a 64-byte
    // line (vmx_tb_base_ok and the sizes' check, vmx_gapfill.h) and the lane's run in it is aligned to its length (vmx_ad_tb_ok).
    auto put_block = [&](uint8_t* at, const unsigned (&bw)[4][2], bool hi) {
        if constexpr (W == 1) {          // byte 0 (X) / 2 (Y) of every step's w01
            const unsigned t01 = vmx_perm(bw[1][0], bw[0][0], 0x06040200u), t23 = vmx_perm(bw[3][0], bw[2][0], 0x06040200u);      // [0.X, 0.Y, 1.X, 1.Y], [2.X, 2.Y, 3.X, 3.Y]
            *(uint32_t*)at = vmx_perm(t23, t01, hi ? 0x07050301u : 0x06040200u);
        } else if constexpr (W == 2) {   // the low (X) / high (Y) half of every step's w01
            const unsigned sel = hi ? 0x07060302u : 0x05040100u;
            vmx_u32x2 v; v.x = vmx_perm(bw[1][0], bw[0][0], sel); v.y = vmx_perm(bw[3][0], bw[2][0], sel);
            *(vmx_u32x2*)at = v;
        } else {                         // the low (X) / high (Y) halves of every step's w01 and w23
            const unsigned sel = hi ? 0x07060302u : 0x05040100u;
            vmx_u32x4 v; v.x = vmx_perm(bw[0][1], bw[0][0], sel); v.y = vmx_perm(bw[1][1], bw[1][0], sel); v.z = vmx_perm(bw[2][1], bw[2][0], sel); v.w = vmx_perm(bw[3][1], bw[3][0], sel);
            *(vmx_u32x4*)at = v;
        }
    };
    // LW = 64: the step's bytes at their cells' addresses in the packed layout. Cell k of the lane on anti-diagonal a is (i0 - k, a - i0 + k), i0 = i1 + 1
    // the lane's largest row: inside the matrix when lo <= i - 1 < hi with lo = max(0, a - 1 - ql), hi = min(tl, a - 1) (both wave-uniform); its offset: vmx_adw_off
    auto put_pk = [&](uint8_t* tb, int tl, int ql, int a, int i1, unsigned w01, unsigned w23, bool hi) {
        const int lo = a - 1 - ql > 0 ? a - 1 - ql : 0, n = (tl < a - 1 ? tl : a - 1) - lo;
        const int sb = vmx_adw_sb(ql), ab = vmx_adw_ab(a);
#pragma unroll
        for (int k = 0; k < NS; ++k) {
            const int ik = i1 - k;
            if ((unsigned)(ik - lo) < (unsigned)n && n > 0) {
                const unsigned w = k < 2 ? w01 : w23;
                tb[vmx_adw_off(sb, ab, ik)] = (uint8_t)(w >> (8 * (k & 1) + (hi ? 16 : 0)));
            }
        }
    };
    // chunk of block b (pairs 16 b + 1 .. 16 b + 16; LW = 64: 64 b + 1 .. 64 b + 64, and so on: 16 stands for LW below): lane m holds the target code lane 0 takes in the block's pair m (row 16 b + 1 + m - h),
    // lane 15 - m the query code lane 15 takes in it (column 16 b + m + h + 16 NS)
    auto load_chunks = [&](int b16, unsigned& tch, unsigned& qch) {
        tch = vmx_pk(tcf(TX, tlX, b16 + 1 + l - hX), tcf(TY, tlY, b16 + 1 + l - hY));
        qch = vmx_pk(qcf(QX, qlX, b16 + (LW - 1) - l + hX + LW * NS), qcf(QY, qlY, b16 + (LW - 1) - l + hY + LW * NS));
    };
    unsigned tch, qch, ntch, nqch;
    load_chunks(0, ntch, nqch);
    for (int p0 = 0; p0 < npairs; p0 += LW) {
        tch = ntch; qch = nqch;
        load_chunks(p0 + LW, ntch, nqch);                       // one block ahead
        int pend = npairs - p0; if (pend > LW) pend = LW;
        // LW = 16: PB = 2 pairs per turn, one block of the traceback layout (p0 is a multiple of 16, so a turn's first pair is odd and a block never straddles a
        // chunk refill; npairs is even, above).
        for (int pp0 = 0; pp0 < pend; pp0 += PB) {
          unsigned bw[2 * PB][2];
#pragma unroll
          for (int hf = 0; hf < PB; ++hf) {
            const int pp = pp0 + hf;
            const int p = p0 + pp + 1;
            // query codes move up one diagonal pair
            {
                const unsigned in = (unsigned)vmx_ad_shl1_in<LW>((int)qcode[0], (int)qch);
#pragma unroll
                for (int k = 0; k + 1 < NS; ++k) qcode[k] = qcode[k + 1];
                qcode[NS - 1] = in;
                qch = (unsigned)vmx_ad_ror1<LW>((int)qch);
            }
            // odd step a = 2p - 1: C_k takes the cell above from A_{k+1} (the last one from the next lane) and the cell to its left from A_k
            unsigned w[NS][5];
            {
                const unsigned nH = (unsigned)vmx_ad_shl1_in<LW>((int)HA[0], (int)K.NH), nE1 = (unsigned)vmx_ad_shl1_in<LW>((int)E1A[0], (int)K.NE1),
                               nE2 = (unsigned)vmx_ad_shl1_in<LW>((int)E2A[0], (int)K.NE2);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const unsigned uH = k + 1 < NS ? HA[k + 1 < NS ? k + 1 : 0] : nH, uE1 = k + 1 < NS ? E1A[k + 1 < NS ? k + 1 : 0] : nE1, uE2 = k + 1 < NS ? E2A[k + 1 < NS ? k + 1 : 0] : nE2;
                    vmx_ad_cell(K, uH, uE1, uE2, HA[k], F1A[k], F2A[k], tcode[k], qcode[k], HC[k], E1C[k], E2C[k], F1C[k], F2C[k], w[k]);
                }
            }
            {
                unsigned w01, w23;
                vmx_ad_pack<NS>(w, w01, w23);
                if constexpr (LW == 16) { vmx_ad_pin(w01); if constexpr (NS > 2) vmx_ad_pin(w23); bw[2 * hf][0] = w01; bw[2 * hf][1] = w23; }      // anti-diagonal a = 2p - 1 is step s = a - 1 = 2p - 2
                else {
                    if (p <= poX) put_pk(pX, tlX, qlX, 2 * p - 1, p - 2 - hX - NS * l, w01, w23, false);
                    if (p <= poY) put_pk(pY, tlY, qlY, 2 * p - 1, p - 2 - hY - NS * l, w01, w23, true);
                }
            }
            // target codes move down one diagonal pair
            {
                const unsigned in = (unsigned)vmx_ad_shr1_in<LW>((int)tcode[NS - 1], (int)tch);
#pragma unroll
                for (int k = NS - 1; k > 0; --k) tcode[k] = tcode[k - 1];
                tcode[0] = in;
                tch = (unsigned)vmx_ad_rol1<LW>((int)tch);
            }
            // even step a = 2p: A_k takes the cell above from C_k and the cell to its left from C_{k-1} (the first one from the previous lane)
            {
                const unsigned nH = (unsigned)vmx_ad_shr1_in<LW>((int)HC[NS - 1], (int)K.NH), nF1 = (unsigned)vmx_ad_shr1_in<LW>((int)F1C[NS - 1], (int)K.NF1),
                               nF2 = (unsigned)vmx_ad_shr1_in<LW>((int)F2C[NS - 1], (int)K.NF2);
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const unsigned lH = k > 0 ? HC[k > 0 ? k - 1 : 0] : nH, lF1 = k > 0 ? F1C[k > 0 ? k - 1 : 0] : nF1, lF2 = k > 0 ? F2C[k > 0 ? k - 1 : 0] : nF2;
                    vmx_ad_cell(K, HC[k], E1C[k], E2C[k], lH, lF1, lF2, tcode[k], qcode[k], HA[k], E1A[k], E2A[k], F1A[k], F2A[k], w[k]);
                }
            }
            {
                unsigned w01, w23;
                vmx_ad_pack<NS>(w, w01, w23);
                if constexpr (LW == 16) { vmx_ad_pin(w01); if constexpr (NS > 2) vmx_ad_pin(w23); bw[2 * hf + 1][0] = w01; bw[2 * hf + 1][1] = w23; }
                else {
                    if (p <= peX) put_pk(pX, tlX, qlX, 2 * p, p - 1 - hX - NS * l, w01, w23, false);
                    if (p <= peY) put_pk(pY, tlY, qlY, 2 * p, p - 1 - hY - NS * l, w01, w23, true);
                }
            }
            // the pair that holds the problem's last anti-diagonal: its cell (tl, ql) was written by this pair's odd or even step
            if (__any(p == poX || p == poY)) {
                const unsigned aX = vmx_ad_pick<NS>(HA, kfX), cX = vmx_ad_pick<NS>(HC, kfX), aY = vmx_ad_pick<NS>(HA, kfY), cY = vmx_ad_pick<NS>(HC, kfY);
                const unsigned vX = (afX & 1) ? cX : aX, vY = (afY & 1) ? cY : aY;
                if (p == poX && l == lfX) finX = (int)((vX & 0xffffu) >> 3) - bias;
                if (p == poY && l == lfY) finY = (int)(vY >> 19) - bias;
            }
          }
          // the block's store: for every problem that has the block's first anti-diagonal (a = 2p - 1 of the turn's first pair p)
          if constexpr (LW == 16) {
              const int p = p0 + pp0 + 1;
              const size_t so = vmx_ad_tb_off(2 * p - 2, 0, W);
              if (p <= poX) put_block(pX + so, bw, false);
              if (p <= poY) put_block(pY + so, bw, true);
          }
        }
    }
    scoreX = __shfl(finX, LW == 16 ? (lane & 48) | (lfX & 15) : lfX & 63);
    scoreY = __shfl(finY, LW == 16 ? (lane & 48) | (lfY & 15) : lfY & 63);
}

// Is the band's result the true optimum with the true traceback? Asked by both launches: the first one for its 16-lane bands (vmx_ad_geom: 32 ns
// diagonals), the second one for the wave-wide band (vmx_ad_geom_nd over VMX_ADW_DPN ns diagonals); the argument only needs g and that every cell of the
// band inside the matrix was computed from its three neighbours in the band, whichever layout the bytes went to.
// A path that leaves the band holds at least g inserted and g deleted bases: impossible when g > min(tl, ql); otherwise it cannot score more than match * (min(tl, ql) - g) minus two gaps of g bases
// (splitting a gap never makes it cheaper). If the band's score beats that bound, every optimal path lies inside the band, where all
// cells it touches and all comparisons the traceback reads (they involve prefix-optimal values of cells on optimal paths only) are exact.
__device__ __forceinline__ bool vmx_ad_proven(int score, int tl, int ql, int g, int match, int o1, int e1, int o2, int e2) {
    const int mn = tl < ql ? tl : ql;
    if (g < 1) return false;
    if (g > mn) return true;
    const long long U = (long long)match * mn - vmx_ad_margin(g, match, o1, e1, o2, e2);      // match * (mn - g) - 2 * gap(g)
    return (long long)score > U;
}
#endif
