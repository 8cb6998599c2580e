// k_fasta_in.hip — the reference FASTA on the device (host side: vmx_ref_fasta_device in vmx_bam.hip; the rule: include/vacmapx.h and DESIGN.md 7c,
// which is vm_index_build_fasta's).
//
// One window of text buf[0, len) with a carried tail in front of it. Lines of a reference are 50-80 bytes, so the work is per chunk of text, as
// in the newline kernels of k_fastx_in.hip: VMX_FQ_CHUNK = 4096 bytes per wavefront, 4 steps of 64 lanes x 16 bytes, every byte class one bit of
// a 16-bit mask per lane.
//   * A byte is KEPT when it is no '\n', is not in a trailing '\r' run, its line does not begin with '>' and a header has been seen.
//   * "In a header line" (H) and "a header has been seen" (S) are the state, H | S << 1. A '>' behind a newline sets both, a newline clears H.
//     In a lane the header lines are a carry chain: (~nl + header starts) flips exactly the bits from every '>' to its newline. Over the lanes
//     of a step the state in front of a lane is read off three ballots. A chunk's effect is a map of the 4 states packed 2 bits each, the
//     format of the FASTQ line maps: the maps compose with fq_compose, in the wavefront with __shfl_up, over a workgroup's 256 chunks through
//     LDS, over the workgroups in launches of their own (k_fa_tile_tot, k_fq_tile_scan, k_fa_states). No workgroup waits for another.
//   * Trailing '\r': the same carry chain on the reversed masks, started by every newline; a run that leaves the lane asks the lanes above
//     (two ballots), a run that leaves the step reads ahead.
//   * The window is cut in front of an incomplete header line (the last header start of the window: an integer maximum) and in front of a
//     '\r' run at its very end (k_fa_result); sequence lines are never carried.
//   * k_fa_count counts kept bytes and header starts per chunk (one packed int64, one scan). k_fa_write compacts a chunk's kept bytes in LDS
//     at the destination's alignment and stores upper-cased letters and codes 16 bytes at a time; it lists the headers (text position, bases
//     in front) and sums the letters that are none of ACGTN. k_fa_hdr_size / k_fa_hdr_copy gather the header lines for the host.
// Every result is a position-determined write, an integer maximum or an integer sum: the bytes do not depend on wave scheduling.
#include <string.h>
#include "vmx_bam.h"
#include "k_fastx_dev.h"

#define FA_WAVES 4                          // wavefronts (chunks) per workgroup of the chunk kernels
#define FA_LDS_VEC (VMX_FQ_CHUNK / 16 + 2)  // 16-byte vectors of a chunk's kept bytes behind up to 15 bytes of padding

struct fa_bits { uint32_t nl, cr, gt, valid; fq_v16 v; };

// the 16 bytes at off (a multiple of 16; buf is a device allocation's base) as bit masks; bytes at and beyond len are masked out, but the vector
// that holds byte len - 1 is loaded whole: up to 15 bytes behind len, inside the 64 bytes of slack behind every window
__device__ __forceinline__ fa_bits fa_load(const uint8_t* buf, int64_t off, int64_t len) {
    fa_bits b;
    b.nl = b.cr = b.gt = b.valid = 0; b.v = fq_v16{0, 0, 0, 0};
    if (off >= len) return b;
    b.v = *(const fq_v16*)(buf + off);
    const int64_t left = len - off;
    b.valid = left < 16 ? (1u << (int)left) - 1u : 0xffffu;
    b.nl = fq_mask16(b.v, 0x0a0a0a0au) & b.valid;
    b.cr = fq_mask16(b.v, 0x0d0d0d0du) & b.valid;
    b.gt = fq_mask16(b.v, 0x3e3e3e3eu) & b.valid;
    return b;
}

__device__ __forceinline__ uint32_t fa_rev16(uint32_t x) {
    x = (x >> 1 & 0x5555u) | (x & 0x5555u) << 1;
    x = (x >> 2 & 0x3333u) | (x & 0x3333u) << 2;
    x = (x >> 4 & 0x0f0fu) | (x & 0x0f0fu) << 4;
    return (x >> 8 & 0xffu) | (x & 0xffu) << 8;
}

// the header events of one step: hs = header starts of this lane ('>' behind a newline; prevnl: the byte in front of the step is one), b1 / b0 =
// lanes whose bytes leave H set / cleared whatever it was, bh = lanes with a header start. prevnl becomes the next step's.
struct fa_events { uint32_t hs; unsigned long long b1, b0, bh; };
__device__ __forceinline__ fa_events fa_step_events(const fa_bits& b, int lane, int& prevnl) {
    fa_events e;
    uint32_t up = __shfl_up(b.nl >> 15, 1);
    if (lane == 0) up = (uint32_t)prevnl;
    e.hs = b.gt & ((b.nl << 1 | up) & 0xffffu);
    const uint32_t a = ~b.nl & 0xffffu;
    const int set1 = (int)((a + e.hs) >> 16 & 1u);
    e.b1 = __ballot(set1);
    e.b0 = __ballot(!set1 && b.nl != 0);
    e.bh = __ballot(e.hs != 0);
    prevnl = (int)(__ballot((int)(b.nl >> 15 & 1u)) >> 63);
    return e;
}

// One step of a chunk: the kept bytes of this lane's 16 (bit mask) and its header starts. H, S: the state in front of the step (uniform), updated.
// end: the window's cut; the end of the text stands for a newline behind a '\r' run (it is one only in the file's last window, and the cut
// leaves no such run in front of any other end).
__device__ __forceinline__ uint32_t fa_step_keep(const uint8_t* buf, int64_t step_off, int64_t end, int lane, const fa_bits& b, int& H, int& S, int& prevnl, uint32_t& hs_out) {
    const fa_events e = fa_step_events(b, lane, prevnl);
    hs_out = e.hs;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned long long m1 = e.b1 & lt, m0 = e.b0 & lt;
    const uint32_t hin = (m1 | m0) ? (uint32_t)(m1 > m0) : (uint32_t)H;     // (disjoint sets: the larger one holds the highest lane)
    const int sin = S | ((e.bh & lt) != 0);
    const uint32_t a = ~b.nl & 0xffffu;
    const uint32_t hm = ((a + (e.hs | hin)) ^ a) & 0xffffu;                 // from every header start (or bit 0, inside a header line) to its newline
    const uint32_t sm = sin ? 0xffffu : e.hs ? ~((e.hs & (0u - e.hs)) - 1u) & 0xffffu : 0u;
    // trailing '\r'
    const int64_t off = step_off + lane * 16;
    uint32_t nlx = b.nl;
    if (off >= end) nlx = 1u; else if (end - off < 16) nlx |= 1u << (int)(end - off);
    const uint32_t noncr = ~b.cr & 0xffffu;
    const unsigned long long ba = __ballot(noncr == 0);
    const unsigned long long bt = __ballot(noncr != 0 && ((noncr & (0u - noncr)) & nlx) != 0);
    const unsigned long long above = ~ba & ~((2ull << lane) - 1ull);
    const int need = above == 0 && (b.cr & 0x8000u);
    uint32_t tin = above ? (uint32_t)(bt >> (__ffsll(above) - 1) & 1ull) : 0u;
    if (__any(need)) {                                                      // a run that leaves the step: read ahead (uniform; one byte unless the text is '\r' upon '\r')
        int64_t i = step_off + 1024;
        while (i < end && buf[i] == '\r') ++i;
        if (need) tin = i >= end || buf[i] == '\n';
    }
    const uint32_t crr = fa_rev16(b.cr);
    const uint32_t add = ((fa_rev16(nlx & 0xffffu) << 1) | tin) & 0xffffu;
    const uint32_t tr = fa_rev16(((crr + add) ^ crr) & crr & 0xffffu);
    const unsigned long long all = e.b1 | e.b0;
    if (all) H = e.b1 > e.b0;
    S |= e.bh != 0;
    return b.valid & ~b.nl & ~tr & ~hm & sm;
}

__device__ __forceinline__ int fa_prevnl(const uint8_t* buf, int64_t off, int ls0) { return off == 0 ? ls0 : buf[off - 1] == '\n'; }

// ------------------------------------------------------------------------------------------------ chunk maps and states

// map[ch] = the effect of chunk ch on the state, res->last_hs = 1 + the window's last header start (0: none; res is cleared before). len > 0.
__global__ void __launch_bounds__(64 * FA_WAVES) k_fa_maps(const uint8_t* buf, int64_t len, int64_t n_chunks, int ls0, uint8_t* map, vmx_fa_result* res) {
    const int64_t ch = (int64_t)blockIdx.x * FA_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (ch >= n_chunks) return;
    int prevnl = fa_prevnl(buf, ch * VMX_FQ_CHUNK, ls0);
    int hmode = 0, sset = 0;                                                // hmode: 0 H stays, 1 cleared, 2 set
    int64_t last = -1;
    for (int s = 0; s < 4; ++s) {
        const int64_t off = ch * VMX_FQ_CHUNK + s * 1024 + lane * 16;
        const fa_bits b = fa_load(buf, off, len);
        const fa_events e = fa_step_events(b, lane, prevnl);
        if (e.b1 | e.b0) hmode = e.b1 > e.b0 ? 2 : 1;
        if (e.bh) {
            sset = 1;
            const int top = 63 - __clzll((long long)e.bh);
            const uint32_t hs = __shfl(e.hs, top);
            last = ch * VMX_FQ_CHUNK + s * 1024 + top * 16 + (31 - __clz((int)hs));
        }
    }
    if (lane != 0) return;
    uint32_t m = 0;
    for (int st = 0; st < 4; ++st) {
        const uint32_t h = hmode == 0 ? (uint32_t)(st & 1) : (uint32_t)(hmode - 1);
        m |= (h | ((uint32_t)(st >> 1) | (uint32_t)sset) << 1) << (2 * st);
    }
    map[ch] = (uint8_t)m;
    if (last >= 0) atomicMax((unsigned long long*)&res->last_hs, (unsigned long long)last + 1ull);
}

// the composition of each workgroup's 256 chunk maps (one lane per chunk)
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fa_tile_tot(const uint8_t* map, int64_t n_chunks, uint8_t* tile_tot) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    const uint32_t v = fq_wave_scan(k < n_chunks ? map[k] : VMX_FQ_MAP_IDENT, lane);
    if (lane == 63) s_w[t >> 6] = v;
    __syncthreads();
    if (t == 0) { uint32_t tot = s_w[0]; for (int w = 1; w < VMX_FQ_LTILE / 64; ++w) tot = fq_compose(tot, s_w[w]); tile_tot[blockIdx.x] = (uint8_t)tot; }
}

// state[ch] = the state in front of chunk ch for ch in [0, n_chunks] (state[n_chunks]: behind the window), from the state s_in in front of the
// window and tile_pre, the exclusive prefix composition of the tiles (k_fq_tile_scan)
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fa_states(const uint8_t* map, const uint8_t* tile_pre, int64_t n_chunks, int s_in, uint8_t* state) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    const uint32_t v = fq_wave_scan(k < n_chunks ? map[k] : VMX_FQ_MAP_IDENT, lane);
    if (lane == 63) s_w[w] = v;
    uint32_t ex = __shfl_up(v, 1);
    if (lane == 0) ex = VMX_FQ_MAP_IDENT;
    __syncthreads();
    uint32_t pre = tile_pre[blockIdx.x];
    for (int j = 0; j < w; ++j) pre = fq_compose(pre, s_w[j]);
    pre = fq_compose(pre, ex);
    if (k <= n_chunks) state[k] = (uint8_t)(pre >> (2 * s_in) & 3u);
}

// where the window is cut: in front of its last header start when the window ends inside that header line, else in front of the '\r' run at its
// very end; the file's last window (closing) is taken whole. end_ls: the byte in front of the cut is a newline (or nothing is in front of it).
__global__ void k_fa_result(const uint8_t* buf, int64_t len, int64_t n_chunks, const uint8_t* state, int ls0, int closing, vmx_fa_result* res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t end = len;
    if (!closing) {
        if (state[n_chunks] & 1) end = (int64_t)res->last_hs - 1;
        else while (end > 0 && buf[end - 1] == '\r') --end;
    }
    res->end = end;
    res->end_ls = end > 0 ? buf[end - 1] == '\n' : ls0;
}

// ------------------------------------------------------------------------------------------------ count and write

// cnt[ch] = kept bytes | header starts << 32 of chunk ch below end, cnt[n_chunks] = 0 (the scan's total slot)
__global__ void __launch_bounds__(64 * FA_WAVES) k_fa_count(const uint8_t* buf, int64_t end, int64_t n_chunks, const uint8_t* state, int ls0, int64_t* cnt) {
    const int64_t ch = (int64_t)blockIdx.x * FA_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (ch >= n_chunks) return;
    int H = state[ch] & 1, S = state[ch] >> 1 & 1;
    int prevnl = fa_prevnl(buf, ch * VMX_FQ_CHUNK, ls0);
    int c = 0, h = 0;
    for (int s = 0; s < 4; ++s) {
        const int64_t so = ch * VMX_FQ_CHUNK + s * 1024;
        const fa_bits b = fa_load(buf, so + lane * 16, end);
        uint32_t hs;
        c += __popc(fa_step_keep(buf, so, end, lane, b, H, S, prevnl, hs));
        h += __popc(hs);
    }
    for (int d = 32; d; d >>= 1) { c += __shfl_down(c, d); h += __shfl_down(h, d); }
    if (lane == 0) cnt[ch] = (int64_t)c | (int64_t)h << 32;
    if (ch == 0 && lane == 0) cnt[n_chunks] = 0;
}

// The kept bytes of chunk ch go to letters[lpad + i] (upper-cased) and codes[base0 + i] for i in [lo32(coff[ch]), lo32(coff[ch + 1])), where
// lpad = base0 & 15: both destinations have the same residue modulo 16 (letters and codes are allocation bases). A wavefront compacts its
// chunk in LDS at that residue, then stores whole 16-byte vectors to aligned addresses and the two ragged ends byte by byte. Header h =
// hi32(coff[ch]) + its rank in the chunk: hpos[h] = its '>' in the text, hbase[h] = base0 + kept bytes in front of it. *other += kept letters
// that are none of ACGTN in either case.
__global__ void __launch_bounds__(64 * FA_WAVES) k_fa_write(const uint8_t* buf, int64_t end, int64_t n_chunks, const uint8_t* state, int ls0, const int64_t* coff, int64_t base0,
                                                            uint8_t* letters, uint8_t* codes, int64_t* hpos, int64_t* hbase, unsigned long long* other) {
    __shared__ fq_v16 s_let[FA_WAVES][FA_LDS_VEC];
    __shared__ fq_v16 s_cod[FA_WAVES][FA_LDS_VEC];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ch = (int64_t)blockIdx.x * FA_WAVES + wv;
    const bool on = ch < n_chunks;
    uint8_t* sl = (uint8_t*)s_let[wv];
    uint8_t* sc = (uint8_t*)s_cod[wv];
    int64_t w_off = 0, hidx = 0;
    int n = 0, pad = 0;
    if (on) {
        const int64_t c0 = coff[ch], c1 = coff[ch + 1];
        w_off = c0 & 0xffffffffll; hidx = c0 >> 32;
        n = (int)((c1 & 0xffffffffll) - w_off);
        pad = (int)((base0 + w_off) & 15);
        int H = state[ch] & 1, S = state[ch] >> 1 & 1;
        int prevnl = fa_prevnl(buf, ch * VMX_FQ_CHUNK, ls0);
        int r = 0, hr = 0, oth = 0;
        for (int s = 0; s < 4; ++s) {
            const int64_t so = ch * VMX_FQ_CHUNK + s * 1024;
            const fa_bits b = fa_load(buf, so + lane * 16, end);
            uint32_t hs;
            const uint32_t keep = fa_step_keep(buf, so, end, lane, b, H, S, prevnl, hs);
            const int c = __popc(keep);
            int inc = c;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
            const int ex = r + inc - c;
            int p = pad + ex;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (keep >> k & 1u) {
                    const uint8_t x = (uint8_t)fq_byte16(b.v, k);
                    const uint8_t u = x & 0xDF;
                    oth += !(u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'N');
                    sl[p] = fq_upper1(x); sc[p] = vmx_code(x); ++p;
                }
            if (__any(hs != 0)) {
                const int hc = __popc(hs);
                int hinc = hc;
                for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(hinc, d); if (lane >= d) hinc += t; }
                int64_t h = hidx + hr + hinc - hc;
                for (uint32_t m = hs; m; m &= m - 1) {
                    const int bit = __ffs((int)m) - 1;
                    hpos[h] = so + lane * 16 + bit;
                    hbase[h] = base0 + w_off + ex + __popc(keep & ((1u << bit) - 1u));
                    ++h;
                }
                hr += __shfl(hinc, 63);
            }
            r += __shfl(inc, 63);
        }
        for (int d = 32; d; d >>= 1) oth += __shfl_down(oth, d);
        if (lane == 0 && oth) atomicAdd(other, (unsigned long long)oth);
    }
    __syncthreads();
    if (!on || n == 0) return;
    uint8_t* dl = letters + (base0 & 15) + w_off - pad;                     // 16-byte aligned, as dc is
    uint8_t* dc = codes + base0 + w_off - pad;
    const int nv = (pad + n + 15) >> 4;
    for (int v = lane; v < nv; v += 64) {
        const int lo = v << 4, hi = lo + 16;
        if (lo >= pad && hi <= pad + n) {
            *(fq_v16*)(dl + lo) = s_let[wv][v];
            *(fq_v16*)(dc + lo) = s_cod[wv][v];
        } else {
            const int a = lo > pad ? lo : pad, e = hi < pad + n ? hi : pad + n;
            for (int j = a; j < e; ++j) { dl[j] = sl[j]; dc[j] = sc[j]; }
        }
    }
}

// ------------------------------------------------------------------------------------------------ header lines

// One wavefront per header: hsz[h] = bytes behind its '>' up to its newline (or the cut), found 64 bytes per ballot; hsz[n] = 0
__global__ void __launch_bounds__(256) k_fa_hdr_size(const uint8_t* buf, int64_t end, const int64_t* hpos, int64_t n, int64_t* hsz) {
    const int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (h > n) return;
    if (h == n) { if (lane == 0) hsz[h] = 0; return; }
    const int64_t a = hpos[h] + 1;
    int64_t e = end;
    for (int64_t base = a; base < end; base += 64) {
        const int64_t i = base + lane;
        const unsigned long long hit = __ballot(i < end && buf[i] == '\n');
        if (hit) { e = base + __ffsll(hit) - 1; break; }
    }
    if (lane == 0) hsz[h] = e - a;
}

// the header lines side by side: blob[hoff[h], hoff[h + 1]) = the bytes behind header h's '>'
__global__ void __launch_bounds__(256) k_fa_hdr_copy(const uint8_t* buf, const int64_t* hpos, const int64_t* hoff, int64_t n, uint8_t* blob) {
    const int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (h >= n) return;
    fq_copy<false>(buf + hpos[h] + 1, blob + hoff[h], hoff[h + 1] - hoff[h], lane);
}
