// k_fasta_reads.hip — FASTA and FASTQ reads on the device by vm_fastx_read's whole rule (host side: reader_window_fasta in vmx_bam.hip, opened with
// VM_READER_FASTA; the rule: include/vacmapx.h and DESIGN.md 7c).
//
// One window of inflated text buf[0, len), a carried tail in front of it, always begins between two records (state 0). The line table ls[] comes
// from k_fq_nl_count / k_fq_nl_pos (k_fastx_in.hip), unchanged.
//   * States: 0 between records, 1 - 3 the FASTQ states, 4 inside a FASTA record. A line is blank, begins with '>' or is anything else, and maps
//     the state before it to the state behind it; the maps (5 states x 3 bits in 16 bits) compose associatively: in the wavefront with __shfl_up,
//     over a workgroup's 256 lines through LDS, over the workgroups in launches of their own (k_fr_line_maps, k_fr_tile_scan, k_fr_line_states).
//     A record starts at a non-blank line in state 0 and at a '>' line in state 4. No workgroup waits for another.
//   * Cut: a FASTA record is complete only when the next record's first line (or the file's end) is in the window; k_fr_result cuts the window
//     in front of its last record start unless the window ends in state 0 or is the file's last and ends in state 4.
//   * Keep ranges: per line the bytes [ka, ka + n) that go to the bases (state 1: the whole line; state 4, no '>': trimmed of blanks and tabs
//     at both ends) or to the qualities (state 3), k_fr_line_keep. One exclusive scan of each column is every line's destination offset, and the
//     value at a record's first line is the record's offset.
//   * Copy by text position (k_fr_copy): a wavefront takes VMX_FQ_CHUNK bytes of the window, finds each byte's line from the newline counts,
//     keeps what lies in that line's range, compacts the kept bytes in LDS at the destination's alignment and stores 16 bytes at a time. No lane
//     walks a line, no wavefront belongs to a line or a record: 60-byte lines and one line of megabases cost the same per byte.
//   * Names and comments: one wavefront per record on its header line (k_fr_hdr_sizes, k_fr_hdr_copy), as k_fq_sizes / k_fq_copy.
// Every result is a position-determined write or an integer minimum: the bytes do not depend on wave scheduling.
#include <string.h>
#include "vmx_bam.h"
#include "k_fastx_dev.h"

#define FR_WAVES 4                          // wavefronts (chunks) per workgroup of k_fr_copy
#define FR_LDS_VEC (VMX_FQ_CHUNK / 16 + 2)  // 16-byte vectors of a chunk's kept bytes behind up to 15 bytes of padding

// first f, then g (5 states, 3 bits each)
__device__ __forceinline__ uint32_t fr_compose(uint32_t f, uint32_t g) {
    uint32_t h = 0;
    for (int s = 0; s < 5; ++s) h |= (g >> (3 * (f >> (3 * s) & 7u)) & 7u) << (3 * s);
    return h;
}

// inclusive prefix composition over the wavefront
__device__ __forceinline__ uint32_t fr_wave_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d); if (lane >= d) v = fr_compose(t, v); }
    return v;
}

// ------------------------------------------------------------------------------------------------ line states

// map[k] of every line (one lane per line: a line that is not blank shows it in its first bytes) and the composition of each workgroup's 256
// lines. Reads buf inside the line only (fq_line: [ls[k], ls[k + 1] - 1), at most len).
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fr_line_maps(const uint8_t* buf, const int64_t* ls, int64_t n_lines, uint16_t* map, uint16_t* tile_tot) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    uint32_t m = VMX_FR_MAP_IDENT;
    if (k < n_lines) {
        int64_t a, b;
        fq_line(buf, ls, k, a, b);
        m = VMX_FR_MAP_BLANK;
        if (a < b && buf[a] == '>') m = VMX_FR_MAP_GT;
        else for (int64_t i = a; i < b; ++i) { const uint8_t c = buf[i]; if (c != ' ' && c != '\t' && c != '\r') { m = VMX_FR_MAP_OTHER; break; } }
        map[k] = (uint16_t)m;
    }
    const uint32_t v = fr_wave_scan(m, lane);
    if (lane == 63) s_w[t >> 6] = v;
    __syncthreads();
    if (t == 0) { uint32_t tot = s_w[0]; for (int w = 1; w < VMX_FQ_LTILE / 64; ++w) tot = fr_compose(tot, s_w[w]); tile_tot[blockIdx.x] = (uint16_t)tot; }
}

// exclusive prefix composition of tile[0 .. n_tiles) in place (one workgroup, as k_fq_tile_scan)
__global__ void __launch_bounds__(1024) k_fr_tile_scan(uint16_t* tile, int64_t n_tiles) {
    __shared__ uint32_t s_w[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t per = (n_tiles + 1023) / 1024, b = t * per, e = b + per < n_tiles ? b + per : n_tiles;
    uint32_t tot = VMX_FR_MAP_IDENT;
    for (int64_t i = b; i < e; ++i) tot = fr_compose(tot, tile[i]);
    const uint32_t v = fr_wave_scan(tot, lane);
    uint32_t ex = __shfl_up(v, 1);
    if (lane == 0) ex = VMX_FR_MAP_IDENT;
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    uint32_t run = VMX_FR_MAP_IDENT;
    for (int j = 0; j < w; ++j) run = fr_compose(run, s_w[j]);
    run = fr_compose(run, ex);
    for (int64_t i = b; i < e; ++i) { const uint32_t x = tile[i]; tile[i] = (uint16_t)run; run = fr_compose(run, x); }
}

// state[k] = the state before line k for k in [0, n_lines] (state[n_lines]: behind the window's last line; the window begins in state 0),
// start[k] = 1 where line k begins a record: not blank in state 0, or a '>' line in state 4; start[n_lines] = 0
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fr_line_states(const uint16_t* map, const uint16_t* tile_pre, int64_t n_lines, uint8_t* state, int64_t* start) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    const uint32_t m = k < n_lines ? map[k] : VMX_FR_MAP_IDENT;
    const uint32_t v = fr_wave_scan(m, lane);
    if (lane == 63) s_w[w] = v;
    uint32_t ex = __shfl_up(v, 1);
    if (lane == 0) ex = VMX_FR_MAP_IDENT;
    __syncthreads();
    uint32_t pre = tile_pre[blockIdx.x];
    for (int j = 0; j < w; ++j) pre = fr_compose(pre, s_w[j]);
    pre = fr_compose(pre, ex);
    const uint32_t st = pre & 7u;
    if (k < n_lines) { state[k] = (uint8_t)st; start[k] = (st == 0 && m != VMX_FR_MAP_BLANK) || (st == 4 && m == VMX_FR_MAP_GT); }
    else if (k == n_lines) { state[k] = (uint8_t)st; start[k] = 0; }
}

// ------------------------------------------------------------------------------------------------ the cut

// Only the last record begun can be incomplete. The window ends in state 0, or it is the file's last and ends in state 4: every record is
// complete and the cut is behind the last line. Otherwise the cut is in front of the last record start (states 1 - 4 imply one), and the header
// of that record, a whole line already, is judged now as record n_rec: byte 0 neither '@' nor '>' (a '>' start is never an error here).
// Reads buf[ls[k]], the first byte of a line that is not blank.
__global__ void k_fr_result(const uint8_t* buf, const int64_t* ls, const uint8_t* state, const int64_t* ridx, const int64_t* rline, int64_t n_lines, int64_t len,
                            int closing, vmx_fr_result* res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t n_st = ridx[n_lines];
    const int es = state[n_lines];
    res->end_state = es;
    if (n_st > 0 && !(es == 0 || (closing && es == 4))) {
        const int64_t k = rline[n_st - 1];
        res->n_rec = n_st - 1; res->end = ls[k]; res->cut_line = k;
        const uint8_t h = buf[ls[k]];
        if (h != '@' && h != '>') atomicMin((unsigned long long*)&res->err_key, (unsigned long long)(n_st - 1) << 8 | (unsigned long long)VMX_FQ_E_HEADER);
    }
    else { res->n_rec = n_st; res->end = ls[n_lines] < len ? ls[n_lines] : len; res->cut_line = n_lines; }
}

// ------------------------------------------------------------------------------------------------ keep ranges

// One lane per line k in [0, n_lines]: the bytes of the line that go to a blob are buf[ka[k], ka[k] + ks[k] + kq[k]); at most one of ks (bases) and
// kq (qualities) is not 0. Lines at and behind the cut, headers, '+' lines and skipped lines keep nothing; slot n_lines is the scans' total
// slot and the table entry of the bytes behind the window's last newline. The blanks and tabs at the two ends of a FASTA body line are walked
// by this one lane. Reads buf inside the line only.
__global__ void __launch_bounds__(256) k_fr_line_keep(const uint8_t* buf, const int64_t* ls, const uint16_t* map, const uint8_t* state, int64_t n_lines, int64_t cut_line,
                                                      int64_t* ka, int64_t* ks, int64_t* kq) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k > n_lines) return;
    int64_t a = 0, ns = 0, nq = 0;
    if (k < cut_line) {
        int64_t b;
        fq_line(buf, ls, k, a, b);
        const int st = state[k];
        if (st == 1) ns = b - a;
        else if (st == 3) nq = b - a;
        else if (st == 4 && map[k] != VMX_FR_MAP_GT) {
            while (a < b && (buf[a] == ' ' || buf[a] == '\t')) ++a;
            while (b > a && (buf[b - 1] == ' ' || buf[b - 1] == '\t')) --b;
            ns = b - a;
        }
    }
    ka[k] = a; ks[k] = ns; kq[k] = nq;
}

// ------------------------------------------------------------------------------------------------ bases and qualities, by text position

// Chunk ch = buf[ch * 4096, ...) (one wavefront). The line of its first byte is coff[ch], the newlines in front of the chunk (the exclusive scan of
// k_fq_nl_count); a lane's line is that plus the newlines of the lanes and steps in front of it. A lane's 16 bytes fall into pieces between its
// newlines; each piece reads its line's range (ka, ks, kq: indices at most the window's newline count <= n_lines, the tables' last slot) and
// keeps the bytes inside it. The kept bytes of the chunk are contiguous in either blob: they begin at so[line] + the part of that line's range
// in front of the chunk. They are compacted in LDS at the destination's residue modulo 16 (seqs and quals are allocation bases), bases
// upper-cased, and stored as whole 16-byte vectors to aligned addresses, the two ragged ends byte by byte.
// Reads buf: whole vectors that begin below len (up to 15 bytes behind len, in the window's slack). Writes seqs[so[L], ...) and quals[qo[L], ...)
// inside [0, so[n_lines]) and [0, qo[n_lines]): every kept byte is counted in ks / kq.
__global__ void __launch_bounds__(64 * FR_WAVES) k_fr_copy(const uint8_t* buf, int64_t len, int64_t n_chunks, const int64_t* coff, const int64_t* ka, const int64_t* ks,
                                                           const int64_t* kq, const int64_t* so, const int64_t* qo, uint8_t* seqs, uint8_t* quals) {
    __shared__ fq_v16 s_seq[FR_WAVES][FR_LDS_VEC];
    __shared__ fq_v16 s_qual[FR_WAVES][FR_LDS_VEC];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t ch = (int64_t)blockIdx.x * FR_WAVES + wv;
    const bool on = ch < n_chunks;
    uint8_t* sl = (uint8_t*)s_seq[wv];
    uint8_t* sq = (uint8_t*)s_qual[wv];
    int64_t ds = 0, dq = 0;
    int rs = 0, rq = 0, pad_s = 0, pad_q = 0;
    if (on) {
        const int64_t cs = ch * VMX_FQ_CHUNK;
        int64_t L = coff[ch];
        {
            const int64_t in = cs - ka[L], ns = ks[L], nq = kq[L];              // the part of the first line's range in front of the chunk
            ds = so[L] + (in < 0 ? 0 : in < ns ? in : ns);
            dq = qo[L] + (in < 0 ? 0 : in < nq ? in : nq);
        }
        pad_s = (int)(ds & 15); pad_q = (int)(dq & 15);
        for (int s = 0; s < 4; ++s) {
            const int64_t off = cs + s * 1024 + lane * 16;
            fq_v16 v = fq_v16{0, 0, 0, 0};
            uint32_t nl = 0;
            if (off < len) {
                v = *(const fq_v16*)(buf + off);
                nl = fq_mask16(v, 0x0a0a0a0au);
                if (len - off < 16) nl &= (1u << (int)(len - off)) - 1u;
            }
            const int c = __popc(nl);
            int inc = c;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
            uint32_t keep_s = 0, keep_q = 0;
            if (off < len) {
                int64_t Ll = L + inc - c;
                uint32_t m = nl;
                for (int seg = 0; seg < 16; ++Ll) {
                    const int e = m ? __ffs(m) - 1 : 16;
                    if (e > seg) {
                        const int64_t ns = ks[Ll], nq = kq[Ll], n = ns | nq;
                        if (n > 0) {
                            const int64_t i0 = ka[Ll] - off;
                            const int64_t lo = i0 > seg ? i0 : seg, hi = i0 + n < e ? i0 + n : e;
                            if (hi > lo) {
                                const uint32_t bits = ((1u << (int)hi) - 1u) & ~((1u << (int)lo) - 1u);
                                if (ns) keep_s |= bits; else keep_q |= bits;
                            }
                        }
                    }
                    seg = e + 1; m &= m - 1;
                }
            }
            const int cnt = __popc(keep_s) | __popc(keep_q) << 16;             // (at most 1024 each per step)
            int cinc = cnt;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(cinc, d); if (lane >= d) cinc += t; }
            const int ex = cinc - cnt;
            int ps = pad_s + rs + (ex & 0xffff), pq = pad_q + rq + (ex >> 16);
            if (keep_s | keep_q) {
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if (keep_s >> k & 1u) sl[ps++] = fq_upper1((uint8_t)fq_byte16(v, k));
                    else if (keep_q >> k & 1u) sq[pq++] = (uint8_t)fq_byte16(v, k);
                }
            }
            const int tot = __shfl(cinc, 63);
            rs += tot & 0xffff; rq += tot >> 16;
            L += __shfl(inc, 63);
        }
    }
    __syncthreads();
    if (!on) return;
    for (int blob = 0; blob < 2; ++blob) {
        const int n = blob ? rq : rs, pad = blob ? pad_q : pad_s;
        if (n == 0) continue;
        uint8_t* d = (blob ? quals + dq : seqs + ds) - pad;                     // 16-byte aligned
        const uint8_t* sb = blob ? sq : sl;
        const fq_v16* sv = blob ? s_qual[wv] : s_seq[wv];
        const int nv = (pad + n + 15) >> 4;
        for (int v = lane; v < nv; v += 64) {
            const int lo = v << 4, hi = lo + 16;
            if (lo >= pad && hi <= pad + n) *(fq_v16*)(d + lo) = sv[v];
            else {
                const int a = lo > pad ? lo : pad, e = hi < pad + n ? hi : pad + n;
                for (int j = a; j < e; ++j) d[j] = sb[j];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ names and comments

// One wavefront per record r in [0, n_rec]: bytes of name and comment of its header line (the name ends at the first blank or tab, found 64
// bytes per ballot), and the record's offsets in the bases and the qualities: the line scans' values at its first line. Slot n_rec: sizes 0, the
// offsets at the cut. The first header whose byte 0 is neither '@' nor '>' goes to err_key. Reads buf inside the header line only.
__global__ void __launch_bounds__(256) k_fr_hdr_sizes(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, int64_t cut_line, const int64_t* so,
                                                      const int64_t* qo, int64_t* nsz, int64_t* csz, int64_t* soff, int64_t* qoff, unsigned long long* err_key) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r > n_rec) return;
    if (r == n_rec) { if (lane == 0) { nsz[r] = 0; csz[r] = 0; soff[r] = so[cut_line]; qoff[r] = qo[cut_line]; } return; }
    const int64_t k = rline[r];
    int64_t a, b;
    fq_line(buf, ls, k, a, b);                                            // (a header is not blank: a < b)
    int64_t sp = b;
    for (int64_t base = a + 1; base < b; base += 64) {
        const int64_t i = base + lane;
        const uint8_t c = i < b ? buf[i] : 0;
        const unsigned long long hit = __ballot(c == ' ' || c == '\t');
        if (hit) { sp = base + __ffsll(hit) - 1; break; }
    }
    if (lane != 0) return;
    const uint8_t h = buf[a];
    if (h != '@' && h != '>') atomicMin(err_key, (unsigned long long)r << 8 | (unsigned long long)VMX_FQ_E_HEADER);
    nsz[r] = sp - (a + 1);
    csz[r] = sp < b ? b - sp - 1 : 0;
    soff[r] = so[k]; qoff[r] = qo[k];
}

// One wavefront per record: name and comment to their blobs at the offsets the scans of k_fr_hdr_sizes' columns gave. Writes [off[r], off[r + 1]).
__global__ void __launch_bounds__(256) k_fr_hdr_copy(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, const int64_t* noff, const int64_t* coff,
                                                     uint8_t* names, uint8_t* comments) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    const int64_t a = ls[rline[r]], nn = noff[r + 1] - noff[r], nc = coff[r + 1] - coff[r];
    fq_copy<false>(buf + a + 1, names + noff[r], nn, lane);
    fq_copy<false>(buf + a + 1 + nn + 1, comments + coff[r], nc, lane);    // (behind the separator; nothing is read when there is no comment)
}
