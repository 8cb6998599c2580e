// k_fastx_in.hip — FASTQ input on the device (host side: vm_fastq_reader in vmx_bam.hip; the rule: include/vacmapx.h and DESIGN.md 7c, which is vm_fastx_read's).
//
// One window of inflated text buf[0, len), a carried tail in front of it, always begins between two records (parser state 0).
//   * Newlines: every wavefront counts the '\n' of 4096 bytes with 16-byte loads (k_fq_nl_count), the counts are scanned, k_fq_nl_pos
//     writes the line starts ls[0 .. n_lines]: line k is buf[ls[k], ls[k + 1] - 1), less one trailing '\r'. The bytes behind the last
//     newline are a line only in the file's last window (`closing`: ls[n_lines] = len + 1, as if a newline stood at len).
//   * States: a line maps the state before it to the state behind it: [1,2,3,0], or [0,2,3,0] when it is blank. The maps pack into a
//     byte and compose associatively, so the state before every line is a prefix composition: in the wavefront with __shfl_up, over a
//     workgroup's 256 lines through LDS, over the workgroups in launches of their own (k_fq_line_maps reduces, k_fq_tile_scan scans
//     the totals in one workgroup, k_fq_line_states applies). No workgroup ever waits for another.
//   * Records: a non-blank line in state 0 starts a record, and its four lines are that one and the next three (states 1, 2 and 3 take
//     any line). The start flags are scanned, k_fq_records lists the first line of every record, k_fq_result cuts the window behind its
//     last complete record.
//   * Fields: one wavefront per record sizes name, comment, bases and qualities (k_fq_sizes; the name ends at the first blank or tab,
//     found 64 bytes per ballot), four scans give the blob offsets, k_fq_copy moves the fields with 16-byte stores.
// Every result is a position-determined write or an integer minimum: the bytes do not depend on wave scheduling.
#include <string.h>
#include "vmx_bam.h"
#include "k_fastx_dev.h"

// bit i: byte off + i is a newline, for the 16 bytes at off (a multiple of 16; buf is a device allocation's base). Bytes at and beyond len
// are masked out, but the vector that holds byte len - 1 is loaded whole: up to 15 bytes behind len, inside the 64 bytes of slack the reader
// keeps behind every window. These are the only loads of this file that pass len.
__device__ __forceinline__ uint32_t fq_nl_bits(const uint8_t* buf, int64_t off, int64_t len) {
    if (off >= len) return 0;
    const fq_v16 v = *(const fq_v16*)(buf + off);
    const uint32_t nl = 0x0a0a0a0au;
    uint32_t m = fq_nibble(fq_eq_bytes(v.x, nl)) | fq_nibble(fq_eq_bytes(v.y, nl)) << 4 | fq_nibble(fq_eq_bytes(v.z, nl)) << 8 | fq_nibble(fq_eq_bytes(v.w, nl)) << 12;
    const int64_t left = len - off;
    if (left < 16) m &= (1u << (int)left) - 1u;
    return m;
}

// ------------------------------------------------------------------------------------------------ newlines

// cnt[ch] = newlines of buf[ch * 4096, ...) (one wavefront each), cnt[n_chunks] = 0 (the scan's total slot); len > 0.
// Reads: fq_nl_bits (below len + 15) and buf[len - 1].
__global__ void __launch_bounds__(256) k_fq_nl_count(const uint8_t* buf, int64_t len, int64_t n_chunks, int64_t* cnt, vmx_fq_result* res) {
    const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (ch >= n_chunks) return;
    int c = 0;
    for (int s = 0; s < 4; ++s) c += __popc(fq_nl_bits(buf, ch * VMX_FQ_CHUNK + s * 1024 + lane * 16, len));
    for (int d = 32; d; d >>= 1) c += __shfl_down(c, d);
    if (lane == 0) cnt[ch] = c;
    if (ch == 0 && lane == 0) { cnt[n_chunks] = 0; res->tail_open = buf[len - 1] != '\n'; }
}

// ls[j + 1] = position behind the j-th newline, ls[0] = 0, and ls[n_lines] = len + 1 when the window is closed by the end of the file.
// coff: the exclusive scan of cnt. Writes ls[1 .. newlines] (newlines <= n_lines: the count of the same bytes) and the two ends.
__global__ void __launch_bounds__(256) k_fq_nl_pos(const uint8_t* buf, int64_t len, int64_t n_chunks, const int64_t* coff, int64_t n_lines, int closing, int64_t* ls) {
    const int64_t ch = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (ch >= n_chunks) return;
    int64_t k = coff[ch];
    for (int s = 0; s < 4; ++s) {
        const int64_t off = ch * VMX_FQ_CHUNK + s * 1024 + lane * 16;
        uint32_t m = fq_nl_bits(buf, off, len);
        const int c = __popc(m);
        int inc = c;
        for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
        int64_t at = k + inc - c;
        while (m) { const int b = __ffs(m) - 1; m &= m - 1; ls[++at] = off + b + 1; }
        k += __shfl(inc, 63);
    }
    if (ch == 0 && lane == 0) { ls[0] = 0; if (closing) ls[n_lines] = len + 1; }
}

// ------------------------------------------------------------------------------------------------ line states

// map[k] of every line (one lane per line: a line that is not blank shows it in its first bytes) and the composition of each workgroup's
// 256 lines. Reads buf inside the line only.
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fq_line_maps(const uint8_t* buf, const int64_t* ls, int64_t n_lines, uint8_t* map, uint8_t* tile_tot) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    uint32_t m = VMX_FQ_MAP_IDENT;
    if (k < n_lines) {
        int64_t a, b;
        fq_line(buf, ls, k, a, b);
        m = VMX_FQ_MAP_BLANK;
        for (int64_t i = a; i < b; ++i) { const uint8_t c = buf[i]; if (c != ' ' && c != '\t' && c != '\r') { m = VMX_FQ_MAP_LINE; break; } }
        map[k] = (uint8_t)m;
    }
    const uint32_t v = fq_wave_scan(m, lane);
    if (lane == 63) s_w[t >> 6] = v;
    __syncthreads();
    if (t == 0) { uint32_t tot = s_w[0]; for (int w = 1; w < VMX_FQ_LTILE / 64; ++w) tot = fq_compose(tot, s_w[w]); tile_tot[blockIdx.x] = (uint8_t)tot; }
}

// exclusive prefix composition of tile[0 .. n_tiles) in place (one workgroup, as k_bam_scan)
__global__ void __launch_bounds__(1024) k_fq_tile_scan(uint8_t* tile, int64_t n_tiles) {
    __shared__ uint32_t s_w[16];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t per = (n_tiles + 1023) / 1024, b = t * per, e = b + per < n_tiles ? b + per : n_tiles;
    uint32_t tot = VMX_FQ_MAP_IDENT;
    for (int64_t i = b; i < e; ++i) tot = fq_compose(tot, tile[i]);
    const uint32_t v = fq_wave_scan(tot, lane);                           // the work-items' partials: in the wavefront, then over the 16 wavefronts
    uint32_t ex = __shfl_up(v, 1);
    if (lane == 0) ex = VMX_FQ_MAP_IDENT;
    if (lane == 63) s_w[w] = v;
    __syncthreads();
    uint32_t run = VMX_FQ_MAP_IDENT;
    for (int j = 0; j < w; ++j) run = fq_compose(run, s_w[j]);
    run = fq_compose(run, ex);
    for (int64_t i = b; i < e; ++i) { const uint32_t x = tile[i]; tile[i] = (uint8_t)run; run = fq_compose(run, x); }
}

// start[k] = 1 where line k begins a record (it is not blank and the state before it is 0; the window begins in state 0), start[n_lines] = 0
__global__ void __launch_bounds__(VMX_FQ_LTILE) k_fq_line_states(const uint8_t* map, const uint8_t* tile_pre, int64_t n_lines, int64_t* start) {
    __shared__ uint32_t s_w[VMX_FQ_LTILE / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int64_t k = (int64_t)blockIdx.x * VMX_FQ_LTILE + t;
    const uint32_t m = k < n_lines ? map[k] : VMX_FQ_MAP_IDENT;
    const uint32_t v = fq_wave_scan(m, lane);
    if (lane == 63) s_w[w] = v;
    uint32_t ex = __shfl_up(v, 1);
    if (lane == 0) ex = VMX_FQ_MAP_IDENT;
    __syncthreads();
    uint32_t pre = tile_pre[blockIdx.x];
    for (int j = 0; j < w; ++j) pre = fq_compose(pre, s_w[j]);
    pre = fq_compose(pre, ex);
    if (k < n_lines) start[k] = (pre & 3u) == 0 && m == VMX_FQ_MAP_LINE;
    else if (k == n_lines) start[k] = 0;
}

// ------------------------------------------------------------------------------------------------ records

// rline[r] = first line of record r (ridx: the exclusive scan of start)
__global__ void __launch_bounds__(256) k_fq_records(const int64_t* start, const int64_t* ridx, int64_t n_lines, int64_t* rline) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n_lines && start[k]) rline[ridx[k]] = k;
}

// only the last record begun can lack lines: the window is cut in front of it, or behind its last line (blank lines follow the last complete record, if any do).
// The header of that record is a whole line already: a first byte other than '@' is reported now, as record n_rec, not when (if ever) its other lines arrive.
// Reads buf[ls[k]], the first byte of a line that is not blank.
__global__ void k_fq_result(const uint8_t* buf, const int64_t* ls, const int64_t* ridx, const int64_t* rline, int64_t n_lines, int64_t len, vmx_fq_result* res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t n_st = ridx[n_lines];
    const int64_t k = n_st > 0 ? rline[n_st - 1] : 0;
    if (n_st > 0 && k + 3 >= n_lines) {
        res->n_rec = n_st - 1; res->end = ls[k]; res->end_state = (int32_t)(n_lines - k);
        const uint8_t h = buf[ls[k]];
        if (h != '@') atomicMin((unsigned long long*)&res->err_key, (unsigned long long)(n_st - 1) << 8 | (unsigned long long)(h == '>' ? VMX_FQ_E_FASTA : VMX_FQ_E_HEADER));
    }
    else { res->n_rec = n_st; res->end = ls[n_lines] < len ? ls[n_lines] : len; res->end_state = 0; }
}

// ------------------------------------------------------------------------------------------------ fields

// One wavefront per complete record: bytes of name, comment, bases and qualities; slot n_rec of each = 0 (the scans' totals). The first header
// that does not begin with '@' goes to err_key. Reads buf inside the record's lines 0, 1 and 3 only (rline[r] + 3 < n_lines).
__global__ void __launch_bounds__(256) k_fq_sizes(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, int64_t* nsz, int64_t* csz, int64_t* ssz, int64_t* qsz,
                                                  unsigned long long* err_key) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r > n_rec) return;
    if (r == n_rec) { if (lane == 0) { nsz[r] = 0; csz[r] = 0; ssz[r] = 0; qsz[r] = 0; } return; }
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
    if (h != '@') atomicMin(err_key, (unsigned long long)r << 8 | (unsigned long long)(h == '>' ? VMX_FQ_E_FASTA : VMX_FQ_E_HEADER));
    nsz[r] = sp - (a + 1);
    csz[r] = sp < b ? b - sp - 1 : 0;
    int64_t sa, sb;
    fq_line(buf, ls, k + 1, sa, sb); ssz[r] = sb - sa;
    fq_line(buf, ls, k + 3, sa, sb); qsz[r] = sb - sa;
}

// One wavefront per record: its four fields to the blobs, at the offsets the scans of k_fq_sizes' columns gave (the field's bytes are re-derived
// from those offsets and the line starts). Writes [off[r], off[r + 1]) of each blob.
__global__ void __launch_bounds__(256) k_fq_copy(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, const int64_t* noff, const int64_t* coff,
                                                 const int64_t* soff, const int64_t* qoff, uint8_t* names, uint8_t* comments, uint8_t* seqs, uint8_t* quals) {
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= n_rec) return;
    const int64_t k = rline[r];
    const int64_t a = ls[k], nn = noff[r + 1] - noff[r], nc = coff[r + 1] - coff[r];
    fq_copy<false>(buf + a + 1, names + noff[r], nn, lane);
    fq_copy<false>(buf + a + 1 + nn + 1, comments + coff[r], nc, lane);    // (behind the separator; nothing is read when there is no comment)
    fq_copy<true>(buf + ls[k + 1], seqs + soff[r], soff[r + 1] - soff[r], lane);
    fq_copy<false>(buf + ls[k + 3], quals + qoff[r], qoff[r + 1] - qoff[r], lane);
}
