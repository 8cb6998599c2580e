// k_fastx_dev.h — device helpers shared by the text parsers (k_fastx_in.hip: FASTQ reads, k_fasta_in.hip: the reference FASTA): byte
// comparison four at a time, the packed state maps and their prefix composition, upper-casing, the wide copy.
#ifndef K_FASTX_DEV_H
#define K_FASTX_DEV_H
#include <string.h>
#include "vmx_bam.h"

struct alignas(16) fq_v16 { uint32_t x, y, z, w; };

// 0x80 in every byte of x that equals the byte repeated in c4 (exact: no carry leaves a byte)
__device__ __forceinline__ uint32_t fq_eq_bytes(uint32_t x, uint32_t c4) {
    x ^= c4;
    const uint32_t t = (x & 0x7f7f7f7fu) + 0x7f7f7f7fu;
    return ~(t | x | 0x7f7f7f7fu);
}
__device__ __forceinline__ uint32_t fq_nibble(uint32_t m) { return (m >> 7 & 1u) | (m >> 14 & 2u) | (m >> 21 & 4u) | (m >> 28 & 8u); }

// bit i: byte i of the 16 in v equals the byte repeated in c4
__device__ __forceinline__ uint32_t fq_mask16(const fq_v16& v, uint32_t c4) {
    return fq_nibble(fq_eq_bytes(v.x, c4)) | fq_nibble(fq_eq_bytes(v.y, c4)) << 4 | fq_nibble(fq_eq_bytes(v.z, c4)) << 8 | fq_nibble(fq_eq_bytes(v.w, c4)) << 12;
}
__device__ __forceinline__ uint32_t fq_byte16(const fq_v16& v, int k) { const uint32_t w = k < 4 ? v.x : k < 8 ? v.y : k < 12 ? v.z : v.w; return w >> (8 * (k & 3)) & 0xffu; }

// line k without its terminator and without one trailing '\r': buf[a, b), 0 <= a <= b <= len (ls[k + 1] - 1 is the newline's position, or len)
__device__ __forceinline__ void fq_line(const uint8_t* buf, const int64_t* ls, int64_t k, int64_t& a, int64_t& b) {
    a = ls[k]; b = ls[k + 1] - 1;
    if (b > a && buf[b - 1] == '\r') --b;
}

// first f, then g
__device__ __forceinline__ uint32_t fq_compose(uint32_t f, uint32_t g) {
    uint32_t h = 0;
    for (int s = 0; s < 4; ++s) h |= (g >> (2 * (f >> (2 * s) & 3u)) & 3u) << (2 * s);
    return h;
}

// inclusive prefix composition over the wavefront
__device__ __forceinline__ uint32_t fq_wave_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(v, d); if (lane >= d) v = fq_compose(t, v); }
    return v;
}

__device__ __forceinline__ uint32_t fq_upper4(uint32_t w) {
    const uint32_t h = w & 0x7f7f7f7fu;
    const uint32_t m = (h + 0x1f1f1f1fu) & ~(h + 0x05050505u) & ~w & 0x80808080u;      // 0x80 where 'a' <= byte <= 'z'
    return w ^ (m >> 2);
}
__device__ __forceinline__ uint8_t fq_upper1(uint8_t c) { return (uint8_t)(c - (((unsigned)(c - 'a') < 26u) << 5)); }

// d[0, sz) = s[0, sz), as k_bam_gather copies: bytes up to the destination's 16-byte boundary, 16-byte stores to aligned addresses (the source
// vector is read at whatever alignment it has), the byte tail. UP: 'a' ... 'z' become upper case. Every load lies inside s[0, sz).
template <bool UP> __device__ __forceinline__ void fq_copy(const uint8_t* s, uint8_t* d, int64_t sz, int lane) {
    int64_t head = (int64_t)((16 - ((uintptr_t)d & 15)) & 15);
    if (head > sz) head = sz;
    if (lane < head) d[lane] = UP ? fq_upper1(s[lane]) : s[lane];
    const int64_t nv = (sz - head) >> 4;
    for (int64_t k = lane; k < nv; k += 64) {
        fq_v16 v;
        memcpy(&v, s + head + (k << 4), 16);
        if (UP) { v.x = fq_upper4(v.x); v.y = fq_upper4(v.y); v.z = fq_upper4(v.z); v.w = fq_upper4(v.w); }
        *(fq_v16*)(d + head + (k << 4)) = v;
    }
    const int64_t t0 = head + (nv << 4);
    if (t0 + lane < sz) d[t0 + lane] = UP ? fq_upper1(s[t0 + lane]) : s[t0 + lane];
}

#endif
