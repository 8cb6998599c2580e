// k_inflate_dev.h — the wave-uniform RFC 1951 decoder pieces shared by k_bgzf_inflate (k_bam_in.hip: one BGZF member per wavefront) and the
// plain-gzip kernels (k_gzip_in.hip: one chunk of a single deflate stream per wavefront). The decoder's state (bit buffer, cursors, the
// symbol in hand) is the same in every lane and is read back through vmx_uniform_i32, so it lives in scalar registers:
//   * compressed input: 512 bytes at a time into an LDS ring (one coalesced load), words from there into a 64-bit bit buffer;
//   * Huffman tables (per wave in LDS): code-length counts by LDS atomics, every symbol's rank among the symbols of its length by 15 ballots
//     per 64 symbols, canonical codes from there; a primary table of 10 (literal / length) or 9 (distance) bits is filled by all lanes,
//     longer codes are decoded canonically, bit by bit, from the per-length counts and the symbols sorted by (length, symbol).
// Code-length sets are accepted exactly where zlib's inflate_table accepts them (bzi_build).
#ifndef K_INFLATE_DEV_H
#define K_INFLATE_DEV_H
#include "vmx_bam.h"

#ifdef VMX_EMU
#define VMX_BAM_CONST static const
#else
#define VMX_BAM_CONST static __constant__
#endif

#define BZI_LIT_BITS 10
#define BZI_DIST_BITS 9
#define BZI_RING 128                    // words of compressed input held in LDS

// every store of this wave is complete and visible to every lane's later loads
__device__ __forceinline__ void bzi_store_fence() {
#ifdef VMX_EMU
    __syncthreads();
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#endif
}

__device__ __forceinline__ uint32_t bzi_u(uint32_t v) { return (uint32_t)vmx_uniform_i32((int)v); }

struct BziIn {
    const uint32_t* w;      // aligned words that cover the deflate data
    uint32_t n_words;
    uint32_t* ring;         // LDS: words [loaded - BZI_RING, loaded)
    uint64_t bb;
    uint32_t nb, wi, loaded;
};

__device__ static void bzi_load(BziIn& s, int lane) {
    vmx_wave_lds_fence();                                               // (every lane has read what it wanted of the old ring)
    for (uint32_t k = (uint32_t)lane; k < BZI_RING; k += 64) { const uint32_t i = s.loaded + k; s.ring[i & (BZI_RING - 1)] = i < s.n_words ? s.w[i] : 0u; }
    s.loaded += BZI_RING;
    vmx_wave_lds_fence();
}

// more than 32 bits in the bit buffer afterwards (zeros beyond the input: the callers compare bzi_bitpos with the data's end)
__device__ __forceinline__ void bzi_ensure(BziIn& s, int lane) {
    if (s.nb <= 32) {
        if (s.wi >= s.loaded) bzi_load(s, lane);
        s.bb |= (uint64_t)bzi_u(s.ring[s.wi & (BZI_RING - 1)]) << s.nb;
        s.nb += 32; ++s.wi;
    }
}
__device__ __forceinline__ uint32_t bzi_take(BziIn& s, uint32_t n) { const uint32_t v = (uint32_t)s.bb & ((1u << n) - 1u); s.bb >>= n; s.nb -= n; return v; }
__device__ __forceinline__ uint32_t bzi_bitpos(const BziIn& s) { return s.wi * 32u - s.nb; }
__device__ static void bzi_seek(BziIn& s, uint32_t byte, int lane) {
    s.wi = byte >> 2; s.loaded = s.wi; s.bb = 0; s.nb = 0;
    bzi_ensure(s, lane);
    (void)bzi_take(s, 8 * (byte & 3));
}

// one Huffman code: per-length counts, first code and first slot per length, the symbols by (length, symbol), the primary table
struct BziCode { int* cnt; int* nc; int* of; uint16_t* sym; uint16_t* tab; int pb; };

__device__ __forceinline__ uint32_t bzi_rev(uint32_t c, int len) { uint32_t r = 0; for (int i = 0; i < len; ++i) { r = r << 1 | (c & 1); c >>= 1; } return r; }

// kind 0: the code-length code, 1: literal / length, 2: distance (zlib's CODES, LENS, DISTS), 3: a fixed code (complete by construction).
// 0 or a VMX_BGZF_E_* code, the same in every lane
__device__ static int bzi_build(const uint8_t* lens, int n, const BziCode& C, int kind, int lane) {
    if (lane < 16) C.cnt[lane] = 0;
    for (int k = lane; k < (1 << C.pb); k += 64) C.tab[k] = 0;
    vmx_wave_lds_fence();
    for (int s = lane; s < n; s += 64) atomicAdd(&C.cnt[lens[s]], 1);
    vmx_wave_lds_fence();
    int left = 1, maxl = 0;
    for (int l = 1; l <= 15; ++l) {
        const int c = vmx_uniform_i32(C.cnt[l]);
        left = (left << 1) - c;
        if (left < 0) return VMX_BGZF_E_LENS;                           // over-subscribed
        if (c) maxl = l;
    }
    vmx_wave_lds_fence();
    if (lane == 0) C.cnt[0] = 0;
    if (maxl == 0) { vmx_wave_lds_fence(); return 0; }                  // no code at all: every use of it is an invalid code
    if (left > 0 && kind != 3 && (kind == 0 || maxl != 1)) return VMX_BGZF_E_LENS;      // incomplete where RFC 1951 (and zlib) forbid it
    if (lane >= 1 && lane < 16) {
        int code = 0, o = 0;
        for (int b = 1; b < lane; ++b) { code = (code + C.cnt[b]) << 1; o += C.cnt[b]; }
        C.nc[lane] = code; C.of[lane] = o;
    }
    vmx_wave_lds_fence();
    int base[16];
#pragma unroll
    for (int l = 0; l < 16; ++l) base[l] = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int s = c0 + lane;
        const int l = s < n ? (int)lens[s] : 0;
        int rank = 0;
#pragma unroll
        for (int L = 1; L <= 15; ++L) {
            const unsigned long long m = __ballot(l == L);
            if (l == L) rank = base[L] + __popcll(m & ((1ull << lane) - 1ull));
            base[L] += __popcll(m);
        }
        if (l) {
            C.sym[C.of[l] + rank] = (uint16_t)s;
            if (l <= C.pb) {
                const uint32_t r = bzi_rev((uint32_t)(C.nc[l] + rank), l);
                for (uint32_t k = r; k < (1u << C.pb); k += 1u << l) C.tab[k] = (uint16_t)(s | l << 9);
            }
        }
    }
    vmx_wave_lds_fence();
    return 0;
}

// the next symbol of code C, or -1 (no such code). More than 32 bits are in the bit buffer
__device__ __forceinline__ int bzi_decode(BziIn& s, const BziCode& C) {
    const uint32_t e = bzi_u(C.tab[(uint32_t)s.bb & ((1u << C.pb) - 1u)]);
    if (e) { (void)bzi_take(s, e >> 9); return (int)(e & 511u); }
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        code |= (int)(s.bb >> (len - 1)) & 1;
        const int count = vmx_uniform_i32(C.cnt[len]);
        if (code - count < first) { (void)bzi_take(s, (uint32_t)len); return (int)bzi_u(C.sym[index + (code - first)]); }
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}

VMX_BAM_CONST uint8_t bzi_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

#endif
