// k_sam_out.h — what the line kernels of k_sam.hip (SAM) and k_paf.hip (PAF) share: the wave-uniform writer of a line and its small helpers.
#ifndef K_SAM_OUT_H
#define K_SAM_OUT_H
#include "vmx_sam_dev.h"

__device__ __forceinline__ unsigned long long sam_lt(int lane) { return (1ull << lane) - 1ull; }
__device__ __forceinline__ int sam_top(unsigned long long m) { return 63 - __clzll((long long)m); }      // highest set bit (m != 0)
__device__ __forceinline__ int sam_ndig(unsigned long long u) { int n = 1; while (u >= 10) { u /= 10; ++n; } return n; }

// a line under construction; every call is made by the whole wave with the same arguments
template <bool W> struct SamOut {
    char* p; int64_t pos; int lane;
    __device__ __forceinline__ void ch(char c) { if (W && lane == 0) p[pos] = c; ++pos; }
    __device__ __forceinline__ void bytes(const char* s, int64_t n) { if (W) for (int64_t x = lane; x < n; x += 64) p[pos + x] = s[x]; pos += n; }
    __device__ __forceinline__ void num(int64_t v) {                    // put_int: sign included
        const bool neg = v < 0;
        const unsigned long long u = neg ? 0ull - (unsigned long long)v : (unsigned long long)v;
        const int nd = sam_ndig(u);
        if (W) {
            if (neg && lane == 0) p[pos] = '-';
            if (lane < nd) { unsigned long long t = u; for (int s = nd - 1 - lane; s > 0; --s) t /= 10; p[pos + (neg ? 1 : 0) + lane] = (char)('0' + t % 10); }
        }
        pos += nd + (neg ? 1 : 0);
    }
};
#endif
