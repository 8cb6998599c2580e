// k_bam.hip — BAM output on the device (SAMv1 §4.2, BGZF §4.1).
//
// Encoder: the SAM text of a window is split at its newlines (k_bam_nl_count / k_bam_scan / k_bam_nl_pos), every line is sized
// (k_bam_size: one work-item per line, a dry run of the encoder), an exclusive scan gives each record its offset, and k_bam_encode
// writes the records. A float token the device cannot convert exactly is listed (vmx_bam_patch) and patched by the host.
//
// Deflate: one workgroup of 1024 work-items per BGZF member (<= 65 280 input bytes, held in LDS). Every step of the LZ77 stage
// is order-insensitive, so the bytes depend on the input only, never on wave scheduling:
//   * CRC32: per-64-byte CRCs combined by multiplication with x^(8 * bytes after the chunk) mod P (zlib's crc32_combine), XOR-reduced.
//   * Match finding in 64 steps of 1024 positions. A 3-byte hash indexes two LDS tables: `first` (atomicMin: the first position of
//     the running step with that hash) and `head` (atomicMax, updated after the step: the last position of an earlier step). prev[p]
//     keeps the head a position saw, so head -> prev -> prev is the last occurrence in each of the three latest steps that had the hash.
//     The 4 candidates (first, head, prev, prev of prev) are compared in that order (nearest first); a strictly longer match wins.
//   * Greedy parse from position 0: every work-item walks its 64-position segment from an assumed entry, entries are replaced by the
//     previous segment's exit until nothing changes (4 rounds at most), then one work-item walks the rest from the first changed entry.
//   * One dynamic Huffman block: LDS histograms (atomicAdd), code lengths by Moffat-Katajainen + the JPEG length limiter (15 / 7 bits),
//     bit offsets by a prefix sum of the tokens' bit lengths, codes OR-ed into an LDS bit buffer. A stored block when it is not larger.
#include "vmx_bam.h"

#ifdef VMX_EMU
#define VMX_BAM_CONST static const
#else
#define VMX_BAM_CONST __constant__
#endif

// ------------------------------------------------------------------------------------------------ scans and newlines

// exclusive scan of v[0..n) in place, v[n] = total (one workgroup; the arrays here hold lines, chunks or members: a few MB at most)
__global__ void __launch_bounds__(1024) k_bam_scan(int64_t* v, int64_t n) {
    __shared__ int64_t s[1024];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024, b = t * per, e = b + per < n ? b + per : n;
    int64_t sum = 0;
    for (int64_t i = b; i < e; ++i) sum += v[i];
    s[t] = sum;
    __syncthreads();
    if (t == 0) {
        int64_t run = 0;
        for (int i = 0; i < 1024; ++i) { const int64_t x = s[i]; s[i] = run; run += x; }
        v[n] = run;
    }
    __syncthreads();
    int64_t run = s[t];
    for (int64_t i = b; i < e; ++i) { const int64_t x = v[i]; v[i] = run; run += x; }
}

__global__ void __launch_bounds__(256) k_bam_nl_count(const char* text, int64_t len, int64_t* cnt) {
    __shared__ int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t b = (int64_t)blockIdx.x * VMX_BAM_NL_CHUNK + threadIdx.x * (VMX_BAM_NL_CHUNK / 256);
    int c = 0;
    for (int64_t i = b; i < b + VMX_BAM_NL_CHUNK / 256 && i < len; ++i) c += text[i] == '\n';
    atomicAdd(&s_n, c);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = s_n;
}

// nl[k] = position of the k-th newline, in text order
__global__ void __launch_bounds__(256) k_bam_nl_pos(const char* text, int64_t len, const int64_t* cnt_off, int64_t* nl) {
    __shared__ int s_c[256];
    const int t = threadIdx.x;
    const int64_t b = (int64_t)blockIdx.x * VMX_BAM_NL_CHUNK + t * (VMX_BAM_NL_CHUNK / 256);
    int c = 0;
    for (int64_t i = b; i < b + VMX_BAM_NL_CHUNK / 256 && i < len; ++i) c += text[i] == '\n';
    s_c[t] = c;
    __syncthreads();
    if (t == 0) { int run = 0; for (int i = 0; i < 256; ++i) { const int x = s_c[i]; s_c[i] = run; run += x; } }
    __syncthreads();
    int64_t k = cnt_off[blockIdx.x] + s_c[t];
    for (int64_t i = b; i < b + VMX_BAM_NL_CHUNK / 256 && i < len; ++i)
        if (text[i] == '\n') nl[k++] = i;
}

// ------------------------------------------------------------------------------------------------ one SAM line -> one BAM record

struct BamOut {
    uint8_t* o;             // nullptr: size pass
    int64_t p;
    int64_t sq_at;          // where SEQ starts (set by bam_line; the wave packs SEQ and QUAL there)
    __device__ __forceinline__ void u8(uint32_t v) { if (o) o[p] = (uint8_t)v; ++p; }
    __device__ __forceinline__ void u16(uint32_t v) { u8(v); u8(v >> 8); }
    __device__ __forceinline__ void u32(uint32_t v) { u16(v); u16(v >> 16); }
};

__device__ __forceinline__ bool bam_digit(char c) { return c >= '0' && c <= '9'; }

__device__ static bool bam_parse_int(const char* s, int64_t n, int64_t* v) {
    int64_t i = 0; bool neg = false;
    if (n > 0 && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
    if (i >= n || n - i > 18) return false;
    int64_t x = 0;
    for (; i < n; ++i) { if (!bam_digit(s[i])) return false; x = x * 10 + (s[i] - '0'); }
    *v = neg ? -x : x;
    return true;
}

// float32 of a decimal token, exact when the device can do it (Clinger's fast path: <= 15 significant digits, |exponent| <= 22,
// one exact product or quotient in double, then the cast strtod + (float) gives). 1: *out set; 0: the host converts it; -1: malformed
__device__ static int bam_parse_float(const char* s, int64_t n, float* out) {
    int64_t i = 0; bool neg = false;
    if (n > 0 && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; i = 1; }
    uint64_t m = 0; int sig = 0, e10 = 0, nd = 0; bool dot = false;
    for (; i < n; ++i) {
        const char c = s[i];
        if (c == '.') { if (dot) return -1; dot = true; continue; }
        if (!bam_digit(c)) break;
        ++nd;
        if (m == 0 && c == '0') { if (dot) --e10; continue; }
        if (sig < 19) { m = m * 10 + (uint64_t)(c - '0'); if (dot) --e10; }
        else if (!dot) ++e10;
        ++sig;
    }
    if (i < n) {
        if (nd == 0) return 0;                                      // nan, inf, hexadecimal: strtod on the host decides
        if (s[i] != 'e' && s[i] != 'E') return -1;
        ++i; bool eneg = false;
        if (i < n && (s[i] == '-' || s[i] == '+')) { eneg = s[i] == '-'; ++i; }
        if (i >= n) return -1;
        int ex = 0;
        for (; i < n; ++i) { if (!bam_digit(s[i])) return -1; if (ex < 100000) ex = ex * 10 + (s[i] - '0'); }
        e10 += eneg ? -ex : ex;
    }
    if (nd == 0) return -1;
    if (m == 0) { *out = neg ? -0.0f : 0.0f; return 1; }
    if (sig > 15 || e10 > 22 || e10 < -22) return 0;
    double p10 = 1.0;
    for (int k = 0; k < (e10 < 0 ? -e10 : e10); ++k) p10 *= 10.0;    // 10^k is exact in double up to k = 22
    double d = (double)m;
    d = e10 < 0 ? d / p10 : d * p10;
    *out = (float)(neg ? -d : d);
    return 1;
}

__device__ static int bam_ref_lookup(const vmx_bam_refs& R, const char* s, int64_t n) {
    uint32_t h = 2166136261u;
    for (int64_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 16777619u; }
    for (uint32_t k = h & (uint32_t)R.hmask;; k = (k + 1) & (uint32_t)R.hmask) {
        const int r = R.htab[k];
        if (r < 0) return -2;
        const int64_t b = R.off[r], l = R.off[r + 1] - b;
        if (l != n) continue;
        int64_t i = 0;
        while (i < n && R.names[b + i] == s[i]) ++i;
        if (i == n) return r;
    }
}

__device__ __forceinline__ int bam_cigar_op(char c) {
    switch (c) { case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5;
                 case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1; }
}

__device__ __forceinline__ uint32_t bam_nt16(char c) {
    switch (c | 0x20) {
        case 'a': return 1; case 'c': return 2; case 'm': return 3; case 'g': return 4; case 'r': return 5; case 's': return 6; case 'v': return 7;
        case 't': return 8; case 'w': return 9; case 'y': return 10; case 'h': return 11; case 'k': return 12; case 'd': return 13; case 'b': return 14;
        default: return c == '=' ? 0 : 15;
    }
}

__device__ static int bam_reg2bin(int64_t beg, int64_t end) {
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// a float value: 4 bytes, converted here or listed for the host (n_patch counts them in the size pass, fills `patch` in the encode pass)
__device__ static int bam_put_float(BamOut& w, const char* s, int64_t n, int64_t text_off, int64_t line, vmx_bam_patch* patch, int32_t* n_patch) {
    float f = 0.0f;
    const int r = bam_parse_float(s, n, &f);
    if (r < 0) return -1;
    if (r == 0) {
        const int k = atomicAdd(n_patch, 1);
        if (w.o) { patch[k].out_off = w.p; patch[k].text_off = text_off; patch[k].text_len = (int32_t)n; patch[k].line = (int32_t)line; }
        f = 0.0f;
    }
    uint32_t u; memcpy(&u, &f, 4);
    w.u32(u);
    return 0;
}

// record bytes of one line (w.o == nullptr: size only) or a negative VMX_BAM_E_* code. fs / fl: the 11 mandatory fields (bam_wave_fields);
// tags_at: the first optional field, -1 when there is none. SEQ and QUAL are left to the wave (w.sq_at).
__device__ static int64_t bam_line(const char* s, int64_t n, const int64_t* fs, const int64_t* fl, int64_t tags_at, int64_t text_off, int64_t line,
                                   const vmx_bam_refs& R, BamOut& w, vmx_bam_patch* patch, int32_t* n_patch) {
    bool more = tags_at >= 0;
    int64_t p = more ? tags_at : n;
    if (fl[0] > 254 || fl[0] == 0) return -VMX_BAM_E_NAME;
    int64_t flag, pos, mapq, pnext, tlen;
    if (!bam_parse_int(s + fs[1], fl[1], &flag) || flag < 0 || flag > 65535) return -VMX_BAM_E_NUM;
    if (!bam_parse_int(s + fs[3], fl[3], &pos) || pos < 0 || pos > 2147483647) return -VMX_BAM_E_NUM;
    if (!bam_parse_int(s + fs[4], fl[4], &mapq) || mapq < 0 || mapq > 255) return -VMX_BAM_E_NUM;
    if (!bam_parse_int(s + fs[7], fl[7], &pnext) || pnext < 0 || pnext > 2147483647) return -VMX_BAM_E_NUM;
    if (!bam_parse_int(s + fs[8], fl[8], &tlen) || tlen < -2147483647LL - 1 || tlen > 2147483647) return -VMX_BAM_E_NUM;
    int ref = -1, nref = -1;
    if (!(fl[2] == 1 && s[fs[2]] == '*')) { ref = bam_ref_lookup(R, s + fs[2], fl[2]); if (ref < 0) return -VMX_BAM_E_REF; }
    if (fl[6] == 1 && s[fs[6]] == '=') nref = ref;
    else if (!(fl[6] == 1 && s[fs[6]] == '*')) { nref = bam_ref_lookup(R, s + fs[6], fl[6]); if (nref < 0) return -VMX_BAM_E_REF; }
    // CIGAR: op count and reference span (every length within BAM's 28 bits)
    const char* cg = s + fs[5]; const int64_t cl = fl[5];
    int64_t nops = 0, span = 0;
    const bool nocig = cl == 1 && cg[0] == '*';
    if (!nocig) {
        if (cl == 0) return -VMX_BAM_E_CIGAR;
        int64_t num = 0; int nd = 0;
        for (int64_t i = 0; i < cl; ++i) {
            const char c = cg[i];
            if (bam_digit(c)) { if (++nd > 9) return -VMX_BAM_E_CIGAR; num = num * 10 + (c - '0'); if (num > VMX_BAM_MAX_OPLEN) return -VMX_BAM_E_CIGAR; continue; }
            const int op = bam_cigar_op(c);
            if (op < 0 || nd == 0) return -VMX_BAM_E_CIGAR;
            ++nops;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += num;
            num = 0; nd = 0;
        }
        if (nd) return -VMX_BAM_E_CIGAR;
    }
    const bool noseq = fl[9] == 1 && s[fs[9]] == '*';
    const int64_t lseq = noseq ? 0 : fl[9];
    const bool noqual = fl[10] == 1 && s[fs[10]] == '*';
    if (!noqual && fl[10] != lseq) return -VMX_BAM_E_QUAL;
    const bool big = nops > 65535;
    if (big && (lseq > VMX_BAM_MAX_OPLEN || span > VMX_BAM_MAX_OPLEN)) return -VMX_BAM_E_CIGAR;     // the kSmN placeholder holds 28-bit lengths too
    const int64_t p0 = w.p;
    w.p += 4;                                                   // block_size, written last
    w.u32((uint32_t)ref); w.u32((uint32_t)(pos - 1));
    w.u8((uint32_t)(fl[0] + 1)); w.u8((uint32_t)mapq);
    w.u16((uint32_t)bam_reg2bin(pos - 1, pos - 1 + (span > 0 ? span : 1)));
    w.u16((uint32_t)(big ? 2 : nops)); w.u16((uint32_t)flag);
    w.u32((uint32_t)lseq); w.u32((uint32_t)nref); w.u32((uint32_t)(pnext - 1)); w.u32((uint32_t)tlen);
    for (int64_t i = 0; i < fl[0]; ++i) w.u8((uint8_t)s[fs[0] + i]);
    w.u8(0);
    // CIGAR (above 65 535 ops: <l_seq>S<span>N here, the real one in CG:B,I after the other tags, as SAMv1 §4.2.2 and htslib)
    if (big) { w.u32((uint32_t)(lseq << 4 | 4)); w.u32((uint32_t)(span << 4 | 3)); }
    else if (!nocig) {
        if (w.o) {
            uint32_t num = 0;
            for (int64_t i = 0; i < cl; ++i) {
                const char c = cg[i];
                if (bam_digit(c)) { num = num * 10 + (c - '0'); continue; }
                w.u32(num << 4 | (uint32_t)bam_cigar_op(c)); num = 0;
            }
        } else w.p += 4 * nops;
    }
    // SEQ, QUAL: written by the whole wave (bam_wave_seq_qual)
    w.sq_at = w.p;
    w.p += (lseq + 1) / 2 + lseq;
    // tags
    while (more) {
        int64_t q = p;
        while (q < n && s[q] != '\t') ++q;
        const char* t = s + p; const int64_t tl = q - p;
        if (tl < 5 || t[2] != ':' || t[4] != ':') return -VMX_BAM_E_TAG;
        const char* v = t + 5; const int64_t vl = tl - 5;
        const char ty = t[3];
        w.u8((uint8_t)t[0]); w.u8((uint8_t)t[1]);
        if (ty == 'A') {
            if (vl != 1) return -VMX_BAM_E_TAG;
            w.u8('A'); w.u8((uint8_t)v[0]);
        } else if (ty == 'i') {
            int64_t x;
            if (!bam_parse_int(v, vl, &x)) return -VMX_BAM_E_TAG;
            if (x < 0) {                                            // the smallest of c C s S i I that holds it, as htslib
                if (x >= -128) { w.u8('c'); w.u8((uint32_t)x); }
                else if (x >= -32768) { w.u8('s'); w.u16((uint32_t)x); }
                else if (x >= -2147483647LL - 1) { w.u8('i'); w.u32((uint32_t)x); }
                else return -VMX_BAM_E_TAG;
            } else {
                if (x <= 255) { w.u8('C'); w.u8((uint32_t)x); }
                else if (x <= 65535) { w.u8('S'); w.u16((uint32_t)x); }
                else if (x <= 4294967295LL) { w.u8('I'); w.u32((uint32_t)x); }
                else return -VMX_BAM_E_TAG;
            }
        } else if (ty == 'f') {
            w.u8('f');
            if (bam_put_float(w, v, vl, text_off + (v - s), line, patch, n_patch) < 0) return -VMX_BAM_E_TAG;
        } else if (ty == 'Z' || ty == 'H') {
            w.u8((uint8_t)ty);
            if (w.o) { for (int64_t i = 0; i < vl; ++i) w.u8((uint8_t)v[i]); } else w.p += vl;
            w.u8(0);
        } else if (ty == 'B') {
            if (vl < 1) return -VMX_BAM_E_TAG;
            const char sub = v[0];
            int64_t lo, hi; int es;
            switch (sub) {
                case 'c': lo = -128; hi = 127; es = 1; break;
                case 'C': lo = 0; hi = 255; es = 1; break;
                case 's': lo = -32768; hi = 32767; es = 2; break;
                case 'S': lo = 0; hi = 65535; es = 2; break;
                case 'i': lo = -2147483647LL - 1; hi = 2147483647; es = 4; break;
                case 'I': lo = 0; hi = 4294967295LL; es = 4; break;
                case 'f': lo = 0; hi = 0; es = 4; break;
                default: return -VMX_BAM_E_TAG;
            }
            if (vl > 1 && v[1] != ',') return -VMX_BAM_E_TAG;
            int64_t cnt = 0;
            for (int64_t i = 1; i < vl; ++i) cnt += v[i] == ',';
            w.u8('B'); w.u8((uint8_t)sub); w.u32((uint32_t)cnt);
            int64_t e = 1;
            for (int64_t k = 0; k < cnt; ++k) {
                const int64_t b = e + 1;
                e = b;
                while (e < vl && v[e] != ',') ++e;
                if (sub == 'f') { if (bam_put_float(w, v + b, e - b, text_off + (v - s) + b, line, patch, n_patch) < 0) return -VMX_BAM_E_TAG; continue; }
                int64_t x;
                if (!bam_parse_int(v + b, e - b, &x) || x < lo || x > hi) return -VMX_BAM_E_TAG;
                if (es == 1) w.u8((uint32_t)x); else if (es == 2) w.u16((uint32_t)x); else w.u32((uint32_t)x);
            }
        } else return -VMX_BAM_E_TAG;
        if (q >= n) break;
        p = q + 1;
    }
    if (big) {
        w.u8('C'); w.u8('G'); w.u8('B'); w.u8('I'); w.u32((uint32_t)nops);
        if (w.o) {
            uint32_t num = 0;
            for (int64_t i = 0; i < cl; ++i) {
                const char c = cg[i];
                if (bam_digit(c)) { num = num * 10 + (c - '0'); continue; }
                w.u32(num << 4 | (uint32_t)bam_cigar_op(c)); num = 0;
            }
        } else w.p += 4 * nops;
    }
    const int64_t size = w.p - p0;
    if (w.o) { const int64_t e = w.p; w.p = p0; w.u32((uint32_t)(size - 4)); w.p = e; }
    return size;
}

__device__ __forceinline__ void bam_line_span(const int64_t* nl, int64_t i, int64_t* b, int64_t* e) { *b = i ? nl[i - 1] + 1 : 0; *e = nl[i]; }

// One wave per line. The tabs that end the 11 mandatory fields are found 64 bytes at a time (a ballot per stride: SEQ and QUAL are most
// of a long read's line), the rest of the record is written by lane 0, SEQ and QUAL by all lanes. tab: this wave's 11 slots in LDS.
// Returns the number of tabs found (<= 11, wave-uniform); fs / fl / *tags_at as bam_line takes them.
__device__ static int bam_wave_fields(const char* s, int64_t n, int64_t* tab, int64_t* fs, int64_t* fl, int64_t* tags_at) {
    const int lane = (int)(threadIdx.x & 63);
    int found = 0;
    for (int64_t b = 0; b < n && found < 11; b += 64) {
        const int64_t i = b + lane;
        const bool t = i < n && s[i] == '\t';
        const unsigned long long m = __ballot(t);
        if (t) { const int r = found + __popcll(m & ((1ull << lane) - 1)); if (r < 11) tab[r] = i; }
        found += __popcll(m);
    }
    (void)__ballot(1);                                              // (the wave meets: every lane's tab slots are written)
    if (found > 11) found = 11;
    for (int k = 0; k < 11; ++k) {
        fs[k] = k == 0 ? 0 : (k <= found ? tab[k - 1] + 1 : n);
        fl[k] = (k < found ? tab[k] : n) - fs[k];
    }
    *tags_at = found == 11 ? tab[10] + 1 : -1;
    return found;
}

__device__ static void bam_wave_seq_qual(const char* s, const int64_t* fs, const int64_t* fl, uint8_t* out) {
    const int lane = (int)(threadIdx.x & 63);
    const char* sq = s + fs[9]; const char* qu = s + fs[10];
    const int64_t lseq = fl[9] == 1 && sq[0] == '*' ? 0 : fl[9];
    const bool noqual = fl[10] == 1 && qu[0] == '*';
    for (int64_t j = lane; j < (lseq + 1) / 2; j += 64)
        out[j] = (uint8_t)(bam_nt16(sq[2 * j]) << 4 | (2 * j + 1 < lseq ? bam_nt16(sq[2 * j + 1]) : 0));
    uint8_t* q = out + (lseq + 1) / 2;
    for (int64_t j = lane; j < lseq; j += 64) q[j] = noqual ? 0xff : (uint8_t)(qu[j] - 33);
}

// the first malformed line wins (key = line << 8 | code, atomicMin): deterministic whatever the order of the work-items
__global__ void __launch_bounds__(256) k_bam_size(const char* text, const int64_t* nl, int64_t n_lines, vmx_bam_refs refs, int64_t* rsz, vmx_bam_status* st) {
    __shared__ int64_t s_tab[4][11];
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_lines) return;                                        // (a whole wave)
    int64_t b, e;
    bam_line_span(nl, i, &b, &e);
    int64_t fs[11], fl[11], tags_at;
    const int nt = bam_wave_fields(text + b, e - b, s_tab[threadIdx.x >> 6], fs, fl, &tags_at);
    if ((threadIdx.x & 63) != 0) return;
    BamOut w{nullptr, 0, 0};
    const int64_t r = nt < 10 ? -VMX_BAM_E_FIELDS : bam_line(text + b, e - b, fs, fl, tags_at, b, i, refs, w, nullptr, &st->n_patch);
    if (r < 0) { atomicMin((unsigned long long*)&st->err_key, (unsigned long long)(i << 8 | -r)); rsz[i] = 0; }
    else rsz[i] = r;
}

__global__ void k_bam_status(const int64_t* roff, int64_t n_lines, vmx_bam_status* st) {
    if (threadIdx.x == 0) st->total = roff[n_lines];
}

__global__ void __launch_bounds__(256) k_bam_encode(const char* text, const int64_t* nl, int64_t n_lines, vmx_bam_refs refs, const int64_t* roff, uint8_t* out,
                                                    vmx_bam_patch* patch, int32_t* n_patch) {
    __shared__ int64_t s_tab[4][11];
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n_lines) return;
    int64_t b, e;
    bam_line_span(nl, i, &b, &e);
    int64_t fs[11], fl[11], tags_at;
    (void)bam_wave_fields(text + b, e - b, s_tab[threadIdx.x >> 6], fs, fl, &tags_at);
    int64_t sq_at = 0;
    if ((threadIdx.x & 63) == 0) {                                   // (the size pass accepted every line)
        BamOut w{out, roff[i], 0};
        (void)bam_line(text + b, e - b, fs, fl, tags_at, b, i, refs, w, patch, n_patch);
        sq_at = w.sq_at;
    }
    sq_at = __shfl(sq_at, 0);
    bam_wave_seq_qual(text + b, fs, fl, out + sq_at);
}

__global__ void __launch_bounds__(256) k_bam_patch(uint8_t* out, const int64_t* off, const uint32_t* val, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int k = 0; k < 4; ++k) out[off[i] + k] = (uint8_t)(val[i] >> (8 * k));
}

// ------------------------------------------------------------------------------------------------ BGZF deflate

// (CRC_POLY, crc_multmodp and crc_x8n: vmx_bam.h, shared with the inflate kernel)

// LSB-first bits into the LDS bit buffer; v < 2^nb, nb <= 16
__device__ __forceinline__ void bz_put(uint32_t* buf, uint32_t off, uint32_t v, int nb) {
    if (nb == 0) return;
    const uint32_t wd = off >> 5, sh = off & 31;
    atomicOr(&buf[wd], v << sh);
    if (sh + nb > 32) atomicOr(&buf[wd + 1], v >> (32 - sh));
}

__device__ __forceinline__ void bz_lsym(int len, int* code, int* eb, int* ev) {
    if (len == 258) { *code = 285; *eb = 0; *ev = 0; return; }
    const int x = len - 3;
    if (x < 8) { *code = 257 + x; *eb = 0; *ev = 0; return; }
    const int nb = 31 - __clz(x);
    *code = 257 + 4 * (nb - 1) + ((x >> (nb - 2)) & 3); *eb = nb - 2; *ev = x & ((1 << (nb - 2)) - 1);
}

__device__ __forceinline__ void bz_dsym(int d, int* code, int* eb, int* ev) {
    const int x = d - 1;
    if (x < 4) { *code = x; *eb = 0; *ev = 0; return; }
    const int nb = 31 - __clz(x);
    *code = 2 * nb + ((x >> (nb - 1)) & 1); *eb = nb - 1; *ev = x & ((1 << (nb - 1)) - 1);
}

// log2(x) in 1/16 units for x >= 1: integer part from the leading bit, four fraction bits by repeated squaring
__device__ __forceinline__ uint32_t bz_log2_q4(uint64_t x) {
    int e = 63 - __clzll((long long)x);
    uint64_t m = e >= 31 ? x >> (e - 31) : x << (31 - e);             // 1.f in Q31
    uint32_t r = (uint32_t)e << 4;
    for (int i = 3; i >= 0; --i) {
        m = (m * m) >> 31;
        if (m >= (1ull << 32)) { r |= 1u << i; m >>= 1; }
    }
    return r;
}

__device__ __forceinline__ uint32_t bz_rev(uint32_t c, int len) { uint32_t r = 0; for (int i = 0; i < len; ++i) { r = r << 1 | (c & 1); c >>= 1; } return r; }

// Huffman code lengths limited to L bits and canonical (bit-reversed) codes of nsym symbols. sorted: the m >= 2 symbols of non-zero
// frequency, ascending by (frequency, symbol); A: work space of m words. One work-item.
__device__ static void bz_huff(const uint32_t* freq, const uint16_t* sorted, int m, int nsym, int L, uint8_t* lens, uint16_t* codes, uint32_t* A) {
    for (int i = 0; i < m; ++i) A[i] = freq[sorted[i]];
    // Moffat & Katajainen, in place: A[i] becomes the depth of sorted[i]
    {
        int root = 0, leaf = 2, next;
        A[0] += A[1];
        for (next = 1; next < m - 1; ++next) {
            if (leaf >= m || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; } else A[next] = A[leaf++];
            if (leaf >= m || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; } else A[next] += A[leaf++];
        }
        A[m - 2] = 0;
        for (next = m - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
        int avbl = 1, used = 0, dpth = 0; root = m - 2; next = m - 1;
        while (avbl > 0) {
            while (root >= 0 && (int)A[root] == dpth) { ++used; --root; }
            while (avbl > used) { A[next--] = dpth; --avbl; }
            avbl = 2 * used; ++dpth; used = 0;
        }
    }
    int cnt[33];
    for (int i = 0; i < 33; ++i) cnt[i] = 0;
    int maxd = 0;
    for (int i = 0; i < m; ++i) { const int d = A[i] > 32 ? 32 : (int)A[i]; ++cnt[d]; if (d > maxd) maxd = d; }
    for (int i = maxd; i > L; --i)                                   // JPEG (ITU T.81 K.3) limiter on the length counts
        while (cnt[i] > 0) { int j = i - 2; while (cnt[j] == 0) --j; cnt[i] -= 2; cnt[i - 1] += 1; cnt[j + 1] += 2; cnt[j] -= 1; }
    for (int i = 0; i < nsym; ++i) lens[i] = 0;
    int idx = 0;
    for (int l = L; l >= 1; --l) for (int c = 0; c < cnt[l]; ++c) lens[sorted[idx++]] = (uint8_t)l;
    int bl[16], nx[16];
    for (int i = 0; i < 16; ++i) bl[i] = 0;
    for (int i = 0; i < nsym; ++i) ++bl[lens[i]];
    bl[0] = 0;
    int code = 0;
    for (int b = 1; b <= 15; ++b) { code = (code + bl[b - 1]) << 1; nx[b] = code; }
    for (int i = 0; i < nsym; ++i) if (lens[i]) codes[i] = (uint16_t)bz_rev((uint32_t)nx[lens[i]]++, lens[i]);
}

VMX_BAM_CONST uint8_t bz_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

__device__ __forceinline__ int bz_step(const uint32_t* match, uint32_t p) { const uint32_t m = match[p]; return m ? (int)(m >> 16) : 1; }

// Phase timing (tools/bam_bench.py phases): built with -DVMX_BGZF_STOP=k the kernel ends after phase k (1 load + byte histogram + CRC, 2 matching, 3 parse,
// 4 histograms + Huffman tables + block header) and writes no valid member; the kernel time of each build gives the phases' cumulative cost.
#ifdef VMX_BGZF_STOP
#define VMX_BGZF_PHASE_END(k, sink) do { __syncthreads(); if ((k) == VMX_BGZF_STOP) { if (t == 0) { msize[mb] = 26; slot[0] = (uint8_t)(sink); } return; } } while (0)   // (sink: the phase's result stays live)
#else
#define VMX_BGZF_PHASE_END(k, sink) do { } while (0)
#endif

// one BGZF member per workgroup: member `first_member + blockIdx.x` of the input, written to its 64 KB slot; msize[member] = its bytes
__global__ void __launch_bounds__(VMX_BGZF_THREADS) k_bgzf_deflate(const uint8_t* in, int64_t n_in, int64_t first_member, uint8_t* slots, int64_t* msize,
                                                                   uint32_t* g_match, uint16_t* g_prev) {
    __shared__ uint8_t s_in[VMX_BGZF_BLOCK + 8];
    __shared__ uint32_t s_u[16384];               // hash tables `first` [0, 8192) and `head` [8192, 16384) while matching, then the output bits
    __shared__ uint32_t s_crctab[256];
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_cost[256];
    __shared__ uint32_t s_x2n[32];
    __shared__ uint32_t s_red[16];
    __shared__ uint32_t s_entry[VMX_BGZF_THREADS], s_aux[VMX_BGZF_THREADS];
    __shared__ uint32_t s_freq[320];              // literal / length [0, 286), distance [288, 318)
    __shared__ uint16_t s_sorted[320];
    __shared__ uint16_t s_code[320];
    __shared__ uint8_t s_len[320];
    __shared__ uint32_t s_work[320];
    __shared__ uint16_t s_rle[320];
    __shared__ int s_flag[4];
    __shared__ uint32_t s_crc, s_hdr_bits;
    __shared__ int s_m[2];

    const int t = threadIdx.x;
    const int64_t mb = first_member + blockIdx.x;
    const int64_t base = mb * VMX_BGZF_BLOCK;
    const int n = (int)(n_in - base < VMX_BGZF_BLOCK ? n_in - base : VMX_BGZF_BLOCK);
    uint32_t* match = g_match + (size_t)blockIdx.x * VMX_BGZF_BLOCK;
    uint16_t* prev = g_prev + (size_t)blockIdx.x * VMX_BGZF_BLOCK;
    uint8_t* slot = slots + (size_t)mb * VMX_BGZF_SLOT;
    uint32_t* s_first = s_u;
    uint32_t* s_head = s_u + 8192;

    for (int i = t; i < n; i += VMX_BGZF_THREADS) s_in[i] = in[base + i];
    for (int i = t; i < 8192; i += VMX_BGZF_THREADS) { s_first[i] = 0xffffffffu; s_head[i] = 0; }
    if (t < 256) { uint32_t c = (uint32_t)t; for (int k = 0; k < 8; ++k) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1; s_crctab[t] = c; }
    if (t == 0) { uint32_t p = 1u << 30; for (int k = 0; k < 32; ++k) { s_x2n[k] = p; p = crc_multmodp(p, p); } }
    if (t < 4) s_flag[t] = 0x7fffffff;
    if (t < 256) s_hist[t] = 0;
    __syncthreads();
    for (int i = t; i < n; i += VMX_BGZF_THREADS) atomicAdd(&s_hist[s_in[i]], 1u);
    __syncthreads();
    // bits a literal of each byte value would cost under the block's byte frequencies: a short match has to beat the literals it replaces
    // (in 1/16 bit, integer arithmetic only, so that every build computes the same decisions)
    if (t < 256) s_cost[t] = s_hist[t] ? bz_log2_q4(((uint64_t)n << 16) / s_hist[t]) - 16 * 16 + 8 : 16 * 16;

    // ---- CRC32: crc(A B) = crc(A) * x^(8|B|) + crc(B)
    {
        const int b = t * 64, e = b + 64 < n ? b + 64 : n;
        uint32_t part = 0;
        if (b < e) {
            uint32_t c = 0xffffffffu;
            for (int i = b; i < e; ++i) c = s_crctab[(c ^ s_in[i]) & 0xff] ^ (c >> 8);
            c = ~c;
            part = crc_multmodp(crc_x8n(s_x2n, (uint32_t)(n - e)), c);
        }
        for (int o = 32; o; o >>= 1) part ^= __shfl_xor(part, o);
        if ((t & 63) == 0) s_red[t >> 6] = part;
    }
    __syncthreads();
    if (t == 0) { uint32_t c = 0; for (int i = 0; i < VMX_BGZF_THREADS / 64; ++i) c ^= s_red[i]; s_crc = c; }

    VMX_BGZF_PHASE_END(1, s_crc);
    // ---- LZ77 matches: match[p] = length << 16 | distance of the best of 4 candidates, 0 for a literal
    const int nsteps = (n + VMX_BGZF_THREADS - 1) / VMX_BGZF_THREADS;
    for (int s = 0; s < nsteps; ++s) {
        const int p = s * VMX_BGZF_THREADS + t;
        const bool hv = p + 2 < n;
        uint32_t h = 0;
        if (hv) {
            h = (((uint32_t)s_in[p] << 16 | (uint32_t)s_in[p + 1] << 8 | s_in[p + 2]) * 2654435761u) >> (32 - VMX_BGZF_HBITS);
            atomicMin(&s_first[h], (uint32_t)(63 - s) << 16 | (uint32_t)p);
        }
        __syncthreads();
        if (p < n) {
            uint32_t best = 0;
            if (hv) {
                const int maxl = n - p < 258 ? n - p : 258;
                const uint32_t f = s_first[h];
                const uint32_t hd = s_head[h];
                prev[p] = (uint16_t)hd;
                int c[4];
                c[0] = (f >> 16) == (uint32_t)(63 - s) && (int)(f & 0xffff) < p ? (int)(f & 0xffff) : -1;
                c[1] = (int)hd - 1;
                c[2] = c[1] >= 0 ? (int)prev[c[1]] - 1 : -1;
                c[3] = c[2] >= 0 ? (int)prev[c[2]] - 1 : -1;
                int bl = 2, bd = 0;
                for (int k = 0; k < 4 && bl < maxl; ++k) {
                    if (c[k] < 0 || p - c[k] > 32768) continue;
                    int l = 0;
                    while (l < maxl && s_in[c[k] + l] == s_in[p + l]) ++l;
                    if (l > bl) { bl = l; bd = p - c[k]; }
                }
                if (bl >= 3 && bl < 16) {
                    // estimated bits of the match (codes of ~7 and ~5 bits plus the extra bits) against those of its literals
                    int c, eb, ev, de;
                    bz_lsym(bl, &c, &eb, &ev); bz_dsym(bd, &c, &de, &ev);
                    uint32_t lit = 0;
                    for (int k = 0; k < bl; ++k) lit += s_cost[s_in[p + k]];
                    if ((uint32_t)(12 + eb + de) * 16 >= lit) bl = 0;
                }
                if (bl >= 3) best = (uint32_t)bl << 16 | (uint32_t)bd;
            }
            match[p] = best;
        }
        __syncthreads();
        if (hv) atomicMax(&s_head[h], (uint32_t)p + 1);
    }

    VMX_BGZF_PHASE_END(2, s_crc);
    // ---- greedy parse: s_entry[seg] = first token start at or after the segment's start
    const int nseg = (n + 63) / 64;
    if (t < nseg) s_entry[t] = 64 * t;
    __syncthreads();
    bool conv = false;
    for (int r = 0; r < 4; ++r) {
        if (t < nseg) {
            uint32_t p = s_entry[t];
            const uint32_t e = (uint32_t)(64 * t + 64 < n ? 64 * t + 64 : n);
            while (p < e) p += bz_step(match, p);
            s_aux[t] = p;
        }
        __syncthreads();
        if (t < nseg) {
            const uint32_t ne = t ? s_aux[t - 1] : 0;
            if (ne != s_entry[t]) { s_entry[t] = ne; atomicMin(&s_flag[r], t); }
        }
        __syncthreads();
        if (s_flag[r] == 0x7fffffff) { conv = true; break; }
    }
    if (!conv && t == 0) {
        uint32_t p = s_entry[s_flag[3]];
        for (int j = s_flag[3]; j < nseg; ++j) {
            s_entry[j] = p;
            const uint32_t e = (uint32_t)(64 * j + 64 < n ? 64 * j + 64 : n);
            while (p < e) p += bz_step(match, p);
        }
    }
    for (int i = t; i < 16384; i += VMX_BGZF_THREADS) s_u[i] = 0;
    if (t < 320) { s_freq[t] = 0; s_len[t] = 0; s_code[t] = 0; }
    __syncthreads();

    VMX_BGZF_PHASE_END(3, s_entry[nseg - 1]);
    // ---- histograms
    const uint32_t seg_b = t < nseg ? s_entry[t] : 0, seg_e = (uint32_t)(64 * t + 64 < n ? 64 * t + 64 : n);
    if (t < nseg) {
        for (uint32_t p = seg_b; p < seg_e;) {
            const uint32_t m = match[p];
            if (!m) { atomicAdd(&s_freq[s_in[p]], 1u); ++p; continue; }
            int c, eb, ev;
            bz_lsym((int)(m >> 16), &c, &eb, &ev); atomicAdd(&s_freq[c], 1u);
            bz_dsym((int)(m & 0xffff), &c, &eb, &ev); atomicAdd(&s_freq[288 + c], 1u);
            p += m >> 16;
        }
    }
    __syncthreads();
    if (t == 0) {
        s_freq[256] += 1;                                                   // end of block
        int nz = 0, one = -1;
        for (int i = 0; i < 30; ++i) if (s_freq[288 + i]) { ++nz; one = i; }
        if (nz == 0) { s_freq[288] = 1; s_freq[289] = 1; }                   // deflate wants at least two distance codes (as zlib's trees.c)
        else if (nz == 1) s_freq[288 + (one == 0 ? 1 : 0)] = 1;
    }
    __syncthreads();
    // rank of every used symbol by (frequency, symbol)
    if (t < 286 || (t >= 288 && t < 318)) {
        const int g0 = t < 286 ? 0 : 288, g1 = t < 286 ? 286 : 318;
        const uint32_t f = s_freq[t];
        if (f) {
            int rk = 0;
            for (int j = g0; j < g1; ++j) { const uint32_t fj = s_freq[j]; rk += fj && (fj < f || (fj == f && j < t)); }
            s_sorted[g0 + rk] = (uint16_t)(t - g0);
        }
    }
    __syncthreads();
    if (t == 0 || t == 64) {                                                // two waves: literal / length and distance trees side by side
        const int g0 = t ? 288 : 0, ns = t ? 30 : 286;
        int m = 0;
        for (int i = 0; i < ns; ++i) m += s_freq[g0 + i] != 0;
        bz_huff(s_freq + g0, s_sorted + g0, m, ns, 15, s_len + g0, s_code + g0, s_work + g0);
    }
    __syncthreads();
    if (t == 0) {
        // dynamic block header: HLIT, HDIST, HCLEN, the code-length code, the run-length coded lengths
        int hlit = 286, hdist = 30;
        while (hlit > 257 && !s_len[hlit - 1]) --hlit;
        while (hdist > 1 && !s_len[288 + hdist - 1]) --hdist;
        const int nl = hlit + hdist;
        int nr = 0;
        uint32_t clf[19];
        for (int i = 0; i < 19; ++i) clf[i] = 0;
        for (int i = 0; i < nl;) {
            const int v = i < hlit ? s_len[i] : s_len[288 + i - hlit];
            int run = 1;
            while (i + run < nl && (i + run < hlit ? s_len[i + run] : s_len[288 + i + run - hlit]) == v) ++run;
            i += run;
            if (v == 0) {
                while (run >= 11) { const int r = run < 138 ? run : 138; s_rle[nr++] = (uint16_t)(18 | (r - 11) << 5); ++clf[18]; run -= r; }
                if (run >= 3) { s_rle[nr++] = (uint16_t)(17 | (run - 3) << 5); ++clf[17]; run = 0; }
            } else {
                s_rle[nr++] = (uint16_t)v; ++clf[v]; --run;
                while (run >= 3) { const int r = run < 6 ? run : 6; s_rle[nr++] = (uint16_t)(16 | (r - 3) << 5); ++clf[16]; run -= r; }
            }
            while (run > 0) { s_rle[nr++] = (uint16_t)v; ++clf[v]; --run; }
        }
        int nz = 0, one = -1;
        for (int i = 0; i < 19; ++i) if (clf[i]) { ++nz; one = i; }
        if (nz == 1) clf[one == 0 ? 1 : 0] = 1;
        uint16_t srt[19]; int m = 0;
        for (int i = 0; i < 19; ++i) {
            if (!clf[i]) continue;
            int j = m++;
            while (j > 0 && clf[srt[j - 1]] > clf[i]) { srt[j] = srt[j - 1]; --j; }
            srt[j] = (uint16_t)i;
        }
        uint8_t cll[19]; uint16_t clc[19]; uint32_t wk[19];
        bz_huff(clf, srt, m, 19, 7, cll, clc, wk);
        int ncl = 19;
        while (ncl > 4 && !cll[bz_cl_order[ncl - 1]]) --ncl;
        uint32_t o = 0;
        bz_put(s_u, o, 1, 1); o += 1;                                        // BFINAL
        bz_put(s_u, o, 2, 2); o += 2;                                        // BTYPE 2: dynamic Huffman
        bz_put(s_u, o, (uint32_t)(hlit - 257), 5); o += 5;
        bz_put(s_u, o, (uint32_t)(hdist - 1), 5); o += 5;
        bz_put(s_u, o, (uint32_t)(ncl - 4), 4); o += 4;
        for (int i = 0; i < ncl; ++i) { bz_put(s_u, o, cll[bz_cl_order[i]], 3); o += 3; }
        for (int i = 0; i < nr; ++i) {
            const int sy = s_rle[i] & 31, ex = s_rle[i] >> 5;
            bz_put(s_u, o, clc[sy], cll[sy]); o += cll[sy];
            if (sy == 16) { bz_put(s_u, o, (uint32_t)ex, 2); o += 2; }
            else if (sy == 17) { bz_put(s_u, o, (uint32_t)ex, 3); o += 3; }
            else if (sy == 18) { bz_put(s_u, o, (uint32_t)ex, 7); o += 7; }
        }
        s_hdr_bits = o;
    }
    __syncthreads();

    VMX_BGZF_PHASE_END(4, s_hdr_bits + s_u[t & 127]);
    // ---- bit lengths of every work-item's tokens, their prefix sum
    uint32_t bits = 0;
    if (t < nseg) {
        for (uint32_t p = seg_b; p < seg_e;) {
            const uint32_t m = match[p];
            if (!m) { bits += s_len[s_in[p]]; ++p; continue; }
            int c, eb, ev;
            bz_lsym((int)(m >> 16), &c, &eb, &ev); bits += s_len[c] + eb;
            bz_dsym((int)(m & 0xffff), &c, &eb, &ev); bits += s_len[288 + c] + eb;
            p += m >> 16;
        }
    }
    uint32_t inc = bits;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o); if ((t & 63) >= o) inc += v; }
    if ((t & 63) == 63) s_red[t >> 6] = inc;
    __syncthreads();
    uint32_t before = inc - bits;
    for (int wv = 0; wv < (t >> 6); ++wv) before += s_red[wv];
    uint32_t sum = 0;
    for (int wv = 0; wv < VMX_BGZF_THREADS / 64; ++wv) sum += s_red[wv];
    const uint32_t total_bits = s_hdr_bits + sum + s_len[256];
    const uint32_t dyn = (total_bits + 7) / 8;
    const bool use_dyn = dyn < (uint32_t)n + 5;                             // a stored block whenever it is not larger
    uint32_t data = 0;
    if (use_dyn) {
        if (t < nseg) {
            uint32_t o = s_hdr_bits + before;
            for (uint32_t p = seg_b; p < seg_e;) {
                const uint32_t m = match[p];
                if (!m) { const int b = s_in[p]; bz_put(s_u, o, s_code[b], s_len[b]); o += s_len[b]; ++p; continue; }
                int c, eb, ev;
                bz_lsym((int)(m >> 16), &c, &eb, &ev);
                bz_put(s_u, o, s_code[c], s_len[c]); o += s_len[c];
                bz_put(s_u, o, (uint32_t)ev, eb); o += eb;
                bz_dsym((int)(m & 0xffff), &c, &eb, &ev);
                bz_put(s_u, o, s_code[288 + c], s_len[288 + c]); o += s_len[288 + c];
                bz_put(s_u, o, (uint32_t)ev, eb); o += eb;
                p += m >> 16;
            }
        }
        if (t == 0) bz_put(s_u, s_hdr_bits + sum, s_code[256], s_len[256]);
        __syncthreads();
        const uint8_t* ob = (const uint8_t*)s_u;
        for (uint32_t i = t; i < dyn; i += VMX_BGZF_THREADS) slot[18 + i] = ob[i];
        data = dyn;
    } else {
        if (t == 0) { slot[18] = 1; slot[19] = (uint8_t)n; slot[20] = (uint8_t)(n >> 8); slot[21] = (uint8_t)~n; slot[22] = (uint8_t)(~n >> 8); }
        for (int i = t; i < n; i += VMX_BGZF_THREADS) slot[23 + i] = s_in[i];
        data = (uint32_t)n + 5;
    }
    if (t == 0) {
        const uint32_t tot = 18 + data + 8, bs = tot - 1;
        const uint8_t hdr[18] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (uint8_t)bs, (uint8_t)(bs >> 8)};
        for (int i = 0; i < 18; ++i) slot[i] = hdr[i];
        uint8_t* tr = slot + 18 + data;
        for (int i = 0; i < 4; ++i) { tr[i] = (uint8_t)(s_crc >> (8 * i)); tr[4 + i] = (uint8_t)((uint32_t)n >> (8 * i)); }
        msize[mb] = tot;
    }
}

// members back to back: moff = exclusive scan of msize
__global__ void __launch_bounds__(256) k_bgzf_compact(const uint8_t* slots, const int64_t* moff, uint8_t* out) {
    const int64_t mb = blockIdx.x;
    const int64_t o = moff[mb], sz = moff[mb + 1] - o;
    const uint8_t* src = slots + (size_t)mb * VMX_BGZF_SLOT;
    for (int64_t i = threadIdx.x; i < sz; i += blockDim.x) out[o + i] = src[i];
}
