// k_gzip_in.hip — plain gzip (RFC 1952 members around one RFC 1951 stream each) inflated on the device in parallel chunks.
// A deflate stream has no index, but a block can be decoded from its first bit by anyone who knows where that bit is; what such a decoder
// lacks is the 32 KB in front. So (the method of pugz and rapidgzip):
//   k_gz_find     per chunk of the compressed window, the first bit at which a non-final dynamic block header is valid in full. Each lane
//                 tests one bit position on bits it holds in registers (BFINAL 0, BTYPE 2, HLIT and HDIST at most 29, a complete
//                 code-length code); the survivors, in ballot order, get the whole wave: gz_dyn_header, the very function the decoder reads
//                 a dynamic header with, so "valid" here is what the decoder accepts.
//   k_gz_count /  one wavefront per start: from there to the first block boundary at or after the next start. Output is 16-bit symbols: a
//   k_gz_decode   byte, or VMX_GZ_MARK | j = "byte j of the 32 KB in front of this wave's first byte". A match copies what it finds, markers
//                 included. Sizes are not known in advance (and the ratio is unbounded), so the same body runs twice: k_gz_count stores
//                 nothing and leaves sizes, the host links the chain and scans the sizes, k_gz_decode writes at the final offsets.
//                 A final block is followed by its trailer (noted with the text position) and, if there is one, the next member's header;
//                 from a member's start on every distance is checked exactly, as it is in a wave that begins at a member header. The stop rule
//                 holds at a header too (a wave whose stop is at or in front of it ends there: a file is cut between members); no candidate
//                 is ever a header, so such an end links to nothing and the host moves the stop on.
//   k_gz_window   one workgroup walks the waves in order: the window behind wave k is the last 32 KB of (window behind k - 1, k's symbols
//                 with their markers replaced); both windows in LDS. It leaves every wave's incoming window in global memory.
//   k_gz_resolve  all text in parallel, 64 bytes per lane: markers replaced from the wave's incoming window, bytes stored 16 at a time, and
//                 the CRC32 of every member as partials (per lane, combined per wave where the wave's text lies in one member) that are
//                 multiplied to the member's end (crc_x8n, crc_multmodp) and xor-ed into the member's accumulator.
// A candidate may be false (deflate data can hold a valid header by chance, or verbatim inside a stored block). A wave started at one decodes
// garbage, so: every input read is bounded by the compressed window (BziIn.n_words, and byte reads compared with n_bytes first), every loop
// consumes input bits, the count pass stores nothing but its result, and the write pass runs for linked waves only and stores no more
// than the count pass counted. Such a wave ends with an error or at some boundary; the host's link check then drops it.
// THE ORDERING RULE OF THE MATCH COPY is k_bgzf_inflate's (k_inflate_dev.h, k_bam_in.hip): bzi_store_fence() between the wave's stores and
// a copy's loads whenever the source range reaches beyond `safe`.
#include "k_inflate_dev.h"

struct alignas(16) gz_v16 { uint32_t x, y, z, w; };

struct GzTabs { uint8_t* lens; BziCode CL, CD, CC; };

__device__ static void gz_seek_bit(BziIn& s, uint32_t bit, int lane) {
    bzi_seek(s, bit >> 3, lane);                                        // (at least 8 bits are left in the buffer)
    (void)bzi_take(s, bit & 7);
}

// the dynamic block header behind BFINAL and BTYPE: both codes built in T. 0 or a VMX_BGZF_E_* code, the same in every lane
__device__ static int gz_dyn_header(BziIn& in, uint32_t end_bits, const GzTabs& T, int lane) {
    uint8_t* s_lens = T.lens;
    bzi_ensure(in, lane);
    const int hlit = (int)bzi_take(in, 5) + 257, hdist = (int)bzi_take(in, 5) + 1, hclen = (int)bzi_take(in, 4) + 4;
    if (hlit > 286 || hdist > 30) return VMX_BGZF_E_HEADER;
    if (lane < 19) s_lens[320 + lane] = 0;
    vmx_wave_lds_fence();
    for (int i = 0; i < hclen; ++i) {
        bzi_ensure(in, lane);
        const uint32_t v = bzi_take(in, 3);
        if (lane == 0) s_lens[320 + bzi_cl_order[i]] = (uint8_t)v;
    }
    vmx_wave_lds_fence();
    if (bzi_bitpos(in) > end_bits) return VMX_BGZF_E_INPUT;
    int err = bzi_build(s_lens + 320, 19, T.CC, 0, lane);
    if (err) return err;
    int have = 0, prev = 0;
    const int want = hlit + hdist;
    while (have < want) {
        bzi_ensure(in, lane);
        const int sy = bzi_decode(in, T.CC);
        if (sy < 0) return VMX_BGZF_E_HEADER;
        int rep = 1, val = sy;
        if (sy == 16) { if (have == 0) return VMX_BGZF_E_HEADER; val = prev; rep = 3 + (int)bzi_take(in, 2); }
        else if (sy == 17) { val = 0; rep = 3 + (int)bzi_take(in, 3); }
        else if (sy == 18) { val = 0; rep = 11 + (int)bzi_take(in, 7); }
        if (have + rep > want) return VMX_BGZF_E_HEADER;
        if (lane < rep) s_lens[have + lane] = (uint8_t)val;
        if (lane + 64 < rep) s_lens[have + lane + 64] = (uint8_t)val;
        if (lane + 128 < rep) s_lens[have + lane + 128] = (uint8_t)val;
        have += rep; prev = val;
        if (bzi_bitpos(in) > end_bits) return VMX_BGZF_E_INPUT;
    }
    vmx_wave_lds_fence();
    if (vmx_uniform_i32(s_lens[256]) == 0) return VMX_BGZF_E_HEADER;    // no end-of-block code
    // the distance lengths move behind slot 288 so that both builds read from a fixed place
    uint8_t dl = 0;
    if (lane < hdist) dl = s_lens[hlit + lane];
    vmx_wave_lds_fence();
    if (lane < 32) s_lens[288 + lane] = lane < hdist ? dl : (uint8_t)0;
    vmx_wave_lds_fence();
    if ((err = bzi_build(s_lens, hlit, T.CL, 1, lane)) != 0) return err;
    return bzi_build(s_lens + 288, hdist, T.CD, 2, lane);
}

#define GZ_TABS_DECL \
    __shared__ uint16_t s_ltab[1 << BZI_LIT_BITS]; \
    __shared__ uint16_t s_dtab[1 << BZI_DIST_BITS];                     /* (the code-length code's table while a dynamic header is read) */ \
    __shared__ uint16_t s_lsym[288], s_dsym[32]; \
    __shared__ uint8_t s_lens[320 + 32];                                /* literal / length and distance lengths; [320, 339): the code-length code's */ \
    __shared__ int s_cnt[2][16], s_nc[2][16], s_of[2][16]; \
    __shared__ uint32_t s_ring[BZI_RING]; \
    const GzTabs T{s_lens, BziCode{s_cnt[0], s_nc[0], s_of[0], s_lsym, s_ltab, BZI_LIT_BITS}, BziCode{s_cnt[1], s_nc[1], s_of[1], s_dsym, s_dtab, BZI_DIST_BITS}, \
                   BziCode{s_cnt[1], s_nc[1], s_of[1], s_dsym, s_dtab, 7}}

// ------------------------------------------------------------------------------------------------ k_gz_find
// cand[c]: the first bit in chunk c (bytes [c, c + 1) * chunk_bytes of the window), at or after min_bit, where a non-final dynamic block header is valid, or VMX_GZ_NONE.
// One wavefront per chunk, chunks first_chunk + blockIdx.x. 128 bits from the lane's position are in registers: 17 header bits and up to 19 x 3 bits of
// code-length code lengths, whose Kraft sum (in 1/128ths) must be exactly 128 — bzi_build's rule for kind 0: neither over-subscribed nor incomplete.
__global__ void __launch_bounds__(64) k_gz_find(const uint8_t* comp, uint32_t n_bytes, uint32_t chunk_bytes, uint32_t first_chunk, uint32_t min_bit, uint32_t* cand) {
    GZ_TABS_DECL;
    const int lane = (int)threadIdx.x;
    const uint32_t c = first_chunk + blockIdx.x;
    const uint64_t lo64 = (uint64_t)c * chunk_bytes * 8, hi64 = lo64 + (uint64_t)chunk_bytes * 8, end64 = (uint64_t)n_bytes * 8;
    const uint32_t end_bits = (uint32_t)end64;
    const uint32_t lo = (uint32_t)(lo64 > min_bit ? lo64 : min_bit), hi = (uint32_t)(hi64 < end64 ? hi64 : end64);
    BziIn in;
    in.w = (const uint32_t*)comp; in.n_words = (n_bytes + 3) >> 2; in.ring = s_ring;
    uint32_t found = VMX_GZ_NONE;
    for (uint32_t base = lo; base < hi && found == VMX_GZ_NONE; base += 64) {
        const uint32_t pos = base + (uint32_t)lane;
        bool ok = pos < hi && pos + 29 <= end_bits;                     // 17 bits and at least 4 code lengths
        if (ok) {
            const uint32_t wi = pos >> 5, sh = pos & 31;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = wi + k < in.n_words ? in.w[wi + k] : 0u;
            const uint64_t a = (uint64_t)w[0] | (uint64_t)w[1] << 32, b = (uint64_t)w[2] | (uint64_t)w[3] << 32;
            const uint64_t v0 = sh ? a >> sh | b << (64 - sh) : a, v1 = b >> sh;          // bits [0, 64) and [64, 128 - sh) from pos
            const uint32_t hclen = ((uint32_t)(v0 >> 13) & 15u) + 4u;
            ok = (v0 & 7u) == 4u && ((uint32_t)(v0 >> 3) & 31u) <= 29u && ((uint32_t)(v0 >> 8) & 31u) <= 29u && pos + 17 + 3 * hclen <= end_bits;
            if (ok) {
                const uint64_t x = v0 >> 17 | v1 << 47;                 // the code lengths: 57 bits at most
                uint32_t sum = 0;
#pragma unroll
                for (uint32_t i = 0; i < 19; ++i) { const uint32_t l = (uint32_t)(x >> (3 * i)) & 7u; if (i < hclen && l) sum += 128u >> l; }
                ok = sum == 128u;
            }
        }
        unsigned long long m = __ballot(ok);
        while (m) {
            const uint32_t p = base + (uint32_t)(__ffsll(m) - 1);
            m &= m - 1;
            gz_seek_bit(in, p, lane);
            bzi_ensure(in, lane);
            (void)bzi_take(in, 3);
            if (gz_dyn_header(in, end_bits, T, lane) == 0) { found = p; break; }
        }
    }
    if (lane == 0) cand[c] = found;
}

// ------------------------------------------------------------------------------------------------ k_gz_count / k_gz_decode

__device__ __forceinline__ uint32_t gz_byte(const uint8_t* comp, uint32_t p) { return bzi_u(comp[p]); }

// One wavefront. WRITE false: nothing is stored but *res. WRITE true: symbols to sym[0, W.n_sym), member ends to ev[0, W.n_ev).
template <bool WRITE>
__device__ __forceinline__ void gz_wave(const uint8_t* comp, uint32_t n_bytes, const vmx_gz_wave W, vmx_gz_res* res, uint16_t* out, vmx_gz_member* ev, const GzTabs& T,
                                        uint32_t* s_ring, int lane) {
    const uint32_t end_bits = n_bytes * 8u;
    BziIn in;
    in.w = (const uint32_t*)comp; in.n_words = (n_bytes + 3) >> 2; in.ring = s_ring;
    const BziCode& CL = T.CL; const BziCode& CD = T.CD;
    uint8_t* s_lens = T.lens;
    gz_seek_bit(in, W.start_bit, lane);
    uint32_t opos = 0, safe = 0, nl = 0, lit = 0, n_ev = 0, mstart = 0, blk_bit = W.start_bit, rflags = 0, end_bit = W.start_bit;
    bool known = (W.flags & VMX_GZ_F_HEADER) != 0, at_header = known, fixed_built = false, resume_hdr = known;
    uint32_t resume_bit = W.start_bit;                                   // the latest place a wave can begin at: a block's first bit or a member header
    int err = 0;
#define GZ_FAIL(code) do { err = (code); goto done; } while (0)
#define GZ_FLUSH() do { if (WRITE && (uint32_t)lane < nl) out[opos + lane] = (uint16_t)lit; opos += nl; nl = 0; } while (0)
    for (;;) {
        if (at_header) {
            // RFC 1952 2.3: ID1 ID2 CM FLG MTIME(4) XFL OS, then FEXTRA, FNAME, FCOMMENT, FHCRC. Zero bytes between members are padding (gzip(1) and Python's gzip skip them)
            // The stop rule is applied here too: a wave whose stop lies at or in front of this header ends at the header (R_HEADER), so that a
            // window can be cut between members. A candidate is never a header, so such an end links to nothing and the host moves the stop on.
            // The padding skip and the FNAME / FCOMMENT scans below read one wave-uniform byte per step: bounded by n_bytes, and accepted as
            // serial because headers are tens of bytes in real files (a false start reaches this branch only behind a final block and a trailer).
            uint32_t p = bzi_bitpos(in) >> 3;
            blk_bit = p * 8u; resume_bit = blk_bit; resume_hdr = true;
            if (blk_bit >= W.stop_bit) { end_bit = blk_bit; rflags |= VMX_GZ_R_HEADER; break; }
            while (p < n_bytes && gz_byte(comp, p) == 0) ++p;
            if (p >= n_bytes) { rflags |= VMX_GZ_R_END; end_bit = end_bits; break; }
            blk_bit = p * 8u;
            if (p + 10 > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
            if (gz_byte(comp, p) != 0x1f || gz_byte(comp, p + 1) != 0x8b) GZ_FAIL(VMX_GZ_E_MAGIC);
            if (gz_byte(comp, p + 2) != 8) GZ_FAIL(VMX_GZ_E_METHOD);
            const uint32_t flg = gz_byte(comp, p + 3);
            p += 10;
            if (flg & 4u) {
                if (p + 2 > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
                p += 2 + (gz_byte(comp, p) | gz_byte(comp, p + 1) << 8);
                if (p > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
            }
            for (uint32_t f = 8; f <= 16; f <<= 1)
                if (flg & f) {
                    while (p < n_bytes && gz_byte(comp, p) != 0) ++p;
                    if (p >= n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
                    ++p;
                }
            if (flg & 2u) { p += 2; if (p > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT); }
            bzi_seek(in, p, lane);
            at_header = false; known = true; mstart = opos;
        }
        const uint32_t bp = bzi_bitpos(in);
        end_bit = bp;
        if (bp >= W.stop_bit) break;
        blk_bit = bp; resume_bit = bp; resume_hdr = false;
        bzi_ensure(in, lane);
        if (bp + 3 > end_bits) GZ_FAIL(VMX_BGZF_E_INPUT);
        const uint32_t bfinal = bzi_take(in, 1), btype = bzi_take(in, 2);
        if (btype == 3) GZ_FAIL(VMX_BGZF_E_BTYPE);
        if (btype == 0) {
            GZ_FLUSH();
            (void)bzi_take(in, in.nb & 7);
            bzi_ensure(in, lane);
            const uint32_t len = bzi_take(in, 16);
            bzi_ensure(in, lane);
            const uint32_t nlen = bzi_take(in, 16);
            const uint32_t p = bzi_bitpos(in) >> 3;
            if (p > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
            if (len != (nlen ^ 0xffffu)) GZ_FAIL(VMX_BGZF_E_STORED);
            if (p + len > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
            if (opos > 0x7fff0000u) GZ_FAIL(VMX_GZ_E_BIG);
            if (WRITE) {
                if (opos + len > W.n_sym) GZ_FAIL(VMX_BGZF_E_LONG);
                const uint8_t* src = comp + p;
                for (uint32_t i = (uint32_t)lane; i < len; i += 64) out[opos + i] = (uint16_t)src[i];
            }
            opos += len;
            bzi_seek(in, p + len, lane);
        } else {
            if (btype == 1) {
                if (!fixed_built) {                                     // (a run of fixed blocks, as 2 000 empty members are, builds the tables once)
                    for (int i = lane; i < 288; i += 64) s_lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                    if (lane < 32) s_lens[288 + lane] = 5;
                    vmx_wave_lds_fence();
                    (void)bzi_build(s_lens, 288, CL, 3, lane);
                    (void)bzi_build(s_lens + 288, 32, CD, 3, lane);
                    fixed_built = true;
                }
            } else {
                fixed_built = false;
                if ((err = gz_dyn_header(in, end_bits, T, lane)) != 0) goto done;
            }
            for (;;) {
                bzi_ensure(in, lane);
                if (bzi_bitpos(in) > end_bits) GZ_FAIL(VMX_BGZF_E_INPUT);
                const int sy = bzi_decode(in, CL);
                if (sy < 0) GZ_FAIL(VMX_BGZF_E_CODE);
                if (sy < 256) {
                    if (WRITE && opos + nl >= W.n_sym) GZ_FAIL(VMX_BGZF_E_LONG);
                    if ((uint32_t)lane == nl) lit = (uint32_t)sy;
                    if (++nl == 64) GZ_FLUSH();
                    continue;
                }
                if (sy == 256) break;
                if (sy > 285) GZ_FAIL(VMX_BGZF_E_CODE);
                const int ls = sy - 257;
                uint32_t len;
                if (ls < 8) len = 3u + (uint32_t)ls;
                else if (ls == 28) len = 258;
                else { const uint32_t eb = (uint32_t)(ls >> 2) - 1u; len = 3u + ((4u + (uint32_t)(ls & 3)) << eb) + bzi_take(in, eb); }
                bzi_ensure(in, lane);
                const int ds = bzi_decode(in, CD);
                if (ds < 0 || ds > 29) GZ_FAIL(VMX_BGZF_E_CODE);
                uint32_t dist;
                if (ds < 4) dist = 1u + (uint32_t)ds;
                else { const uint32_t eb = (uint32_t)(ds >> 1) - 1u; dist = 1u + ((2u + (uint32_t)(ds & 1)) << eb) + bzi_take(in, eb); }
                if (bzi_bitpos(in) > end_bits) GZ_FAIL(VMX_BGZF_E_INPUT);
                GZ_FLUSH();
                if (known && dist > opos - mstart) GZ_FAIL(VMX_BGZF_E_DIST);
                if (opos > 0x7fff0000u) GZ_FAIL(VMX_GZ_E_BIG);
                if (WRITE) {
                    if (opos + len > W.n_sym) GZ_FAIL(VMX_BGZF_E_LONG);
                    // source symbol k of the match sits at s0 + k (k < dist; the copy repeats with period dist); below 0 lies the unknown window
                    const int32_t s0 = (int32_t)opos - (int32_t)dist;
                    if (s0 + (int32_t)(len < dist ? len : dist) > (int32_t)safe) { bzi_store_fence(); safe = opos; }
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64) {
                        const int32_t at = s0 + (int32_t)(dist >= len ? i : i % dist);
                        out[opos + i] = at < 0 ? (uint16_t)(VMX_GZ_MARK | (uint32_t)(VMX_GZ_WIN + at)) : out[at];
                    }
                }
                opos += len;
            }
        }
        if (bfinal) {
            GZ_FLUSH();
            (void)bzi_take(in, in.nb & 7);
            const uint32_t p = bzi_bitpos(in) >> 3;
            blk_bit = p * 8u;
            if (bzi_bitpos(in) > end_bits || p + 8 > n_bytes) GZ_FAIL(VMX_BGZF_E_INPUT);
            if (WRITE) {
                if (n_ev >= W.n_ev) GZ_FAIL(VMX_BGZF_E_LONG);
                uint32_t t[2];
                for (int k = 0; k < 2; ++k) t[k] = gz_byte(comp, p + 4 * k) | gz_byte(comp, p + 4 * k + 1) << 8 | gz_byte(comp, p + 4 * k + 2) << 16 | gz_byte(comp, p + 4 * k + 3) << 24;
                if (lane == 0) ev[n_ev] = vmx_gz_member{opos, t[0], t[1], p + 8};
            }
            ++n_ev;
            bzi_seek(in, p + 8, lane);
            at_header = true;
        }
    }
    GZ_FLUSH();
done:
    if (known) rflags |= VMX_GZ_R_MEMBER;
    if (resume_hdr) rflags |= VMX_GZ_R_RESUME_HDR;
    if (lane == 0) *res = vmx_gz_res{end_bit, (uint32_t)err, blk_bit, rflags, opos + nl, n_ev, opos + nl - mstart, resume_bit};
#undef GZ_FAIL
#undef GZ_FLUSH
}

// the count pass of the waves todo[blockIdx.x]: res[wave] = where it ended, what it would store, its error
__global__ void __launch_bounds__(64) k_gz_count(const uint8_t* comp, uint32_t n_bytes, const vmx_gz_wave* tab, const uint32_t* todo, vmx_gz_res* res) {
    GZ_TABS_DECL;
    const uint32_t w = todo[blockIdx.x];
    gz_wave<false>(comp, n_bytes, tab[w], res + w, nullptr, nullptr, T, s_ring, (int)threadIdx.x);
}

// the write pass of the linked waves (all of tab): symbols at sym + ooff, member ends at ev + eoff
__global__ void __launch_bounds__(64) k_gz_decode(const uint8_t* comp, uint32_t n_bytes, const vmx_gz_wave* tab, vmx_gz_res* res, uint16_t* sym, vmx_gz_member* ev) {
    GZ_TABS_DECL;
    const vmx_gz_wave W = tab[blockIdx.x];
    gz_wave<true>(comp, n_bytes, W, res + blockIdx.x, sym + W.ooff, ev + W.eoff, T, s_ring, (int)threadIdx.x);
}

// ------------------------------------------------------------------------------------------------ k_gz_window
// One workgroup. win0: the window in front of wave 0 (nullptr: nothing). win_in + k * VMX_GZ_WIN: the window in front of wave k; win_out: behind the last.
__global__ void __launch_bounds__(1024) k_gz_window(const uint16_t* sym, const vmx_gz_wave* tab, int64_t n_waves, const uint8_t* win0, uint8_t* win_in, uint8_t* win_out) {
    __shared__ gz_v16 s_w[2][VMX_GZ_WIN / 16];
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < VMX_GZ_WIN / 16; t += 1024) s_w[0][t] = win0 ? ((const gz_v16*)win0)[t] : gz_v16{0, 0, 0, 0};
    __syncthreads();
    for (int64_t k = 0; k < n_waves; ++k) {
        const int cur = (int)(k & 1);
        const uint8_t* w = (const uint8_t*)s_w[cur];
        uint8_t* nw = (uint8_t*)s_w[cur ^ 1];
        gz_v16* dst = (gz_v16*)(win_in + k * VMX_GZ_WIN);
        for (int t = tid; t < VMX_GZ_WIN / 16; t += 1024) dst[t] = s_w[cur][t];
        const uint32_t n = tab[k].n_sym;
        const uint16_t* s = sym + tab[k].ooff;
        for (uint32_t t = (uint32_t)tid; t < VMX_GZ_WIN; t += 1024) {
            const uint64_t idx = (uint64_t)n + t;                       // position in (window, the wave's text) of byte t of the last 32 KB
            uint32_t b;
            if (idx < VMX_GZ_WIN) b = w[idx];
            else { const uint32_t v = s[idx - VMX_GZ_WIN]; b = v & VMX_GZ_MARK ? w[v & (VMX_GZ_WIN - 1)] : v; }
            nw[t] = (uint8_t)b;
        }
        __syncthreads();
    }
    const int last = (int)(n_waves & 1);
    for (int t = tid; t < VMX_GZ_WIN / 16; t += 1024) ((gz_v16*)win_out)[t] = s_w[last][t];
}

// ------------------------------------------------------------------------------------------------ k_gz_resolve

__device__ __forceinline__ void gz_xor(uint32_t* p, uint32_t v) {
#ifdef VMX_EMU
    __atomic_fetch_xor(p, v, __ATOMIC_RELAXED);
#else
    atomicXor(p, v);
#endif
}

// Text bytes [P, P + 64) per lane, P = (blockIdx.x * 256 + threadIdx.x) * 64; sym, out: 16-byte aligned, 64 entries of slack behind `total`.
// ev_end[m]: text position where member m ends (non-decreasing; the open member's end, where the text ends inside one, is `total` or beyond).
// crc_acc[m] ^= crc(piece) * x^(8 * (ev_end[m] - piece's end)) for every piece of member m: after the launch it holds the member's CRC32
// (or, for a member that began in an earlier window, what has to be combined with the carried CRC).
// A marker that reaches before its member's start (tab[k].hist) is the first error by text position: err_key = atomicMin(position).
__global__ void __launch_bounds__(256) k_gz_resolve(const uint16_t* sym, const vmx_gz_wave* tab, int64_t n_waves, const uint8_t* win_in, const uint64_t* ev_end, int64_t n_ev,
                                                    int64_t total, vmx_crc_x2n x2n, uint8_t* out, uint32_t* crc_acc, unsigned long long* err_key) {
    __shared__ uint32_t crctab[256];
    __shared__ uint32_t s_x2n[32];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    { uint32_t c = (uint32_t)tid; for (int j = 0; j < 8; ++j) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1; crctab[tid] = c; }
    if (tid < 32) s_x2n[tid] = x2n.v[tid];
    __syncthreads();
    const int64_t P = ((int64_t)blockIdx.x * 256 + tid) * 64;
    const int64_t E = P + 64 < total ? P + 64 : total;
    // the wave that holds byte P: the last one whose ooff is at or below P (waves without text share their successor's ooff)
    int64_t k = 0;
    { int64_t a = 0, b = n_waves; while (b - a > 1) { const int64_t m = (a + b) >> 1; if (tab[m].ooff <= P) a = m; else b = m; } k = a; }
    int64_t kend = P < total ? tab[k].ooff + tab[k].n_sym : 0;
    uint32_t hist = P < total ? tab[k].hist : 0;
    // the member that holds byte P: the first one that ends behind P
    int64_t m = 0;
    { int64_t a = 0, b = n_ev; while (a < b) { const int64_t h = (a + b) >> 1; if ((int64_t)ev_end[h] <= P) a = h + 1; else b = h; } m = a; }
    int64_t mend = m < n_ev ? (int64_t)ev_end[m] : INT64_MAX;
    uint32_t c = 0xffffffffu;
    uint32_t first_c = 0; int64_t first_m = -1, first_end = 0; int n_flush = 0;
    unsigned long long bad = ~0ull;
    for (int q = 0; q < 4; ++q) {
        const int64_t Q = P + 16 * q;
        if (Q >= total) break;
        const gz_v16 sa = ((const gz_v16*)(sym + Q))[0], sb = ((const gz_v16*)(sym + Q))[1];
        const uint32_t sw[8] = {sa.x, sa.y, sa.z, sa.w, sb.x, sb.y, sb.z, sb.w};
        uint32_t ow[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int64_t pos = Q + i;
            if (pos < E) {
                while (pos >= kend) { ++k; kend = tab[k].ooff + tab[k].n_sym; hist = tab[k].hist; }
                while (pos >= mend) { ++m; mend = m < n_ev ? (int64_t)ev_end[m] : INT64_MAX; }
                const uint32_t v = (sw[i >> 1] >> (16 * (i & 1))) & 0xffffu;
                uint32_t b = v;
                if (v & VMX_GZ_MARK) {
                    const uint32_t j = v & (VMX_GZ_WIN - 1);
                    if (j < VMX_GZ_WIN - hist && bad == ~0ull) bad = (unsigned long long)pos;
                    b = win_in[k * VMX_GZ_WIN + j];
                }
                ow[i >> 2] |= b << (8 * (i & 3));
                c = crctab[(c ^ b) & 0xff] ^ (c >> 8);
                if (pos + 1 == E || pos + 1 == mend) {                  // a piece ends: with the lane's bytes or with the member
                    if (n_flush == 0) { first_c = ~c; first_m = m; first_end = pos + 1; }
                    else if (m < n_ev) gz_xor(crc_acc + m, crc_multmodp(crc_x8n(s_x2n, (uint32_t)(mend - (pos + 1))), ~c));
                    ++n_flush; c = 0xffffffffu;
                }
            }
        }
        *(gz_v16*)(out + Q) = gz_v16{ow[0], ow[1], ow[2], ow[3]};
    }
    if (bad != ~0ull) atomicMin(err_key, bad);
    // the lane's first piece: where the whole wave's 4 096 bytes are one piece each of one member, the 64 partials are combined first
    const int64_t m0 = vmx_uniform_i64(__shfl(first_m, 0));
    const bool simple = n_flush == 1 && first_end == P + 64 && first_m == m0 && first_m < n_ev;
    if (__all(simple)) {
        uint32_t part = crc_multmodp(crc_x8n(s_x2n, (uint32_t)(63 - lane) * 64u), first_c);
        for (int o = 32; o; o >>= 1) part ^= __shfl_xor(part, o);
        if (lane == 0) gz_xor(crc_acc + m0, crc_multmodp(crc_x8n(s_x2n, (uint32_t)((int64_t)ev_end[m0] - (P + 64 * 64))), part));
    } else if (n_flush && first_m >= 0 && first_m < n_ev) {
        gz_xor(crc_acc + first_m, crc_multmodp(crc_x8n(s_x2n, (uint32_t)((int64_t)ev_end[first_m] - first_end)), first_c));
    }
}
