// k_bam_in.hip — BAM input on the device (SAMv1 §4.1 BGZF, §4.2 records; RFC 1951).
//
// Inflate: one BGZF member per wavefront (workgroups of one wave). The host has walked the member headers (vmx_bam.hip) and hands over a
// table of (deflate data, its size, ISIZE, CRC32, output offset): members inflate independently into one contiguous buffer, and a member's
// window is its own output, so there is no LDS window. The decoder's state (bit buffer, cursors, the symbol in hand) is the same in every
// lane and is read back through vmx_uniform_i32, so it lives in scalar registers; the lanes differ only in what they load and store:
//   * compressed input: 512 bytes at a time into an LDS ring (one coalesced load), words from there into a 64-bit bit buffer;
//   * Huffman tables (per wave in LDS; the kernel uses 4 960 B in all): code-length counts by LDS atomics, every symbol's rank among the symbols of its
//     length by 15 ballots per 64 symbols, canonical codes from there; a primary table of 10 (literal / length) or 9 (distance) bits is
//     filled by all lanes, longer codes (rare: the primary table covers every code of probability above 2^-10) are decoded canonically,
//     bit by bit, from the per-length counts and the symbols sorted by (length, symbol);
//   * literals are staged one per lane in a register and stored 64 at a time; a match is copied by all lanes, 64 bytes per step.
// THE ORDERING RULE OF THE MATCH COPY: a back-reference reads bytes this wave stored a moment ago, mostly from other lanes. The compiler
// orders a work-item's own store -> load, not lane 3's store -> lane 7's load. bzi_store_fence() (release fence, s_waitcnt vmcnt(0): every
// store of the wave has been acknowledged; acquire fence) stands between the stores and the copy's loads whenever the source range reaches
// beyond `safe`, the output position of the latest fence; sources below it were complete before the loads were issued. dist < len copies
// read src[i mod dist]: every source byte lies below the match's first byte, none is written by the copy itself.
// Every input read is bounded by the member's deflate size, every output write by its ISIZE, every distance by the bytes produced so far.
// Code-length sets are accepted exactly where zlib's inflate_table accepts them. The first bad member wins (atomicMin on member << 8 | code).
//
// Records: k_bam_in_walk follows the block_size chain (serial by nature: one dependent load per record), k_bam_in_sizes sizes every
// record's name, bases and qualities, and after four scans (names, bases, qualities, kept records) k_bam_in_decode writes them, one wave per record, 64 bases per step.
// Auxiliary fields (only when tags were asked for): k_bam_in_aux_size / k_bam_in_aux_write, at the end of this file.
#include "vmx_bam.h"
#include "k_inflate_dev.h"                // BziIn, bzi_build, bzi_decode, bzi_store_fence, bzi_cl_order: shared with k_gzip_in.hip

__global__ void __launch_bounds__(64) k_bgzf_inflate(const uint8_t* comp, const vmx_bgzf_member* tab, int64_t n_members, uint8_t* out_all, vmx_crc_x2n x2n,
                                                     unsigned long long* err_key) {
    __shared__ uint16_t s_ltab[1 << BZI_LIT_BITS];                      // (the CRC table and x^(2^k) lie over it once the last block is decoded)
    __shared__ uint16_t s_dtab[1 << BZI_DIST_BITS];                     // (the code-length code's table while a dynamic header is read)
    __shared__ uint16_t s_lsym[288], s_dsym[32];
    __shared__ uint8_t s_lens[320 + 32];                                // literal / length and distance lengths; [320, 339): the code-length code's
    __shared__ int s_cnt[2][16], s_nc[2][16], s_of[2][16];
    __shared__ uint32_t s_ring[BZI_RING];
    const int lane = (int)threadIdx.x;
    const int64_t mb = blockIdx.x;
    if (mb >= n_members) return;
    const vmx_bgzf_member M = tab[mb];
    uint8_t* out = out_all + M.ooff;
    const uint32_t isize = M.isize;
    const uint8_t* cdata = comp + M.coff;
    const uint32_t a = (uint32_t)((uintptr_t)cdata & 3);
    const uint32_t end_byte = a + (uint32_t)M.csize;                    // the deflate data: bytes [a, end_byte) of the words
    BziIn in;
    in.w = (const uint32_t*)(cdata - a); in.n_words = (end_byte + 3) >> 2; in.ring = s_ring;
    const BziCode CL{s_cnt[0], s_nc[0], s_of[0], s_lsym, s_ltab, BZI_LIT_BITS};
    const BziCode CD{s_cnt[1], s_nc[1], s_of[1], s_dsym, s_dtab, BZI_DIST_BITS};
    const BziCode CC{s_cnt[1], s_nc[1], s_of[1], s_dsym, s_dtab, 7};
    bzi_seek(in, a, lane);
    uint32_t opos = 0, safe = 0, nl = 0, lit = 0;
    int err = 0;
#define BZI_FAIL(code) do { err = (code); goto done; } while (0)
#define BZI_FLUSH() do { if ((uint32_t)lane < nl) out[opos + lane] = (uint8_t)lit; opos += nl; nl = 0; } while (0)
    for (;;) {
        bzi_ensure(in, lane);
        if (bzi_bitpos(in) + 3 > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
        const uint32_t bfinal = bzi_take(in, 1), btype = bzi_take(in, 2);
        if (btype == 3) BZI_FAIL(VMX_BGZF_E_BTYPE);
        if (btype == 0) {
            BZI_FLUSH();
            (void)bzi_take(in, in.nb & 7);
            bzi_ensure(in, lane);
            const uint32_t len = bzi_take(in, 16);
            bzi_ensure(in, lane);
            const uint32_t nlen = bzi_take(in, 16);
            const uint32_t p = bzi_bitpos(in) >> 3;
            if (p > end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
            if (len != (nlen ^ 0xffffu)) BZI_FAIL(VMX_BGZF_E_STORED);
            if (p + len > end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
            if (opos + len > isize) BZI_FAIL(VMX_BGZF_E_LONG);
            const uint8_t* src = (const uint8_t*)in.w + p;
            for (uint32_t i = (uint32_t)lane; i < len; i += 64) out[opos + i] = src[i];
            opos += len;
            bzi_seek(in, p + len, lane);
        } else {
            if (btype == 1) {
                for (int i = lane; i < 288; i += 64) s_lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                if (lane < 32) s_lens[288 + lane] = 5;
                vmx_wave_lds_fence();
                (void)bzi_build(s_lens, 288, CL, 3, lane);
                (void)bzi_build(s_lens + 288, 32, CD, 3, lane);
            } else {
                bzi_ensure(in, lane);
                const int hlit = (int)bzi_take(in, 5) + 257, hdist = (int)bzi_take(in, 5) + 1, hclen = (int)bzi_take(in, 4) + 4;
                if (hlit > 286 || hdist > 30) BZI_FAIL(VMX_BGZF_E_HEADER);
                if (lane < 19) s_lens[320 + lane] = 0;
                vmx_wave_lds_fence();
                for (int i = 0; i < hclen; ++i) {
                    bzi_ensure(in, lane);
                    const uint32_t v = bzi_take(in, 3);
                    if (lane == 0) s_lens[320 + bzi_cl_order[i]] = (uint8_t)v;
                }
                vmx_wave_lds_fence();
                if (bzi_bitpos(in) > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
                if ((err = bzi_build(s_lens + 320, 19, CC, 0, lane)) != 0) goto done;
                int have = 0, prev = 0;
                const int want = hlit + hdist;
                while (have < want) {
                    bzi_ensure(in, lane);
                    const int sy = bzi_decode(in, CC);
                    if (sy < 0) BZI_FAIL(VMX_BGZF_E_HEADER);
                    int rep = 1, val = sy;
                    if (sy == 16) { if (have == 0) BZI_FAIL(VMX_BGZF_E_HEADER); val = prev; rep = 3 + (int)bzi_take(in, 2); }
                    else if (sy == 17) { val = 0; rep = 3 + (int)bzi_take(in, 3); }
                    else if (sy == 18) { val = 0; rep = 11 + (int)bzi_take(in, 7); }
                    if (have + rep > want) BZI_FAIL(VMX_BGZF_E_HEADER);
                    if (lane < rep) s_lens[have + lane] = (uint8_t)val;
                    if (lane + 64 < rep) s_lens[have + lane + 64] = (uint8_t)val;
                    if (lane + 128 < rep) s_lens[have + lane + 128] = (uint8_t)val;
                    have += rep; prev = val;
                    if (bzi_bitpos(in) > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
                }
                vmx_wave_lds_fence();
                if (vmx_uniform_i32(s_lens[256]) == 0) BZI_FAIL(VMX_BGZF_E_HEADER);        // no end-of-block code
                // the distance lengths move behind slot 288 so that both builds read from a fixed place
                uint8_t dl = 0;
                if (lane < hdist) dl = s_lens[hlit + lane];
                vmx_wave_lds_fence();
                if (lane < 32) s_lens[288 + lane] = lane < hdist ? dl : (uint8_t)0;
                vmx_wave_lds_fence();
                if ((err = bzi_build(s_lens, hlit, CL, 1, lane)) != 0) goto done;
                if ((err = bzi_build(s_lens + 288, hdist, CD, 2, lane)) != 0) goto done;
            }
            for (;;) {
                bzi_ensure(in, lane);
                if (bzi_bitpos(in) > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
                const int sy = bzi_decode(in, CL);
                if (sy < 0) BZI_FAIL(VMX_BGZF_E_CODE);
                if (sy < 256) {
                    if (opos + nl >= isize) BZI_FAIL(VMX_BGZF_E_LONG);
                    if ((uint32_t)lane == nl) lit = (uint32_t)sy;
                    if (++nl == 64) BZI_FLUSH();
                    continue;
                }
                if (sy == 256) break;
                if (sy > 285) BZI_FAIL(VMX_BGZF_E_CODE);
                const int ls = sy - 257;
                uint32_t len;
                if (ls < 8) len = 3u + (uint32_t)ls;
                else if (ls == 28) len = 258;
                else { const uint32_t eb = (uint32_t)(ls >> 2) - 1u; len = 3u + ((4u + (uint32_t)(ls & 3)) << eb) + bzi_take(in, eb); }
                bzi_ensure(in, lane);
                const int ds = bzi_decode(in, CD);
                if (ds < 0 || ds > 29) BZI_FAIL(VMX_BGZF_E_CODE);
                uint32_t dist;
                if (ds < 4) dist = 1u + (uint32_t)ds;
                else { const uint32_t eb = (uint32_t)(ds >> 1) - 1u; dist = 1u + ((2u + (uint32_t)(ds & 1)) << eb) + bzi_take(in, eb); }
                if (bzi_bitpos(in) > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
                BZI_FLUSH();
                if (dist > opos) BZI_FAIL(VMX_BGZF_E_DIST);
                if (opos + len > isize) BZI_FAIL(VMX_BGZF_E_LONG);
                const uint32_t s0 = opos - dist;
                if (s0 + (len < dist ? len : dist) > safe) { bzi_store_fence(); safe = opos; }
                if (dist >= len) {
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64) out[opos + i] = out[s0 + i];
                } else {
                    for (uint32_t i = (uint32_t)lane; i < len; i += 64) out[opos + i] = out[s0 + i % dist];
                }
                opos += len;
            }
        }
        if (bfinal) break;
    }
    BZI_FLUSH();
    if (bzi_bitpos(in) > 8 * end_byte) BZI_FAIL(VMX_BGZF_E_INPUT);
    if (((bzi_bitpos(in) + 7) >> 3) != end_byte) BZI_FAIL(VMX_BGZF_E_TAIL);
    if (opos != isize) BZI_FAIL(VMX_BGZF_E_SHORT);
    {
        // CRC32 of the output: 64 chunks, combined as the deflate kernel combines its own (vmx_bam.h)
        uint32_t* crctab = (uint32_t*)s_ltab;
        uint32_t* s_x2n = crctab + 256;
        vmx_wave_lds_fence();
        for (int k = lane; k < 256; k += 64) { uint32_t c = (uint32_t)k; for (int j = 0; j < 8; ++j) c = c & 1 ? (c >> 1) ^ CRC_POLY : c >> 1; crctab[k] = c; }
        if (lane < 32) s_x2n[lane] = x2n.v[lane];
        bzi_store_fence();                                              // (the LDS stores too: __syncthreads in the emulator, program order on the device)
        vmx_wave_lds_fence();
        const uint32_t chunk = (isize + 63) / 64;
        const uint32_t b = (uint32_t)lane * chunk < isize ? (uint32_t)lane * chunk : isize, e = b + chunk < isize ? b + chunk : isize;
        uint32_t part = 0;
        if (b < e) {
            uint32_t c = 0xffffffffu;
            uint32_t i = b;
            for (; i + 8 <= e; i += 8) {                                    // eight loads in flight, then the dependent table look-ups
                uint8_t v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = out[i + k];
#pragma unroll
                for (int k = 0; k < 8; ++k) c = crctab[(c ^ v[k]) & 0xff] ^ (c >> 8);
            }
            for (; i < e; ++i) c = crctab[(c ^ out[i]) & 0xff] ^ (c >> 8);
            part = crc_multmodp(crc_x8n(s_x2n, isize - e), ~c);
        }
        for (int o = 32; o; o >>= 1) part ^= __shfl_xor(part, o);
        if (part != M.crc) err = VMX_BGZF_E_CRC;
    }
done:
    if (err && lane == 0) atomicMin(err_key, (unsigned long long)mb << 8 | (unsigned long long)err);
#undef BZI_FAIL
#undef BZI_FLUSH
}

// ------------------------------------------------------------------------------------------------ records

__device__ __forceinline__ uint32_t bin_u32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// records [begin, ...) of buf: roff[i] = offset of record i, until the next one is not complete below `end`. A block_size below 32 or
// smaller than what l_read_name, n_cigar_op and l_seq need, or above VMX_BAM_IN_MAX_RECORD, ends the walk with an error (record << 8 | code). One work-item: the chain
// block_size -> next record is serial; the loads of one record's fields are independent of each other.
__global__ void k_bam_in_walk(const uint8_t* buf, int64_t begin, int64_t end, int64_t max_rec, int64_t* roff, vmx_bam_in_walk* res) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    VMX_SETPRIO(3);
    int64_t p = begin, n = 0;
    uint64_t bad = ~0ull;
    while (p + 36 <= end && n < max_rec) {
        const uint8_t* r = buf + p;
        const int64_t bs = (int64_t)bin_u32(r);
        const int64_t l_name = r[12], n_cig = (int64_t)r[16] | (int64_t)r[17] << 8, l_seq = (int64_t)bin_u32(r + 20);
        if (bs < 32 || bs > VMX_BAM_IN_MAX_RECORD || l_name < 1 || l_seq > 0x7fffffff || 32 + l_name + 4 * n_cig + (l_seq + 1) / 2 + l_seq > bs) { bad = (uint64_t)n << 8 | VMX_BAM_IN_E_SIZE; break; }
        if (p + 4 + bs > end) break;
        roff[n++] = p;
        p += 4 + bs;
    }
    roff[n] = p;
    res->n_rec = n; res->end = p; res->err_key = bad;
}

// per record: bytes of its name, bases and qualities; keep = 0 for a record without bases (dropped, as the reference skips it)
__global__ void __launch_bounds__(256) k_bam_in_sizes(const uint8_t* buf, const int64_t* roff, int64_t n, int64_t* nsz, int64_t* ssz, int64_t* qsz, int64_t* keep) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > n) return;
    if (i == n) { nsz[i] = 0; ssz[i] = 0; qsz[i] = 0; keep[i] = 0; return; }        // (the scans' totals land here)
    const uint8_t* r = buf + roff[i];
    const int64_t l_name = r[12], n_cig = (int64_t)r[16] | (int64_t)r[17] << 8, l_seq = (int64_t)bin_u32(r + 20);
    const bool k = l_seq > 0;
    const uint8_t* q = r + 36 + l_name + 4 * n_cig + (l_seq + 1) / 2;
    nsz[i] = k ? l_name - 1 : 0; ssz[i] = k ? l_seq : 0; qsz[i] = k && q[0] != 0xff ? l_seq : 0; keep[i] = k ? 1 : 0;
}

// one wave per record. noff / soff / qoff / kidx: exclusive scans of k_bam_in_sizes' columns (n + 1 entries); the kept records' offsets go to
// out_*off[kidx], the totals to out_*off[kidx[n]]. A reverse-strand record (flag & 16) is turned back to the read's own orientation:
// bases reversed with A <-> T, C <-> G and every other letter kept, qualities reversed.
__global__ void __launch_bounds__(256) k_bam_in_decode(const uint8_t* buf, const int64_t* roff, int64_t n, const int64_t* noff, const int64_t* soff, const int64_t* qoff,
                                                       const int64_t* kidx, char* names, char* seqs, char* quals, int64_t* out_noff, int64_t* out_soff, int64_t* out_qoff) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (i > n) return;
    const int64_t k = kidx[i];
    if (i == n) { if (lane == 0) { out_noff[k] = noff[n]; out_soff[k] = soff[n]; out_qoff[k] = qoff[n]; } return; }
    if (kidx[i + 1] == k) return;                                       // dropped
    const uint8_t* r = buf + roff[i];
    const int64_t l_name = r[12], n_cig = (int64_t)r[16] | (int64_t)r[17] << 8, l_seq = (int64_t)bin_u32(r + 20);
    const bool rev = (r[18] & 16) != 0;
    const int64_t no = noff[i], so = soff[i], qo = qoff[i];
    if (lane == 0) { out_noff[k] = no; out_soff[k] = so; out_qoff[k] = qo; }
    for (int64_t j = lane; j < l_name - 1; j += 64) names[no + j] = (char)r[36 + j];
    const uint8_t* sq = r + 36 + l_name + 4 * n_cig;
    const uint8_t* qu = sq + (l_seq + 1) / 2;
    const bool hasq = qoff[i + 1] != qo;
    const uint64_t fwd_lo = 0x565352474d43413dull, fwd_hi = 0x4e42444b48595754ull;      // "=ACMGRSV" "TWYHKDBN", first letter in the low byte
    const uint64_t rc_lo = 0x565352434d47543dull, rc_hi = 0x4e42444b48595741ull;       // "=TGMCRSV" "AWYHKDBN"
    const uint64_t lo = rev ? rc_lo : fwd_lo, hi = rev ? rc_hi : fwd_hi;
    for (int64_t j = lane; j < l_seq; j += 64) {
        const uint32_t b = sq[j >> 1];
        const uint32_t c = j & 1 ? b & 15u : b >> 4;
        const int64_t at = rev ? l_seq - 1 - j : j;
        seqs[so + at] = (char)((c < 8 ? lo >> (8 * c) : hi >> (8 * (c - 8))) & 0xff);
        if (hasq) quals[qo + at] = (char)(qu[j] + 33);
    }
}

// ------------------------------------------------------------------------------------------------ auxiliary fields -> SAM text
// k_bam_in_aux_size / k_bam_in_aux_write: the aux region of a record (SAMv1 §4.2.4: tag[2] type[1] value, from the end of the qualities to the
// end of block_size) as the tab-separated `XX:T:value` text the emitters take as a read's comment. One wave per record, launched only when
// tags were asked for; the size pass is the write pass without its stores (one body, bax_record<WRITE>). The field chain is serial and
// wave-uniform (cursor, tag, type, count: scalar registers); what is inside a field belongs to the wave: the NUL of a Z / H value is found
// by ballot, 64 bytes per step, with the printable / hex check in the same ballots; a B array is taken 64 elements per step, every lane
// making the text of its own element in two 64-bit registers (`,` sign digits: at most 16 bytes), a 32-bit wave scan placing them.
// A float's text is the shortest %.{p}g, p = 1 ... 9, that strtod followed by a cast reads back as the same float32: exact integer
// arithmetic on a fixed 320-bit integer (bax_scaled), no floating point at all, so that BAM in -> BAM out keeps the bits.
// WHAT BOUNDS EVERY ACCESS: a load is made at an offset below the record's end (4 + block_size, which k_bam_in_walk has checked against the
// window) only after the field's extent has been compared with that end; a store is made at an offset that the size pass's arithmetic,
// repeated here on the same bytes, has summed into the record's allotment coff[i + 1] - coff[i]; a record whose allotment is 0 (nothing
// selected, or malformed) stores nothing. ORDERING: whether a field is kept or dropped needs a sweep over its value; the write pass makes
// that sweep again on the input rather than taking a flag from the size pass, and no lane loads a byte that this launch stored, so
// there is no store -> load ordering to keep and bzi_store_fence() is not needed here.
// The first malformed record wins (atomicMin on record << 8 | code); fields that SAM text cannot express are left out and counted.

struct BaxText { uint64_t lo, hi; int len; };       // up to 16 characters, the first in lo's low byte

__device__ __forceinline__ void bax_put(BaxText& t, int pos, uint32_t c) { if (pos < 8) t.lo |= (uint64_t)c << (8 * pos); else t.hi |= (uint64_t)c << (8 * (pos - 8)); }
__device__ __forceinline__ uint32_t bax_get(const BaxText& t, int pos) { return (uint32_t)((pos < 8 ? t.lo >> (8 * pos) : t.hi >> (8 * (pos - 8))) & 0xffu); }
__device__ __forceinline__ int bax_ndig(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
// the nd decimal digits of v (leading zeros where v has fewer) at positions [at, at + nd)
__device__ __forceinline__ void bax_digits(BaxText& t, int at, uint32_t v, int nd) { for (int k = nd - 1; k >= 0; --k) { bax_put(t, at + k, '0' + v % 10u); v /= 10u; } }

__device__ __forceinline__ BaxText bax_int(int64_t v, bool comma) {
    BaxText t{0, 0, 0};
    int at = 0;
    if (comma) bax_put(t, at++, ',');
    if (v < 0) bax_put(t, at++, '-');
    const uint32_t a = (uint32_t)(v < 0 ? -v : v);
    const int nd = bax_ndig(a);
    bax_digits(t, at, a, nd);
    t.len = at + nd;
    return t;
}

#define BAX_W 10                        // 320 bits: a 55-bit integer times 10^62 is the largest value held
struct BaxBig { uint32_t w[BAX_W]; };   // (indexed by unrolled loops only: registers, no scratch)
__device__ __forceinline__ void bax_mul(BaxBig& b, uint32_t f) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < BAX_W; ++i) { c += (uint64_t)b.w[i] * f; b.w[i] = (uint32_t)c; c >>= 32; }
}
__device__ __forceinline__ uint32_t bax_div(BaxBig& b, uint32_t d) {
    uint64_t r = 0;
#pragma unroll
    for (int i = BAX_W - 1; i >= 0; --i) { r = r << 32 | b.w[i]; b.w[i] = (uint32_t)(r / d); r %= d; }
    return (uint32_t)r;
}
__device__ __forceinline__ void bax_shl(BaxBig& b, int n) {
    for (; n >= 32; n -= 32) {
#pragma unroll
        for (int i = BAX_W - 1; i >= 1; --i) b.w[i] = b.w[i - 1];
        b.w[0] = 0;
    }
    if (n) {
#pragma unroll
        for (int i = BAX_W - 1; i >= 1; --i) b.w[i] = b.w[i] << n | b.w[i - 1] >> (32 - n);
        b.w[0] <<= n;
    }
}
// true when a set bit was shifted out
__device__ __forceinline__ bool bax_shr(BaxBig& b, int n) {
    uint32_t lost = 0;
    for (; n >= 32; n -= 32) {
        lost |= b.w[0];
#pragma unroll
        for (int i = 0; i < BAX_W - 1; ++i) b.w[i] = b.w[i + 1];
        b.w[BAX_W - 1] = 0;
    }
    if (n) {
        lost |= b.w[0] & ((1u << n) - 1u);
#pragma unroll
        for (int i = 0; i < BAX_W - 1; ++i) b.w[i] = b.w[i] >> n | b.w[i + 1] << (32 - n);
        b.w[BAX_W - 1] >>= n;
    }
    return lost != 0;
}
// floor(N * 2^q * 10^s), which the callers know to be below 2^64; *sticky: the exact value is not an integer
__device__ static uint64_t bax_scaled(uint64_t N, int q, int s, bool* sticky) {
    BaxBig b;
#pragma unroll
    for (int i = 2; i < BAX_W; ++i) b.w[i] = 0;
    b.w[0] = (uint32_t)N; b.w[1] = (uint32_t)(N >> 32);
    bool st = false;
    if (s >= 0) {
        for (; s >= 9; s -= 9) bax_mul(b, 1000000000u);
        uint32_t f = 1;
        for (; s > 0; --s) f *= 10u;
        bax_mul(b, f);
        if (q >= 0) bax_shl(b, q); else st = bax_shr(b, -q);
    } else {
        if (q >= 0) bax_shl(b, q); else st = bax_shr(b, -q);
        s = -s;
        for (; s >= 9; s -= 9) st |= bax_div(b, 1000000000u) != 0;
        uint32_t f = 1;
        for (; s > 0; --s) f *= 10u;
        st |= bax_div(b, f) != 0;
    }
    *sticky = st;
    return (uint64_t)b.w[0] | (uint64_t)b.w[1] << 32;
}

// a finite float32 as the shortest %.{p}g (p = 1 ... 9) that reads back: the value is m * 2^e exactly; V = its first 18 decimal digits
// (and whether more follow) gives every p's correctly rounded candidate (ties to even); a candidate reads back when strtod's double lands
// where the cast to float32 gives the value again, i.e. between the midpoints to the neighbouring floats, moved by half a double ulp
// (outwards and inclusive for an even m, where both roundings tie towards it, inwards and exclusive for an odd m). Those two bounds
// are dyadic too and go through the same scaling, so the test is a comparison of 64-bit integers.
__device__ static BaxText bax_float(uint32_t bits, bool comma) {
    BaxText t{0, 0, 0};
    int at = 0;
    if (comma) bax_put(t, at++, ',');
    if (bits >> 31) bax_put(t, at++, '-');
    const uint32_t ex = (bits >> 23) & 0xffu, fr = bits & 0x7fffffu;
    if (ex == 0 && fr == 0) { bax_put(t, at++, '0'); t.len = at; return t; }
    const uint32_t m = ex ? fr | 0x800000u : fr;
    const int e = ex ? (int)ex - 150 : -149;
    const int k = 31 - __clz((int)m) + e;                               // floor(log2 x)
    int E = (k * 78913) >> 18;                                          // floor(k log10 2): floor(log10 x) or one less
    bool sx, sl, su;
    uint64_t V = bax_scaled(m, e, 17 - E, &sx);
    if (V >= 1000000000000000000ull) { ++E; sx |= V % 10u != 0; V /= 10u; }
    const bool low_edge = fr == 0 && ex > 1;                            // a power of two: the floats below are spaced half as wide
    const uint64_t Ml = low_edge ? 4ull * m - 1 : 2ull * m - 1, Mh = 2ull * m + 1;
    const int gl = low_edge ? e - 2 : e - 1, gh = e - 1;
    const int bl = 64 - __clzll((long long)Ml), bh = 64 - __clzll((long long)Mh);
    const bool even = (m & 1u) == 0;
    const uint64_t TL = bax_scaled((Ml << (54 - bl)) + (even ? ~0ull : 1ull), gl + bl - 54, 17 - E, &sl);
    const uint64_t TU = bax_scaled((Mh << (54 - bh)) + (even ? 1ull : ~0ull), gh + bh - 54, 17 - E, &su);
    const uint64_t lo_ok = even ? TL + (sl ? 1u : 0u) : TL + 1u, hi_ok = even ? TU : TU - (su ? 0u : 1u);      // a candidate C reads back: lo_ok <= C <= hi_ok
    uint64_t q = 0, pw = 100000000000000000ull, tp = 10;               // 10^(18 - p), 10^p
    int p = 1;
    for (;; ++p, pw /= 10u, tp *= 10u) {
        q = V / pw;
        const uint64_t rem = V % pw, half = pw / 2u;
        if (rem > half || (rem == half && (sx || (q & 1u)))) ++q;
        const uint64_t C = q * pw;
        if ((C >= lo_ok && C <= hi_ok) || p == 9) break;
    }
    int X = E;
    if (q == tp) { q /= 10u; ++X; }
    int L = p;
    uint32_t d = (uint32_t)q;
    while (L > 1 && d % 10u == 0) { d /= 10u; --L; }
    if (X < -4 || X >= p) {                                             // d.ddde+XX
        uint32_t pl = 1;
        for (int i = 1; i < L; ++i) pl *= 10u;
        bax_put(t, at++, '0' + d / pl);
        if (L > 1) { bax_put(t, at++, '.'); bax_digits(t, at, d % pl, L - 1); at += L - 1; }
        bax_put(t, at++, 'e'); bax_put(t, at++, X < 0 ? '-' : '+');
        bax_digits(t, at, (uint32_t)(X < 0 ? -X : X), 2); at += 2;
    } else if (X >= 0) {
        const int ip = X + 1;                                           // digits before the point
        if (L <= ip) {
            bax_digits(t, at, d, L); at += L;
            for (int i = L; i < ip; ++i) bax_put(t, at++, '0');
        } else {
            uint32_t pl = 1;
            for (int i = ip; i < L; ++i) pl *= 10u;
            bax_digits(t, at, d / pl, ip); at += ip;
            bax_put(t, at++, '.');
            bax_digits(t, at, d % pl, L - ip); at += L - ip;
        }
    } else {
        bax_put(t, at++, '0'); bax_put(t, at++, '.');
        for (int i = -1; i > X; --i) bax_put(t, at++, '0');
        bax_digits(t, at, d, L); at += L;
    }
    t.len = at;
    return t;
}

template <bool WRITE>
__device__ __forceinline__ void bax_record(const uint8_t* buf, const int64_t* roff, int64_t n, const uint16_t* sel, int n_sel, int all, const int64_t* coff, const int64_t* kidx,
                                           int64_t* csz, char* out, int64_t* out_coff, unsigned long long* err_key, unsigned long long* n_drop) {
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = (int)(threadIdx.x & 63);
    if (i > n) return;
    if (i == n) {
        if (lane == 0) { if (WRITE) out_coff[kidx[n]] = coff[n]; else csz[n] = 0; }
        return;
    }
    const uint8_t* r = buf + vmx_uniform_i64(roff[i]);
    const uint32_t bs = bzi_u(bin_u32(r)), l_name = bzi_u(r[12]), n_cig = bzi_u((uint32_t)r[16] | (uint32_t)r[17] << 8), l_seq = bzi_u(bin_u32(r + 20));
    if (l_seq == 0) { if (!WRITE && lane == 0) csz[i] = 0; return; }      // a dropped record: its aux bytes are never looked at
    char* o = nullptr;
    if (WRITE) {
        const int64_t at = coff[i];
        if (lane == 0) out_coff[kidx[i]] = at;
        if (coff[i + 1] == at) return;                                  // nothing to write
        o = out + at;
    }
    uint32_t p = 36u + l_name + 4u * n_cig + (l_seq + 1u) / 2u + l_seq;   // (k_bam_in_walk: p <= end)
    const uint32_t end = 4u + bs;
    uint32_t w = 0, drops = 0;
    int err = 0;
#define BAX_PREFIX(tc) do { \
        const uint32_t tab_ = w ? 1u : 0u; \
        if (WRITE && (uint32_t)lane < 5u + tab_) { const int j_ = lane - (int)tab_; o[w + lane] = (char)(j_ < 0 ? '\t' : j_ == 0 ? t0 : j_ == 1 ? t1 : j_ == 3 ? (uint32_t)(tc) : (uint32_t)':'); } \
        w += 5u + tab_; \
    } while (0)
    while (p < end) {
        if (end - p < 3u) { err = VMX_BAM_IN_E_AUX_SHORT; break; }
        const uint32_t t0 = bzi_u(r[p]), t1 = bzi_u(r[p + 1]), ty = bzi_u(r[p + 2]);
        p += 3;
        bool selected = all != 0;
        if (!selected) {
            const uint32_t tg = t0 | t1 << 8;
            for (int b0 = 0; b0 < n_sel && !selected; b0 += 64) selected = __ballot(b0 + lane < n_sel && sel[b0 + lane] == tg) != 0;
        }
        const uint32_t fs = ty == 'A' || ty == 'c' || ty == 'C' ? 1u : ty == 's' || ty == 'S' ? 2u : ty == 'i' || ty == 'I' || ty == 'f' ? 4u : 0u;
        if (fs) {
            if (end - p < fs) { err = VMX_BAM_IN_E_AUX_FIXED; break; }
            uint32_t v = 0;
            for (uint32_t k = 0; k < fs; ++k) v |= (uint32_t)r[p + k] << (8 * k);
            v = bzi_u(v);
            if (selected) {
                if (ty == 'A') {
                    if (v < 0x20u || v > 0x7eu) ++drops;
                    else { BAX_PREFIX('A'); if (WRITE && lane == 0) o[w] = (char)v; w += 1; }
                } else if (ty == 'f' && ((v >> 23) & 0xffu) == 0xffu) ++drops;
                else {
                    const int64_t x = ty == 'c' ? (int64_t)(int8_t)v : ty == 's' ? (int64_t)(int16_t)v : ty == 'i' ? (int64_t)(int32_t)v : (int64_t)v;
                    const BaxText t = ty == 'f' ? bax_float(v, false) : bax_int(x, false);
                    BAX_PREFIX(ty == 'f' ? 'f' : 'i');
                    if (WRITE && lane < t.len) o[w + lane] = (char)bax_get(t, lane);
                    w += bzi_u((uint32_t)t.len);
                }
            }
            p += fs;
        } else if (ty == 'Z' || ty == 'H') {
            uint32_t len = 0;
            bool found = false, bad = false;
            for (uint32_t q = p; q < end && !found; q += 64) {
                const bool in = q + (uint32_t)lane < end;
                const uint32_t b = in ? (uint32_t)r[q + lane] : 1u;
                const bool isbad = ty == 'Z' ? (b < 0x20u || b > 0x7eu) : !(b - '0' < 10u || (b | 0x20u) - 'a' < 6u);
                const unsigned long long mz = __ballot(in && b == 0), mb = __ballot(in && b != 0 && isbad);
                if (mz) { const int f = __ffsll(mz) - 1; found = true; len = q - p + (uint32_t)f; bad |= (mb & ((1ull << f) - 1ull)) != 0; }
                else bad |= mb != 0;
            }
            if (!found) { err = VMX_BAM_IN_E_AUX_NUL; break; }
            if (ty == 'H' && (len & 1u)) bad = true;
            if (selected) {
                if (bad) ++drops;
                else {
                    BAX_PREFIX(ty);
                    if (WRITE) for (uint32_t j = (uint32_t)lane; j < len; j += 64) o[w + j] = (char)r[p + j];
                    w += len;
                }
            }
            p += len + 1u;
        } else if (ty == 'B') {
            if (end - p < 5u) { err = VMX_BAM_IN_E_AUX_COUNT; break; }
            const uint32_t st = bzi_u(r[p]), cnt = bzi_u(bin_u32(r + p + 1));
            const uint32_t es = st == 'c' || st == 'C' ? 1u : st == 's' || st == 'S' ? 2u : st == 'i' || st == 'I' || st == 'f' ? 4u : 0u;
            if (!es) { err = VMX_BAM_IN_E_AUX_SUBTYPE; break; }
            if ((uint64_t)cnt * es > (uint64_t)(end - p - 5u)) { err = VMX_BAM_IN_E_AUX_COUNT; break; }
            const uint8_t* a = r + p + 5u;
            if (selected) {
                bool drop = false;
                if (st == 'f')                                              // one non-finite value drops the field, before anything of it is written
                    for (uint32_t j0 = 0; j0 < cnt && !drop; j0 += 64) {
                        const uint32_t j = j0 + (uint32_t)lane;
                        drop = __ballot(j < cnt && (a[4 * (size_t)j + 3] & 0x7fu) == 0x7fu && (a[4 * (size_t)j + 2] & 0x80u)) != 0;
                    }
                if (drop) ++drops;
                else {
                    BAX_PREFIX('B');
                    if (WRITE && lane == 0) o[w] = (char)st;
                    w += 1;
                    for (uint32_t j0 = 0; j0 < cnt; j0 += 64) {
                        const uint32_t j = j0 + (uint32_t)lane;
                        BaxText t{0, 0, 0};
                        if (j < cnt) {
                            const uint8_t* s = a + (size_t)j * es;
                            uint32_t v = s[0];
                            if (es >= 2) v |= (uint32_t)s[1] << 8;
                            if (es == 4) v |= (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
                            if (st == 'f') t = bax_float(v, true);
                            else t = bax_int(st == 'c' ? (int64_t)(int8_t)v : st == 's' ? (int64_t)(int16_t)v : st == 'i' ? (int64_t)(int32_t)v : (int64_t)v, true);
                        }
                        const int inc = vmx_wave_incl_scan_i32(t.len);
                        if (WRITE) for (int k = 0; k < t.len; ++k) o[w + (uint32_t)(inc - t.len + k)] = (char)bax_get(t, k);
                        w += (uint32_t)vmx_readlane(inc, 63);
                    }
                }
            }
            p += 5u + cnt * es;
        } else { err = VMX_BAM_IN_E_AUX_TYPE; break; }
    }
#undef BAX_PREFIX
    if (WRITE) return;
    if (lane == 0) {
        csz[i] = err ? 0 : (int64_t)w;
        if (err) atomicMin(err_key, (unsigned long long)i << 8 | (unsigned long long)err);
        else if (drops) atomicAdd(n_drop, (unsigned long long)drops);
    }
}

__global__ void __launch_bounds__(256) k_bam_in_aux_size(const uint8_t* buf, const int64_t* roff, int64_t n, const uint16_t* sel, int n_sel, int all, int64_t* csz,
                                                         unsigned long long* err_key, unsigned long long* n_drop) {
    bax_record<false>(buf, roff, n, sel, n_sel, all, nullptr, nullptr, csz, nullptr, nullptr, err_key, n_drop);
}

__global__ void __launch_bounds__(256) k_bam_in_aux_write(const uint8_t* buf, const int64_t* roff, int64_t n, const uint16_t* sel, int n_sel, int all, const int64_t* coff,
                                                          const int64_t* kidx, char* out, int64_t* out_coff) {
    bax_record<true>(buf, roff, n, sel, n_sel, all, coff, kidx, nullptr, out, out_coff, nullptr, nullptr);
}
