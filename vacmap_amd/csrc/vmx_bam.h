// vmx_bam.h — BAM on the device. Output: SAM text -> BAM records (k_bam_*), BGZF deflate (k_bgzf_deflate), kernels in k_bam.hip. Input: BGZF inflate
// (k_bgzf_inflate), record walk and decode (k_bam_in_*), kernels in k_bam_in.hip. The C-ABI of both is in vmx_bam.hip.
#ifndef VMX_BAM_H
#define VMX_BAM_H
#include "vmx_device.h"

#define VMX_BGZF_BLOCK 65280            // input bytes per BGZF member (htslib's 0xff00: even a stored member fits in 65 536 bytes)
#define VMX_BGZF_SLOT 65536             // output slot of one member before compaction
#define VMX_BGZF_THREADS 1024
#define VMX_BGZF_HBITS 13               // 3-byte hash -> 8192 buckets
#define VMX_BGZF_LAUNCH 1024            // members per deflate launch: bounds the per-member global scratch (match + chain tables, 384 KB each)
#define VMX_BAM_NL_CHUNK 16384          // text bytes per workgroup of the newline kernels
#define VMX_BAM_MAX_OPLEN ((1 << 28) - 1)   // a CIGAR operation's length field has 28 bits

// the @SQ names of the header as an open-addressing hash table (FNV-1a, linear probing): htab[h] = reference index or -1
struct vmx_bam_refs {
    const char* names;
    const int64_t* off;
    const int32_t* htab;
    int32_t hmask;
    int32_t n_ref;
};

// a float the device does not convert exactly (> 15 significant digits, exponent outside +-22, nan / inf): the host patches 4 bytes
struct vmx_bam_patch {
    int64_t out_off;        // record bytes offset of the 4-byte value
    int64_t text_off;       // token in the SAM text
    int32_t text_len;
    int32_t line;           // 0-based line of the call's text
};

// what the size pass reports back to the host in one small copy
struct vmx_bam_status {
    int64_t total;          // record bytes of all lines
    uint64_t err_key;       // first malformed line << 8 | its VMX_BAM_E_* code; all ones when none
    int32_t n_patch;        // host-path floats
    int32_t pad;
};

enum { VMX_BAM_E_FIELDS = 1, VMX_BAM_E_NUM = 2, VMX_BAM_E_CIGAR = 3, VMX_BAM_E_REF = 4, VMX_BAM_E_QUAL = 5, VMX_BAM_E_NAME = 6, VMX_BAM_E_TAG = 7 };

__global__ void k_bam_nl_count(const char* text, int64_t len, int64_t* cnt);
__global__ void k_bam_nl_pos(const char* text, int64_t len, const int64_t* cnt_off, int64_t* nl);
__global__ void k_bam_scan(int64_t* v, int64_t n);
__global__ void k_bam_size(const char* text, const int64_t* nl, int64_t n_lines, vmx_bam_refs refs, int64_t* rsz, vmx_bam_status* st);
__global__ void k_bam_status(const int64_t* roff, int64_t n_lines, vmx_bam_status* st);
__global__ void k_bam_encode(const char* text, const int64_t* nl, int64_t n_lines, vmx_bam_refs refs, const int64_t* roff, uint8_t* out,
                             vmx_bam_patch* patch, int32_t* n_patch);
__global__ void k_bam_patch(uint8_t* out, const int64_t* off, const uint32_t* val, int64_t n);
__global__ void k_bgzf_deflate(const uint8_t* in, int64_t n_in, int64_t first_member, uint8_t* slots, int64_t* msize, uint32_t* g_match, uint16_t* g_prev);
__global__ void k_bgzf_compact(const uint8_t* slots, const int64_t* moff, uint8_t* out);

// CRC32 pieces shared by the deflate and the inflate kernel: crc(A B) = crc(A) * x^(8|B|) + crc(B), all modulo the (reflected) CRC polynomial
#define CRC_POLY 0xedb88320u

// a(x) * b(x) modulo the CRC polynomial (reflected; zlib's multmodp). a must not be 0
__host__ __device__ static inline uint32_t crc_multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) { p ^= b; if ((a & (m - 1)) == 0) break; }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

// x^(8 n) modulo the polynomial; x2n[k] = x^(2^k)
__device__ static inline uint32_t crc_x8n(const uint32_t* x2n, uint32_t n) {
    uint32_t mul = 1u << 31;
    uint32_t k = 3;
    for (uint32_t r = n; r; r >>= 1, ++k) if (r & 1) mul = crc_multmodp(x2n[k & 31], mul);
    return mul;
}

// BAM input on the device (k_bam_in.hip): BGZF inflate, record walk, record decode
struct vmx_bgzf_member {
    int64_t coff;           // the member's deflate data in the compressed buffer
    int64_t ooff;           // where its ISIZE bytes go in the inflated buffer (exclusive scan of ISIZE)
    int32_t csize;          // deflate bytes (BSIZE + 1 - header - trailer)
    uint32_t isize, crc;    // the trailer
    int32_t pad;
};
struct vmx_crc_x2n { uint32_t v[32]; };
enum { VMX_BGZF_E_BTYPE = 1, VMX_BGZF_E_STORED = 2, VMX_BGZF_E_INPUT = 3, VMX_BGZF_E_LONG = 4, VMX_BGZF_E_SHORT = 5, VMX_BGZF_E_CRC = 6, VMX_BGZF_E_LENS = 7,
       VMX_BGZF_E_CODE = 8, VMX_BGZF_E_DIST = 9, VMX_BGZF_E_TAIL = 10, VMX_BGZF_E_HEADER = 11 };
enum { VMX_BAM_IN_E_SIZE = 1, VMX_BAM_IN_E_AUX_SHORT = 2, VMX_BAM_IN_E_AUX_TYPE = 3, VMX_BAM_IN_E_AUX_SUBTYPE = 4, VMX_BAM_IN_E_AUX_FIXED = 5, VMX_BAM_IN_E_AUX_NUL = 6,
       VMX_BAM_IN_E_AUX_COUNT = 7 };
#define VMX_BAM_IN_MAX_RECORD (1 << 29)      // a larger block_size is taken for corrupt at once (a 300 Mb read is 450 MB), not carried window after window to the end of the file
// what the record walk leaves: records found, where the incomplete tail begins, the first bad record (all ones: none)
struct vmx_bam_in_walk { int64_t n_rec, end; uint64_t err_key; };
__global__ void k_bgzf_inflate(const uint8_t* comp, const vmx_bgzf_member* tab, int64_t n_members, uint8_t* out, vmx_crc_x2n x2n, unsigned long long* err_key);
__global__ void k_bam_in_walk(const uint8_t* buf, int64_t begin, int64_t end, int64_t max_rec, int64_t* roff, vmx_bam_in_walk* res);
__global__ void k_bam_in_sizes(const uint8_t* buf, const int64_t* roff, int64_t n, int64_t* nsz, int64_t* ssz, int64_t* qsz, int64_t* keep);
__global__ void k_bam_in_decode(const uint8_t* buf, const int64_t* roff, int64_t n, const int64_t* noff, const int64_t* soff, const int64_t* qoff, const int64_t* kidx,
                                char* names, char* seqs, char* quals, int64_t* out_noff, int64_t* out_soff, int64_t* out_qoff);
// auxiliary fields as comment text: sel = the selected tags (first letter in the low byte), all != 0: every field; csz / coff: bytes per record and their exclusive scan
__global__ void k_bam_in_aux_size(const uint8_t* buf, const int64_t* roff, int64_t n, const uint16_t* sel, int n_sel, int all, int64_t* csz, unsigned long long* err_key,
                                  unsigned long long* n_drop);
__global__ void k_bam_in_aux_write(const uint8_t* buf, const int64_t* roff, int64_t n, const uint16_t* sel, int n_sel, int all, const int64_t* coff, const int64_t* kidx,
                                   char* out, int64_t* out_coff);

// Plain gzip on the device (k_gzip_in.hip): one deflate stream inflated in parallel chunks. A decode wave begins at a block
// start inside the compressed window (a gzip member header, or a candidate that k_gz_find judged a valid non-final dynamic block header) and
// ends at the first block boundary at or after stop_bit. Its output is 16-bit symbols: 0 ... 255 a byte, VMX_GZ_MARK | j byte j of the
// 32 KB in front of the wave's first output byte.
#define VMX_GZ_WIN 32768
#define VMX_GZ_MARK 0x8000u
#define VMX_GZ_NONE 0xffffffffu          // no candidate in the chunk / no stop: decode to the end of the window
#define VMX_GZ_F_HEADER 1u              // (vmx_gz_wave.flags) a gzip member header stands at start_bit: what is in front is known to be nothing
#define VMX_GZ_R_END 1u                 // (vmx_gz_res.flags) the wave met the end of the compressed window behind a member's trailer
#define VMX_GZ_R_HEADER 4u              // (vmx_gz_res.flags) the wave ended at a member header (or the padding in front of one), not at a block
#define VMX_GZ_R_RESUME_HDR 8u          // (vmx_gz_res.flags) resume_bit is a member header
#define VMX_GZ_R_MEMBER 2u              // (vmx_gz_res.flags) a member began inside the wave (or at its start): `open` counts from the last such start
#define VMX_GZ_TILE 16384               // text bytes per workgroup of k_gz_resolve: 256 lanes x 64 bytes
struct vmx_gz_wave {
    uint32_t start_bit, stop_bit, flags;
    uint32_t hist;          // k_gz_resolve: bytes of the open member in front of the wave's first byte, at most VMX_GZ_WIN: a marker below VMX_GZ_WIN - hist reaches before the member
    int64_t ooff, eoff;     // write pass: the wave's first symbol and its first member entry
    uint32_t n_sym, n_ev;   // what the count pass counted: the write pass stores no more
};
// err: 0 or VMX_BGZF_E_* / VMX_GZ_E_*; err_bit: where the block (or header) with the error begins; open: text bytes behind the last member start (all of n_sym without one)
// resume_bit: the latest place in front of the error (or the end) where a wave can begin: a block's first bit, or a member header (R_RESUME_HDR)
struct vmx_gz_res { uint32_t end_bit, err, err_bit, flags, n_sym, n_ev, open, resume_bit; };
// a member's end as the wave that decoded its final block met it: text position (from the wave's first symbol), the trailer, the file byte behind the trailer
struct vmx_gz_member { uint32_t opos, crc, isize, next_byte; };
enum { VMX_GZ_E_MAGIC = 20, VMX_GZ_E_METHOD = 21, VMX_GZ_E_BIG = 22, VMX_GZ_E_MARK = 23 };
__global__ void k_gz_find(const uint8_t* comp, uint32_t n_bytes, uint32_t chunk_bytes, uint32_t first_chunk, uint32_t min_bit, uint32_t* cand);
__global__ void k_gz_count(const uint8_t* comp, uint32_t n_bytes, const vmx_gz_wave* tab, const uint32_t* todo, vmx_gz_res* res);
__global__ void k_gz_decode(const uint8_t* comp, uint32_t n_bytes, const vmx_gz_wave* tab, vmx_gz_res* res, uint16_t* sym, vmx_gz_member* ev);
__global__ void k_gz_window(const uint16_t* sym, const vmx_gz_wave* tab, int64_t n_waves, const uint8_t* win0, uint8_t* win_in, uint8_t* win_out);
__global__ void k_gz_resolve(const uint16_t* sym, const vmx_gz_wave* tab, int64_t n_waves, const uint8_t* win_in, const uint64_t* ev_end, int64_t n_ev, int64_t total,
                             vmx_crc_x2n x2n, uint8_t* out, uint32_t* crc_acc, unsigned long long* err_key);

// FASTQ input on the device (k_fastx_in.hip): newlines, line states, records, field sizes, field copy over one window of inflated text
#define VMX_FQ_CHUNK 4096               // text bytes per wavefront of the newline kernels: 4 steps of 64 lanes x 16 bytes
#define VMX_FQ_LTILE 256                // lines per workgroup of the state kernels
// a line's effect on the parser state (0 header, 1 sequence, 2 '+', 3 qualities) as a map of 4 states packed 2 bits each, state s in bits 2s
#define VMX_FQ_MAP_LINE 0x39u           // [1, 2, 3, 0]: a line that is not blank
#define VMX_FQ_MAP_BLANK 0x38u          // [0, 2, 3, 0]: a blank line is skipped in state 0 only
#define VMX_FQ_MAP_IDENT 0xe4u          // [0, 1, 2, 3]
enum { VMX_FQ_E_FASTA = 1, VMX_FQ_E_HEADER = 2 };
// what the parse leaves: complete records, the offset behind them (the rest is carried), the first bad header (record << 8 | code, all ones: none),
// the state after the window's last line, whether the window's last byte is something else than a newline
struct vmx_fq_result { int64_t n_rec, end; uint64_t err_key; int32_t end_state, tail_open; };
__global__ void k_fq_nl_count(const uint8_t* buf, int64_t len, int64_t n_chunks, int64_t* cnt, vmx_fq_result* res);
__global__ void k_fq_nl_pos(const uint8_t* buf, int64_t len, int64_t n_chunks, const int64_t* coff, int64_t n_lines, int closing, int64_t* ls);
__global__ void k_fq_line_maps(const uint8_t* buf, const int64_t* ls, int64_t n_lines, uint8_t* map, uint8_t* tile_tot);
__global__ void k_fq_tile_scan(uint8_t* tile, int64_t n_tiles);
__global__ void k_fq_line_states(const uint8_t* map, const uint8_t* tile_pre, int64_t n_lines, int64_t* start);
__global__ void k_fq_records(const int64_t* start, const int64_t* ridx, int64_t n_lines, int64_t* rline);
__global__ void k_fq_result(const uint8_t* buf, const int64_t* ls, const int64_t* ridx, const int64_t* rline, int64_t n_lines, int64_t len, vmx_fq_result* res);
__global__ void k_fq_sizes(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, int64_t* nsz, int64_t* csz, int64_t* ssz, int64_t* qsz,
                           unsigned long long* err_key);
__global__ void k_fq_copy(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, const int64_t* noff, const int64_t* coff, const int64_t* soff,
                          const int64_t* qoff, uint8_t* names, uint8_t* comments, uint8_t* seqs, uint8_t* quals);

// FASTA and FASTQ reads on the device (k_fasta_reads.hip): the general record rule of vm_fastx_read over the line table of k_fq_nl_pos. States 0 between
// records, 1 - 3 the FASTQ states, 4 inside a FASTA record; a line's class (blank, '>' first, other) maps the state before it to the state behind
// it, 5 states packed 3 bits each, state s in bits 3s
#define VMX_FR_MAP_BLANK 0x40d0u        // [0, 2, 3, 0, 4]
#define VMX_FR_MAP_GT 0x40d4u           // [4, 2, 3, 0, 4]: a '>' line starts a FASTA record between records and inside one
#define VMX_FR_MAP_OTHER 0x40d1u        // [1, 2, 3, 0, 4]
#define VMX_FR_MAP_IDENT 0x4688u        // [0, 1, 2, 3, 4]
// what the record pass leaves: complete records, the offset behind them (the rest is carried), the line the cut stands in front of (n_lines: none), the
// first bad header (record << 8 | VMX_FQ_E_HEADER, all ones: none), the state behind the window's last line
struct vmx_fr_result { int64_t n_rec, end, cut_line; uint64_t err_key; int32_t end_state, pad; };
__global__ void k_fr_line_maps(const uint8_t* buf, const int64_t* ls, int64_t n_lines, uint16_t* map, uint16_t* tile_tot);
__global__ void k_fr_tile_scan(uint16_t* tile, int64_t n_tiles);
__global__ void k_fr_line_states(const uint16_t* map, const uint16_t* tile_pre, int64_t n_lines, uint8_t* state, int64_t* start);
__global__ void k_fr_result(const uint8_t* buf, const int64_t* ls, const uint8_t* state, const int64_t* ridx, const int64_t* rline, int64_t n_lines, int64_t len,
                            int closing, vmx_fr_result* res);
__global__ void k_fr_line_keep(const uint8_t* buf, const int64_t* ls, const uint16_t* map, const uint8_t* state, int64_t n_lines, int64_t cut_line, int64_t* ka,
                               int64_t* ks, int64_t* kq);
__global__ void k_fr_copy(const uint8_t* buf, int64_t len, int64_t n_chunks, const int64_t* coff, const int64_t* ka, const int64_t* ks, const int64_t* kq,
                          const int64_t* so, const int64_t* qo, uint8_t* seqs, uint8_t* quals);
__global__ void k_fr_hdr_sizes(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, int64_t cut_line, const int64_t* so, const int64_t* qo,
                               int64_t* nsz, int64_t* csz, int64_t* soff, int64_t* qoff, unsigned long long* err_key);
__global__ void k_fr_hdr_copy(const uint8_t* buf, const int64_t* ls, const int64_t* rline, int64_t n_rec, const int64_t* noff, const int64_t* coff, uint8_t* names,
                              uint8_t* comments);

// The reference FASTA on the device (k_fasta_in.hip): per chunk of VMX_FQ_CHUNK bytes, state = in a header line | a header has been seen << 1; a
// chunk's map has the format of the FASTQ line maps (k_fq_tile_scan scans the tiles of both)
// what the passes over a window leave: 1 + its last header start (0: none), where it is cut, whether a newline stands in front of the cut
struct vmx_fa_result { uint64_t last_hs; int64_t end; int32_t end_ls, pad; };
__global__ void k_fa_maps(const uint8_t* buf, int64_t len, int64_t n_chunks, int ls0, uint8_t* map, vmx_fa_result* res);
__global__ void k_fa_tile_tot(const uint8_t* map, int64_t n_chunks, uint8_t* tile_tot);
__global__ void k_fa_states(const uint8_t* map, const uint8_t* tile_pre, int64_t n_chunks, int s_in, uint8_t* state);
__global__ void k_fa_result(const uint8_t* buf, int64_t len, int64_t n_chunks, const uint8_t* state, int ls0, int closing, vmx_fa_result* res);
__global__ void k_fa_count(const uint8_t* buf, int64_t end, int64_t n_chunks, const uint8_t* state, int ls0, int64_t* cnt);
__global__ void k_fa_write(const uint8_t* buf, int64_t end, int64_t n_chunks, const uint8_t* state, int ls0, const int64_t* coff, int64_t base0, uint8_t* letters,
                           uint8_t* codes, int64_t* hpos, int64_t* hbase, unsigned long long* other);
__global__ void k_fa_hdr_size(const uint8_t* buf, int64_t end, const int64_t* hpos, int64_t n, int64_t* hsz);
__global__ void k_fa_hdr_copy(const uint8_t* buf, const int64_t* hpos, const int64_t* hoff, int64_t n, uint8_t* blob);

// coordinate sort, merge and CSI (k_bam_sort.hip)
#define VMX_BAM_RUN_SHIFT 40            // value of the merge sort: run << 40 | index in run
#define VMX_BAM_RUN_MASK ((1ULL << VMX_BAM_RUN_SHIFT) - 1)
__global__ void k_bam_sort_keys(const uint8_t* rec, const int64_t* roff, int64_t n, uint64_t* key, uint64_t* val);
__global__ void k_bam_sort_sizes(const int64_t* roff, const uint64_t* perm, int64_t n, int64_t* ssz, int64_t* so);
__global__ void k_bam_gather(const uint8_t* src, const int64_t* so, const int64_t* doff, int64_t dbase, uint8_t* dst, int64_t n);
__global__ void k_bam_merge_vals(const int64_t* rstart, int32_t n_runs, int64_t n, uint64_t* val);
__global__ void k_bam_merge_sizes(const uint64_t* gval, const int64_t* roff_all, const int64_t* rstart, int64_t n, int64_t* gsz);
__global__ void k_bam_merge_cuts(const int64_t* goff, int64_t n, int64_t chunk_bytes, int64_t n_chunks, int64_t* cut, int64_t* cutoff);
__global__ void k_bam_merge_runmax(const uint64_t* gval, const int64_t* cut, int64_t n_chunks, int32_t n_runs, int64_t n, unsigned long long* rmax);
__global__ void k_bam_merge_src(const uint64_t* gval, int64_t m, const int64_t* roff_all, const int64_t* rstart, const int64_t* sbase, int64_t* so);
__global__ void k_bam_index_entries(const uint8_t* rec, const int64_t* doff, int64_t dbase, int64_t m, const int64_t* moff, int64_t file_base,
                                    uint64_t* e_key, uint64_t* e_vbeg, uint64_t* e_vend, int32_t* e_beg, uint32_t* e_end, uint32_t* e_unm);
__global__ void k_csi_iota(uint64_t* v, int64_t n);
__global__ void k_csi_flags(const uint64_t* skey, const uint64_t* sidx, const uint64_t* vbeg, const uint64_t* vend, int64_t n, int64_t* flag);
__global__ void k_csi_chunks(const uint64_t* skey, const uint64_t* sidx, const uint64_t* vbeg, const uint64_t* vend, const int64_t* flag, const int64_t* cpos, int64_t n,
                             uint64_t* ckey, uint64_t* cbeg, uint64_t* cend);
__global__ void k_csi_linear(const uint64_t* e_key, const uint64_t* vbeg, const int32_t* e_beg, const uint32_t* e_end, int64_t n, int32_t n_ref, const int64_t* wbase,
                             unsigned long long* lin);
__global__ void k_csi_loffset(const uint64_t* ckey, int64_t nc, int32_t n_ref, const int64_t* wbase, const unsigned long long* lin, uint64_t* cloff);
__global__ void k_csi_refstats(const uint64_t* e_key, const uint64_t* vbeg, const uint64_t* vend, const uint32_t* e_unm, int64_t n, int32_t n_ref, uint64_t* rbeg,
                               uint64_t* rend, unsigned long long* cnt);

#endif
