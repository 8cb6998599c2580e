/* vacmapx.h — C-ABI of libvacmapx.so: MI355X-native seed -> non-linear chain -> extend for long reads.
 *
 * Drop-in boundary: these entry points are what the reference's Python would bind through ctypes
 * in place of its native dependencies `vacmap_index` (pip vacmap-index==0.0.3) and `edlib`, plus ONE batched
 * entry (`vm_align_batch`) that replaces the whole per-read function `get_readmap_DP_test`
 * (/root/reference/src/vacmap/mammap_clrnano.py:24023-24084) called by the worker loop (:24117).
 * Every compute entry runs hand-written HIP kernels on gfx950; there is no CPU fallback: without a GPU / the HIP
 * runtime, `vm_ctx_create` fails with VM_ERR_NO_DEVICE and every compute call returns VM_ERR_NO_CTX.
 *
 * Conventions: plain pointers and sizes; inputs are borrowed for the duration of the call; outputs are
 * library-allocated host memory released with vm_free(); every function returns 0 or a negative vm_status;
 * vm_last_error() gives a thread-local message. Anchor rows are int64 (q, r, s, l) = (read pos, global ref pos,
 * strand +-1, length) exactly like the reference's (n,4) int64 arrays (:23985).
 */
#ifndef VACMAPX_H
#define VACMAPX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum vm_status {
    VM_OK = 0,
    VM_ERR_ARG = -1,
    VM_ERR_NO_DEVICE = -2,      /* no HIP device / runtime: the product never falls back to the CPU */
    VM_ERR_NO_CTX = -3,
    VM_ERR_OOM = -4,
    VM_ERR_IO = -5,
    VM_ERR_HIP = -6,
    VM_ERR_UNSUPPORTED = -7,
    /* per-read statuses (status_per_read of vm_align_batch); the reference skips such reads (:24116-24125) */
    VM_READ_RAISED = -10,       /* the reference's Python would have raised inside the per-read path */
    VM_READ_CAPACITY = -20,     /* a device work buffer overflowed for this read (reported, never silently truncated) */
    VM_READ_FASTPATH = -21,     /* internal hand-off to the `_fast` chain kernels (:23570, :24914, :27380); never returned by vm_align_batch */
    VM_READ_UNSUPPORTED = -22   /* -mode asm only: a long contig whose carried slice leaves the stored part of the score index (k_chain_linked.hip):
                                   reported, not approximated. (The MAPQ-0 edlib tie-break of mammap_asm.py:21302-21326 is built: it no longer refuses.) */
} vm_status;

enum { VM_MODE_H = 0, VM_MODE_L = 1, VM_MODE_S = 2, VM_MODE_R = 3,   /* -mode (src/vacmap/vacmap:87) */
       /* -mode asm runs src/vacmap/mammap_asm.py, an older fork of the path. Every "read" of vm_align_batch is then an assembly contig and takes
        * the route of assembly_get_readmap_DP_test (:23204): below 500 000 bases that module's per-read function (:19681, check_num = -1), in one
        * batch with the others; from 500 000 bases on the batch-linked path, contig by contig (vm_align_asm). */
       VM_MODE_ASM = 4 };

/* option dict `pdict` of the reference driver (src/vacmap/vacmap:177-296) as one POD */
typedef struct vm_params {
    int32_t mode;            /* VM_MODE_* */
    int32_t check_num;       /* -c (100) */
    int32_t mid_occ;         /* -1 = index default (mammap_clrnano.py:23985) */
    int32_t global_maxdiff;  /* -globalmaxdiff (50) */
    int32_t local_maxdiff;   /* -localmaxdiff (30) */
    int32_t local_kmersize;  /* 9 (src/vacmap/vacmap:255) */
    int32_t eqx;             /* --eqx */
    int32_t hardclip;        /* --H */
    int32_t nodiscard;       /* --nodiscard */
    int32_t reserved;
    double global_skipcost;  /* -globalpenalty */
    double local_skipcost;   /* -localpenalty */
    double maxdivergence;    /* -maxdivergence */
} vm_params;
void vm_params_default(vm_params* p, int mode);            /* mode defaults of src/vacmap/vacmap:257-296 */

/* ------------------------------------------------------------------ index (replaces mp.Aligner, vacmap:344-367) */
typedef struct vm_index vm_index;
typedef struct vm_ctx vm_ctx;

/* one context = one GPU (device_id) + its streams and work buffers; one per host thread per GPU */
int vm_ctx_create(int device_id, vm_ctx** out);
void vm_ctx_destroy(vm_ctx*);
/* How many contexts share this GPU (batches in flight, one host thread each; default 1). A context that runs alone sizes its
 * latency-bound kernels to fill the device; with several in flight they are launched narrower (the local seeding kernel at 3 / 2
 * workgroups per CU for 1 / >= 2 contexts) so that another batch's VALU-bound gap-fill kernel can be resident beside them. */
int vm_ctx_set_inflight(vm_ctx*, int n_contexts);
/* on != 0: the context's host thread sleeps while it waits for the GPU inside vm_align_batch instead of spinning (default: spin, lowest
 * latency). For processes whose other threads need the cores — vacmap_amd.driver's SAM emitters under a CPU quota. */
int vm_ctx_set_blocking_sync(vm_ctx*, int on);
int vm_device_count(void);
/* diagnostics of the chain DPs with four reads per wavefront (csrc/k_chain_rows.hip; replays mammap_clrnano.py:24912-24928, :24944-25003): eight counters summed
 * over every launch of the process since they were switched on — [0] anchors, [1] scans that left the register window and went on through S_arg / S in HBM,
 * [2] insertions placed through HBM, [3] opcount of the global chain; [4..7] the same of the local chains. enable: 1 switch on (first call allocates), 0 read,
 * -1 read and reset. out8 may be NULL. Off by default (the kernels get a NULL counter block); the GPU tests assert that the rare paths did run. */
int vm_debug_chain_counters(int enable, unsigned long long* out8);
/* free / total bytes of the context's device (hipMemGetInfo): the driver drops a context when the grow-only work pools of the batches in flight
 * leave less than a safety margin of HBM free after their sizing run */
int vm_ctx_mem_info(vm_ctx*, int64_t* free_bytes, int64_t* total_bytes);

/* build the minimizer index of a FASTA file / in-memory contigs ON THE GPU and keep it resident in HBM
 * (replaces `mp.Aligner(path, w=, k=)`, src/vacmap/vacmap:344; index.py:26) */
int vm_index_build_fasta(vm_ctx*, const char* fasta_path, int k, int w, vm_index** out);
/* The rule of a reference FASTA, for both entries. A line is the bytes between newlines; the bytes behind the last newline are a line as well.
 * All trailing '\r' of a line are removed; an empty line is skipped. A line whose first byte is '>' starts a contig: its name is the bytes
 * behind '>' up to the first blank or tab (it may be empty), and a header without sequence lines gives a contig of length 0. Any other line
 * is appended whole to the current contig (interior blanks and '\r' stay and become "other letters"), or dropped when no header has been
 * seen. The host copy of the bases has a-z upper-cased; the device codes are A C G T -> 0 1 2 3 in either case, everything else 4.
 * A file that begins with the gzip magic 1f 8b is read as a gzip stream of any number of members (plain gzip and BGZF): vm_index_build_fasta
 * through zlib. vm_index_build_fasta_device parses the text on the GPU (csrc/k_fasta_in.hip) window by window: plain files are read into
 * page-locked memory, BGZF members are inflated on the GPU, plain gzip is inflated by zlib on a host thread. The index is the one
 * vm_index_build_fasta builds, byte for byte (.vmx file, device codes, count of other letters). A header line that does not fit in one window
 * (256 MB of text; BGZF: 512 MB) returns VM_ERR_UNSUPPORTED: the caller falls back to vm_index_build_fasta. stats (may be NULL; n_stats
 * doubles are written, 8 are defined): seconds of [0] file read and upload, [1] inflate, [2] parse kernels, [3] download of the bases,
 * [4] index build, then [5] bytes of text, [6] windows, [7] contigs. */
int vm_index_build_fasta_device(vm_ctx*, const char* fasta_path, int k, int w, vm_index** out, double* stats, int n_stats);
/* vm_index_build_fasta_device with options. flags 0: exactly vm_index_build_fasta_device. VM_READER_GZIP_DEVICE: a plain-gzip file (no BGZF BC
 * subfield in its first member) is inflated on the GPU in parallel chunks, window after window (as vm_fastq_reader_open_opts describes), instead
 * of by zlib on a host thread; stats[1] is then the seconds of that inflate. The index is the same, byte for byte. VM_ERR_UNSUPPORTED (a single
 * deflate block that does not end inside one window of VMX_BAM_IN_CHUNK compressed bytes, a header line longer than a window): the caller falls back. */
#ifndef VM_READER_GZIP_DEVICE
#define VM_READER_GZIP_DEVICE 1
#endif
int vm_index_build_fasta_device_opts(vm_ctx*, const char* fasta_path, int k, int w, int flags, vm_index** out, double* stats, int n_stats);
int vm_index_build_mem(vm_ctx*, int nseq, const char* const* names, const char* const* seqs, const int64_t* lens,
                       int k, int w, vm_index** out);
/* own on-disk format `<ref>.w<w>_k<k>.vmx` (the reference's naming rule `<ref>.w<w>_k<k>.mmi`, vacmap:326): contig table, bases and the
 * sorted position column; the loader recomputes the hashes on the GPU and rejects a file whose header, sizes, positions or order are
 * inconsistent (VM_ERR_IO) before anything is used */
int vm_index_save(const vm_index*, const char* path);
int vm_index_load(vm_ctx*, const char* path, vm_index** out);
/* minimap2 index files (`minimap2 -d`, on-disk format v3), the files the reference builds and reuses as `<ref>.w<w>_k<k>.mmi`
 * (src/vacmap/vacmap:324-344, index.py:26). load: the file's minimizer set and 4-bit sequence become the HBM-resident index; every
 * stored hash is re-derived from the sequence on the GPU and a mismatch rejects the file (VM_ERR_IO). Homopolymer-compressed,
 * sequence-less and multi-part files are VM_ERR_UNSUPPORTED. save: writes the index in that format (bucket_bits < 0: minimap2's 14). */
int vm_index_load_mmi(vm_ctx*, const char* path, vm_index** out);
int vm_index_save_mmi(const vm_index*, const char* path, int bucket_bits);
void vm_index_free(vm_index*);
int vm_index_k(const vm_index*);                            /* Aligner.k      (:24024) */
int vm_index_w(const vm_index*);
int vm_index_nseq(const vm_index*);
int vm_index_mid_occ(const vm_index*);
int64_t vm_index_n_minimizers(const vm_index*);
int64_t vm_index_n_distinct(const vm_index*);               /* distinct minimizer hashes (= occupied table slots) */
/* Aligner.seq_offset (vacmap:358-361): name, length, global offset of contig i */
int vm_index_seq_info(const vm_index*, int i, const char** name, int64_t* len, int64_t* offset);
/* Aligner.seq(name)  (vacmap:363): copies upper-case bases [start,end) of contig i; returns the count */
int64_t vm_index_seq(const vm_index*, int i, int64_t start, int64_t end, char* out);
/* device-resident sorted minimizer arrays copied back to the host (tests): hashes[n], positions[n] (gpos<<1|strand) */
int vm_index_minimizers(const vm_index*, uint64_t** hashes, uint64_t** positions, int64_t* n);
/* raw device pointers + sizes of the index blob pieces, for the multi-GPU broadcast (RCCL over xGMI) */
int vm_index_blob_count(const vm_index*);
int vm_index_blob(const vm_index*, int i, void** dev_ptr, int64_t* bytes);
/* metadata (k, w, contig names/lengths, table geometry) needed to allocate an empty replica on another GPU / process:
 * sender: meta_size + meta_get; receiver: vm_index_from_meta, then the blobs are filled by the broadcast */
int vm_index_meta_size(const vm_index*, int64_t* bytes);
int vm_index_meta_get(const vm_index*, void* buf, int64_t bytes);
int vm_index_from_meta(vm_ctx*, const void* buf, int64_t bytes, vm_index** out);

/* ------------------------------------------------------------------ stage entry points (batched; GPU) */
/* minimizer sketch of n reads: outputs concatenated per read, off[n+1] (tests; part of `.map`) */
int vm_sketch_batch(vm_ctx*, int k, int w, int64_t n, const char* seqs, const int64_t* offsets,
                    uint64_t** hash, int32_t** pos, int8_t** strand, int64_t** off);
/* `.map(seq, check_num=, mid_occ=)` (:23985) for n reads: anchors rows concatenated, anchor_off[n+1] */
int vm_map_batch(vm_ctx*, const vm_index*, int check_num, int mid_occ, int64_t n, const char* seqs,
                 const int64_t* offsets, int64_t** anchors, int64_t** anchor_off);
/* single-read form with the exact shape of the reference call */
int vm_map(vm_ctx*, const vm_index*, const char* seq, int64_t len, int check_num, int mid_occ, int64_t** anchors, int64_t* n);

/* global non-linear chain of n reads: strand flip (:21202) + hit2work_1 (:23491) + decode_hit (:23981).
 * in: anchors (as returned by map), readlens. out per read: need_reverse, mapq, signed score (0 = unmapped),
 * paths (primary + secondaries, descending read order): path_off[n_paths_total+1], read_path_off[n+1] */
typedef struct vm_chains_out {
    int32_t* need_reverse;   /* n */
    int32_t* mapq;           /* n */
    double* score;           /* n */
    int32_t* fast_used;      /* n: 1 if GC-fast (:25033) produced the chain */
    int64_t* read_path_off;  /* n+1: first path of each read */
    int64_t* path_off;       /* total_paths+1: first anchor row of each path */
    int64_t* path_anchors;   /* rows */
    /* raw DP state of the LAST run of the exact DP (tests; null unless want_raw) : concatenated per read */
    double* S; int64_t* P; int64_t* S_arg; int64_t* gmax; int64_t* opcount;
} vm_chains_out;
/* Runs the global chain stage of vm_align_batch (S2 + G1-G3 + selection). A read of two anchors or fewer is not chained (unmapped, :23986):
 * gmax -1, its S / P / S_arg undefined. -mode asm: a contig of 500 kb and more is not chained either (gmax -4, no path): vm_align_batch
 * takes it through the linked DPs (vm_chain_linked). The device keeps an anchor's q in 32 bits and its l, s in 16: a batch with a row whose l is outside
 * 0 ... 65535, whose q or q + l is outside int32 or whose s is outside int16 is refused as a whole (VM_ERR_UNSUPPORTED, the message names the row); map() never
 * returns such a row. */
int vm_chain_global_batch(vm_ctx*, const vm_params*, int kmersize, int64_t n, const int64_t* anchors,
                          const int64_t* anchor_off, const int64_t* readlens, int want_raw, vm_chains_out* out);
void vm_chains_out_free(vm_chains_out*);

/* local re-seeding + local chain (:28479) of n reads. reads must be in chain orientation (reverse-complemented by the
 * caller when need_reverse). out: chain rows per read (descending read order), raw local anchors (pre-DP order) */
typedef struct vm_local_out {
    int32_t* status;         /* n: 0 or VM_READ_* */
    int32_t* variant;        /* n: 0 = LC-exact (:27305), 1 = LC-mm (:28250) */
    double* score;           /* n */
    int64_t* chain_off;      /* n+1 */
    int64_t* chain;          /* rows */
    int64_t* raw_off;        /* n+1 */
    int64_t* raw;            /* rows, sorted by (q+l) stable = the DP's input order */
} vm_local_out;
int vm_local_chain_batch(vm_ctx*, const vm_index*, const vm_params*, int64_t n, const char* seqs, const int64_t* offsets,
                         const int64_t* read_path_off, const int64_t* path_off, const int64_t* path_anchors, vm_local_out* out);
void vm_local_out_free(vm_local_out*);

/* The local chain DPs alone (L3 LC-exact :27305, L4 LC-mm :28250, L5 their `_fast` twins :26938 / :27891; mode R: `_scar`, mammap_noprefercloser.py:23419) on
 * GIVEN anchor rows: the second half of vm_local_chain_batch, the same function with the same routing (four reads per wavefront or one wavefront per read,
 * LDS-resident or not, the `_fast` launch behind them). rows: 4 int64 per row (q, r, s, l), read r's at row_off[r] ... row_off[r + 1], already in the DP's input
 * order — stable by q + l, in mode R by q. n_guides_total[r]: the guide chains L1 would have kept for the read (1: LC-exact, more: LC-mm; mode R runs `_scar`
 * whatever it says). readlens[r]: the read's length (the `_fast` twins size their score buckets from it); every row ends inside its read. flags:
 * VM_LOCAL_DP_WANT_SP asks for S / P; VM_LOCAL_DP_DEVICE_LIST takes the read list built on the device (the route every batch after a context's first takes;
 * it needs the row kernels). A batch with a row the device's fields cannot carry (l outside 0 ... 65535, q or q + l outside int32, s other than +1 / -1) is refused
 * as a whole with VM_ERR_UNSUPPORTED, the message names the row; rows out of order, a negative q, a row that ends behind its read or a guide count below 1 are VM_ERR_ARG.
 * (The order check is also what keeps the reference's non-terminating `continue` of the `_fast` twins, :27103, out of k_chain_local_fast: in order of read end only row 0
 * can be a candidate that ends at or behind the current row, and only before the first advance, when its bucket holds one entry.)
 * out per read: status (0, or VM_READ_RAISED where the reference's `_fast` twin would raise or never return), variant (0 LC-exact, 1 LC-mm, 2 `_scar`), fast_used
 * (the opcount switch :27380 / :28333 was taken), score, the chain (descending read order, overlaps trimmed) and, with VM_LOCAL_DP_WANT_SP, S / P laid out like
 * rows. sp_valid: bit 0 S, bit 1 P of the read are defined — P of every chained read, S unless the one-wavefront form kept it in LDS; a read without rows
 * has status 0, score 0 and an empty chain. */
#define VM_LOCAL_DP_WANT_SP 1
#define VM_LOCAL_DP_DEVICE_LIST 2
typedef struct vm_local_dp_out {
    int32_t* status;         /* n */
    int32_t* variant;        /* n */
    int32_t* fast_used;      /* n */
    int32_t* sp_valid;       /* n */
    double* score;           /* n */
    int64_t* chain_off;      /* n+1 */
    int64_t* chain;          /* rows */
    double* S; int64_t* P;   /* row_off[n] each; NULL without VM_LOCAL_DP_WANT_SP */
} vm_local_dp_out;
int vm_local_dp_batch(vm_ctx*, const vm_params*, int64_t n, const int64_t* rows, const int64_t* row_off, const int32_t* n_guides_total,
                      const int64_t* readlens, int flags, vm_local_dp_out* out);
void vm_local_dp_out_free(vm_local_dp_out*);

/* One batch of -mode asm's LINKED chain DPs on the device (contigs of 500 kb and more, src/vacmap/mammap_asm.py:23228-23275 / :23328-23373):
 * which = 0 linked GC-exact (:21686), 2 linked LC (:21504). rows: n x 4 int64, the n_pre anchors carried from the previous batch first, the
 * new ones sorted by read position behind them; pre_S / pre_P, g_max_scores, g_max_index, prereadloc: the carried state (n_pre may be 0).
 * out: S[n], P[n]; the HOT part of the score-sorted index S_arg (its last n_hot entries in the reference's order — the n_cold entries below can
 * never be visited, k_chain_linked.hip); gmax (-1: GC-exact's bail-out); and what :23250-23272 carries into the next batch: carry_status 0
 * with saved = 0 (`continue`: best chain ends in a carried or fresh anchor) or saved = 1 and carry_S / carry_P / carry_rows [n_carry], or
 * a negative status when the device refuses (slice reaches the cold entries, bail-out) or the reference raises. Rows that the device's fields cannot carry
 * (l outside 0 ... 65535, q or q + l outside int32, s outside int16) are refused with VM_ERR_UNSUPPORTED, as by vm_chain_global_batch. */
typedef struct vm_linked_out {
    int64_t gmax, n_hot, n_cold, opcount; double cold_max;
    double* S; int64_t* P; int64_t* S_arg_hot;
    int32_t carry_status, saved; int64_t n_carry; double* carry_S; int64_t* carry_P; int64_t* carry_rows; double carry_g_max_scores; int64_t carry_prereadloc;
} vm_linked_out;
int vm_chain_linked(vm_ctx*, int which, int kmersize, double skipcost, int maxdiff, int maxgap, int64_t n, const int64_t* rows, int64_t n_pre,
                    const double* pre_S, const int64_t* pre_P, double g_max_scores, int64_t g_max_index, int64_t prereadloc, vm_linked_out* out);
void vm_linked_out_free(vm_linked_out*);

/* `mp.k_cigar(target, query, match, mismatch, o1, e1, o2, e2, bw=-1, zdropvalue=-1, eqx)` (:21554): global dual-affine
 * alignment with traceback, n problems. t/q concatenated with offsets [n+1]. out: CIGAR strings concatenated
 * (NUL-separated) with cigar_off[n+1], scores[n] */
typedef struct vm_score { int32_t match, mismatch, o1, e1, o2, e2; } vm_score;
int vm_k_cigar_batch(vm_ctx*, const vm_score*, int eqx, int64_t n, const char* t, const int64_t* t_off, const char* q,
                     const int64_t* q_off, char** cigars, int64_t** cigar_off, int32_t** scores);
/* The same problems through vm_align_batch's gap fill (mammap_clrnano.py:21554, :21598 call sites), as one chunk with the batch's traceback
 * layout and queue order: longest-first device queue, banded eight-per-wavefront fill first (anti-diagonal form on a fixed band of 32 * ns
 * diagonals, traceback slots as wide as each problem's own band needs), the problems whose band is not PROVEN optimal filled again in full
 * by a second launch, per-problem layout flag for the traceback. CIGARs must equal vm_k_cigar_batch's. band_flag[n]: 16 + ns = the band's
 * result was proven and kept, 1 = a larger problem of the second launch in the packed whole-wave layout, 0 = full matrix. stats[6] = {small
 * problems tried in a band, proven, sent to the second launch (not proven, or small but never tried), problems outside the small class,
 * second-launch problems kept from a wave-wide band, second-launch problems of that class filled in full}. No scores (that form never
 * captures them). */
int vm_k_cigar_batch_banded(vm_ctx*, const vm_score*, int eqx, int64_t n, const char* t, const int64_t* t_off, const char* q,
                            const int64_t* q_off, char** cigars, int64_t** cigar_off, int32_t** band_flag, int64_t* stats);
/* `mp.k_cigar(..., 4,4,4,4, bw=100, zdropvalue=50)` (:2381): banded x-drop extension from (0,0) (spec VMX-DP-X); out t_e[n], q_e[n],
 * score[n]. bw: the band |i - j| <= bw, 0 <= bw <= 496; bw < 0 = no band, accepted when every problem has a side of at most 496 bases.
 * Anything else returns VM_ERR_UNSUPPORTED and computes nothing: the kernel's LDS ring holds a diagonal of at most 497 cells.
 * vm_k_cigar with zdrop >= 0 takes this path with its bw. */
int vm_k_extend_batch(vm_ctx*, int match, int mismatch, int o, int e, int bw, int zdrop, int64_t n, const char* t,
                      const int64_t* t_off, const char* q, const int64_t* q_off, int32_t** t_e, int32_t** q_e, int32_t** score);
/* single-problem form with the reference's argument list; out mirrors the returned tuple (cigar, q_e, t_e) */
typedef struct vm_cigar_out { char* cigar; int32_t q_e, t_e, score; } vm_cigar_out;
int vm_k_cigar(vm_ctx*, const char* t, int64_t tl, const char* q, int64_t ql, const vm_score* sc, int bw, int zdrop,
               int eqx, vm_cigar_out* out);
/* `edlib.align(query, target, task='distance')['editDistance']` (:19251), n problems */
int vm_edit_distance_batch(vm_ctx*, int64_t n, const char* q, const int64_t* q_off, const char* t, const int64_t* t_off,
                           int64_t** dist);
int64_t vm_edit_distance(vm_ctx*, const char* q, int64_t ql, const char* t, int64_t tl);
/* banded forms used by the divergence filter of vm_align_batch: bound[i] >= editDistance, equal to it when the optimal path stays
 * inside the band; -1 when |len(q) - len(t)| exceeds the tier's window (not eligible). tier 1: four problems per wavefront, band of
 * +-320 rows, window 256; tier 2: one problem per wavefront, +-768 rows, window 512. The filter keeps a segment when
 * bound / min(len) <= maxdivergence and passes it to the next tier (finally the exact kernel) otherwise, so its decisions equal the
 * reference's. */
int vm_edit_distance_bound_batch(vm_ctx*, int tier, int64_t n, const char* q, const int64_t* q_off, const char* t, const int64_t* t_off,
                                 int64_t** bound);

/* ------------------------------------------------------------------ the batched path (the GPU entry) */
/* record = one 9-tuple of get_onemapinfolist (:20760): (readid, contig, strand, q_st, q_en, r_st, r_en, mapq, cigar) */
typedef struct vm_record {
    int32_t read_idx;
    int32_t contig;          /* index into vm_index_seq_info */
    int32_t strand;          /* +1 '+', -1 '-' (label as emitted by the reference, :20760/:20776/:20810/:20826) */
    int32_t mapq;
    int64_t q_st, q_en;      /* aligned-strand coordinates (:20762-20763) */
    int64_t r_st, r_en;      /* contig-local */
    int64_t cigar_off, cigar_len;   /* into cigar_blob (NUL-terminated strings) */
} vm_record;

typedef struct vm_batch_stats {     /* measured on the device, for bench.py's roofline arithmetic */
    int64_t n_reads, read_bases, n_minimizers, n_hits, n_anchors, n_local_hits, n_local_anchors;
    int64_t n_segments, n_ed_problems, ed_cells, n_ext_problems, ext_cells, n_dp_problems, dp_cells;
    int64_t n_records, cigar_bytes, aligned_bases, n_unmapped, n_failed;
    int64_t dp_string_bytes;        /* target+query bases read by the gap-fill DP */
    double ms_total;                /* device time of the whole batch (HIP events on the ctx stream) */
    double ms_stage[16];            /* 0 seed, 1 global chain, 2 local, 3 divergence filter, 4 edge extension, 5 gap fill + records,
                                       6 nofilter redo, 7 result download */
    double ms_gapfill_fill;         /* k_gapfill_fill launches only (HIP events on the stream the kernel runs on) */
    double ms_gapfill_trace;        /* k_gapfill_trace launches only */
    int64_t n_gapfill_launches;
    int64_t n_ed_full;              /* divergence-filter problems the banded kernels could not settle (re-run unbanded) */
    int64_t n_ed_tier2;             /* problems the four-per-wave band could not settle (re-run in the wide band) */
    int64_t n_ed_tier1;             /* problems the anchor bound could not settle (re-run in the four-per-wave band) */
    int64_t n_dp_redo;              /* gap-fill problems whose band was not proven optimal (or that were too large to try one): filled again in full */
    int64_t dp_redo_tb_bytes;       /* traceback bytes of those (second pool); dp_cells counts all traceback bytes written */
    double ms_local_seed;           /* k_local_seed, the batch's main launch (HIP events on the stream it runs on) */
    double ms_cluster;              /* k_cluster_big + k_cluster (hit clustering of the seed stage) */
    int64_t n_host_syncs;           /* host waits for the device inside this batch (sizing read-backs + result download) */
    int64_t n_local_general;        /* reads the guide-banded local seeding kernel handed to the general one (k_local_seed) */
    int64_t n_ext_retries;          /* times the batch was run again because a pool of the extend stage was too small (pools x4 per retry) */
    int64_t n_batch_retries;        /* times the whole batch was run again because an assumption made instead of a host wait did not hold (a pool sized from the context's history) */
    int64_t n_dp_redo_wide;         /* of n_dp_redo: larger problems (whole-wave class) whose result the second launch kept from a wave-wide band */
    int64_t n_dp_redo_full;         /* of n_dp_redo: larger problems the second launch filled in full (wide band not proven, no band holds both corners, or scores out of range) */
} vm_batch_stats;

/* Align n reads (replaces get_readmap_DP_test per read). seqs concatenated, offsets[n+1].
 * recs are ordered by (read_idx, emission order of the reference). status_per_read[n]: 0 (n_recs may be 0 = unmapped,
 * :24132) or a negative VM_READ_* (read skipped like the reference's swallowed exception). stats may be NULL. */
int vm_align_batch(vm_ctx*, const vm_index*, const vm_params*, int64_t n_reads, const char* seqs, const int64_t* offsets,
                   vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats);
/* the same with reads already resident in HBM (bench: inputs resident when the timed region starts).
 * vm_reads_upload copies host reads to the device once; vm_align_resident runs the path on them. */
typedef struct vm_reads vm_reads;
int vm_reads_upload(vm_ctx*, int64_t n_reads, const char* seqs, const int64_t* offsets, vm_reads** out);
/* upload another batch into an existing reads object: its device buffers are reused (grow-only); no alignment of it may be in flight. A host thread with a context of
 * its own streams batches into HBM ahead of the aligning contexts — the upload of batch i + 1 runs under the kernels of batch i */
int vm_reads_reupload(vm_ctx*, vm_reads*, int64_t n_reads, const char* seqs, const int64_t* offsets);
void vm_reads_free(vm_reads*);
int vm_align_resident(vm_ctx*, const vm_index*, const vm_params*, const vm_reads*, vm_record** recs, int64_t* n_recs,
                      char** cigar_blob, int32_t* status_per_read, vm_batch_stats* stats);

/* -mode asm on ONE assembly contig, the route of assembly_get_readmap_DP_test (mammap_asm.py:23204): below split_len bases the fork's per-read
 * function (= vm_align_batch with VM_MODE_ASM), otherwise 100 kb seeding windows, chain DPs linked across batches of more than batch_anchors
 * anchors, the second linked round over 9-mer anchors, ass_extend_func. split_len / batch_anchors / window <= 0: the reference's 500000 / 500000 /
 * 100000 (tests shrink them to reach the linked path on small inputs; split_len may only be lowered). p->mode must be VM_MODE_ASM. *status: 0,
 * VM_READ_RAISED, VM_READ_CAPACITY or VM_READ_UNSUPPORTED (see that status). The host runs the reference's loop (batch assembly, tracebacks, cut points); seeding, chain DPs,
 * re-seeding and extension run on the device. */
int vm_align_asm(vm_ctx*, const vm_index*, const vm_params* p, const char* contig, int64_t len, int64_t split_len, int64_t batch_anchors, int64_t window,
                 vm_record** recs, int64_t* n_recs, char** cigar_blob, int32_t* status);

/* Diagnostic for the stage tests of the extend phase (E1 / E3 / E4): runs vm_align_batch's path and returns every read's segment lists
 * as they stand, in the first (filtering) run of extend_func (:19238), after
 *   stage 0  rebuild_chain_break (:23437)
 *   stage 3  divergence filter, both rounds of extend_edge_test (:2302) and the drop_misplaced_alignment_test loop (:726)
 *   stage 5  merge_conjacent_alignment (:16736) and fix_simple_inv (:24226)
 * rows: int64 (segment index, q, r, s, l) concatenated over the reads, row_off[n + 1] (both vm_free). Reads without a local chain have none. */
int vm_align_trace(vm_ctx*, const vm_index*, const vm_params*, int64_t n_reads, const char* seqs, const int64_t* offsets, int stage,
                   int64_t** rows, int64_t** row_off);

/* ------------------------------------------------------------------ native I/O around the batched path (host threads, no GPU work)
 * SAM text for the records of one batch — the consumer of the path, get_bam_dict_str / _comments (mammap_clrnano.py:20841, :21022) with
 * reassign_mapq (:11661), merged CIGARs (:4773), NM (output_functions.py:300), optional MD / cs (:19012 / :19062), SA tag, S / H clipping,
 * approximate SA CIGARs, CG tag switch, comment copying (:20686). Options mirror the driver's `pdict` keys of those functions. */
typedef struct vm_sam_opts {
    int32_t md, shortcs, cigar2cg, markunbalancetra, hardclip, fakecigar;
    const char* rg_id;           /* RG:Z: value on every line; NULL = none (the reference's driver always sets one, vacmap:211-214) */
    int32_t asm_mode;            /* 1: the emitter of -mode asm, iterator_get_bam_dict_str / _comments (mammap_asm.py:22757, :22942): NM = the CIGAR's X / D / I
                                  * counts as mergecigar_nm_ takes them (:23125), MAPQ written as 60 (1 for 0) in the column and in SA, the second record
                                  * primary when the first has MAPQ 1 and it has not (:22847-22850) */
    int32_t keep_unmapped;       /* 1: a read that emits no record line emits one unmapped line instead (FLAG 4, see vm_sam_emit). Lies in what was the
                                  * struct's tail padding: its size is unchanged, and a caller that zeroes the struct has the option off */
} vm_sam_opts;
/* reads as blobs with offsets[n + 1] (quals / comments and their offsets may be NULL; a read whose quality string is empty or of another
 * length than its sequence gets '*'); recs / cigar_blob / status as returned by vm_align_batch for these reads. text: the lines
 * ('\n'-terminated) of all reads in read order, text_off[n + 1] delimits every read's lines (both vm_free). A read whose emission raises in
 * the reference (index past a sequence end) or whose status is not 0 emits no record line and counts in n_skipped, like the worker's except
 * (:24127-24134); a read without records emits none either.
 * keep_unmapped = 0: such a read emits nothing (the reference's behaviour). keep_unmapped = 1: it emits exactly one line, at its place in the text,
 *   QNAME 4 * 0 0 * * 0 0 SEQ QUAL [RG:Z:rg_id] [comment fields]
 * MAPQ 0 (the SAM specification's recommended practice for an unmapped read); SEQ the read as given, whole and in its own orientation whatever
 * hardclip says, '*' for an empty read; QUAL by the record lines' rule; the comment fields by the record lines' filter (:20686), the line's own tags
 * being SA, NM, MD, cs (never copied) and RG under rg_id; no NM, SA, MD, cs; asm_mode changes nothing on it. n_lines counts these lines; n_skipped
 * keeps its meaning (status not 0, or the emission raised). A read that emits record lines emits them unchanged. */
int vm_sam_emit(const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs, const int64_t* seq_off,
                const char* quals, const int64_t* qual_off, const char* comments, const int64_t* com_off, const vm_record* recs, int64_t n_recs,
                const char* cigar_blob, const int32_t* status, int nthreads, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped);
/* The same lines made on the GPU (k_sam.hip: merged CIGAR, NM, MD / cs, SA and the line text are device work; the host validates, uploads and
 * fetches the text): vm_sam_emit's arguments without comments and nthreads, plus the context whose stream and buffers the call uses (one call at a
 * time per context; any number of contexts may share an index). Returns what vm_sam_emit returns for the same inputs byte for byte, text_off, n_lines
 * and n_skipped included (text and text_off: vm_free), under keep_unmapped too: the unmapped lines are made by a wave per read (k_sam_unmapped), also in
 * a batch without any record. VM_ERR_UNSUPPORTED when the index keeps a host copy of a reference with letters other than
 * ACGTN (the device holds N for them, vm_sam_emit prints them); comments are copied by vm_sam_emit_device_comments below. VM_ERR_ARG for what vm_sam_emit refuses, for
 * a record of an unknown contig and for a CIGAR operator count of 2^31 or more. Three host waits per call.
 * vm_sam_emit_device_times: wall seconds of the context's latest call (either entry): upload, passes, the text's way back. */
int vm_sam_emit_device(vm_ctx*, const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const char* quals, const int64_t* qual_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob,
                       const int32_t* status, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped);
/* vm_sam_emit_device that also copies the reads' comments (emit_read()'s rule of :20686, applied by k_sam_lines): comments / com_off as vm_sam_emit
 * takes them, after qual_off. comments == NULL or com_off == NULL: no comments, exactly vm_sam_emit_device. The blob is uploaded from its first to its
 * last used byte. VM_ERR_ARG also for decreasing com_off and for a NULL blob under offsets that span bytes. Returns vm_sam_emit's bytes, text_off,
 * n_lines and n_skipped for the same inputs; under keep_unmapped the unmapped lines carry their reads' comment fields as vm_sam_emit's do. */
int vm_sam_emit_device_comments(vm_ctx*, const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                                const int64_t* seq_off, const char* quals, const int64_t* qual_off, const char* comments, const int64_t* com_off,
                                const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text, int64_t** text_off,
                                int64_t* n_lines, int64_t* n_skipped);
int vm_sam_emit_device_times(vm_ctx*, double* seconds3);
/* PAF text for the same records. THE RULE: a PAF line exists exactly where vm_sam_emit writes a record line for the same inputs and options; the reads
 * skipped (status not 0, or the emission raises), reassign_mapq under markunbalancetra, the order inside a read (span descending, the later record first
 * among equals), text_off[n + 1], n_lines and n_skipped are vm_sam_emit's. The line of a record, in that order:
 *   QNAME qlen qs qe strand TNAME tlen r_st r_en nmatch alen MAPQ tp:A:P NM:i:nm [cg:Z:cg] [MD:Z:md cs:Z:cs]        (tab-separated, '\n' at the end)
 * qlen: the read's length. qs, qe: on the read as sequenced, q_st / q_en for '+' and qlen - q_en / qlen - q_st for '-', printed as signed integers and
 * not clamped. tlen: the contig's length in the index. r_st, r_en: as the record holds them. MAPQ and nm: the numbers the SAM line prints in its MAPQ
 * column and in NM:i: (asm_mode's 60 / 1 and its NM rule included). alen: the sum of the lengths of the merged CIGAR's M = X I D operators. nmatch:
 * alen - nm, signed (defined from the line's own NM: a PAF line raises exactly where the SAM line does, and no mode walks the sequences once more).
 * cg: the merged CIGAR text without its leading maximal run of S / H operators and without its trailing one (interior S / H stay); when nothing is
 * left the tab and the field are omitted; cigar2cg's '*' rule does not apply. md set: MD:Z: and cs:Z: with the SAM line's strings (empty where SAM
 * prints them empty; shortcs as in SAM). No SEQ, QUAL, RG, SA or comment fields: hardclip, fakecigar, cigar2cg and rg_id change nothing.
 * keep_unmapped: a read that emits no record line emits
 *   QNAME qlen 0 0 * * 0 0 0 0 0 0
 * at its place; it counts in n_lines, and n_skipped keeps its meaning.
 * vm_paf_emit: vm_sam_emit's arguments without quals / qual_off and comments / com_off; host threads as vm_sam_emit uses them. */
int vm_paf_emit(const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs, const int64_t* seq_off,
                const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, int nthreads, char** text, int64_t** text_off,
                int64_t* n_lines, int64_t* n_skipped);
/* The same lines (THE RULE above) made on the GPU: vm_sam_emit_device's arguments without quals / qual_off. The records, their order, the merged CIGAR,
 * NM, MD and cs come from the SAM emitter's kernels (k_sam_count, k_sam_order, k_sam_ops); the lines from k_paf_lines (k_paf.hip), which also finds alen
 * and the cg range in the merged text. Returns vm_paf_emit's bytes, text_off, n_lines and n_skipped for the same inputs (text and text_off: vm_free).
 * VM_ERR_UNSUPPORTED and VM_ERR_ARG as vm_sam_emit_device returns them. Three host waits per call; vm_sam_emit_device_times covers this entry too. */
int vm_paf_emit_device(vm_ctx*, const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text,
                       int64_t** text_off, int64_t* n_lines, int64_t* n_skipped);
/* Per-window depth of coverage from the same records. An accumulator (vm_depth) is made for one index, a window size W >= 1 and a MAPQ threshold Q.
 * THE RULE.
 * Windows: contig c of length L_c has ceil(L_c / W) windows, window j covers [jW, min((j + 1)W, L_c)); the windows of all contigs are concatenated in
 * index order and win_off[nseq + 1] delimits each contig's windows (a contig of length 0 has none).
 * Which records count: a record contributes exactly when vm_sam_emit writes a record line for it for the same inputs and options (a read with a status
 * other than 0, a read without records and a read whose emission raises contribute nothing) and the number that line prints in its MAPQ column (after
 * reassign_mapq under markunbalancetra; asm_mode's 60 / 1) is >= Q.
 * What a record contributes: its CIGAR is walked in the order the SAM line prints it, from the 0-based contig-local r_st. M = X D N advance the reference
 * position, I S H P do not. Every reference position under an M, = or X counts 1; positions under D and N count 0 (samtools depth without -J). Merging
 * adjacent operators changes nothing, so an implementation may walk the record's own text or the merged text. A position below 0 or at or beyond L_c
 * counts nothing.
 * Unaffected by: keep_unmapped lines count nothing; hardclip, fakecigar, cigar2cg, md, shortcs and rg_id change nothing.
 * What accumulates: counts[w] = the number of (record, position) pairs counted inside window w, int64, summed over every call since creation. Sums of
 * integers do not depend on order: every implementation, schedule, split of the reads into calls and number of ranks gives identical counts.
 * Text (integers only, so every build prints the same bytes): VM_DEPTH_REGIONS is one line per window, empty ones included, contigs in index order,
 *   TNAME \t start \t end \t mean \n
 * VM_DEPTH_SUMMARY one line per contig,
 *   TNAME \t length \t bases \t mean \n
 * (bases = the sum of the contig's counts, mean taken over length) and a last line "total" over all contigs. mean of (count, len) has exactly two
 * decimals: h = (200 * count + len) div (2 * len) hundredths (half up; h = 0 when len = 0), printed as h div 100, '.', and two digits of h mod 100.
 * vm_depth_create: with a context the counts live in that context's HBM, without one in host memory. VM_ERR_ARG for window < 1, min_mapq outside
 * 0 .. 255 and more than 2^28 windows in all.
 * vm_depth_add: host code on a host accumulator (VM_ERR_ARG on a device one); vm_paf_emit's arguments up to nthreads and its refusals; it shares the
 * host emitters' per-record stage, so the raises are theirs. Threads add with atomic integer adds.
 * vm_depth_add_device: vm_paf_emit_device's arguments up to status, on the context the accumulator was made on (VM_ERR_ARG otherwise); k_sam_count,
 * k_sam_order and k_sam_ops as they are, then k_depth_add (k_depth.hip). No line text; n_lines and n_skipped are vm_sam_emit's. Refusals: the device SAM
 * entry's. Two host waits.
 * vm_ctx_attach_depth (NULL detaches): while an accumulator made on the context is attached, every vm_sam_emit_device, vm_sam_emit_device_comments and
 * vm_paf_emit_device call on the context also launches k_depth_add behind the write pass of k_sam_ops, on the same stream: no additional host wait, no
 * additional upload, the same returned bytes, the counts of a stand-alone vm_depth_add_device on the same inputs. The index must be the accumulator's
 * (VM_ERR_ARG). A call refused for its arguments or records adds nothing.
 * vm_depth_merge: dst += src for any mix of host and device accumulators; VM_ERR_ARG unless contig lengths and window agree. vm_depth_add_counts:
 * dst += a table that vm_depth_counts returned (another process's, say); VM_ERR_ARG unless n_windows is the accumulator's.
 * vm_depth_counts: host copies of counts[n_windows] and win_off[nseq + 1] (both vm_free). vm_depth_text: which = VM_DEPTH_REGIONS / VM_DEPTH_SUMMARY
 * (text: vm_free, n bytes, 0-terminated); a device accumulator makes the text on the device (k_depth_sums, k_depth_lines), a host one in host code. */
typedef struct vm_depth vm_depth;
enum { VM_DEPTH_REGIONS = 0, VM_DEPTH_SUMMARY = 1 };
int vm_depth_create(vm_ctx* ctx_or_null, const vm_index*, int64_t window, int min_mapq, vm_depth** out);
void vm_depth_free(vm_depth*);
int vm_depth_add(vm_depth*, const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                 const int64_t* seq_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, int nthreads, int64_t* n_lines,
                 int64_t* n_skipped);
int vm_depth_add_device(vm_depth*, vm_ctx*, const vm_index*, const vm_sam_opts*, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                        const int64_t* seq_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, int64_t* n_lines,
                        int64_t* n_skipped);
int vm_ctx_attach_depth(vm_ctx*, vm_depth* depth_or_null);
int vm_depth_merge(vm_depth* dst, vm_depth* src);
int vm_depth_add_counts(vm_depth* dst, const int64_t* counts, int64_t n_windows);
int vm_depth_counts(vm_depth*, int64_t** counts, int64_t** win_off, int64_t* n_windows);
int vm_depth_text(vm_depth*, int which, char** text, int64_t* n);
/* `mp.fastx_read(path, read_comment=)` (vacmap:445): FASTA / FASTQ, plain or gzip. vm_fastx_read returns up to max_reads records (stopping
 * early once max_bases bases are held) as blobs: names, UPPER-CASED sequences (vacmap:476), qualities (empty for FASTA), comments (header
 * text after the first blank, else tab). Returns the record count, 0 at the end of the input, or a negative vm_status. */
/* entries idx[0..n) of a blob copied back to back (out may be NULL to size it): returns the byte count, out_off[n + 1] */
int64_t vm_blob_gather(const char* blob, const int64_t* off, const int64_t* idx, int64_t n, char* out, int64_t* out_off);
/* the same over several blobs: output entry j = entry idx[j] of blob part[j]; returns the bytes written (out must hold them) */
/* the same merge into a regular file through a shared mapping, copied by nthreads threads: the file is extended from file_off (its current end) by the
 * merged size. Returns the bytes written, -1 on error, -2 when fd cannot be mapped (pipe, terminal): use vm_blob_write_parts then */
int64_t vm_blob_write_parts_mmap(int fd, int64_t file_off, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n, int nthreads);
int64_t vm_blob_gather_parts(const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n, char* out);
/* page-locked host memory for the read blobs a caller hands to vm_align_batch: the upload is then a DMA the host thread does not wait for
 * (from pageable memory the runtime stages it through bounce buffers on the calling thread: ~10 ms per 60 MB batch, more under memory load) */
void* vm_pinned_alloc(int64_t bytes, int device);      /* device: the GPU the calling process works on (the allocation must not open a context on GPU 0 from every rank); -1 = the thread's current one */
void vm_pinned_free(void* p);
/* vm_blob_gather_parts written to a file descriptor with writev() instead of into a buffer; returns the bytes written or -1 */
int64_t vm_blob_write_parts(int fd, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n);
typedef struct vm_fastx vm_fastx;
int vm_fastx_open(const char* path, vm_fastx** out);
/* the records whose FIRST byte lies in [begin, end) of a plain FASTA / FASTQ file (end < 0: to the end of the file): N readers over N consecutive
 * ranges see every record exactly once — the sharded driver gives every rank a range and its parser threads slices of it (the reference has one
 * reader process, vacmap:445-497). Compressed input: VM_ERR_UNSUPPORTED for begin > 0. */
int vm_fastx_open_range(const char* path, int64_t begin, int64_t end, vm_fastx** out);
void vm_fastx_close(vm_fastx*);
int64_t vm_fastx_read(vm_fastx*, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs, int64_t** seq_off, char** quals,
                      int64_t** qual_off, char** comments, int64_t** com_off);

/* ------------------------------------------------------------------ BAM output (SAMv1 §4.2, BGZF §4.1) on the device
 * A writer holds the header's @SQ names (device hash table) and grow-only device / page-locked buffers; use it from one thread at a time.
 * SAM text is split at its newlines, every line becomes one BAM record (refID from the @SQ order, '*' = -1, RNEXT '=' = RNAME's; bin =
 * reg2bin(pos, pos + reference span, 1 for CIGAR '*'); above 65 535 CIGAR operations <qlen>S<span>N plus a CG:B,I tag; 'i' tags in the
 * smallest of c C s S i I; 'f' as strtod + a cast to float). A malformed line makes the call return VM_ERR_ARG and vm_last_error() names
 * its 1-based line number in the call's text. Results are malloc'ed (vm_free). BGZF members hold <= 65 280 input bytes each, carry no EOF
 * marker, and depend on the input bytes only. */
typedef struct vm_bam_writer vm_bam_writer;
int vm_bam_writer_create(vm_ctx*, const char* sam_header, int64_t len, vm_bam_writer** out);
void vm_bam_writer_free(vm_bam_writer*);
/* the BAM header (magic, l_text, text, n_ref, references) as BGZF members */
int vm_bam_header(vm_bam_writer*, char** out, int64_t* n);
/* uncompressed BAM records of the lines of sam[0, len) */
int vm_bam_encode(vm_bam_writer*, const char* sam, int64_t len, char** out, int64_t* n);
/* the lines of entries idx[j] of blob part[j] (the arguments of vm_blob_gather_parts), encoded and compressed into BGZF members */
int vm_bam_compress_parts(vm_bam_writer*, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n,
                          char** out, int64_t* n_out);
/* n arbitrary bytes as BGZF members */
int vm_bgzf_compress(vm_ctx*, const void* in, int64_t n, char** out, int64_t* n_out);

/* BAM input on the GPU (driver: --bam-reader native). vm_bgzf_decompress is the counterpart of vm_bgzf_compress: any series of complete BGZF
 * members (any writer's: stored, fixed and dynamic blocks, empty members, with or without the EOF block) -> their bytes (vm_free). A member
 * that does not inflate to its ISIZE and CRC32 makes the call fail with VM_ERR_IO; vm_last_error() names the member's offset.
 * vm_bam_reader_open: VM_ERR_UNSUPPORTED when the file is gzip without the BGZF BC subfield, VM_ERR_ARG when the inflated stream does not begin
 * with BAM\1, VM_ERR_IO for everything else that is wrong with the file. vm_bam_reader_read has vm_fastx_read's signature and return
 * convention: names, bases (a reverse-strand record turned back to the read's orientation: reversed, ACGTN complemented) and qualities + 33
 * (empty when the record has none); comments are empty unless the reader was opened with tags (vm_bam_reader_open_tags); records without bases are dropped. The reader reads the file ahead on a thread
 * of its own. vm_bam_reader_stats: seconds of I/O thread work, waiting for it, upload + inflate, record walk, sizes + scans + decode, download,
 * handing out; then windows, file bytes, inflated bytes, records handed to the caller's windows, records dropped (12 numbers; a 13th with tags: auxiliary fields left out), as of the
 * latest window the caller has begun to take (the window decoded ahead is not in them yet).
 * An open reader owns its context (it decodes ahead on a thread of its own): close it before other calls use the context or destroy it. */
int vm_bgzf_decompress(vm_ctx*, const void* in, int64_t n, char** out, int64_t* n_out);
typedef struct vm_bam_reader vm_bam_reader;
int vm_bam_reader_open(vm_ctx*, const char* path, vm_bam_reader** out);
/* vm_bam_reader_open that also carries the records' auxiliary fields (SAMv1 4.2.4) to the caller: vm_bam_reader_read then fills comments / com_off
 * with every read's selected fields as SAM text, `XX:T:value` joined by one tab in record order, made on the GPU (the form vm_sam_emit appends
 * as a read's comment). tags: NULL or "" = exactly vm_bam_reader_open; "*" = every field; otherwise two-character tags separated by commas
 * ("MM,ML,MN"); anything else is VM_ERR_ARG. A c C s S i I -> :A: / :i:, f -> :f: (the shortest %.{p}g, p = 1 ... 9, that strtod and a cast read
 * back as the same float32), Z / H verbatim, B -> :B:t,v1,v2,... Duplicated tags are passed through; nothing is re-oriented for a reverse-strand
 * record (MM / ML and the kinetics arrays are defined on the read as sequenced, which is what the reader restores). A field that SAM text
 * cannot hold (a byte outside 0x20-0x7e in A or Z, an H that is not an even number of hex digits, a non-finite f or B:f element) is left out
 * and counted: the 13th number of vm_bam_reader_stats. Malformed aux data (fewer than 3 bytes left, an unknown type or sub-type, a value,
 * string or array that runs past the record) fails the read with VM_ERR_IO, the first bad record named. Aux bytes are looked at only when
 * tags were asked for, and never in a record that is dropped for having no bases. */
int vm_bam_reader_open_tags(vm_ctx*, const char* path, const char* tags, vm_bam_reader** out);
int64_t vm_bam_reader_read(vm_bam_reader*, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs, int64_t** seq_off, char** quals,
                           int64_t** qual_off, char** comments, int64_t** com_off);
int vm_bam_reader_stats(const vm_bam_reader*, double* out, int n);
void vm_bam_reader_close(vm_bam_reader*);

/* Plain gzip on the GPU. vm_gzip_decompress: any series of complete gzip members (RFC 1952: any writer's, FEXTRA / FNAME / FCOMMENT / FHCRC
 * headers, stored, fixed and dynamic blocks, empty members, zero bytes between members) -> their bytes (vm_free). A member's deflate stream has
 * no index, so it is inflated in parallel chunks: block starts are searched for in every VMX_GZ_CHUNK compressed bytes (environment; default
 * 32768, at least 1024), every start is decoded by a wavefront of its own with the unknown 32 KB in front of it kept as markers, the chain of
 * chunks is linked (a start that the chain steps over was a false candidate and is dropped), the 32 KB windows are passed along, and the
 * markers are replaced. Every member's CRC32 and ISIZE are checked. Errors: VM_ERR_IO for input that is truncated ("truncated"),
 * for a bad code, distance or stored length (the message names the file offset of the block), for a member whose CRC32 or ISIZE does not match
 * (its file offset) and for anything that is not a gzip member where one must begin; VM_ERR_UNSUPPORTED for more than 256 MB of compressed
 * data or 4 GB of text in one call.
 * vm_gzip_decompress_stats is the same call and also fills stats[0, n_stats), whether it succeeds or not: chunks started (waves that began
 * decoding), candidates rejected by the link check, chunks decoded again after a rejection, text bytes decoded by the first chain (the wave
 * that starts at the first member's header), then seconds in the search, the count and write passes with the link check, the window pass,
 * the marker pass (8 numbers). Device memory of a call: 3 bytes per text byte, the compressed data, and 32 KB per chunk started. */
int vm_gzip_decompress(vm_ctx*, const void* in, int64_t n, char** out, int64_t* n_out);
int vm_gzip_decompress_stats(vm_ctx*, const void* in, int64_t n, char** out, int64_t* n_out, double* stats, int n_stats);

/* Bgzipped FASTQ on the GPU (driver: --fastx-reader native): the BGZF members of x.fastq.gz are inflated as for BAM input and the text is parsed on
 * the device into the four blobs of vm_fastx_read, by vm_fastx_read's own rule for four-line FASTQ:
 *   lines     a line ends at '\n', one trailing '\r' is dropped; the bytes after the file's last '\n' form a line if there are any.
 *   blank     a line is blank when, after that drop, every byte is a space, a tab or '\r' (an empty line is blank).
 *   states    0 expects a header, 1 the bases, 2 the '+' line, 3 the qualities. In state 0 a blank line is skipped and any other line is a
 *             header; in states 1, 2 and 3 every line, blank or not, is taken and leads to the next state (3 leads to 0). So blank lines are
 *             skipped between records only, an empty bases or quality line is an empty field, the '+' line is not looked at, and a quality
 *             line may begin with '@'.
 *   header    byte 0 is '@'; the name is what follows up to the first space or tab, the comment everything behind that one separator
 *             (empty without one): "@ x" has an empty name and the comment "x".
 *   fields    in the bases a-z become upper case, every other byte stays; qualities are copied as they are; the two lengths are not compared.
 * Errors: the file ends in state 1, 2 or 3: VM_ERR_IO, "truncated FASTQ record". A header whose byte 0 is neither '@' nor '>': VM_ERR_IO,
 * "not FASTA/FASTQ: " and the line's first 40 bytes. A header that begins with '>': VM_ERR_UNSUPPORTED (vm_fastx_read would read a multi-line
 * FASTA record there; this reader is FASTQ only), the message names the 1-based record. A header is judged as soon as its line is complete, whether or not
 * the record's other lines exist. As with vm_fastx_read, the call that meets an error returns only the error: the records in front of a bad
 * header have been handed out by earlier calls as far as those calls reached, and what the failing call had gathered is dropped. A truncated, non-BGZF or corrupt member (CRC32, ISIZE) later in the file: VM_ERR_IO, the message names its file offset.
 * vm_fastq_reader_open reads up to the first record: VM_ERR_UNSUPPORTED when the file is not gzip, is gzip without the BGZF BC subfield, or its
 * first record begins with '>' (use vm_fastx_open then); VM_ERR_IO for an empty or unreadable file. vm_fastq_reader_read has vm_fastx_read's
 * signature and return convention. vm_fastq_reader_stats: seconds of I/O thread work, waiting for it, upload + inflate, newlines + states +
 * records, sizes + scans + copy, download, handing out; then windows, file bytes, inflated bytes, records (11 numbers), as of the latest window
 * the caller has begun to take.
 * An open reader owns its context (it parses ahead on a thread of its own): close it before other calls use the context or destroy it. */
typedef struct vm_fastq_reader vm_fastq_reader;
int vm_fastq_reader_open(vm_ctx*, const char* path, vm_fastq_reader** out);
/* vm_fastq_reader_open with options. flags 0: exactly vm_fastq_reader_open. VM_READER_GZIP_DEVICE: a file whose first member lacks the BGZF BC
 * subfield (plain gzip: gzip, pigz, a basecaller's output, concatenated .gz files) is inflated on the GPU in parallel chunks (vm_gzip_decompress's
 * kernels) instead of being refused: the file is taken in windows of VMX_BAM_IN_CHUNK compressed bytes; carried from window to window are the bit
 * position of the next block (always a verified block start or a member header), the 32 KB in front of it on the device, and the running CRC32 and size
 * of the open member; of a window's chain the leading chunks whose text fits VMX_BAM_IN_MAXINF are taken (always one), the rest start the next
 * window. The file is read ahead on a thread of its own while the device works on a window. A single block that does not end inside one window's
 * compressed bytes: VM_ERR_UNSUPPORTED (use vm_fastx_open); from vm_fastq_reader_open the caller can fall back, from a later vm_fastq_reader_read
 * records have been handed out and the refusal is fatal to the run (with the default VMX_BAM_IN_CHUNK of 64 MB no deflate writer makes such a block). Truncation, a bad code,
 * distance or stored length, a CRC32 or ISIZE mismatch: VM_ERR_IO with the file offset of the block or member, from the read call that reaches it.
 * vm_fastq_reader_stats then has 8 more numbers behind its 11, of the windows inflated so far: chunks started, candidates rejected, chunks decoded
 * again, text bytes of the file's first chain, seconds in find / decode / window / resolve.
 * VM_READER_FASTA (alone or with VM_READER_GZIP_DEVICE): the reader parses by vm_fastx_read's whole rule, FASTA records included, and hands out its
 * four blobs. Lines and blank lines as above; a line whose byte 0 is '>' is class G, any other line that is not blank class O. States: 0 between
 * records, 1 - 3 the FASTQ states, 4 inside a FASTA record. State 0: a blank line is skipped, G starts a FASTA record (-> 4), O starts a FASTQ
 * record (-> 1; byte 0 must be '@', else VM_ERR_IO "not FASTA/FASTQ: " and the line's first 40 bytes). States 1, 2, 3 take any line (-> 2, 3, 0).
 * State 4: G starts the next FASTA record, every other line, blank or not, '@...' and '+' lines too, is body (-> 4). Header of both kinds: the
 * name is bytes 1 to the first space or tab, the comment everything behind that one separator. A FASTA body line, after the '\r' drop, is
 * stripped of spaces and tabs (not '\r') at both ends, upper-cased and appended; interior bytes stay. FASTQ lines are whole. A FASTA record has
 * empty qualities, and one without body lines empty bases. The file may end in state 4 (the last record is complete); ending in state 1, 2 or 3
 * is "truncated FASTQ record". VM_ERR_UNSUPPORTED for '>' does not occur. A record is carried from window to window until the line that starts
 * the next record (or the file's end) is in the window: device memory alone bounds its length. Without this flag the reader is exactly the
 * FASTQ-only one, the same kernels included. Flag bits other than these two: VM_ERR_ARG. */
#ifndef VM_READER_GZIP_DEVICE
#define VM_READER_GZIP_DEVICE 1
#endif
#define VM_READER_FASTA 2
int vm_fastq_reader_open_opts(vm_ctx*, const char* path, int flags, vm_fastq_reader** out);
int64_t vm_fastq_reader_read(vm_fastq_reader*, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs, int64_t** seq_off, char** quals,
                             int64_t** qual_off, char** comments, int64_t** com_off);
int vm_fastq_reader_stats(const vm_fastq_reader*, double* out, int n);
void vm_fastq_reader_close(vm_fastq_reader*);

/* Coordinate-sorted BAM and its CSI index (driver: --bam-writer native-sort). Order: ascending uint32(refID) << 32 | uint32(pos + 1) << 1 | reverse
 * strand, ties in the order the lines arrived; refID -1 last. An external sort: every vm_bam_sorter_add_parts call encodes its lines and returns
 * their records in sorted order, uncompressed (a run; the caller writes it to a file of its own, an empty call leaves no run); the sorter keeps
 * the run's keys and record sizes. vm_bam_sorter_plan takes the run files' paths in call order and file_base = the bytes the output file holds
 * already (the header's members), sorts all keys once and cuts the output into *n_chunks chunks of about chunk_bytes record bytes;
 * vm_bam_sorter_chunk(k), called for k = 0, 1, ... in order, returns chunk k's BGZF members (possibly none) and records its index entries;
 * vm_bam_sorter_index returns the complete .csi file (min_shift 14, depth 5, BGZF with the EOF member). The sorter borrows the writer: free it first. */
typedef struct vm_bam_sorter vm_bam_sorter;
int vm_bam_sorter_create(vm_bam_writer*, int64_t chunk_bytes, vm_bam_sorter** out);
void vm_bam_sorter_free(vm_bam_sorter*);
int vm_bam_sorter_add_parts(vm_bam_sorter*, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n,
                            char** out, int64_t* n_out);
int vm_bam_sorter_plan(vm_bam_sorter*, const char* const* run_paths, int64_t n_paths, int64_t file_base, int64_t* n_chunks);
int vm_bam_sorter_chunk(vm_bam_sorter*, int64_t k, char** out, int64_t* n_out);
int vm_bam_sorter_index(vm_bam_sorter*, char** out, int64_t* n_out);

/* cost tables C0 as uploaded to the device (tests): which = 0 extra,1 readgap_h,2 readgap_r,3 large_readgap (f32),
 * 4 log2cache, 5 log2int (f64). returns length, *data = host copy read back FROM THE DEVICE (vm_free) */
int64_t vm_table(vm_ctx*, int which, void** data);

void vm_free(void*);
const char* vm_last_error(void);
const char* vm_version(void);

#ifdef __cplusplus
}
#endif
#endif
