// vmx_sam_dev.h — the device SAM emitter (k_sam.hip: kernels, vmx_sam_dev.hip: host side). What it computes is vm_sam_emit's
// emit_read() (vmx_sam.hip), byte for byte; DESIGN §7d describes the passes.
#ifndef VMX_SAM_DEV_H
#define VMX_SAM_DEV_H
#include "vmx_host.h"

// everything a call reads, as device pointers. The read blobs are uploaded from their first used byte: *_base is what has to be taken off an offset.
struct vmx_sam_in {
    int64_t n_reads, n_recs;
    const char* names; const int64_t* name_off; int64_t name_base;
    const char* seqs; const int64_t* seq_off; int64_t seq_base;
    const char* quals; const int64_t* qual_off; int64_t qual_base;      // quals == nullptr: no qualities at all
    const char* comments; const int64_t* com_off; int64_t com_base;     // comments == nullptr: no read has a comment
    const vm_record* recs; const char* cigars; int64_t cigars_len;
    const int32_t* status;                                              // nullptr: every read has status 0
    const uint8_t* codes; const int64_t* coff; int32_t nseq;            // the index's reference codes (0..3 = ACGT, 4 = N) and contig offsets[nseq + 1]
    const char* cnames; const int64_t* cname_off;                       // contig names back to back, offsets[nseq + 1]
    int32_t md, shortcs, cigar2cg, markunbalancetra, hardclip, fakecigar, asm_mode, keep_unmapped;
    const char* rg; int32_t rg_len;                                     // rg == nullptr: no RG:Z: tag
};

// per emitted record (position p = first[read] + rank in the emitted order)
// LINE SLOTS. Without keep_unmapped a line is a record: slot = p, n_recs slots. With it every read has one slot more, behind its records' slots, for
// its unmapped line (size 0 when the read emits record lines): the slot of position p of read r is p + r, the read's own slot first[r + 1] + r,
// n_recs + n_reads slots in read order. vmx_sam_slot / vmx_sam_slots say so; read r's lines begin at loff[vmx_sam_slot(A, first[r], r)].
struct vmx_sam_rinfo { int64_t cig_len, md_len, cs_len, n_ops, nm; int32_t flags, pad; };
enum { VMX_SAM_F_RAISED = 1, VMX_SAM_F_ABORTED = 2 };                   // the read raises / MD and cs are empty (an operator outside =XIDSH)
enum { VMX_SAM_E_COUNT = 1, VMX_SAM_E_RECORD = 2 };                     // res[0] bits: an operator count >= 2^31 / a record that names no read or no contig

struct vmx_sam_work {
    int64_t* cnt; int64_t* first;                 // records per read, their exclusive scan (n_reads + 1 each)
    int32_t* keep;                                // reassign_mapq's survivors, per record
    int32_t* ord; int32_t* mq; int32_t* flag;     // per emitted position: the record, its MAPQ as written, its FLAG
    int32_t* rflag;                               // per read: 1 = the read raises
    vmx_sam_rinfo* ri;
    int64_t* tsz; int64_t* toff; char* scratch;   // merged CIGAR + MD + cs text per emitted record: sizes, offsets (n_recs + 1), bytes
    int64_t* lsz; int64_t* loff;                  // line sizes and offsets by line slot (vmx_sam_slots + 1)
    unsigned long long* res;                      // [0] VMX_SAM_E_* bits, [1] lines, [2] skipped reads
};

__host__ __device__ inline int64_t vmx_sam_slot(const vmx_sam_in& A, int64_t p, int64_t r) { return A.keep_unmapped ? p + r : p; }
__host__ __device__ inline int64_t vmx_sam_slots(const vmx_sam_in& A) { return A.n_recs + (A.keep_unmapped ? A.n_reads : 0); }

__global__ void k_sam_count(vmx_sam_in A, vmx_sam_work K);
__global__ void k_sam_order(vmx_sam_in A, vmx_sam_work K);
__global__ void k_sam_ops(vmx_sam_in A, vmx_sam_work K, int write);
__global__ void k_sam_lines(vmx_sam_in A, vmx_sam_work K, char* text, int write);
__global__ void k_sam_unmapped(vmx_sam_in A, vmx_sam_work K, char* text, int write);
__global__ void k_sam_text_off(vmx_sam_in A, vmx_sam_work K, int64_t* text_off);
// k_paf.hip. pinfo: per emitted position (cg begin, cg end, alen), stored by the size pass and loaded by the write pass
__global__ void k_paf_lines(vmx_sam_in A, vmx_sam_work K, int64_t* pinfo, char* text, int write);

// grow-only buffers of a context's device emitter
struct vmx_sam_bufs {
    vmx::DevBuf names, name_off, seqs, seq_off, quals, qual_off, comments, com_off, recs, cigars, status, rg;
    vmx::DevBuf cnt, first, keep, ord, mq, flag, rflag, ri, tsz, toff, scratch, lsz, loff, res, tmp;
    vmx::DevBuf text, text_off;
    vmx::DevBuf pinfo;                                                              // PAF: three int64 per emitted position (k_paf_lines)
    vmx::DevBuf cnames, cname_off; uint64_t names_of = 0;                           // the contig-name blob and the serial of the index it was made for (vm_index.serial: never 0)
    std::string h_cnames; std::vector<int64_t> h_cname_off;
    double s_upload = 0, s_kernel = 0, s_download = 0;                              // wall seconds of the last call by phase
};
struct vmx_sam_totals { int64_t text_bytes, n_lines, n_skipped; };

// The emitter on device pointers: `in` complete but for cnames / cname_off (taken from the context's blob for `mi`). The text lands in S->text
// (tot->text_bytes bytes), the per-read offsets in S->text_off (n_reads + 1). Two host waits; the caller fetches what it wants and waits once more.
// paf: the lines are PAF lines (k_paf_lines in the place of k_sam_lines and k_sam_unmapped; `in` without qualities, comments and rg).
// dep: a depth accumulator made on c (vmx_depth.h) that k_depth_add adds the call's records to, behind the write pass of k_sam_ops; lines = false: no
// line kernel runs and no text is made (vm_depth_add_device: tot->text_bytes = 0, n_lines and n_skipped as ever).
int vmx_sam_emit_dev(vm_ctx* c, const struct vm_index* mi, vmx_sam_in in, vmx_sam_totals* tot, bool paf = false, struct vm_depth* dep = nullptr, bool lines = true);
vmx_sam_bufs* vmx_ctx_sam_bufs(vm_ctx* c);
#endif
