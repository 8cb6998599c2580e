// vmx_index_priv.h — the index object and the build steps shared by vmx_index.hip (build / .vmx) and vmx_mmi.hip (minimap2 .mmi files).
#ifndef VMX_INDEX_PRIV_H
#define VMX_INDEX_PRIV_H
#include "vmx_host.h"
#include "vmx_index_prim.h"
#include <string>
#include <vector>

#include <mutex>
// every index object of the process has a number of its own: what a cache remembers an index by (a freed index's ADDRESS is handed to the next one)
static inline uint64_t vmx_index_next_serial() { static std::atomic<uint64_t> n{0}; return ++n; }
struct vm_index {
    vm_ctx* ctx = nullptr;
    const uint64_t serial = vmx_index_next_serial();
    int k = 0, w = 0, mid_occ = 10, table_bits = 0;
    std::vector<std::string> names;
    std::vector<int64_t> lens, offsets;     // offsets has nseq+1 entries
    std::string bases;                      // upper-case concatenation (host copy for Aligner.seq); empty on replicas (has_host_seq = false)
    int64_t n_min = 0, n_distinct = 0;
    vmx::DevBuf d_codes, d_pos, d_table, d_off;
    bool has_host_seq = true;
    int64_t n_other_letters = 0;            // letters of the uploaded reference that are none of ACGTN (d_codes holds N for them; the host copy keeps them): counted once by vmx_index_upload_codes
    std::once_flag host_seq_once;           // replicas decode their host copy of the bases from HBM once, whichever emitter thread asks first (vmx_sam.hip)
};

static inline unsigned grid1d(int64_t n, int64_t cap = 65536) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap)); }
#define VMX_PRIM(expr) do { int _e = (expr); if (_e != 0) return vmx::hip_fail((hipError_t)_e, #expr, __FILE__, __LINE__); } while (0)
// exclusive scan of n int64 on the context's stream; tmp: the caller's scratch buffer (grows as the primitive asks)
static inline int vmx_scan64(vm_ctx* c, vmx::DevBuf& tmp, const int64_t* in, int64_t* out, size_t n) {
    size_t tb = 0;
    VMX_PRIM(vmx_prim_excl_scan_i64(nullptr, &tb, in, out, n, c->stream));
    VMX_TRY(tmp.reserve(tb ? tb : 8));
    VMX_PRIM(vmx_prim_excl_scan_i64(tmp.p, &tb, in, out, n, c->stream));
    return 0;
}

// host bases (ASCII, one pointer per contig) -> mi->d_codes
int vmx_index_upload_codes(vm_index* mi, const char* const* seqs);
// the reference FASTA at path parsed on the device (vmx_bam.hip, kernels: k_fasta_in.hip) -> mi->names, lens, offsets, bases, d_codes (without the 64
// bytes of padding) and n_other_letters. st[0 .. 8): seconds of file read, inflate, parse kernels, download of the bases, [4] the caller's, text bytes, windows, contigs
int vmx_ref_fasta_device(vm_ctx* c, const char* path, vm_index* mi, double* st, int flags = 0);      // flags: VM_READER_GZIP_DEVICE
// sorted (hash, position) pairs on the device (positions in mi->d_pos) -> distinct keys, occurrence cap, hash table, contig offsets.
// d_keys is consumed (released).
int vmx_index_finish_device(vm_index* mi, vmx::DevBuf& d_keys, int64_t n);
// hash of every stored position recomputed from the codes (err[0] += positions that are not valid canonical k-mer starts inside one
// contig or whose strand bit is wrong) and the strict (hash, position) order check (err[1] += violations)
__global__ void k_idx_pos_keys(const uint8_t* codes, const int64_t* coff, int nseq, const uint64_t* pos, int64_t n, int k, uint64_t* keys, int32_t* err);
__global__ void k_idx_check_sorted(const uint64_t* keys, const uint64_t* pos, int64_t n, int32_t* err);
// letters of n reference bytes that are none of ACGTN in either case (k_sam.hip; counted by vmx_index_upload_codes for the device SAM emitter)
__global__ void k_sam_count_other(const char* in, int64_t n, unsigned long long* count);
__global__ void k_idx_fill_hashes(const vmx_slot* tab, int64_t nslots, uint64_t* hashes);
#endif
