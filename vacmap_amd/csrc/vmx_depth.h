// vmx_depth.h — the depth-of-coverage accumulator (vacmapx.h states the rule at vm_depth_add). Host side: vmx_depth.hip (create, merge, counts, text)
// and vmx_sam.hip (vm_depth_add, beside the host emitters whose per-record stage it shares); kernels: k_depth.hip; the device adds are launched by
// vmx_sam_emit_dev (vmx_sam_dev.hip). DESIGN §7d, "Depth of coverage".
#ifndef VMX_DEPTH_H
#define VMX_DEPTH_H
#include "vmx_sam_dev.h"

// what the depth kernels read of an accumulator, as device pointers
struct vmx_depth_dev {
    unsigned long long* counts;       // [n_win]
    const int64_t* win_off;           // [nseq + 1]
    int64_t window; int32_t min_mapq;
};

struct vm_depth {
    vm_ctx* ctx = nullptr;            // nullptr: the counts live in h_counts
    uint64_t index_serial = 0;        // the index the accumulator was made for (an attached accumulator only adds for that one)
    int64_t window = 0; int min_mapq = 0;
    std::vector<std::string> names; std::vector<int64_t> lens, win_off;      // win_off: nseq + 1
    int64_t n_win = 0;
    std::vector<int64_t> h_counts;
    vmx::DevBuf d_counts, d_win_off, d_lens, d_cnames, d_cname_off;          // device accumulator: counts, layout and contig names (uploaded once, by create)
    vmx::DevBuf d_sums, d_lsz, d_loff, d_text, d_tmp;                        // text: per-contig sums (nseq + 1, the last one the total), line sizes / offsets, bytes
    vmx_depth_dev dev() const { return vmx_depth_dev{d_counts.as<unsigned long long>(), d_win_off.as<const int64_t>(), window, (int32_t)min_mapq}; }
};

// k_depth.hip
__global__ void k_depth_add(vmx_sam_in A, vmx_sam_work K, vmx_depth_dev D);
__global__ void k_depth_merge(unsigned long long* dst, const unsigned long long* src, int64_t n);
__global__ void k_depth_sums(const unsigned long long* counts, const int64_t* win_off, int32_t nseq, unsigned long long* sums);
__global__ void k_depth_lines(const unsigned long long* counts, const int64_t* win_off, const int64_t* lens, const char* cnames, const int64_t* cname_off, int32_t nseq,
                              int64_t window, const unsigned long long* sums, int which, int64_t total_len, int64_t n_items, int64_t* lsz, const int64_t* loff, char* text,
                              int write);

// the mean of the rule in hundredths: (200 * count + len) div (2 * len), 0 for len = 0
__host__ __device__ inline unsigned long long vmx_depth_hundredths(unsigned long long count, unsigned long long len) { return len ? (200ull * count + len) / (2ull * len) : 0ull; }
#endif
