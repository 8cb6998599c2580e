// vmx_bam.h — BAM output on the device: SAM text -> BAM records (k_bam_*), BGZF deflate (k_bgzf_*). Kernels in k_bam.hip, the C-ABI in vmx_bam.hip.
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

#endif
