// vmx_bam.hip — C-ABI of the BAM writer (include/vacmapx.h): SAM text -> BAM records -> BGZF members, on the device (kernels: k_bam.hip).
// A writer owns grow-only device buffers and one page-locked staging buffer: after the first windows, a call allocates nothing but its
// malloc'ed result. Host work per call: gathering the text into the staging buffer, three small waits (line count, record sizes and
// errors, compressed size) and the few float tokens the device cannot convert exactly (vmx_bam_patch).
#include "vmx_host.h"
#include "vmx_bam.h"
#include "vmx_index_prim.h"
#include <fcntl.h>
#include <unistd.h>
#include <algorithm>
#include <cstdlib>
#include <future>
#include <thread>
#include <string>
#include <vector>

using namespace vmx;

namespace {

struct BgzfBufs { DevBuf slots, msize, match, prev, out; };

// grow-only page-locked buffer with head-room. An outgrown buffer is parked, not freed: hipHostFree waits for the whole device (the aligner
// contexts' batches included), so the parked ones go when the writer does, as DevBuf parks its outgrown device buffers
struct HostPinned {
    char* p = nullptr; size_t cap = 0;
    std::vector<char*> parked;
    int reserve(size_t n) {
        if (n <= cap && p) return 0;
        if (p) parked.push_back(p);
        p = nullptr; cap = 0;
        const size_t want = n + n / 2 + 4096;
        if (hipHostMalloc((void**)&p, want, 0) != hipSuccess) { p = nullptr; set_error("page-locked host allocation failed"); return VM_ERR_OOM; }
        cap = want;
        return 0;
    }
    ~HostPinned() { for (char* q : parked) (void)hipHostFree(q); if (p) (void)hipHostFree(p); }
};

// vm_blob_gather_parts by several threads (one memcpy stream runs at a few GB/s: a window's text is hundreds of MB)
int64_t gather_parts_mt(const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n, char* out) {
    std::vector<int64_t> at((size_t)n + 1, 0);
    for (int64_t j = 0; j < n; ++j) at[j + 1] = at[j] + offs[part[j]][idx[j] + 1] - offs[part[j]][idx[j]];
    const int64_t tot = at[n];
    const int nt = tot < (8 << 20) ? 1 : 8;
    auto run = [&](int k) {
        const int64_t lo = std::lower_bound(at.begin(), at.end() - 1, tot * k / nt) - at.begin();
        const int64_t hi = std::lower_bound(at.begin(), at.end() - 1, tot * (k + 1) / nt) - at.begin();
        for (int64_t j = lo; j < (k + 1 == nt ? n : hi); ++j) memcpy(out + at[j], blobs[part[j]] + offs[part[j]][idx[j]], (size_t)(at[j + 1] - at[j]));
    };
    if (nt == 1) { run(0); return tot; }
    std::vector<std::thread> th;
    for (int k = 0; k < nt; ++k) th.emplace_back(run, k);
    for (auto& t : th) t.join();
    return tot;
}

int sync(vm_ctx* c) {
    const hipError_t e = vmx_stream_sync(c);
    if (e != hipSuccess) return hip_fail(e, "stream wait", __FILE__, __LINE__);
    return 0;
}

// BGZF members of n device bytes -> *out (malloc, *n_out bytes); no EOF marker
int bgzf_run(vm_ctx* c, BgzfBufs& z, HostPinned& pin, const void* d_in, int64_t n, char** out, int64_t* n_out) {
    *out = nullptr; *n_out = 0;
    const int64_t nm = (n + VMX_BGZF_BLOCK - 1) / VMX_BGZF_BLOCK;
    if (nm == 0) { *out = (char*)malloc(1); return *out ? 0 : VM_ERR_OOM; }
    const int64_t per = nm < VMX_BGZF_LAUNCH ? nm : VMX_BGZF_LAUNCH;
    VMX_TRY(z.slots.reserve((size_t)nm * VMX_BGZF_SLOT));
    VMX_TRY(z.msize.reserve((size_t)(nm + 1) * 8));
    VMX_TRY(z.match.reserve((size_t)per * VMX_BGZF_BLOCK * 4));
    VMX_TRY(z.prev.reserve((size_t)per * VMX_BGZF_BLOCK * 2));
    VMX_TRY(z.out.reserve((size_t)nm * VMX_BGZF_SLOT));
    for (int64_t f = 0; f < nm; f += per) {
        const int64_t g = nm - f < per ? nm - f : per;
        hipLaunchKernelGGL(k_bgzf_deflate, dim3((unsigned)g), dim3(VMX_BGZF_THREADS), 0, c->stream, (const uint8_t*)d_in, n, f, z.slots.as<uint8_t>(),
                           z.msize.as<int64_t>(), z.match.as<uint32_t>(), z.prev.as<uint16_t>());
    }
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, c->stream, z.msize.as<int64_t>(), nm);
    hipLaunchKernelGGL(k_bgzf_compact, dim3((unsigned)nm), dim3(256), 0, c->stream, z.slots.as<const uint8_t>(), z.msize.as<const int64_t>(), z.out.as<uint8_t>());
    VMX_TRY(pin.reserve(8));
    VMX_HIP(hipMemcpyAsync(pin.p, z.msize.as<int64_t>() + nm, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    int64_t tot; memcpy(&tot, pin.p, 8);
    VMX_TRY(pin.reserve((size_t)tot));
    VMX_HIP(hipMemcpyAsync(pin.p, z.out.p, (size_t)tot, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    *out = (char*)malloc((size_t)tot);
    if (!*out) { set_error("out of host memory"); return VM_ERR_OOM; }
    memcpy(*out, pin.p, (size_t)tot);
    *n_out = tot;
    return 0;
}

uint32_t fnv1a(const char* s, size_t n) { uint32_t h = 2166136261u; for (size_t i = 0; i < n; ++i) { h ^= (uint8_t)s[i]; h *= 16777619u; } return h; }

const char* bam_reason(int code) {
    switch (code) {
        case VMX_BAM_E_FIELDS: return "fewer than 11 fields";
        case VMX_BAM_E_NUM: return "FLAG, POS, MAPQ, PNEXT or TLEN is not a number in range";
        case VMX_BAM_E_CIGAR: return "malformed CIGAR (unknown operation or missing length)";
        case VMX_BAM_E_REF: return "RNAME or RNEXT is not an @SQ name of the header";
        case VMX_BAM_E_QUAL: return "QUAL and SEQ differ in length";
        case VMX_BAM_E_NAME: return "read name empty or longer than 254 characters";
        default: return "malformed optional field";
    }
}

}  // namespace

struct vm_bam_writer {
    vm_ctx* c = nullptr;
    std::string text;                                   // the header text as given
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    DevBuf d_names, d_off, d_htab;
    vmx_bam_refs refs{};
    DevBuf d_text, d_cnt, d_nl, d_rsz, d_rec, d_st, d_patch, d_poff, d_pval;
    BgzfBufs z;
    HostPinned pin, stage;                              // results / small read-backs; the gathered SAM text
    vmx_bam_status st0{0, ~0ull, 0, 0};                 // host sources of asynchronous uploads live as long as the writer
    std::vector<vmx_bam_patch> P;
    std::vector<int64_t> poff;
    std::vector<uint32_t> pval;
    int64_t n_lines = 0;                                // lines of the latest bam_encode_text (d_rsz holds their n_lines + 1 record offsets)
};

// SAM text (host, len bytes; the last line may lack its newline) -> BAM records in w->d_rec, *n_rec bytes
static int bam_encode_text(vm_bam_writer* w, const char* host, int64_t len, int64_t* n_rec) {
    vm_ctx* c = w->c;
    *n_rec = 0;
    w->n_lines = 0;
    if (len <= 0) return 0;
    const bool add_nl = host[len - 1] != '\n';
    const int64_t L = len + (add_nl ? 1 : 0);
    VMX_TRY(w->d_text.reserve((size_t)L));
    VMX_HIP(hipMemcpyAsync(w->d_text.p, host, (size_t)len, hipMemcpyHostToDevice, c->stream));
    if (add_nl) VMX_HIP(hipMemsetAsync(w->d_text.as<char>() + len, '\n', 1, c->stream));
    const int64_t nch = (L + VMX_BAM_NL_CHUNK - 1) / VMX_BAM_NL_CHUNK;
    VMX_TRY(w->d_cnt.reserve((size_t)(nch + 1) * 8));
    hipLaunchKernelGGL(k_bam_nl_count, dim3((unsigned)nch), dim3(256), 0, c->stream, w->d_text.as<const char>(), L, w->d_cnt.as<int64_t>());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, c->stream, w->d_cnt.as<int64_t>(), nch);
    VMX_TRY(w->pin.reserve(sizeof(vmx_bam_status)));
    VMX_HIP(hipMemcpyAsync(w->pin.p, w->d_cnt.as<int64_t>() + nch, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    int64_t n_lines; memcpy(&n_lines, w->pin.p, 8);
    VMX_TRY(w->d_nl.reserve((size_t)n_lines * 8));
    hipLaunchKernelGGL(k_bam_nl_pos, dim3((unsigned)nch), dim3(256), 0, c->stream, w->d_text.as<const char>(), L, w->d_cnt.as<const int64_t>(), w->d_nl.as<int64_t>());
    // sizes, offsets, the first error and the count of host-path floats
    const vmx_bam_status& st0 = w->st0;
    VMX_TRY(w->d_st.reserve(sizeof st0));
    VMX_HIP(hipMemcpyAsync(w->d_st.p, &st0, sizeof st0, hipMemcpyHostToDevice, c->stream));
    VMX_TRY(w->d_rsz.reserve((size_t)(n_lines + 1) * 8));
    const unsigned g = (unsigned)((n_lines + 3) / 4);                     // one wave per line
    vmx_bam_status* dst = w->d_st.as<vmx_bam_status>();
    hipLaunchKernelGGL(k_bam_size, dim3(g), dim3(256), 0, c->stream, w->d_text.as<const char>(), w->d_nl.as<const int64_t>(), n_lines, w->refs, w->d_rsz.as<int64_t>(), dst);
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, c->stream, w->d_rsz.as<int64_t>(), n_lines);
    hipLaunchKernelGGL(k_bam_status, dim3(1), dim3(64), 0, c->stream, w->d_rsz.as<const int64_t>(), n_lines, dst);
    VMX_HIP(hipMemcpyAsync(w->pin.p, dst, sizeof st0, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    vmx_bam_status st; memcpy(&st, w->pin.p, sizeof st);
    if (st.err_key != ~0ull) {
        set_error("SAM line " + std::to_string((long long)(st.err_key >> 8) + 1) + ": " + bam_reason((int)(st.err_key & 0xff)));
        return VM_ERR_ARG;
    }
    const int32_t np = st.n_patch;
    VMX_TRY(w->d_rec.reserve((size_t)st.total + 8));
    VMX_TRY(w->d_patch.reserve((size_t)(np > 0 ? np : 1) * sizeof(vmx_bam_patch)));
    VMX_HIP(hipMemsetAsync(&dst->n_patch, 0, 4, c->stream));
    hipLaunchKernelGGL(k_bam_encode, dim3(g), dim3(256), 0, c->stream, w->d_text.as<const char>(), w->d_nl.as<const int64_t>(), n_lines, w->refs,
                       w->d_rsz.as<const int64_t>(), w->d_rec.as<uint8_t>(), w->d_patch.as<vmx_bam_patch>(), &dst->n_patch);
    if (np > 0) {
        // floats outside the device's exact path: strtod, then a cast to float, as a host SAM parser does
        std::vector<vmx_bam_patch>& P = w->P;
        P.resize((size_t)np);
        VMX_HIP(hipMemcpyAsync(P.data(), w->d_patch.p, P.size() * sizeof(vmx_bam_patch), hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        std::vector<int64_t>& off = w->poff; std::vector<uint32_t>& val = w->pval;
        off.resize((size_t)np); val.resize((size_t)np);
        for (int32_t i = 0; i < np; ++i) {
            const std::string tok(host + P[i].text_off, (size_t)P[i].text_len);
            char* end = nullptr;
            const double d = strtod(tok.c_str(), &end);
            if (tok.empty() || end != tok.c_str() + tok.size()) { set_error("SAM line " + std::to_string(P[i].line + 1) + ": malformed float '" + tok + "'"); return VM_ERR_ARG; }
            const float f = (float)d;
            off[i] = P[i].out_off; memcpy(&val[i], &f, 4);
        }
        VMX_TRY(upload(w->d_poff, off.data(), off.size(), c->stream));
        VMX_TRY(upload(w->d_pval, val.data(), val.size(), c->stream));
        hipLaunchKernelGGL(k_bam_patch, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->stream, w->d_rec.as<uint8_t>(), w->d_poff.as<const int64_t>(),
                           w->d_pval.as<const uint32_t>(), (int64_t)np);
    }
    *n_rec = st.total;
    w->n_lines = n_lines;
    return 0;
}

extern "C" {

int vm_bam_writer_create(vm_ctx* c, const char* sam_header, int64_t len, vm_bam_writer** out) {
    if (out) *out = nullptr;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || (len > 0 && !sam_header)) return VM_ERR_ARG;
    vm_bam_writer* w = new vm_bam_writer();
    w->c = c;
    w->text.assign(sam_header ? sam_header : "", len > 0 ? (size_t)len : 0);
    // @SQ lines in header order: SN and LN
    size_t p = 0;
    const std::string& h = w->text;
    while (p < h.size()) {
        size_t e = h.find('\n', p);
        if (e == std::string::npos) e = h.size();
        if (e - p >= 3 && h.compare(p, 3, "@SQ") == 0) {
            std::string sn; int64_t ln = -1;
            size_t q = p;
            while (q < e) {
                size_t f = h.find('\t', q);
                if (f == std::string::npos || f > e) f = e;
                if (f - q > 3 && h.compare(q, 3, "SN:") == 0) sn = h.substr(q + 3, f - q - 3);
                else if (f - q > 3 && h.compare(q, 3, "LN:") == 0) ln = strtoll(h.c_str() + q + 3, nullptr, 10);
                q = f + 1;
            }
            if (sn.empty() || ln < 0) { delete w; set_error("vm_bam_writer_create: an @SQ line without SN or LN"); return VM_ERR_ARG; }
            w->names.push_back(sn); w->lens.push_back(ln);
        }
        p = e + 1;
    }
    const int nr = (int)w->names.size();
    std::vector<int64_t> off(nr + 1, 0);
    std::string blob;
    for (int i = 0; i < nr; ++i) { blob += w->names[i]; off[i + 1] = (int64_t)blob.size(); }
    int hs = 2;
    while (hs < 2 * nr) hs <<= 1;
    std::vector<int32_t> ht(hs, -1);
    for (int i = 0; i < nr; ++i) {
        uint32_t k = fnv1a(w->names[i].data(), w->names[i].size()) & (uint32_t)(hs - 1);
        bool dup = false;
        while (ht[k] >= 0) { if (w->names[ht[k]] == w->names[i]) { dup = true; break; } k = (k + 1) & (uint32_t)(hs - 1); }
        if (!dup) ht[k] = i;
    }
    int rc = upload(w->d_names, blob.data(), blob.size() ? blob.size() : 1, c->stream);
    if (rc == 0) rc = upload(w->d_off, off.data(), off.size(), c->stream);
    if (rc == 0) rc = upload(w->d_htab, ht.data(), ht.size(), c->stream);
    if (rc == 0 && hipStreamSynchronize(c->stream) != hipSuccess) { set_error("vm_bam_writer_create: upload failed"); rc = VM_ERR_HIP; }
    if (rc < 0) { vm_bam_writer_free(w); return rc; }
    w->refs = vmx_bam_refs{w->d_names.as<const char>(), w->d_off.as<const int64_t>(), w->d_htab.as<const int32_t>(), hs - 1, nr};
    *out = w;
    return 0;
}

void vm_bam_writer_free(vm_bam_writer* w) {
    if (!w) return;
    (void)hipStreamSynchronize(w->c->stream);
    DevBuf* bufs[] = {&w->d_names, &w->d_off, &w->d_htab, &w->d_text, &w->d_cnt, &w->d_nl, &w->d_rsz, &w->d_rec, &w->d_st, &w->d_patch, &w->d_poff, &w->d_pval,
                      &w->z.slots, &w->z.msize, &w->z.match, &w->z.prev, &w->z.out};
    for (DevBuf* b : bufs) b->release();
    delete w;
}

int vm_bam_header(vm_bam_writer* w, char** out, int64_t* n) {
    if (!w || !w->c) return VM_ERR_NO_CTX;
    std::string raw("BAM\1", 4);
    auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) raw.push_back((char)(v >> (8 * i))); };
    put32((uint32_t)w->text.size()); raw += w->text;
    put32((uint32_t)w->names.size());
    for (size_t i = 0; i < w->names.size(); ++i) { put32((uint32_t)w->names[i].size() + 1); raw += w->names[i]; raw.push_back('\0'); put32((uint32_t)w->lens[i]); }
    VMX_TRY(w->d_text.reserve(raw.size()));
    VMX_HIP(hipMemcpyAsync(w->d_text.p, raw.data(), raw.size(), hipMemcpyHostToDevice, w->c->stream));
    return bgzf_run(w->c, w->z, w->pin, w->d_text.p, (int64_t)raw.size(), out, n);
}

int vm_bam_encode(vm_bam_writer* w, const char* sam, int64_t len, char** out, int64_t* n) {
    if (out) *out = nullptr;
    if (n) *n = 0;
    if (!w || !w->c) return VM_ERR_NO_CTX;
    if (!out || !n || (len > 0 && !sam)) return VM_ERR_ARG;
    int64_t nr = 0;
    VMX_TRY(bam_encode_text(w, sam, len, &nr));
    VMX_TRY(w->pin.reserve((size_t)nr + 1));
    if (nr) VMX_HIP(hipMemcpyAsync(w->pin.p, w->d_rec.p, (size_t)nr, hipMemcpyDeviceToHost, w->c->stream));
    VMX_TRY(sync(w->c));
    *out = (char*)malloc((size_t)nr + 1);
    if (!*out) { set_error("out of host memory"); return VM_ERR_OOM; }
    memcpy(*out, w->pin.p, (size_t)nr);
    *n = nr;
    return 0;
}

int vm_bam_compress_parts(vm_bam_writer* w, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n,
                          char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!w || !w->c) return VM_ERR_NO_CTX;
    if (!out || !n_out || n < 0) return VM_ERR_ARG;
    int64_t tot = 0;
    for (int64_t j = 0; j < n; ++j) tot += offs[part[j]][idx[j] + 1] - offs[part[j]][idx[j]];
    VMX_TRY(w->stage.reserve((size_t)tot + 1));
    if (gather_parts_mt(blobs, offs, part, idx, n, w->stage.p) != tot) { set_error("vm_bam_compress_parts: gather failed"); return VM_ERR_ARG; }
    int64_t nr = 0;
    VMX_TRY(bam_encode_text(w, w->stage.p, tot, &nr));
    return bgzf_run(w->c, w->z, w->pin, w->d_rec.p, nr, out, n_out);
}

int vm_bgzf_compress(vm_ctx* c, const void* in, int64_t n, char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || !n_out || n < 0 || (n > 0 && !in)) return VM_ERR_ARG;
    BgzfBufs z; HostPinned pin; DevBuf d_in;
    int rc = d_in.reserve((size_t)(n ? n : 1));
    if (rc == 0 && n && hipMemcpyAsync(d_in.p, in, (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess) { set_error("vm_bgzf_compress: upload failed"); rc = VM_ERR_HIP; }
    if (rc == 0) rc = bgzf_run(c, z, pin, d_in.p, n, out, n_out);
    (void)hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&d_in, &z.slots, &z.msize, &z.match, &z.prev, &z.out};
    for (DevBuf* b : bufs) b->release();
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ coordinate-sorted output and its CSI index
// An external sort whose per-record steps run on the device (kernels: k_bam_sort.hip). Every call leaves a sorted run: its records go back
// to the caller (who writes them to a run file, uncompressed), its keys and size scan stay here. vm_bam_sorter_plan sorts all keys once
// more with the value run << 40 | index and cuts the result into chunks; vm_bam_sorter_chunk reads one contiguous range per run, gathers
// the chunk in global order, compresses it and records the index entries; vm_bam_sorter_index reduces them to the CSI.

#define VMX_PRIM_TRY(expr) do { int _e = (expr); if (_e != 0) return vmx::hip_fail((hipError_t)_e, #expr, __FILE__, __LINE__); } while (0)

struct vm_bam_sorter {
    vm_bam_writer* w = nullptr;
    int64_t chunk_bytes = 0;
    std::vector<std::vector<uint64_t>> keys;            // per run: sorted keys (dropped once the plan has uploaded them)
    std::vector<std::vector<int64_t>> roff;             // per run: n_r + 1 record offsets in the run file
    DevBuf d_k0, d_k1, d_v0, d_v1, d_tmp, d_ssz, d_soff, d_so, d_out;
    bool planned = false;
    std::vector<int> fds;
    int64_t n = 0, total = 0, n_chunks = 0, file_off = 0;
    std::vector<int64_t> cut, cutoff, lo, hi;           // lo / hi: [chunk][run] index ranges
    DevBuf d_gval, d_goff, d_roff_all, d_rstart, d_cut, d_cutoff, d_rmax, d_sbase, d_stage, d_chunk;
    HostPinned stage[2];                                // chunk k is read into stage[k & 1]: the next chunk's ranges are read while this one is on the device
    std::vector<int64_t> sbase[2];
    std::future<int> pre;                               // the read of chunk pre_k (-1: none in flight)
    int64_t pre_k = -1;
    std::string pre_err;
    DevBuf e_key, e_vbeg, e_vend, e_beg, e_end, e_unm;  // one index entry per record, in file order
    DevBuf d_ckey, d_cbeg, d_cend, d_cloff, d_wbase, d_lin, d_rbeg, d_rend, d_cnt;
};

namespace {

int prim_sort64(vm_ctx* c, DevBuf& tmp, const uint64_t* kin, uint64_t* kout, const uint64_t* vin, uint64_t* vout, size_t n) {
    size_t tb = 0;
    VMX_PRIM_TRY(vmx_prim_sort_pairs_u64(nullptr, &tb, kin, kout, vin, vout, n, 64, c->stream));
    VMX_TRY(tmp.reserve(tb ? tb : 8));
    VMX_PRIM_TRY(vmx_prim_sort_pairs_u64(tmp.p, &tb, kin, kout, vin, vout, n, 64, c->stream));
    return 0;
}

int prim_scan64(vm_ctx* c, DevBuf& tmp, const int64_t* in, int64_t* out, size_t n) {
    size_t tb = 0;
    VMX_PRIM_TRY(vmx_prim_excl_scan_i64(nullptr, &tb, in, out, n, c->stream));
    VMX_TRY(tmp.reserve(tb ? tb : 8));
    VMX_PRIM_TRY(vmx_prim_excl_scan_i64(tmp.p, &tb, in, out, n, c->stream));
    return 0;
}

inline unsigned grid256(int64_t n) { return (unsigned)((n + 255) / 256); }

template <class T> int fetch(vm_ctx* c, std::vector<T>& h, const DevBuf& d, size_t n) {
    h.resize(n);
    if (n) VMX_HIP(hipMemcpyAsync(h.data(), d.p, n * sizeof(T), hipMemcpyDeviceToHost, c->stream));
    return 0;
}

// the run ranges of chunk k -> stage[k & 1] (one sequential read per run), sbase[k & 1][r] = where run r's range starts there - the range's offset in the run
int read_chunk(vm_bam_sorter* s, int64_t k, std::string* err) {
    const int32_t nr = (int32_t)s->fds.size();
    const int64_t bytes = s->cutoff[k + 1] - s->cutoff[k];
    HostPinned& st = s->stage[k & 1];
    std::vector<int64_t>& sbase = s->sbase[k & 1];
    sbase.assign((size_t)nr, 0);
    if (s->cut[k + 1] == s->cut[k]) return 0;
    if (st.reserve((size_t)bytes) < 0) { *err = "page-locked host allocation failed"; return VM_ERR_OOM; }
    int64_t at = 0;
    for (int32_t r = 0; r < nr; ++r) {
        const int64_t lo = s->lo[(size_t)k * nr + r], hi = s->hi[(size_t)k * nr + r];
        const int64_t b0 = s->roff[r][lo], b1 = s->roff[r][hi];
        sbase[r] = at - b0;
        if (at + (b1 - b0) > bytes) { *err = "vm_bam_sorter_chunk: run ranges exceed the chunk"; return VM_ERR_HIP; }
        for (int64_t got = 0; got < b1 - b0;) {
            const ssize_t q = pread(s->fds[r], st.p + at + got, (size_t)(b1 - b0 - got), (off_t)(b0 + got));
            if (q <= 0) { *err = "vm_bam_sorter_chunk: short read from a run file"; return VM_ERR_ARG; }
            got += q;
        }
        at += b1 - b0;
    }
    if (at != bytes) { *err = "vm_bam_sorter_chunk: run ranges do not add up to the chunk"; return VM_ERR_HIP; }
    return 0;
}

const unsigned char kBgzfEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" {

int vm_bam_sorter_create(vm_bam_writer* w, int64_t chunk_bytes, vm_bam_sorter** out) {
    if (out) *out = nullptr;
    if (!w || !w->c) return VM_ERR_NO_CTX;
    if (!out || chunk_bytes <= 0) return VM_ERR_ARG;
    vm_bam_sorter* s = new vm_bam_sorter();
    s->w = w; s->chunk_bytes = chunk_bytes;
    *out = s;
    return 0;
}

void vm_bam_sorter_free(vm_bam_sorter* s) {
    if (!s) return;
    if (s->pre_k >= 0) (void)s->pre.get();
    (void)hipStreamSynchronize(s->w->c->stream);
    for (int fd : s->fds) if (fd >= 0) close(fd);
    DevBuf* bufs[] = {&s->d_k0, &s->d_k1, &s->d_v0, &s->d_v1, &s->d_tmp, &s->d_ssz, &s->d_soff, &s->d_so, &s->d_out, &s->d_gval, &s->d_goff, &s->d_roff_all, &s->d_rstart,
                      &s->d_cut, &s->d_cutoff, &s->d_rmax, &s->d_sbase, &s->d_stage, &s->d_chunk, &s->e_key, &s->e_vbeg, &s->e_vend, &s->e_beg, &s->e_end, &s->e_unm,
                      &s->d_ckey, &s->d_cbeg, &s->d_cend, &s->d_cloff, &s->d_wbase, &s->d_lin, &s->d_rbeg, &s->d_rend, &s->d_cnt};
    for (DevBuf* b : bufs) b->release();
    delete s;
}

int vm_bam_sorter_add_parts(vm_bam_sorter* s, const char* const* blobs, const int64_t* const* offs, const int32_t* part, const int64_t* idx, int64_t n,
                            char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!s || !s->w || !s->w->c) return VM_ERR_NO_CTX;
    if (!out || !n_out || n < 0) return VM_ERR_ARG;
    if (s->planned) { set_error("vm_bam_sorter_add_parts: the merge has been planned"); return VM_ERR_ARG; }
    vm_bam_writer* w = s->w; vm_ctx* c = w->c;
    int64_t tot = 0;
    for (int64_t j = 0; j < n; ++j) tot += offs[part[j]][idx[j] + 1] - offs[part[j]][idx[j]];
    VMX_TRY(w->stage.reserve((size_t)tot + 1));
    if (gather_parts_mt(blobs, offs, part, idx, n, w->stage.p) != tot) { set_error("vm_bam_sorter_add_parts: gather failed"); return VM_ERR_ARG; }
    int64_t nr = 0;
    VMX_TRY(bam_encode_text(w, w->stage.p, tot, &nr));
    const int64_t m = w->n_lines;
    if (m == 0 || nr == 0) { *out = (char*)malloc(1); return *out ? 0 : VM_ERR_OOM; }
    if (s->keys.size() >= (size_t)1 << (64 - VMX_BAM_RUN_SHIFT - 1) || (uint64_t)m > VMX_BAM_RUN_MASK) { set_error("vm_bam_sorter_add_parts: too many runs"); return VM_ERR_ARG; }
    VMX_TRY(s->d_k0.reserve((size_t)m * 8)); VMX_TRY(s->d_k1.reserve((size_t)m * 8));
    VMX_TRY(s->d_v0.reserve((size_t)m * 8)); VMX_TRY(s->d_v1.reserve((size_t)m * 8));
    VMX_TRY(s->d_ssz.reserve((size_t)(m + 1) * 8)); VMX_TRY(s->d_soff.reserve((size_t)(m + 1) * 8)); VMX_TRY(s->d_so.reserve((size_t)m * 8));
    VMX_TRY(s->d_out.reserve((size_t)nr + 16));
    hipLaunchKernelGGL(k_bam_sort_keys, dim3(grid256(m)), dim3(256), 0, c->stream, w->d_rec.as<const uint8_t>(), w->d_rsz.as<const int64_t>(), m, s->d_k0.as<uint64_t>(),
                       s->d_v0.as<uint64_t>());
    VMX_TRY(prim_sort64(c, s->d_tmp, s->d_k0.as<const uint64_t>(), s->d_k1.as<uint64_t>(), s->d_v0.as<const uint64_t>(), s->d_v1.as<uint64_t>(), (size_t)m));
    hipLaunchKernelGGL(k_bam_sort_sizes, dim3(grid256(m + 1)), dim3(256), 0, c->stream, w->d_rsz.as<const int64_t>(), s->d_v1.as<const uint64_t>(), m, s->d_ssz.as<int64_t>(),
                       s->d_so.as<int64_t>());
    VMX_TRY(prim_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_soff.as<int64_t>(), (size_t)m + 1));
    hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, c->stream, w->d_rec.as<const uint8_t>(), s->d_so.as<const int64_t>(),
                       s->d_soff.as<const int64_t>(), (int64_t)0, s->d_out.as<uint8_t>(), m);
    VMX_TRY(w->pin.reserve((size_t)nr));
    VMX_HIP(hipMemcpyAsync(w->pin.p, s->d_out.p, (size_t)nr, hipMemcpyDeviceToHost, c->stream));
    s->keys.emplace_back(); s->roff.emplace_back();
    int rc = fetch(c, s->keys.back(), s->d_k1, (size_t)m);
    if (rc == 0) rc = fetch(c, s->roff.back(), s->d_soff, (size_t)m + 1);
    if (rc == 0) rc = sync(c);
    if (rc == 0 && s->roff.back()[m] != nr) { set_error("vm_bam_sorter_add_parts: sorted sizes do not add up"); rc = VM_ERR_HIP; }
    if (rc == 0 && !(*out = (char*)malloc((size_t)nr))) { set_error("out of host memory"); rc = VM_ERR_OOM; }
    if (rc < 0) { s->keys.pop_back(); s->roff.pop_back(); return rc; }
    memcpy(*out, w->pin.p, (size_t)nr);
    *n_out = nr;
    return 0;
}

int vm_bam_sorter_plan(vm_bam_sorter* s, const char* const* run_paths, int64_t n_paths, int64_t file_base, int64_t* n_chunks) {
    if (n_chunks) *n_chunks = 0;
    if (!s || !s->w || !s->w->c) return VM_ERR_NO_CTX;
    if (!n_chunks || s->planned || n_paths != (int64_t)s->roff.size() || file_base < 0) { set_error("vm_bam_sorter_plan: one path per run, once"); return VM_ERR_ARG; }
    vm_ctx* c = s->w->c;
    const int32_t nr = (int32_t)n_paths;
    s->planned = true;
    s->file_off = file_base;
    for (int32_t r = 0; r < nr; ++r) {
        const int fd = open(run_paths[r], O_RDONLY);
        if (fd < 0) { set_error(std::string("vm_bam_sorter_plan: cannot open ") + run_paths[r]); return VM_ERR_ARG; }
        s->fds.push_back(fd);
    }
    std::vector<int64_t> rstart((size_t)nr + 1, 0);
    for (int32_t r = 0; r < nr; ++r) rstart[r + 1] = rstart[r] + (int64_t)s->keys[r].size();
    const int64_t n = s->n = rstart[nr];
    if (n == 0) return 0;
    std::vector<uint64_t> K((size_t)n);
    std::vector<int64_t> R((size_t)(n + nr));
    for (int32_t r = 0; r < nr; ++r) {
        memcpy(K.data() + rstart[r], s->keys[r].data(), s->keys[r].size() * 8);
        memcpy(R.data() + rstart[r] + r, s->roff[r].data(), s->roff[r].size() * 8);
        std::vector<uint64_t>().swap(s->keys[r]);
    }
    VMX_TRY(upload(s->d_k0, K.data(), K.size(), c->stream));
    VMX_TRY(upload(s->d_roff_all, R.data(), R.size(), c->stream));
    VMX_TRY(upload(s->d_rstart, rstart.data(), rstart.size(), c->stream));
    VMX_TRY(s->d_k1.reserve((size_t)n * 8)); VMX_TRY(s->d_v0.reserve((size_t)n * 8)); VMX_TRY(s->d_gval.reserve((size_t)n * 8));
    VMX_TRY(s->d_ssz.reserve((size_t)(n + 1) * 8)); VMX_TRY(s->d_goff.reserve((size_t)(n + 1) * 8));
    hipLaunchKernelGGL(k_bam_merge_vals, dim3(grid256(n)), dim3(256), 0, c->stream, s->d_rstart.as<const int64_t>(), nr, n, s->d_v0.as<uint64_t>());
    VMX_TRY(prim_sort64(c, s->d_tmp, s->d_k0.as<const uint64_t>(), s->d_k1.as<uint64_t>(), s->d_v0.as<const uint64_t>(), s->d_gval.as<uint64_t>(), (size_t)n));
    hipLaunchKernelGGL(k_bam_merge_sizes, dim3(grid256(n + 1)), dim3(256), 0, c->stream, s->d_gval.as<const uint64_t>(), s->d_roff_all.as<const int64_t>(),
                       s->d_rstart.as<const int64_t>(), n, s->d_ssz.as<int64_t>());
    VMX_TRY(prim_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_goff.as<int64_t>(), (size_t)n + 1));
    VMX_HIP(hipMemcpyAsync(&s->total, s->d_goff.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));                                                // (also: K, R and rstart have been read)
    const int64_t nch = s->n_chunks = (s->total + s->chunk_bytes - 1) / s->chunk_bytes;
    VMX_TRY(s->d_cut.reserve((size_t)(nch + 1) * 8)); VMX_TRY(s->d_cutoff.reserve((size_t)(nch + 1) * 8)); VMX_TRY(s->d_rmax.reserve((size_t)nch * nr * 8));
    hipLaunchKernelGGL(k_bam_merge_cuts, dim3(grid256(nch + 1)), dim3(256), 0, c->stream, s->d_goff.as<const int64_t>(), n, s->chunk_bytes, nch, s->d_cut.as<int64_t>(),
                       s->d_cutoff.as<int64_t>());
    VMX_HIP(hipMemsetAsync(s->d_rmax.p, 0, (size_t)nch * nr * 8, c->stream));
    hipLaunchKernelGGL(k_bam_merge_runmax, dim3(grid256(n)), dim3(256), 0, c->stream, s->d_gval.as<const uint64_t>(), s->d_cut.as<const int64_t>(), nch, nr, n,
                       s->d_rmax.as<unsigned long long>());
    std::vector<uint64_t> rmax;
    VMX_TRY(fetch(c, s->cut, s->d_cut, (size_t)nch + 1));
    VMX_TRY(fetch(c, s->cutoff, s->d_cutoff, (size_t)nch + 1));
    VMX_TRY(fetch(c, rmax, s->d_rmax, (size_t)nch * nr));
    VMX_TRY(sync(c));
    s->lo.assign((size_t)nch * nr, 0); s->hi.assign((size_t)nch * nr, 0);
    std::vector<int64_t> at((size_t)nr, 0);
    for (int64_t k = 0; k < nch; ++k)
        for (int32_t r = 0; r < nr; ++r) {
            const int64_t e = std::max<int64_t>(at[r], (int64_t)rmax[(size_t)k * nr + r]);
            if (e > (int64_t)s->roff[r].size() - 1) { set_error("vm_bam_sorter_plan: run range out of bounds"); return VM_ERR_HIP; }
            s->lo[(size_t)k * nr + r] = at[r]; s->hi[(size_t)k * nr + r] = e;
            at[r] = e;
        }
    VMX_TRY(s->d_sbase.reserve((size_t)nr * 8));
    int64_t widest = 0;                                              // both staging buffers are allocated here: the reading thread allocates nothing
    for (int64_t k = 0; k < nch; ++k) widest = std::max(widest, s->cutoff[k + 1] - s->cutoff[k]);
    VMX_TRY(s->stage[0].reserve((size_t)widest)); VMX_TRY(s->stage[nch > 1 ? 1 : 0].reserve((size_t)widest));
    VMX_TRY(s->e_key.reserve((size_t)n * 8)); VMX_TRY(s->e_vbeg.reserve((size_t)n * 8)); VMX_TRY(s->e_vend.reserve((size_t)n * 8));
    VMX_TRY(s->e_beg.reserve((size_t)n * 4)); VMX_TRY(s->e_end.reserve((size_t)n * 4)); VMX_TRY(s->e_unm.reserve((size_t)n * 4));
    *n_chunks = nch;
    return 0;
}

int vm_bam_sorter_chunk(vm_bam_sorter* s, int64_t k, char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!s || !s->w || !s->w->c) return VM_ERR_NO_CTX;
    if (!out || !n_out || !s->planned || k < 0 || k >= s->n_chunks) return VM_ERR_ARG;
    vm_bam_writer* w = s->w; vm_ctx* c = w->c;
    const int32_t nr = (int32_t)s->fds.size();
    const int64_t i0 = s->cut[k], m = s->cut[k + 1] - i0, bytes = s->cutoff[k + 1] - s->cutoff[k];
    std::string err;
    int rc;
    if (s->pre_k == k) { rc = s->pre.get(); err = s->pre_err; s->pre_k = -1; }
    else {
        if (s->pre_k >= 0) { (void)s->pre.get(); s->pre_k = -1; }
        rc = read_chunk(s, k, &err);
    }
    if (rc < 0) { set_error(err); return rc; }
    if (k + 1 < s->n_chunks) { s->pre_k = k + 1; s->pre_err.clear(); s->pre = std::async(std::launch::async, read_chunk, s, k + 1, &s->pre_err); }
    if (m == 0) { *out = (char*)malloc(1); return *out ? 0 : VM_ERR_OOM; }          // (a record larger than a chunk leaves the next ones empty)
    const HostPinned& stage = s->stage[k & 1];
    const std::vector<int64_t>& sbase = s->sbase[k & 1];
    VMX_TRY(s->d_stage.reserve((size_t)bytes + 16)); VMX_TRY(s->d_chunk.reserve((size_t)bytes + 16)); VMX_TRY(s->d_so.reserve((size_t)m * 8));
    VMX_HIP(hipMemcpyAsync(s->d_stage.p, stage.p, (size_t)bytes, hipMemcpyHostToDevice, c->stream));
    VMX_HIP(hipMemcpyAsync(s->d_sbase.p, sbase.data(), (size_t)nr * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_bam_merge_src, dim3(grid256(m)), dim3(256), 0, c->stream, s->d_gval.as<const uint64_t>() + i0, m, s->d_roff_all.as<const int64_t>(),
                       s->d_rstart.as<const int64_t>(), s->d_sbase.as<const int64_t>(), s->d_so.as<int64_t>());
    hipLaunchKernelGGL(k_bam_gather, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, c->stream, s->d_stage.as<const uint8_t>(), s->d_so.as<const int64_t>(),
                       s->d_goff.as<const int64_t>() + i0, s->cutoff[k], s->d_chunk.as<uint8_t>(), m);
    VMX_TRY(bgzf_run(c, w->z, w->pin, s->d_chunk.p, bytes, out, n_out));            // (leaves the chunk's member offsets in z.msize)
    hipLaunchKernelGGL(k_bam_index_entries, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, c->stream, s->d_chunk.as<const uint8_t>(), s->d_goff.as<const int64_t>() + i0,
                       s->cutoff[k], m, w->z.msize.as<const int64_t>(), s->file_off, s->e_key.as<uint64_t>() + i0, s->e_vbeg.as<uint64_t>() + i0,
                       s->e_vend.as<uint64_t>() + i0, s->e_beg.as<int32_t>() + i0, s->e_end.as<uint32_t>() + i0, s->e_unm.as<uint32_t>() + i0);
    s->file_off += *n_out;
    return 0;
}

int vm_bam_sorter_index(vm_bam_sorter* s, char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!s || !s->w || !s->w->c) return VM_ERR_NO_CTX;
    if (!out || !n_out || !s->planned) return VM_ERR_ARG;
    vm_bam_writer* w = s->w; vm_ctx* c = w->c;
    const int64_t n = s->n;
    const int32_t n_ref = (int32_t)w->names.size();
    std::vector<uint64_t> ckey, cbeg, cend, cloff, rbeg((size_t)n_ref, 0), rend((size_t)n_ref, 0), cnt((size_t)2 * n_ref + 1, 0);
    if (n > 0) {
        // entries by (reference, bin), file order inside; chunk heads; the chunk list
        VMX_TRY(s->d_k1.reserve((size_t)n * 8)); VMX_TRY(s->d_v0.reserve((size_t)n * 8)); VMX_TRY(s->d_v1.reserve((size_t)n * 8));
        VMX_TRY(s->d_ssz.reserve((size_t)(n + 1) * 8)); VMX_TRY(s->d_soff.reserve((size_t)(n + 1) * 8));
        hipLaunchKernelGGL(k_csi_iota, dim3(grid256(n)), dim3(256), 0, c->stream, s->d_v0.as<uint64_t>(), n);
        VMX_TRY(prim_sort64(c, s->d_tmp, s->e_key.as<const uint64_t>(), s->d_k1.as<uint64_t>(), s->d_v0.as<const uint64_t>(), s->d_v1.as<uint64_t>(), (size_t)n));
        hipLaunchKernelGGL(k_csi_flags, dim3(grid256(n + 1)), dim3(256), 0, c->stream, s->d_k1.as<const uint64_t>(), s->d_v1.as<const uint64_t>(),
                           s->e_vbeg.as<const uint64_t>(), s->e_vend.as<const uint64_t>(), n, s->d_ssz.as<int64_t>());
        VMX_TRY(prim_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_soff.as<int64_t>(), (size_t)n + 1));
        int64_t nc = 0;
        VMX_HIP(hipMemcpyAsync(&nc, s->d_soff.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        VMX_TRY(s->d_ckey.reserve((size_t)nc * 8)); VMX_TRY(s->d_cbeg.reserve((size_t)nc * 8)); VMX_TRY(s->d_cend.reserve((size_t)nc * 8)); VMX_TRY(s->d_cloff.reserve((size_t)nc * 8));
        hipLaunchKernelGGL(k_csi_chunks, dim3(grid256(n)), dim3(256), 0, c->stream, s->d_k1.as<const uint64_t>(), s->d_v1.as<const uint64_t>(), s->e_vbeg.as<const uint64_t>(),
                           s->e_vend.as<const uint64_t>(), s->d_ssz.as<const int64_t>(), s->d_soff.as<const int64_t>(), n, s->d_ckey.as<uint64_t>(), s->d_cbeg.as<uint64_t>(),
                           s->d_cend.as<uint64_t>());
        // the 16 kb windows' first records, each bin's loffset, the per-reference figures
        std::vector<int64_t> wbase((size_t)n_ref + 1, 0);
        for (int32_t r = 0; r < n_ref; ++r) wbase[r + 1] = wbase[r] + (w->lens[r] >> 14) + 1;
        VMX_TRY(upload(s->d_wbase, wbase.data(), wbase.size(), c->stream));
        VMX_TRY(s->d_lin.reserve((size_t)wbase[n_ref] * 8 + 8));
        VMX_HIP(hipMemsetAsync(s->d_lin.p, 0xff, (size_t)wbase[n_ref] * 8 + 8, c->stream));
        hipLaunchKernelGGL(k_csi_linear, dim3(grid256(n)), dim3(256), 0, c->stream, s->e_key.as<const uint64_t>(), s->e_vbeg.as<const uint64_t>(), s->e_beg.as<const int32_t>(),
                           s->e_end.as<const uint32_t>(), n, n_ref, s->d_wbase.as<const int64_t>(), s->d_lin.as<unsigned long long>());
        hipLaunchKernelGGL(k_csi_loffset, dim3(grid256(nc)), dim3(256), 0, c->stream, s->d_ckey.as<const uint64_t>(), nc, n_ref, s->d_wbase.as<const int64_t>(),
                           s->d_lin.as<const unsigned long long>(), s->d_cloff.as<uint64_t>());
        VMX_TRY(s->d_rbeg.reserve((size_t)n_ref * 8 + 8)); VMX_TRY(s->d_rend.reserve((size_t)n_ref * 8 + 8)); VMX_TRY(s->d_cnt.reserve(cnt.size() * 8));
        VMX_HIP(hipMemsetAsync(s->d_rbeg.p, 0, (size_t)n_ref * 8 + 8, c->stream));
        VMX_HIP(hipMemsetAsync(s->d_rend.p, 0, (size_t)n_ref * 8 + 8, c->stream));
        VMX_HIP(hipMemsetAsync(s->d_cnt.p, 0, cnt.size() * 8, c->stream));
        hipLaunchKernelGGL(k_csi_refstats, dim3(grid256(n)), dim3(256), 0, c->stream, s->e_key.as<const uint64_t>(), s->e_vbeg.as<const uint64_t>(),
                           s->e_vend.as<const uint64_t>(), s->e_unm.as<const uint32_t>(), n, n_ref, s->d_rbeg.as<uint64_t>(), s->d_rend.as<uint64_t>(),
                           s->d_cnt.as<unsigned long long>());
        VMX_TRY(fetch(c, ckey, s->d_ckey, (size_t)nc)); VMX_TRY(fetch(c, cbeg, s->d_cbeg, (size_t)nc)); VMX_TRY(fetch(c, cend, s->d_cend, (size_t)nc));
        VMX_TRY(fetch(c, cloff, s->d_cloff, (size_t)nc));
        VMX_TRY(fetch(c, rbeg, s->d_rbeg, (size_t)n_ref)); VMX_TRY(fetch(c, rend, s->d_rend, (size_t)n_ref)); VMX_TRY(fetch(c, cnt, s->d_cnt, cnt.size()));
        VMX_TRY(sync(c));
    }
    // CSI (min_shift 14, depth 5, no aux): the host only serialises the bins
    std::string raw("CSI\1", 4);
    auto put32 = [&](uint32_t v) { for (int i = 0; i < 4; ++i) raw.push_back((char)(v >> (8 * i))); };
    auto put64 = [&](uint64_t v) { for (int i = 0; i < 8; ++i) raw.push_back((char)(v >> (8 * i))); };
    put32(14); put32(5); put32(0); put32((uint32_t)n_ref);
    size_t k = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        const size_t k0 = k;
        uint32_t nbin = 0;
        while (k < ckey.size() && ckey[k] >> 32 == (uint64_t)r) { if (k == k0 || ckey[k] != ckey[k - 1]) ++nbin; ++k; }
        const bool any = cnt[2 * (size_t)r] + cnt[2 * (size_t)r + 1] > 0;
        put32(nbin + (any ? 1 : 0));
        for (size_t a = k0; a < k;) {
            size_t b = a;
            while (b < k && ckey[b] == ckey[a]) ++b;
            put32((uint32_t)ckey[a]); put64(cloff[a]); put32((uint32_t)(b - a));
            for (size_t x = a; x < b; ++x) { put64(cbeg[x]); put64(cend[x]); }
            a = b;
        }
        if (any) { put32(37450); put64(0); put32(2); put64(rbeg[r]); put64(rend[r]); put64(cnt[2 * (size_t)r]); put64(cnt[2 * (size_t)r + 1]); }
    }
    put64(cnt[2 * (size_t)n_ref]);
    VMX_TRY(s->d_out.reserve(raw.size()));
    VMX_HIP(hipMemcpyAsync(s->d_out.p, raw.data(), raw.size(), hipMemcpyHostToDevice, c->stream));
    char* z = nullptr; int64_t nz = 0;
    VMX_TRY(bgzf_run(c, w->z, w->pin, s->d_out.p, (int64_t)raw.size(), &z, &nz));
    char* full = (char*)realloc(z, (size_t)nz + sizeof kBgzfEof);
    if (!full) { free(z); set_error("out of host memory"); return VM_ERR_OOM; }
    memcpy(full + nz, kBgzfEof, sizeof kBgzfEof);
    *out = full; *n_out = nz + (int64_t)sizeof kBgzfEof;
    return 0;
}

}  // extern "C"
