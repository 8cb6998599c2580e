// vmx_bam.hip — C-ABI of the BAM writer (include/vacmapx.h): SAM text -> BAM records -> BGZF members, on the device (kernels: k_bam.hip).
// A writer owns grow-only device buffers and one page-locked staging buffer: after the first windows, a call allocates nothing but its
// malloc'ed result. Host work per call: gathering the text into the staging buffer, three small waits (line count, record sizes and
// errors, compressed size) and the few float tokens the device cannot convert exactly (vmx_bam_patch).
#include "vmx_host.h"
#include "vmx_bam.h"
#include <algorithm>
#include <cstdlib>
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
};

// SAM text (host, len bytes; the last line may lack its newline) -> BAM records in w->d_rec, *n_rec bytes
static int bam_encode_text(vm_bam_writer* w, const char* host, int64_t len, int64_t* n_rec) {
    vm_ctx* c = w->c;
    *n_rec = 0;
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
