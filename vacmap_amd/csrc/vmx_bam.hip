// vmx_bam.hip — C-ABI of the BAM writer (include/vacmapx.h): SAM text -> BAM records -> BGZF members, on the device (kernels: k_bam.hip), and, at the
// end of the file, of the BAM reader (BGZF members -> records -> read blobs; kernels: k_bam_in.hip) and of the reader of bgzipped FASTQ, which
// shares the BAM reader's file / inflate half (BgzfIn) and its hand-out (HandOut) (kernels: k_fastx_in.hip).
// A writer owns grow-only device buffers and one page-locked staging buffer: after the first windows, a call allocates nothing but its
// malloc'ed result. Host work per call: gathering the text into the staging buffer, three small waits (line count, record sizes and
// errors, compressed size) and the few float tokens the device cannot convert exactly (vmx_bam_patch).
#include "vmx_host.h"
#include "vmx_bam.h"
#include "vmx_index_priv.h"
#include "vmx_fasta_rule.h"
#include <fcntl.h>
#include <zlib.h>
#include <unistd.h>
#include <algorithm>
#include <cctype>
#include <cstring>
#include <cstdlib>
#include <future>
#include <thread>
#include <string>
#include <vector>

using namespace vmx;

namespace {

struct BgzfBufs { DevBuf slots, msize, match, prev, out; };

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
    return rc;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ coordinate-sorted output and its CSI index
// An external sort whose per-record steps run on the device (kernels: k_bam_sort.hip). Every call leaves a sorted run: its records go back
// to the caller (who writes them to a run file, uncompressed), its keys and size scan stay here. vm_bam_sorter_plan sorts all keys once
// more with the value run << 40 | index and cuts the result into chunks; vm_bam_sorter_chunk reads one contiguous range per run, gathers
// the chunk in global order, compresses it and records the index entries; vm_bam_sorter_index reduces them to the CSI.


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
    VMX_PRIM(vmx_prim_sort_pairs_u64(nullptr, &tb, kin, kout, vin, vout, n, 64, c->stream));
    VMX_TRY(tmp.reserve(tb ? tb : 8));
    VMX_PRIM(vmx_prim_sort_pairs_u64(tmp.p, &tb, kin, kout, vin, vout, n, 64, c->stream));
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
    VMX_TRY(vmx_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_soff.as<int64_t>(), (size_t)m + 1));
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
    VMX_TRY(vmx_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_goff.as<int64_t>(), (size_t)n + 1));
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
        VMX_TRY(vmx_scan64(c, s->d_tmp, s->d_ssz.as<const int64_t>(), s->d_soff.as<int64_t>(), (size_t)n + 1));
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

// ------------------------------------------------------------------------------------------------ BAM input
// The host walks the BGZF member headers of a compressed chunk (magic, FLG.FEXTRA, the BC subfield among the extra subfields, BSIZE, the
// trailer's CRC32 and ISIZE) and sums ISIZE into output offsets; the device inflates every member (k_bgzf_inflate), walks the records,
// sizes and decodes them (k_bam_in_*). A reader reads the file ahead on an I/O thread into two page-locked staging buffers; the tail of a
// window that holds no complete record is carried to the front of the next window's inflate buffer with a device copy.

namespace {

struct MemberTab {
    std::vector<vmx_bgzf_member> m;
    std::vector<int64_t> foff;                          // every member's offset in the file (messages)
    int64_t consumed = 0, inflated = 0;
};

inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// the complete members of p[0, n) (file offset of p[0]: base), until their ISIZE sum would pass max_inf (one member is always taken).
// *not_bgzf: a gzip member without the BC subfield was met
int walk_members(const uint8_t* p, int64_t n, int64_t base, int64_t max_inf, MemberTab& T, std::string* err, bool* not_bgzf) {
    T.m.clear(); T.foff.clear(); T.consumed = 0; T.inflated = 0;
    *not_bgzf = false;
    int64_t at = 0;
    while (n - at >= 18) {
        const uint8_t* h = p + at;
        const std::string where = " at file offset " + std::to_string((long long)(base + at));
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8) { *err = "not a gzip member" + where; return VM_ERR_IO; }
        if (h[3] != 4) { *not_bgzf = true; *err = "gzip member without the BGZF extra field (FLG " + std::to_string((int)h[3]) + ")" + where; return VM_ERR_UNSUPPORTED; }
        const int64_t xlen = (int64_t)h[10] | (int64_t)h[11] << 8;
        if (n - at < 12 + xlen) break;
        int64_t bsize = -1;
        for (int64_t q = 12; q + 4 <= 12 + xlen;) {
            const int64_t slen = (int64_t)h[q + 2] | (int64_t)h[q + 3] << 8;
            if (q + 4 + slen > 12 + xlen) { *err = "malformed gzip extra field" + where; return VM_ERR_IO; }
            if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2) bsize = (int64_t)h[q + 4] | (int64_t)h[q + 5] << 8;
            q += 4 + slen;
        }
        if (bsize < 0) { *not_bgzf = true; *err = "gzip member without the BGZF BC subfield" + where; return VM_ERR_UNSUPPORTED; }
        const int64_t total = bsize + 1;
        if (total < 12 + xlen + 8) { *err = "BGZF member with a BSIZE smaller than its header and trailer" + where; return VM_ERR_IO; }
        if (n - at < total) break;
        const uint32_t isize = le32(h + total - 4);
        if (isize > (1u << 28)) { *err = "BGZF member with an ISIZE beyond what its size can hold" + where; return VM_ERR_IO; }
        if (!T.m.empty() && T.inflated + (int64_t)isize > max_inf) break;
        T.m.push_back(vmx_bgzf_member{at + 12 + xlen, T.inflated, (int32_t)(total - 12 - xlen - 8), isize, le32(h + total - 8), 0});
        T.foff.push_back(base + at);
        T.inflated += isize; at += total;
    }
    T.consumed = at;
    return 0;
}

const char* bgzf_reason(int code) {
    switch (code) {
        case VMX_BGZF_E_BTYPE: return "reserved block type 3";
        case VMX_BGZF_E_STORED: return "stored block whose LEN is not the complement of NLEN";
        case VMX_BGZF_E_INPUT: return "deflate data runs past the member's end (truncated member)";
        case VMX_BGZF_E_LONG: return "deflate data holds more bytes than ISIZE";
        case VMX_BGZF_E_SHORT: return "deflate data holds fewer bytes than ISIZE";
        case VMX_BGZF_E_CRC: return "CRC32 mismatch";
        case VMX_BGZF_E_LENS: return "over-subscribed or incomplete set of code lengths";
        case VMX_BGZF_E_CODE: return "invalid literal / length or distance code";
        case VMX_BGZF_E_DIST: return "distance reaches before the member's start";
        case VMX_BGZF_E_TAIL: return "deflate data ends before the member's trailer";
        default: return "malformed dynamic block header";
    }
}

const vmx_crc_x2n& crc_x2n_table() {
    static const vmx_crc_x2n t = [] { vmx_crc_x2n x; uint32_t p = 1u << 30; for (int k = 0; k < 32; ++k) { x.v[k] = p; p = crc_multmodp(p, p); } return x; }();
    return t;
}

struct InflateBufs { DevBuf comp, tab, key; };

// the members T of the n_comp compressed bytes at `comp` (host) -> d_out[0, T.inflated); waits for the result
int inflate_run(vm_ctx* c, InflateBufs& z, HostPinned& pin, const uint8_t* comp, int64_t n_comp, const MemberTab& T, uint8_t* d_out) {
    const int64_t nm = (int64_t)T.m.size();
    if (nm == 0) return 0;
    VMX_TRY(z.comp.reserve((size_t)n_comp + 16));
    VMX_TRY(z.tab.reserve((size_t)nm * sizeof(vmx_bgzf_member)));
    VMX_TRY(z.key.reserve(8));
    VMX_TRY(pin.reserve(64));
    VMX_HIP(hipMemcpyAsync(z.comp.p, comp, (size_t)n_comp, hipMemcpyHostToDevice, c->stream));
    VMX_HIP(hipMemcpyAsync(z.tab.p, T.m.data(), (size_t)nm * sizeof(vmx_bgzf_member), hipMemcpyHostToDevice, c->stream));
    VMX_HIP(hipMemsetAsync(z.key.p, 0xff, 8, c->stream));
    hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)nm), dim3(64), 0, c->stream, z.comp.as<const uint8_t>(), z.tab.as<const vmx_bgzf_member>(), nm, d_out,
                       crc_x2n_table(), z.key.as<unsigned long long>());
    VMX_HIP(hipMemcpyAsync(pin.p, z.key.p, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    uint64_t key; memcpy(&key, pin.p, 8);
    if (key != ~0ull) {
        const int64_t mb = (int64_t)(key >> 8);
        set_error("BGZF member at file offset " + std::to_string((long long)(mb < nm ? T.foff[mb] : -1)) + ": " + bgzf_reason((int)(key & 0xff)));
        return VM_ERR_IO;
    }
    return 0;
}

struct Grow {
    char* p = nullptr; size_t n = 0, cap = 0;
    bool append(const char* s, size_t k) {
        if (n + k > cap) { const size_t want = (n + k) + (n + k) / 2 + 64; char* q = (char*)realloc(p, want); if (!q) return false; p = q; cap = want; }
        // a window's bases are hundreds of MB: the copy (into fresh pages) is split over VMX_BAM_IN_COPY_THREADS threads (default 4; 1: one memcpy);
        // measured against one memcpy by `tools/bam_bench.py input`
        int nt = 1;
        if (k >= ((size_t)8 << 20)) { const char* e = getenv("VMX_BAM_IN_COPY_THREADS"); const int v = e ? atoi(e) : 4; nt = v < 1 ? 1 : v > 16 ? 16 : v; }
        if (nt == 1) { if (k) memcpy(p + n, s, k); }
        else {
            std::vector<std::thread> th;
            for (int t = 0; t < nt; ++t) th.emplace_back([=] { const size_t a = k * t / nt, b = k * (t + 1) / nt; memcpy(p + n + a, s + a, b - a); });
            for (auto& t : th) t.join();
        }
        n += k;
        return true;
    }
    char* release() { char* q = p ? p : (char*)malloc(1); p = nullptr; n = cap = 0; return q; }
    ~Grow() { free(p); }
};

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct DecodedWin { HostPinned names, seqs, quals, comments, off; int64_t n = 0; };     // a window's reads on the host: blobs and 3 (4 with tags) x (n + 1) offsets

struct BamInChunk { HostPinned stage; MemberTab T; int64_t fpos = 0, got = 0; int rc = 0; std::string err; bool not_bgzf = false; double busy = 0; };

// The file and inflate half of a reader of BGZF input (vm_bam_reader, vm_fastq_reader): the file read ahead in chunks, the windows inflated behind the carried tail
struct BgzfIn {
    vm_ctx* c = nullptr;
    int fd = -1;
    int64_t fsize = 0, chunk_bytes = 0, max_inf = 0;
    BamInChunk ch[2];
    int slot = 0;                                       // the chunk the next window takes
    std::future<void> pre; bool pre_on = false; bool file_done = false; int64_t next_fpos = 0;
    InflateBufs z;
    DevBuf d_inf[2]; int which = 0; int64_t tail_off = 0, carry = 0;     // the bytes of d_inf[which] from tail_off on go in front of the next window
    HostPinned pin;
};

// The hand-out half: two decoded windows, the one the caller takes records from and the one a producer thread fills
struct HandOut {
    DecodedWin win[2]; int cur = 0; int64_t at = 0;     // records [at, win[cur].n) are not handed out yet; the other slot is being produced
    std::future<int> prod; bool prod_on = false; std::string prod_err;      // the next window, decoded ahead on a thread of its own
    double handout_s = 0;
};

}  // namespace

struct vm_bam_reader {
    vm_ctx* c = nullptr;
    BgzfIn in;
    bool hdr_done = false;
    DevBuf d_roff, d_walk, d_sz, d_off, d_tmp, d_names, d_seqs, d_quals, d_ooff;
    // tags asked for (vm_bam_reader_open_tags): the selection on the device, per-record comment bytes, their scan, the blob, the kept records' offsets, error key + drop counter
    bool tags_on = false; int tags_all = 0; std::vector<uint16_t> tags;
    DevBuf d_sel, d_csz, d_coff, d_comments, d_ocoff, d_aux;
    int64_t n_aux_dropped = 0;
    HandOut h;
    int64_t n_seen = 0, n_dropped = 0;                  // records walked / without bases
    double st[13] = {0};                                // written by whoever produces a window
    double pub[13] = {0};                               // what vm_bam_reader_stats reads: st as of the latest window the caller's thread has taken over
};

namespace {
// the plain-gzip file half (defined with the gzip host code below); null in a reader of BGZF
struct GzipIn;
int gzip_in_window(BgzfIn* r, GzipIn* g, double* st, int64_t* avail_out);
void gzip_in_free(GzipIn* g);
GzipIn* gzip_in_new();
double gzip_in_stat(const GzipIn* g, int i);
}

struct vm_fastq_reader {
    vm_ctx* c = nullptr;
    BgzfIn in;
    GzipIn* gz = nullptr;
    ~vm_fastq_reader() { gzip_in_free(gz); }
    DevBuf d_cnt, d_coff, d_ls, d_map, d_tile, d_start, d_ridx, d_rline, d_res, d_sz, d_off, d_tmp, d_names, d_seqs, d_quals, d_comments;
    bool fasta = false;                                 // VM_READER_FASTA: reader_window_fasta parses the windows (kernels: k_fasta_reads.hip)
    DevBuf d_state, d_ka, d_ks, d_kq, d_so, d_qo, d_fres;
    HandOut h;
    int64_t n_seen = 0;                                 // complete records of the windows so far
    int fail_rc = 0; std::string fail_msg;              // a bad header ends the input behind the records in front of it: the next window is this error
    double st[13] = {0}, pub[13] = {0};                 // as the BAM reader's, the first 11
};

namespace {

void read_chunk_in(BgzfIn* r, int slot, int64_t fpos) {
    BamInChunk& k = r->ch[slot];
    const double t0 = now_s();
    k.fpos = fpos; k.got = 0; k.rc = 0; k.err.clear(); k.T.m.clear(); k.T.foff.clear(); k.T.consumed = 0; k.T.inflated = 0;
    const int64_t want = std::min<int64_t>(r->chunk_bytes, r->fsize - fpos);
    while (k.got < want) {
        const ssize_t q = pread(r->fd, k.stage.p + k.got, (size_t)(want - k.got), (off_t)(fpos + k.got));
        if (q < 0) { k.rc = VM_ERR_IO; k.err = "read error at file offset " + std::to_string((long long)(fpos + k.got)); return; }
        if (q == 0) break;
        k.got += q;
    }
    if (k.got > 0) {
        k.rc = walk_members((const uint8_t*)k.stage.p, k.got, fpos, r->max_inf, k.T, &k.err, &k.not_bgzf);
        if (k.rc == 0 && k.T.m.empty()) {
            k.rc = VM_ERR_IO;
            k.err = fpos + k.got >= r->fsize ? "truncated file: the BGZF member at file offset " + std::to_string((long long)fpos) + " is not complete"
                                             : "BGZF member at file offset " + std::to_string((long long)fpos) + " is larger than the reader's chunk";
        }
    }
    k.busy = now_s() - t0;
}

// 1: the BAM header ends at *end; 0: more bytes are needed; -1: not BAM
int parse_bam_header(const uint8_t* h, int64_t n, int64_t* end) {
    if (n < 4) return 0;
    if (memcmp(h, "BAM\1", 4) != 0) return -1;
    if (n < 8) return 0;
    int64_t p = 8 + (int64_t)le32(h + 4);
    if (n < p + 4) return 0;
    const int64_t n_ref = le32(h + p); p += 4;
    for (int64_t i = 0; i < n_ref; ++i) {
        if (n < p + 4) return 0;
        p += 4 + (int64_t)le32(h + p) + 4;
    }
    if (n < p) return 0;
    *end = p;
    return 1;
}

// The next chunk's members inflated behind the carried tail: 1 (d_inf[which] holds *avail bytes, 64 more are reserved behind them; the caller sets
// tail_off and carry anew), 0 when the file has been read to its end, or a negative status. st: the reader's statistics (I/O busy 0, I/O wait 1,
// inflate 2, windows 7, file bytes 8, inflated bytes 9)
int bgzf_in_window(BgzfIn* r, double* st, int64_t* avail_out) {
    vm_ctx* c = r->c;
    if (r->file_done) return 0;
    double t0 = now_s();
    if (r->pre_on) { r->pre.get(); r->pre_on = false; }
    else read_chunk_in(r, r->slot, r->next_fpos);
    st[1] += now_s() - t0;
    BamInChunk& k = r->ch[r->slot];
    st[0] += k.busy;
    if (k.rc < 0) { set_error(k.err); return k.rc; }
    r->next_fpos = k.fpos + k.T.consumed;
    if (k.T.m.empty() || r->next_fpos >= r->fsize) r->file_done = true;
    else { r->pre_on = true; r->pre = std::async(std::launch::async, read_chunk_in, r, r->slot ^ 1, r->next_fpos); }
    r->slot ^= 1;
    if (k.T.m.empty()) return 0;                                              // (an empty file tail: the caller's end-of-file checks)
    // inflate behind the carried tail
    t0 = now_s();
    DevBuf& dst = r->d_inf[r->which ^ 1];
    const int64_t avail = r->carry + k.T.inflated;
    VMX_TRY(dst.reserve((size_t)avail + 64));
    if (r->carry) VMX_HIP(hipMemcpyAsync(dst.p, r->d_inf[r->which].as<uint8_t>() + r->tail_off, (size_t)r->carry, hipMemcpyDeviceToDevice, c->stream));
    VMX_TRY(inflate_run(c, r->z, r->pin, (const uint8_t*)k.stage.p, k.T.consumed, k.T, dst.as<uint8_t>() + r->carry));
    r->which ^= 1;
    st[2] += now_s() - t0; st[7] += 1; st[8] += (double)k.T.consumed; st[9] += (double)k.T.inflated;
    *avail_out = avail;
    return 1;
}

// the file opened, its size, the chunk and window sizes, both staging buffers
int bgzf_in_open(BgzfIn* r, vm_ctx* c, const char* path) {
    r->c = c;
    r->fd = open(path, O_RDONLY);
    if (r->fd < 0) { set_error(std::string("cannot open ") + path); return VM_ERR_IO; }
    r->fsize = (int64_t)lseek(r->fd, 0, SEEK_END);
    // VMX_BAM_IN_CHUNK / VMX_BAM_IN_MAXINF: compressed bytes per read and inflated bytes per window (tests cross many windows with small files)
    r->chunk_bytes = 64 << 20; r->max_inf = (int64_t)512 << 20;
    if (const char* e = getenv("VMX_BAM_IN_CHUNK")) r->chunk_bytes = std::max<int64_t>(atoll(e), 1 << 17);
    if (const char* e = getenv("VMX_BAM_IN_MAXINF")) r->max_inf = std::max<int64_t>(atoll(e), 1 << 16);
    if (r->fsize < 0) { set_error(std::string("cannot seek in ") + path); return VM_ERR_IO; }
    const size_t stage = (size_t)std::min<int64_t>(r->chunk_bytes, std::max<int64_t>(r->fsize, 1));
    VMX_TRY(r->ch[0].stage.reserve(stage));
    VMX_TRY(r->ch[1].stage.reserve(stage));
    VMX_TRY(r->pin.reserve(256));
    return 0;
}

void bgzf_in_close(BgzfIn* r) {
    if (r->pre_on) { r->pre.get(); r->pre_on = false; }
    if (r->c) (void)hipStreamSynchronize(r->c->stream);
    if (r->fd >= 0) { close(r->fd); r->fd = -1; }
}

// the next window into win[slot]: 1 (its records decoded, possibly none), 0 at the end of the file, or a negative status
int reader_window(vm_bam_reader* r, int slot) {
    vm_ctx* c = r->c;
    DecodedWin& D = r->h.win[slot];
    D.n = 0;
    int64_t avail = 0;
    const int irc = bgzf_in_window(&r->in, r->st, &avail);
    if (irc < 0) return irc;
    if (irc == 0) {
        if (r->in.carry > 0) { set_error(r->hdr_done ? "truncated file: BAM record " + std::to_string((long long)r->n_seen + 1) + " is not complete" : "truncated file: the BAM header is not complete"); return VM_ERR_IO; }
        return 0;
    }
    BgzfIn& in = r->in;
    DevBuf& dst = in.d_inf[in.which];
    double t0;
    int64_t begin = 0;
    if (!r->hdr_done) {
        std::vector<uint8_t> H;
        for (int64_t have = 0;;) {
            const int64_t want = std::min<int64_t>(avail, std::max<int64_t>(have * 4, 1 << 16));
            H.resize((size_t)want);
            if (want) VMX_HIP(hipMemcpy(H.data(), dst.p, (size_t)want, hipMemcpyDeviceToHost));
            have = want;
            const int pr = parse_bam_header(H.data(), have, &begin);
            if (pr < 0) { set_error("not a BAM file: the inflated stream does not begin with BAM\\1"); return VM_ERR_ARG; }
            if (pr > 0) break;
            if (have == avail) {
                if (in.file_done && avail < 4) { set_error("not a BAM file: the inflated stream does not begin with BAM\\1"); return VM_ERR_ARG; }
                in.tail_off = 0; in.carry = avail; return 1;
            }
        }
        r->hdr_done = true;
    }
    // records
    t0 = now_s();
    const int64_t max_rec = (avail - begin) / 36 + 1;
    VMX_TRY(r->d_roff.reserve((size_t)(max_rec + 1) * 8));
    VMX_TRY(r->d_walk.reserve(sizeof(vmx_bam_in_walk)));
    hipLaunchKernelGGL(k_bam_in_walk, dim3(1), dim3(64), 0, c->stream, dst.as<const uint8_t>(), begin, avail, max_rec, r->d_roff.as<int64_t>(), r->d_walk.as<vmx_bam_in_walk>());
    VMX_HIP(hipMemcpyAsync(in.pin.p, r->d_walk.p, sizeof(vmx_bam_in_walk), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    vmx_bam_in_walk W; memcpy(&W, in.pin.p, sizeof W);
    r->st[3] += now_s() - t0;
    if (W.err_key != ~0ull) {
        set_error("BAM record " + std::to_string((long long)(r->n_seen + (int64_t)(W.err_key >> 8)) + 1) + ": block_size is below 32, smaller than its name, CIGAR and bases, or above 512 MB");
        return VM_ERR_IO;
    }
    const int64_t n = W.n_rec, rec0 = r->n_seen;
    r->n_seen += n;
    in.tail_off = W.end; in.carry = avail - W.end;
    if (n == 0) return 1;
    t0 = now_s();
    const size_t col = (size_t)(n + 1);
    VMX_TRY(r->d_sz.reserve(col * 8 * 4)); VMX_TRY(r->d_off.reserve(col * 8 * 4)); VMX_TRY(r->d_ooff.reserve(col * 8 * 3));
    int64_t* sz = r->d_sz.as<int64_t>(); int64_t* off = r->d_off.as<int64_t>(); int64_t* oo = r->d_ooff.as<int64_t>();
    hipLaunchKernelGGL(k_bam_in_sizes, dim3(grid256(n + 1)), dim3(256), 0, c->stream, dst.as<const uint8_t>(), r->d_roff.as<const int64_t>(), n, sz, sz + col, sz + 2 * col, sz + 3 * col);
    for (int j = 0; j < 4; ++j) VMX_TRY(vmx_scan64(c, r->d_tmp, sz + j * col, off + j * col, col));
    int64_t* tot = (int64_t*)in.pin.p;
    for (int j = 0; j < 4; ++j) VMX_HIP(hipMemcpyAsync(tot + j, off + j * col + n, 8, hipMemcpyDeviceToHost, c->stream));
    const unsigned aux_grid = (unsigned)((n + 1 + 3) / 4);
    if (r->tags_on) {                                                   // the comment text's size pass, its scan, the first malformed record and the dropped fields
        VMX_TRY(r->d_csz.reserve(col * 8)); VMX_TRY(r->d_coff.reserve(col * 8)); VMX_TRY(r->d_ocoff.reserve(col * 8)); VMX_TRY(r->d_aux.reserve(16));
        VMX_HIP(hipMemsetAsync(r->d_aux.p, 0xff, 8, c->stream));
        VMX_HIP(hipMemsetAsync(r->d_aux.as<uint8_t>() + 8, 0, 8, c->stream));
        hipLaunchKernelGGL(k_bam_in_aux_size, dim3(aux_grid), dim3(256), 0, c->stream, dst.as<const uint8_t>(), r->d_roff.as<const int64_t>(), n, r->d_sel.as<const uint16_t>(),
                           (int)r->tags.size(), r->tags_all, r->d_csz.as<int64_t>(), r->d_aux.as<unsigned long long>(), r->d_aux.as<unsigned long long>() + 1);
        VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_csz.as<const int64_t>(), r->d_coff.as<int64_t>(), col));
        VMX_HIP(hipMemcpyAsync(tot + 4, r->d_coff.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, c->stream));
        VMX_HIP(hipMemcpyAsync(tot + 5, r->d_aux.p, 16, hipMemcpyDeviceToHost, c->stream));
    }
    VMX_TRY(sync(c));
    const int64_t tn = tot[0], ts = tot[1], tq = tot[2], nk = tot[3], tc = r->tags_on ? tot[4] : 0;
    if (r->tags_on) {
        uint64_t key; memcpy(&key, tot + 5, 8);
        if (key != ~0ull) {
            static const char* const why[] = {"fewer than 3 bytes are left for a field", "unknown field type", "unknown B array sub-type", "a fixed-size value runs past the record's end",
                                              "a Z or H value has no NUL inside the record", "a B array runs past the record's end"};
            const int code = (int)(key & 0xff);
            set_error("BAM record " + std::to_string((long long)(rec0 + (int64_t)(key >> 8)) + 1) + ": malformed auxiliary data: " +
                      (code >= VMX_BAM_IN_E_AUX_SHORT && code <= VMX_BAM_IN_E_AUX_COUNT ? why[code - VMX_BAM_IN_E_AUX_SHORT] : "unknown"));
            return VM_ERR_IO;
        }
        r->n_aux_dropped += tot[6];
    }
    r->n_dropped += n - nk;
    VMX_TRY(r->d_names.reserve((size_t)tn + 8)); VMX_TRY(r->d_seqs.reserve((size_t)ts + 8)); VMX_TRY(r->d_quals.reserve((size_t)tq + 8));
    hipLaunchKernelGGL(k_bam_in_decode, dim3((unsigned)((n + 1 + 3) / 4)), dim3(256), 0, c->stream, dst.as<const uint8_t>(), r->d_roff.as<const int64_t>(), n, off, off + col,
                       off + 2 * col, off + 3 * col, r->d_names.as<char>(), r->d_seqs.as<char>(), r->d_quals.as<char>(), oo, oo + col, oo + 2 * col);
    if (r->tags_on) {
        VMX_TRY(r->d_comments.reserve((size_t)tc + 8));
        hipLaunchKernelGGL(k_bam_in_aux_write, dim3(aux_grid), dim3(256), 0, c->stream, dst.as<const uint8_t>(), r->d_roff.as<const int64_t>(), n, r->d_sel.as<const uint16_t>(),
                           (int)r->tags.size(), r->tags_all, r->d_coff.as<const int64_t>(), off + 3 * col, r->d_comments.as<char>(), r->d_ocoff.as<int64_t>());
    }
    VMX_TRY(sync(c));
    r->st[4] += now_s() - t0;
    t0 = now_s();
    VMX_TRY(D.names.reserve((size_t)tn + 8)); VMX_TRY(D.seqs.reserve((size_t)ts + 8)); VMX_TRY(D.quals.reserve((size_t)tq + 8)); VMX_TRY(D.off.reserve((size_t)(nk + 1) * 8 * 4));
    if (tn) VMX_HIP(hipMemcpyAsync(D.names.p, r->d_names.p, (size_t)tn, hipMemcpyDeviceToHost, c->stream));
    if (ts) VMX_HIP(hipMemcpyAsync(D.seqs.p, r->d_seqs.p, (size_t)ts, hipMemcpyDeviceToHost, c->stream));
    if (tq) VMX_HIP(hipMemcpyAsync(D.quals.p, r->d_quals.p, (size_t)tq, hipMemcpyDeviceToHost, c->stream));
    for (int j = 0; j < 3; ++j) VMX_HIP(hipMemcpyAsync((int64_t*)D.off.p + j * (nk + 1), oo + j * col, (size_t)(nk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if (r->tags_on) {
        VMX_TRY(D.comments.reserve((size_t)tc + 8));
        if (tc) VMX_HIP(hipMemcpyAsync(D.comments.p, r->d_comments.p, (size_t)tc, hipMemcpyDeviceToHost, c->stream));
        VMX_HIP(hipMemcpyAsync((int64_t*)D.off.p + 3 * (nk + 1), r->d_ocoff.p, (size_t)(nk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    }
    VMX_TRY(sync(c));
    r->st[5] += now_s() - t0;
    D.n = nk; r->st[10] += (double)nk; r->st[11] = (double)r->n_dropped; r->st[12] = (double)r->n_aux_dropped;
    return 1;
}

// ------------------------------------------------------------------------------------------------ FASTQ windows (kernels: k_fastx_in.hip)

// the first 40 bytes of the header line of the window's record `rec`, as vm_fastx_read quotes them (the stream is idle)
int fq_header_text(vm_fastq_reader* r, const uint8_t* buf, int64_t rec, std::string* out) {
    int64_t k = 0, ab[2] = {0, 0};
    VMX_HIP(hipMemcpy(&k, r->d_rline.as<int64_t>() + rec, 8, hipMemcpyDeviceToHost));
    VMX_HIP(hipMemcpy(ab, r->d_ls.as<int64_t>() + k, 16, hipMemcpyDeviceToHost));
    char line[48];
    const int64_t raw = std::min<int64_t>(ab[1] - 1 - ab[0], 41);
    if (raw > 0) VMX_HIP(hipMemcpy(line, buf + ab[0], (size_t)raw, hipMemcpyDeviceToHost));
    int64_t len = raw;
    if (len > 0 && len < 41 && line[len - 1] == '\r') --len;              // (the line's last byte: its '\r' is not part of it)
    out->assign(line, (size_t)std::min<int64_t>(len, 40));
    return 0;
}

// The line table of a window buf[0, avail): ls[0 .. *n_lines] (k_fq_nl_count, the scan of its counts in d_coff, k_fq_nl_pos). last: the bytes behind the
// last newline are a line (*closing, when there are any). *n_lines == 0: the window holds no line yet and nothing more is launched. d_res is
// reset (its error key to all ones). Waits for the counts.
int fq_line_table(vm_fastq_reader* r, const uint8_t* buf, int64_t avail, bool last, int64_t* n_lines, int* closing) {
    vm_ctx* c = r->c;
    BgzfIn& in = r->in;
    const int64_t nch = (avail + VMX_FQ_CHUNK - 1) / VMX_FQ_CHUNK;
    VMX_TRY(r->d_cnt.reserve((size_t)(nch + 1) * 8)); VMX_TRY(r->d_coff.reserve((size_t)(nch + 1) * 8)); VMX_TRY(r->d_res.reserve(sizeof(vmx_fq_result)));
    vmx_fq_result* res = r->d_res.as<vmx_fq_result>();
    VMX_HIP(hipMemsetAsync(res, 0xff, sizeof(vmx_fq_result), c->stream));
    const unsigned gch = (unsigned)((nch + 3) / 4);
    hipLaunchKernelGGL(k_fq_nl_count, dim3(gch), dim3(256), 0, c->stream, buf, avail, nch, r->d_cnt.as<int64_t>(), res);
    VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_cnt.as<const int64_t>(), r->d_coff.as<int64_t>(), (size_t)nch + 1));
    VMX_HIP(hipMemcpyAsync(in.pin.p, r->d_coff.as<int64_t>() + nch, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_HIP(hipMemcpyAsync(in.pin.p + 8, res, sizeof(vmx_fq_result), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    int64_t n_nl; memcpy(&n_nl, in.pin.p, 8);
    vmx_fq_result R; memcpy(&R, in.pin.p + 8, sizeof R);
    *closing = last && R.tail_open ? 1 : 0;
    *n_lines = n_nl + *closing;
    if (*n_lines == 0) return 0;
    VMX_TRY(r->d_ls.reserve((size_t)(*n_lines + 1) * 8));
    hipLaunchKernelGGL(k_fq_nl_pos, dim3(gch), dim3(256), 0, c->stream, buf, avail, nch, r->d_coff.as<const int64_t>(), *n_lines, *closing, r->d_ls.as<int64_t>());
    return 0;
}

// download of a parsed window's n records: names, bases, qualities, comments and their offsets, in the order the hand-out reads them. off: the device
// columns name, comment, bases, qualities of `col` entries each; tn, tc, ts, tq: the blobs' bytes
int fq_download(vm_fastq_reader* r, DecodedWin& D, int64_t n, const int64_t* off, size_t col, int64_t tn, int64_t tc, int64_t ts, int64_t tq) {
    vm_ctx* c = r->c;
    const double t0 = now_s();
    VMX_TRY(D.names.reserve((size_t)tn + 8)); VMX_TRY(D.seqs.reserve((size_t)ts + 8)); VMX_TRY(D.quals.reserve((size_t)tq + 8)); VMX_TRY(D.comments.reserve((size_t)tc + 8));
    VMX_TRY(D.off.reserve((size_t)(n + 1) * 8 * 4));
    if (tn) VMX_HIP(hipMemcpyAsync(D.names.p, r->d_names.p, (size_t)tn, hipMemcpyDeviceToHost, c->stream));
    if (ts) VMX_HIP(hipMemcpyAsync(D.seqs.p, r->d_seqs.p, (size_t)ts, hipMemcpyDeviceToHost, c->stream));
    if (tq) VMX_HIP(hipMemcpyAsync(D.quals.p, r->d_quals.p, (size_t)tq, hipMemcpyDeviceToHost, c->stream));
    if (tc) VMX_HIP(hipMemcpyAsync(D.comments.p, r->d_comments.p, (size_t)tc, hipMemcpyDeviceToHost, c->stream));
    static const int col_of[4] = {0, 2, 3, 1};                              // host order names, bases, qualities, comments <- device columns name, comment, bases, qualities
    for (int j = 0; j < 4; ++j) VMX_HIP(hipMemcpyAsync((int64_t*)D.off.p + j * (n + 1), off + col_of[j] * col, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    r->st[5] += now_s() - t0;
    D.n = n; r->st[10] += (double)n;
    return 1;
}

int reader_window_fasta(vm_fastq_reader* r, int slot);

// the next window into win[slot]: 1 (its complete records parsed, possibly none), 0 at the end of the file, or a negative status
int reader_window(vm_fastq_reader* r, int slot) {
    if (r->fasta) return reader_window_fasta(r, slot);
    vm_ctx* c = r->c;
    BgzfIn& in = r->in;
    DecodedWin& D = r->h.win[slot];
    D.n = 0;
    if (r->fail_rc < 0) { set_error(r->fail_msg); return r->fail_rc; }
    int64_t avail = 0;
    const int irc = r->gz ? gzip_in_window(&in, r->gz, r->st, &avail) : bgzf_in_window(&in, r->st, &avail);
    if (irc < 0) return irc;
    if (irc == 0) {
        if (in.carry > 0) { set_error("truncated FASTQ record: the file ends inside record " + std::to_string((long long)r->n_seen + 1)); return VM_ERR_IO; }
        return 0;
    }
    const bool last = in.file_done;                                         // the bytes behind the last newline are a line only here
    const uint8_t* buf = in.d_inf[in.which].as<const uint8_t>();
    if (avail == 0) { in.tail_off = 0; in.carry = 0; return 1; }
    // newlines
    double t0 = now_s();
    int64_t n_lines = 0; int closing = 0;
    VMX_TRY(fq_line_table(r, buf, avail, last, &n_lines, &closing));
    if (n_lines == 0) { in.tail_off = 0; in.carry = avail; r->st[3] += now_s() - t0; return 1; }      // (a line longer than the window so far)
    vmx_fq_result* res = r->d_res.as<vmx_fq_result>();
    vmx_fq_result R;
    // states and records
    const int64_t ntile = (n_lines + VMX_FQ_LTILE) / VMX_FQ_LTILE;           // (covers line index n_lines, the scan's total slot)
    VMX_TRY(r->d_map.reserve((size_t)n_lines)); VMX_TRY(r->d_tile.reserve((size_t)ntile));
    VMX_TRY(r->d_start.reserve((size_t)(n_lines + 1) * 8)); VMX_TRY(r->d_ridx.reserve((size_t)(n_lines + 1) * 8)); VMX_TRY(r->d_rline.reserve((size_t)(n_lines + 1) * 8));
    const int64_t* ls = r->d_ls.as<const int64_t>();
    hipLaunchKernelGGL(k_fq_line_maps, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, buf, ls, n_lines, r->d_map.as<uint8_t>(), r->d_tile.as<uint8_t>());
    hipLaunchKernelGGL(k_fq_tile_scan, dim3(1), dim3(1024), 0, c->stream, r->d_tile.as<uint8_t>(), ntile);
    hipLaunchKernelGGL(k_fq_line_states, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, r->d_map.as<const uint8_t>(), r->d_tile.as<const uint8_t>(), n_lines, r->d_start.as<int64_t>());
    VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_start.as<const int64_t>(), r->d_ridx.as<int64_t>(), (size_t)n_lines + 1));
    hipLaunchKernelGGL(k_fq_records, dim3(grid256(n_lines)), dim3(256), 0, c->stream, r->d_start.as<const int64_t>(), r->d_ridx.as<const int64_t>(), n_lines, r->d_rline.as<int64_t>());
    hipLaunchKernelGGL(k_fq_result, dim3(1), dim3(64), 0, c->stream, buf, ls, r->d_ridx.as<const int64_t>(), r->d_rline.as<const int64_t>(), n_lines, avail, res);
    VMX_HIP(hipMemcpyAsync(in.pin.p, res, sizeof(vmx_fq_result), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    memcpy(&R, in.pin.p, sizeof R);
    r->st[3] += now_s() - t0;
    if (R.n_rec < 0 || R.end < 0 || R.end > avail) { set_error("vm_fastq_reader: the record pass left an offset outside the window"); return VM_ERR_HIP; }
    in.tail_off = R.end; in.carry = avail - R.end;
    int64_t n = R.n_rec;
    const int64_t rec0 = r->n_seen;
    // sizes, offsets, the first bad header (k_fq_result has looked at the header of the record that lacks lines, k_fq_sizes looks at the complete ones), the copy
    t0 = now_s();
    const size_t col = (size_t)(n + 1);
    VMX_TRY(r->d_sz.reserve(col * 8 * 4)); VMX_TRY(r->d_off.reserve(col * 8 * 4));
    int64_t* sz = r->d_sz.as<int64_t>(); int64_t* off = r->d_off.as<int64_t>();
    const int64_t* rline = r->d_rline.as<const int64_t>();
    uint64_t key = R.err_key;
    if (n > 0) {
        hipLaunchKernelGGL(k_fq_sizes, dim3((unsigned)((n + 1 + 3) / 4)), dim3(256), 0, c->stream, buf, ls, rline, n, sz, sz + col, sz + 2 * col, sz + 3 * col, (unsigned long long*)&res->err_key);
        for (int j = 0; j < 4; ++j) VMX_TRY(vmx_scan64(c, r->d_tmp, sz + j * col, off + j * col, col));
        VMX_HIP(hipMemcpyAsync(in.pin.p, &res->err_key, 8, hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        memcpy(&key, in.pin.p, 8);
    }
    if (key != ~0ull) {                                                     // the records in front of the bad header are good; the input ends there
        const int64_t bad = (int64_t)(key >> 8);
        const std::string num = std::to_string((long long)(rec0 + bad) + 1);
        if ((int)(key & 0xff) == VMX_FQ_E_FASTA) {
            r->fail_rc = VM_ERR_UNSUPPORTED;
            r->fail_msg = "record " + num + " begins with '>': FASTA is not read on the device, use the host reader (vm_fastx_read; driver: --fastx-reader host)";
        } else {
            std::string text;
            VMX_TRY(fq_header_text(r, buf, bad, &text));
            r->fail_rc = VM_ERR_IO;
            r->fail_msg = "not FASTA/FASTQ: " + text;
        }
        n = bad;
        if (n == 0) { set_error(r->fail_msg); return r->fail_rc; }
    }
    if (n == 0) return 1;
    r->n_seen += n;
    int64_t* tot = (int64_t*)in.pin.p;
    for (int j = 0; j < 4; ++j) VMX_HIP(hipMemcpyAsync(tot + j, off + j * col + n, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    const int64_t tn = tot[0], tc = tot[1], ts = tot[2], tq = tot[3];
    VMX_TRY(r->d_names.reserve((size_t)tn + 16)); VMX_TRY(r->d_comments.reserve((size_t)tc + 16)); VMX_TRY(r->d_seqs.reserve((size_t)ts + 16)); VMX_TRY(r->d_quals.reserve((size_t)tq + 16));
    hipLaunchKernelGGL(k_fq_copy, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, buf, ls, rline, n, off, off + col, off + 2 * col, off + 3 * col, r->d_names.as<uint8_t>(),
                       r->d_comments.as<uint8_t>(), r->d_seqs.as<uint8_t>(), r->d_quals.as<uint8_t>());
    VMX_TRY(sync(c));
    r->st[4] += now_s() - t0;
    return fq_download(r, D, n, off, col, tn, tc, ts, tq);
}

// ------------------------------------------------------------------------------------------------ FASTA and FASTQ windows (VM_READER_FASTA; kernels: k_fasta_reads.hip)

// reader_window under VM_READER_FASTA: the same file half, line table, statistics and download; the record rule is vm_fastx_read's whole one.
// A window is cut in front of its last record start unless it ends between records, or is the file's last and ends inside a FASTA record.
int reader_window_fasta(vm_fastq_reader* r, int slot) {
    vm_ctx* c = r->c;
    BgzfIn& in = r->in;
    DecodedWin& D = r->h.win[slot];
    D.n = 0;
    if (r->fail_rc < 0) { set_error(r->fail_msg); return r->fail_rc; }
    int64_t avail = 0;
    const int irc = r->gz ? gzip_in_window(&in, r->gz, r->st, &avail) : bgzf_in_window(&in, r->st, &avail);
    if (irc < 0) return irc;
    if (irc == 0) {
        if (in.carry == 0) return 0;
        // the file ended at a window's edge: the carried tail (a FASTA record waiting for its successor, or a FASTQ record that lacks lines) is the closing window
        DevBuf& dst = in.d_inf[in.which ^ 1];
        VMX_TRY(dst.reserve((size_t)in.carry + 64));
        VMX_HIP(hipMemcpyAsync(dst.p, in.d_inf[in.which].as<uint8_t>() + in.tail_off, (size_t)in.carry, hipMemcpyDeviceToDevice, c->stream));
        in.which ^= 1;
        avail = in.carry;
    }
    const bool last = in.file_done;                                         // the bytes behind the last newline are a line only here
    const uint8_t* buf = in.d_inf[in.which].as<const uint8_t>();
    if (avail == 0) { in.tail_off = 0; in.carry = 0; return 1; }
    // newlines
    double t0 = now_s();
    int64_t n_lines = 0; int closing = 0;
    VMX_TRY(fq_line_table(r, buf, avail, last, &n_lines, &closing));
    if (n_lines == 0) { in.tail_off = 0; in.carry = avail; r->st[3] += now_s() - t0; return 1; }      // (a line longer than the window so far)
    VMX_TRY(r->d_fres.reserve(sizeof(vmx_fr_result)));
    vmx_fr_result* fres = r->d_fres.as<vmx_fr_result>();
    VMX_HIP(hipMemsetAsync(fres, 0xff, sizeof(vmx_fr_result), c->stream));
    // states, records, the cut
    const int64_t ntile = (n_lines + VMX_FQ_LTILE) / VMX_FQ_LTILE;           // (covers line index n_lines, the scans' total slot)
    const size_t lcol = (size_t)(n_lines + 1);
    VMX_TRY(r->d_map.reserve(lcol * 2)); VMX_TRY(r->d_tile.reserve((size_t)ntile * 2)); VMX_TRY(r->d_state.reserve(lcol));
    VMX_TRY(r->d_start.reserve(lcol * 8)); VMX_TRY(r->d_ridx.reserve(lcol * 8)); VMX_TRY(r->d_rline.reserve(lcol * 8));
    const int64_t* ls = r->d_ls.as<const int64_t>();
    hipLaunchKernelGGL(k_fr_line_maps, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, buf, ls, n_lines, r->d_map.as<uint16_t>(), r->d_tile.as<uint16_t>());
    hipLaunchKernelGGL(k_fr_tile_scan, dim3(1), dim3(1024), 0, c->stream, r->d_tile.as<uint16_t>(), ntile);
    hipLaunchKernelGGL(k_fr_line_states, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, r->d_map.as<const uint16_t>(), r->d_tile.as<const uint16_t>(), n_lines,
                       r->d_state.as<uint8_t>(), r->d_start.as<int64_t>());
    VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_start.as<const int64_t>(), r->d_ridx.as<int64_t>(), lcol));
    hipLaunchKernelGGL(k_fq_records, dim3(grid256(n_lines)), dim3(256), 0, c->stream, r->d_start.as<const int64_t>(), r->d_ridx.as<const int64_t>(), n_lines, r->d_rline.as<int64_t>());
    hipLaunchKernelGGL(k_fr_result, dim3(1), dim3(64), 0, c->stream, buf, ls, r->d_state.as<const uint8_t>(), r->d_ridx.as<const int64_t>(), r->d_rline.as<const int64_t>(), n_lines,
                       avail, last ? 1 : 0, fres);
    VMX_HIP(hipMemcpyAsync(in.pin.p, fres, sizeof(vmx_fr_result), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    vmx_fr_result R; memcpy(&R, in.pin.p, sizeof R);
    r->st[3] += now_s() - t0;
    if (R.n_rec < 0 || R.end < 0 || R.end > avail || R.cut_line < 0 || R.cut_line > n_lines) { set_error("vm_fastq_reader: the record pass left an offset outside the window"); return VM_ERR_HIP; }
    in.tail_off = R.end; in.carry = avail - R.end;
    const bool truncated = last && R.end_state >= 1 && R.end_state <= 3;      // the file ends inside a FASTQ record: the error of the call behind this window's records
    if (last) in.carry = 0;
    int64_t n = R.n_rec;
    const int64_t rec0 = r->n_seen;
    // keep ranges and their scans, header sizes, the first bad header (k_fr_result has looked at the header of the record the cut stands in front of)
    t0 = now_s();
    const size_t col = (size_t)(n + 1);
    VMX_TRY(r->d_ka.reserve(lcol * 8)); VMX_TRY(r->d_ks.reserve(lcol * 8)); VMX_TRY(r->d_kq.reserve(lcol * 8)); VMX_TRY(r->d_so.reserve(lcol * 8)); VMX_TRY(r->d_qo.reserve(lcol * 8));
    VMX_TRY(r->d_sz.reserve(col * 8 * 2)); VMX_TRY(r->d_off.reserve(col * 8 * 4));
    int64_t* sz = r->d_sz.as<int64_t>(); int64_t* off = r->d_off.as<int64_t>();
    const int64_t* rline = r->d_rline.as<const int64_t>();
    uint64_t key = R.err_key;
    if (n > 0) {
        hipLaunchKernelGGL(k_fr_line_keep, dim3(grid256(n_lines + 1)), dim3(256), 0, c->stream, buf, ls, r->d_map.as<const uint16_t>(), r->d_state.as<const uint8_t>(), n_lines, R.cut_line,
                           r->d_ka.as<int64_t>(), r->d_ks.as<int64_t>(), r->d_kq.as<int64_t>());
        VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_ks.as<const int64_t>(), r->d_so.as<int64_t>(), lcol));
        VMX_TRY(vmx_scan64(c, r->d_tmp, r->d_kq.as<const int64_t>(), r->d_qo.as<int64_t>(), lcol));
        hipLaunchKernelGGL(k_fr_hdr_sizes, dim3((unsigned)((n + 1 + 3) / 4)), dim3(256), 0, c->stream, buf, ls, rline, n, R.cut_line, r->d_so.as<const int64_t>(), r->d_qo.as<const int64_t>(),
                           sz, sz + col, off + 2 * col, off + 3 * col, (unsigned long long*)&fres->err_key);
        for (int j = 0; j < 2; ++j) VMX_TRY(vmx_scan64(c, r->d_tmp, sz + j * col, off + j * col, col));
        VMX_HIP(hipMemcpyAsync(in.pin.p, &fres->err_key, 8, hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        memcpy(&key, in.pin.p, 8);
    }
    if (key != ~0ull) {                                                     // the records in front of the bad header are good; the input ends there
        const int64_t bad = (int64_t)(key >> 8);
        std::string text;
        VMX_TRY(fq_header_text(r, buf, bad, &text));
        r->fail_rc = VM_ERR_IO;
        r->fail_msg = "not FASTA/FASTQ: " + text;
        n = bad;
        if (n == 0) { set_error(r->fail_msg); return r->fail_rc; }
    }
    else if (truncated) {
        r->fail_rc = VM_ERR_IO;
        r->fail_msg = "truncated FASTQ record: the file ends inside record " + std::to_string((long long)(rec0 + n) + 1);
        if (n == 0) { set_error(r->fail_msg); return r->fail_rc; }
    }
    if (n == 0) return 1;
    r->n_seen += n;
    int64_t* tot = (int64_t*)in.pin.p;
    for (int j = 0; j < 4; ++j) VMX_HIP(hipMemcpyAsync(tot + j, off + j * col + n, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_HIP(hipMemcpyAsync(tot + 4, r->d_so.as<int64_t>() + n_lines, 8, hipMemcpyDeviceToHost, c->stream));        // what k_fr_copy writes: every kept byte in front of the cut
    VMX_HIP(hipMemcpyAsync(tot + 5, r->d_qo.as<int64_t>() + n_lines, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    const int64_t tn = tot[0], tc = tot[1], ts = tot[2], tq = tot[3], ws = tot[4], wq = tot[5];
    if (ts > ws || tq > wq || ws > avail || wq > avail) { set_error("vm_fastq_reader: the keep ranges do not add up"); return VM_ERR_HIP; }
    VMX_TRY(r->d_names.reserve((size_t)tn + 16)); VMX_TRY(r->d_comments.reserve((size_t)tc + 16)); VMX_TRY(r->d_seqs.reserve((size_t)ws + 16)); VMX_TRY(r->d_quals.reserve((size_t)wq + 16));
    const int64_t cch = (R.end + VMX_FQ_CHUNK - 1) / VMX_FQ_CHUNK;             // (nothing is kept at or behind the cut)
    if (cch > 0)
        hipLaunchKernelGGL(k_fr_copy, dim3((unsigned)((cch + 3) / 4)), dim3(256), 0, c->stream, buf, avail, cch, r->d_coff.as<const int64_t>(), r->d_ka.as<const int64_t>(),
                           r->d_ks.as<const int64_t>(), r->d_kq.as<const int64_t>(), r->d_so.as<const int64_t>(), r->d_qo.as<const int64_t>(), r->d_seqs.as<uint8_t>(), r->d_quals.as<uint8_t>());
    hipLaunchKernelGGL(k_fr_hdr_copy, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, c->stream, buf, ls, rline, n, off, off + col, r->d_names.as<uint8_t>(), r->d_comments.as<uint8_t>());
    VMX_TRY(sync(c));
    r->st[4] += now_s() - t0;
    return fq_download(r, D, n, off, col, tn, tc, ts, tq);
}

// ------------------------------------------------------------------------------------------------ hand-out, shared by both readers

// the producer thread: the device belongs to the reader's context, the message to the thread that asks for it
template <class R> int reader_produce(R* r, int slot) {
    (void)hipSetDevice(r->c->device);
    const int rc = reader_window(r, slot);
    if (rc < 0) r->h.prod_err = vm_last_error();
    return rc;
}

// win[cur] is drained: the window produced ahead becomes the current one and the next is started in the drained slot
template <class R> int reader_next(R* r) {
    HandOut& h = r->h;
    const int nxt = h.cur ^ 1;
    int rc;
    if (h.prod_on) { rc = h.prod.get(); h.prod_on = false; if (rc < 0) set_error(h.prod_err); }
    else rc = reader_window(r, nxt);
    memcpy(r->pub, r->st, sizeof r->pub);                               // (no window is in production here)
    if (rc < 0) return rc;
    h.cur = nxt; h.at = 0;
    if (rc == 0) { h.win[nxt].n = 0; return 0; }
    h.prod_on = true; h.prod_err.clear();
    h.prod = std::async(std::launch::async, reader_produce<R>, r, nxt ^ 1);
    return 1;
}

// up to max_reads records, cut where max_bases is reached as vm_fastx_read cuts; what is not handed out stays for the next call.
// with_comments: the windows hold a fourth blob and offset column
template <class R> int64_t reader_read(R* r, bool with_comments, const char* who, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs,
                                       int64_t** seq_off, char** quals, int64_t** qual_off, char** comments, int64_t** com_off) {
    const std::string oom = std::string(who) + ": out of host memory";
    HandOut& h = r->h;
    try {
        Grow nb, sb, qb, cb;
        std::vector<int64_t> no(1, 0), so(1, 0), qo(1, 0), co(1, 0);
        int64_t n = 0;
        bool end = false;
        while (n < max_reads && (int64_t)sb.n < max_bases && !end) {
            if (h.at >= h.win[h.cur].n) {
                const int rc = reader_next(r);
                if (rc < 0) return rc;
                if (rc == 0) end = true;
                continue;
            }
            const double t0 = now_s();
            const DecodedWin& D = h.win[h.cur];
            const int64_t nk = D.n;
            const int64_t* hn = (const int64_t*)D.off.p; const int64_t* hs = hn + (nk + 1); const int64_t* hq = hs + (nk + 1);
            const int64_t a = h.at;
            int64_t m = 0;
            while (a + m < nk && n + m < max_reads && (int64_t)sb.n + (hs[a + m] - hs[a]) < max_bases) ++m;
            if (!nb.append(D.names.p + hn[a], (size_t)(hn[a + m] - hn[a])) || !sb.append(D.seqs.p + hs[a], (size_t)(hs[a + m] - hs[a])) ||
                !qb.append(D.quals.p + hq[a], (size_t)(hq[a + m] - hq[a]))) { set_error(oom); return VM_ERR_OOM; }
            const int64_t n0 = no.back() - hn[a], s0 = so.back() - hs[a], q0 = qo.back() - hq[a];
            for (int64_t j = 1; j <= m; ++j) { no.push_back(n0 + hn[a + j]); so.push_back(s0 + hs[a + j]); qo.push_back(q0 + hq[a + j]); }
            if (with_comments) {                                        // the comments are cut where the records are
                const int64_t* hc = hq + (nk + 1);
                if (!cb.append(D.comments.p + hc[a], (size_t)(hc[a + m] - hc[a]))) { set_error(oom); return VM_ERR_OOM; }
                const int64_t c0 = co.back() - hc[a];
                for (int64_t j = 1; j <= m; ++j) co.push_back(c0 + hc[a + j]);
            }
            h.at += m; n += m;
            h.handout_s += now_s() - t0;
        }
        auto giveo = [](const std::vector<int64_t>& v, int64_t** p) { *p = (int64_t*)malloc(8 * v.size()); memcpy(*p, v.data(), 8 * v.size()); };
        *names = nb.release(); *seqs = sb.release(); *quals = qb.release(); *comments = cb.release();
        giveo(no, name_off); giveo(so, seq_off); giveo(qo, qual_off);
        if (!with_comments) co.assign((size_t)n + 1, 0);
        giveo(co, com_off);
        return n;
    }
    catch (const std::bad_alloc&) { set_error(oom); return VM_ERR_OOM; }
}

template <class R> void reader_close(R* r) {
    if (r->h.prod_on) (void)r->h.prod.get();
    bgzf_in_close(&r->in);
    delete r;
}

// ---- plain gzip (kernels: k_gzip_in.hip) ----
// One compressed window (vm_gzip_decompress: the whole input; a reader: VMX_BAM_IN_CHUNK bytes of the file) is searched for block starts per chunk of VMX_GZ_CHUNK bytes, every start is decoded by a
// wave of its own in a count pass, and the host links the chain on the small table that pass leaves: wave k is verified when wave k - 1 is
// and ended exactly at k's first bit. A start the chain steps over was false: it is dropped, and its verified predecessor is counted again
// up to the next start that remains. Only an error of a verified wave is the file's error. The verified waves are then written at their
// final offsets, the windows are passed along, markers are replaced and the members' CRC32 and ISIZE are compared.
struct GzipBufs { DevBuf comp, cand, tab, todo, res, sym, ev, win_in, win_out, ev_end, acc, key, out; };
// chunks started, candidates rejected, chunks decoded again, text bytes of the first chain, seconds in find / decode / window / resolve
struct GzipStats { double v[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };

const char* gzip_reason(int code) {
    switch (code) {
        case VMX_GZ_E_MAGIC: return "not a gzip member (bad magic)";
        case VMX_GZ_E_METHOD: return "gzip member with an unknown compression method";
        case VMX_GZ_E_BIG: return "more than 2 GB of text behind one block start";
        case VMX_BGZF_E_LONG: return "the write pass met more text than the count pass";
        default: return bgzf_reason(code);
    }
}

int gzip_wave_error(const vmx_gz_res& R, int64_t base_foff) {
    const std::string at = std::to_string((long long)(base_foff + (R.err_bit >> 3)));
    if (R.err == VMX_BGZF_E_INPUT) { set_error("truncated gzip input: what begins at file offset " + at + " is not complete"); return VM_ERR_IO; }
    if (R.err == VMX_GZ_E_BIG) { set_error(std::string("gzip: ") + gzip_reason((int)R.err) + " (file offset " + at + ")"); return VM_ERR_UNSUPPORTED; }
    if (R.err == VMX_GZ_E_MAGIC || R.err == VMX_GZ_E_METHOD) { set_error(std::string(gzip_reason((int)R.err)) + " at file offset " + at); return VM_ERR_IO; }
    set_error(std::string("gzip: ") + gzip_reason((int)R.err) + " in the block at file offset " + at);
    return R.err == VMX_BGZF_E_LONG ? VM_ERR_HIP : VM_ERR_IO;
}

// x^(8 n) modulo the CRC polynomial, and crc(A B) from crc(A), crc(B) and |B| (zlib's crc32_combine), on the host
uint32_t crc_x8n_host(uint64_t n) {
    const vmx_crc_x2n& t = crc_x2n_table();
    uint32_t mul = 1u << 31, k = 3;
    for (uint64_t r = n; r; r >>= 1, ++k) if (r & 1) mul = crc_multmodp(t.v[k & 31], mul);
    return mul;
}
uint32_t crc_combine_host(uint32_t a, uint32_t b, uint64_t len_b) { return crc_multmodp(crc_x8n_host(len_b), a) ^ b; }

// What is carried from one compressed window of a file to the next (GzipIn): where the next window begins (a verified block start or a member
// header), the 32 KB in front of it on the device, and of the member that is open there its text bytes so far, their CRC32 and its file offset
struct GzipCarry {
    uint32_t start_bit = 0; bool at_header = true;
    DevBuf win; bool have_win = false;
    uint64_t open = 0; uint32_t crc = 0; int64_t member_foff = 0;
};

// One compressed window: comp[0, n) (host), whose byte 0 is byte base_foff of the file; K says where in it the first wave begins and is
// left saying where the next window begins: *consumed_bits from comp[0]. last: the file ends with comp[n - 1], so input that runs out is
// truncation; otherwise the chain is cut at the last place in the window where a wave can begin. Of the linked waves the leading ones whose
// text fits max_text are taken (always one). The text -> z.out[0, *n_text). *done: the stream ended with the window. Waits for the result.
int gzip_window_run(vm_ctx* c, GzipBufs& z, HostPinned& pin, const uint8_t* comp, int64_t n, int64_t base_foff, bool last, int64_t max_text, GzipCarry& K, GzipStats& S,
                    int64_t* n_text, int64_t* consumed_bits, bool* done) {
    *n_text = 0; *consumed_bits = K.start_bit; *done = false;
    if (n > ((int64_t)1 << 28)) { set_error("gzip: more than 256 MB of compressed data in one window"); return VM_ERR_UNSUPPORTED; }
    int64_t chunk = 32768;                                              // (the best of 16, 32, 64 and 128 KB for FastqReader: profiles/gzip_input_reader.json)
    if (const char* e = getenv("VMX_GZ_CHUNK")) chunk = std::min<int64_t>(std::max<int64_t>(atoll(e), 1024), 1 << 26);
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    const uint32_t nb = (uint32_t)n;
    auto wave_error = [&](const vmx_gz_res& r) { return gzip_wave_error(r, base_foff); };
    int64_t cut_wave = -1;
    double t0 = now_s();
    VMX_TRY(z.comp.reserve((size_t)n + 64));
    VMX_TRY(z.cand.reserve((size_t)n_chunks * 4));
    VMX_HIP(hipMemsetAsync(z.comp.as<uint8_t>() + (n & ~(int64_t)3), 0, 32, c->stream));        // the last word's bytes behind the data are zeros
    VMX_HIP(hipMemcpyAsync(z.comp.p, comp, (size_t)n, hipMemcpyHostToDevice, c->stream));
    VMX_HIP(hipMemsetAsync(z.cand.p, 0xff, (size_t)n_chunks * 4, c->stream));
    if (n_chunks > 1)
        hipLaunchKernelGGL(k_gz_find, dim3((unsigned)(n_chunks - 1)), dim3(64), 0, c->stream, z.comp.as<const uint8_t>(), nb, (uint32_t)chunk, 1u, K.start_bit + 1u, z.cand.as<uint32_t>());
    VMX_TRY(pin.reserve((size_t)n_chunks * 4));
    VMX_HIP(hipMemcpyAsync(pin.p, z.cand.p, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    S.v[4] += now_s() - t0;
    // the waves: where the window begins, then every candidate
    std::vector<vmx_gz_wave> W;
    W.push_back(vmx_gz_wave{K.start_bit, VMX_GZ_NONE, K.at_header ? VMX_GZ_F_HEADER : 0u, 0, 0, 0, 0, 0});
    for (int64_t k = 1; k < n_chunks; ++k) {
        uint32_t b; memcpy(&b, pin.p + 4 * k, 4);
        if (b != VMX_GZ_NONE) W.push_back(vmx_gz_wave{b, VMX_GZ_NONE, 0, 0, 0, 0, 0, 0});
    }
    const int64_t nw = (int64_t)W.size();
    for (int64_t k = 0; k + 1 < nw; ++k) W[k].stop_bit = W[k + 1].start_bit;
    S.v[0] += (double)nw;
    // count passes and the link check
    t0 = now_s();
    std::vector<vmx_gz_res> R((size_t)nw);
    std::vector<uint32_t> todo((size_t)nw), chain{0};
    std::vector<char> alive((size_t)nw, 1);
    for (int64_t k = 0; k < nw; ++k) todo[k] = (uint32_t)k;
    VMX_TRY(z.tab.reserve((size_t)nw * sizeof(vmx_gz_wave)));
    VMX_TRY(z.todo.reserve((size_t)nw * 4));
    VMX_TRY(z.res.reserve((size_t)nw * sizeof(vmx_gz_res)));
    VMX_TRY(pin.reserve((size_t)nw * sizeof(vmx_gz_res)));
    int64_t cur = 0, sum_before = 0;
    bool linked = false;
    while (!linked) {
        VMX_HIP(hipMemcpyAsync(z.tab.p, W.data(), (size_t)nw * sizeof(vmx_gz_wave), hipMemcpyHostToDevice, c->stream));
        VMX_HIP(hipMemcpyAsync(z.todo.p, todo.data(), todo.size() * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_gz_count, dim3((unsigned)todo.size()), dim3(64), 0, c->stream, z.comp.as<const uint8_t>(), nb, z.tab.as<const vmx_gz_wave>(),
                           z.todo.as<const uint32_t>(), z.res.as<vmx_gz_res>());
        VMX_HIP(hipMemcpyAsync(pin.p, z.res.p, (size_t)nw * sizeof(vmx_gz_res), hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        for (uint32_t k : todo) memcpy(&R[k], pin.p + (size_t)k * sizeof(vmx_gz_res), sizeof(vmx_gz_res));
        todo.clear();
        for (;;) {
            const vmx_gz_res& r = R[cur];
            if (cur > 0 && sum_before >= max_text) {
                // the waves in front fill the window's text: this one and what follows start the next window, and whatever is wrong with them is
                // that window's error, behind the records of this one
                chain.pop_back();
                for (int64_t k = cur; k < nw; ++k) alive[k] = 0;
                linked = true;
                break;
            }
            if (r.err == VMX_BGZF_E_INPUT && !last) {
                // the window ends inside this wave: it is cut at the last place where a wave can begin, or, where that is its own start, left out
                if (r.resume_bit > W[cur].start_bit) { W[cur].stop_bit = r.resume_bit; cut_wave = cur; todo.push_back((uint32_t)cur); break; }
                if (cur == 0) { set_error("gzip: the block at file offset " + std::to_string((long long)(base_foff + (W[0].start_bit >> 3))) + " does not end inside one chunk of the reader"); return VM_ERR_UNSUPPORTED; }
                chain.pop_back();
                for (int64_t k = cur; k < nw; ++k) alive[k] = 0;
                linked = true;
                break;
            }
            if (r.err) return wave_error(r);
            int64_t nx = cur + 1;
            const bool at_end = (r.flags & VMX_GZ_R_END) != 0 || cur == cut_wave;       // (what lies behind a cut wave belongs to the next window)
            while (nx < nw && (!alive[nx] || at_end || W[nx].start_bit < r.end_bit)) { if (alive[nx]) { alive[nx] = 0; if (cur != cut_wave) S.v[1] += 1; } ++nx; }
            if (at_end) { linked = true; break; }
            if (nx < nw && W[nx].start_bit == r.end_bit) { chain.push_back((uint32_t)nx); sum_before += r.n_sym; cur = nx; continue; }
            const uint32_t stop = nx < nw ? W[nx].start_bit : VMX_GZ_NONE;
            if (stop == W[cur].stop_bit) { set_error("gzip: the block chain does not advance"); return VM_ERR_HIP; }
            W[cur].stop_bit = stop; todo.push_back((uint32_t)cur); S.v[2] += 1;
            break;
        }
    }
    if (K.at_header && K.start_bit == 0 && base_foff == 0) S.v[3] = (double)R[0].n_sym;
    // the leading verified waves whose text fits, at their final offsets
    int64_t nv = 0, total = 0, n_ev = 0;
    uint64_t open = K.open;
    std::vector<vmx_gz_wave> V;
    for (size_t i = 0; i < chain.size(); ++i) {
        const vmx_gz_res& r = R[chain[i]];
        if (i > 0 && total + (int64_t)r.n_sym > max_text) break;
        vmx_gz_wave v = W[chain[i]];
        v.hist = (uint32_t)std::min<uint64_t>(open, VMX_GZ_WIN); v.ooff = total; v.eoff = n_ev; v.n_sym = r.n_sym; v.n_ev = r.n_ev;
        V.push_back(v);
        open = r.flags & VMX_GZ_R_MEMBER ? (uint64_t)r.open : open + r.n_sym;
        total += r.n_sym; n_ev += r.n_ev; ++nv;
    }
    const bool all = nv == (int64_t)chain.size();
    const vmx_gz_res& rl = R[chain[nv - 1]];
    const bool next_hdr = all ? (rl.flags & (VMX_GZ_R_END | VMX_GZ_R_HEADER)) != 0 : false;
    *consumed_bits = all ? (int64_t)rl.end_bit : (int64_t)W[chain[nv]].start_bit;
    *done = all && last && (rl.flags & VMX_GZ_R_END) != 0;
    if (nv == 0) return 0;                                              // (cannot be: wave 0 is verified by definition or the call has returned)
    if (total >= ((int64_t)1 << 32)) { set_error("gzip: 4 GB of text or more in one window"); return VM_ERR_UNSUPPORTED; }
    VMX_TRY(z.sym.reserve((size_t)(total + 64) * 2));
    VMX_TRY(z.out.reserve((size_t)total + 128));
    VMX_TRY(z.ev.reserve((size_t)(n_ev + 1) * sizeof(vmx_gz_member)));
    VMX_TRY(z.ev_end.reserve((size_t)(n_ev + 1) * 8));
    VMX_TRY(z.acc.reserve((size_t)(n_ev + 1) * 4));
    VMX_TRY(z.win_in.reserve((size_t)nv * VMX_GZ_WIN));
    VMX_TRY(z.win_out.reserve(VMX_GZ_WIN));
    VMX_TRY(z.key.reserve(8));
    VMX_TRY(pin.reserve((size_t)nv * sizeof(vmx_gz_res) + (size_t)(n_ev + 1) * sizeof(vmx_gz_member) + 64));
    VMX_HIP(hipMemcpyAsync(z.tab.p, V.data(), (size_t)nv * sizeof(vmx_gz_wave), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gz_decode, dim3((unsigned)nv), dim3(64), 0, c->stream, z.comp.as<const uint8_t>(), nb, z.tab.as<const vmx_gz_wave>(), z.res.as<vmx_gz_res>(),
                       z.sym.as<uint16_t>(), z.ev.as<vmx_gz_member>());
    char* p_ev = pin.p + (size_t)nv * sizeof(vmx_gz_res);
    VMX_HIP(hipMemcpyAsync(pin.p, z.res.p, (size_t)nv * sizeof(vmx_gz_res), hipMemcpyDeviceToHost, c->stream));
    if (n_ev) VMX_HIP(hipMemcpyAsync(p_ev, z.ev.p, (size_t)n_ev * sizeof(vmx_gz_member), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    for (int64_t i = 0; i < nv; ++i) {
        vmx_gz_res r; memcpy(&r, pin.p + (size_t)i * sizeof(vmx_gz_res), sizeof r);
        const vmx_gz_res& q = R[chain[i]];
        if (r.err) return wave_error(r);
        if (r.n_sym != q.n_sym || r.n_ev != q.n_ev || r.end_bit != q.end_bit) { set_error("gzip: the write pass and the count pass disagree"); return VM_ERR_HIP; }
    }
    std::vector<vmx_gz_member> M((size_t)n_ev);
    std::vector<uint64_t> ev_end((size_t)n_ev + 1);
    if (n_ev) memcpy(M.data(), p_ev, (size_t)n_ev * sizeof(vmx_gz_member));
    for (int64_t i = 0; i < nv; ++i) for (int64_t e = V[i].eoff; e < V[i].eoff + V[i].n_ev; ++e) ev_end[e] = (uint64_t)(V[i].ooff + M[e].opos);
    ev_end[n_ev] = (uint64_t)total;                                     // the member that is open where the text ends: its piece's CRC32 is carried
    S.v[5] += now_s() - t0;
    if (total) {
        t0 = now_s();
        hipLaunchKernelGGL(k_gz_window, dim3(1), dim3(1024), 0, c->stream, z.sym.as<const uint16_t>(), z.tab.as<const vmx_gz_wave>(), nv,
                           K.have_win ? K.win.as<const uint8_t>() : (const uint8_t*)nullptr, z.win_in.as<uint8_t>(), z.win_out.as<uint8_t>());
        VMX_TRY(sync(c));
        S.v[6] += now_s() - t0;
        t0 = now_s();
        VMX_HIP(hipMemcpyAsync(z.ev_end.p, ev_end.data(), (size_t)(n_ev + 1) * 8, hipMemcpyHostToDevice, c->stream));
        VMX_HIP(hipMemsetAsync(z.acc.p, 0, (size_t)(n_ev + 1) * 4, c->stream));
        VMX_HIP(hipMemsetAsync(z.key.p, 0xff, 8, c->stream));
        hipLaunchKernelGGL(k_gz_resolve, dim3((unsigned)((total + VMX_GZ_TILE - 1) / VMX_GZ_TILE)), dim3(256), 0, c->stream, z.sym.as<const uint16_t>(),
                           z.tab.as<const vmx_gz_wave>(), nv, z.win_in.as<const uint8_t>(), z.ev_end.as<const uint64_t>(), n_ev + 1, total, crc_x2n_table(), z.out.as<uint8_t>(),
                           z.acc.as<uint32_t>(), z.key.as<unsigned long long>());
        VMX_HIP(hipMemcpyAsync(pin.p, z.key.p, 8, hipMemcpyDeviceToHost, c->stream));
        VMX_HIP(hipMemcpyAsync(pin.p + 64, z.acc.p, (size_t)(n_ev + 1) * 4, hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
        S.v[7] += now_s() - t0;
        uint64_t key; memcpy(&key, pin.p, 8);
        if (key != ~0ull) {
            int64_t i = 0;
            while (i + 1 < nv && V[i + 1].ooff <= (int64_t)key) ++i;
            set_error("gzip: " + std::string(bgzf_reason(VMX_BGZF_E_DIST)) + " in the blocks from file offset " + std::to_string((long long)(base_foff + (V[i].start_bit >> 3))));
            return VM_ERR_IO;
        }
    }
    // every member that ends in this window: its CRC32 and ISIZE, with what was carried for the one that was open; then the new carry
    uint64_t begin = 0;
    for (int64_t e = 0; e <= n_ev; ++e) {
        uint32_t piece = 0;
        if (total) memcpy(&piece, pin.p + 64 + 4 * e, 4);
        const uint64_t len = ev_end[e] - begin;
        const uint32_t crc = e == 0 ? crc_combine_host(K.crc, piece, len) : piece;
        const uint64_t size = e == 0 ? K.open + len : len;
        if (e == n_ev) { K.crc = crc; K.open = size; break; }
        const std::string where = "gzip member at file offset " + std::to_string((long long)K.member_foff) + ": ";
        if ((uint32_t)size != M[e].isize) { set_error(where + "ISIZE mismatch"); return VM_ERR_IO; }
        if (crc != M[e].crc) { set_error(where + "CRC32 mismatch"); return VM_ERR_IO; }
        begin = ev_end[e]; K.member_foff = base_foff + (int64_t)M[e].next_byte;
        if (e == 0) { K.crc = 0; K.open = 0; }
    }
    if (total) {
        VMX_TRY(K.win.reserve(VMX_GZ_WIN));
        VMX_HIP(hipMemcpyAsync(K.win.p, z.win_out.p, VMX_GZ_WIN, hipMemcpyDeviceToDevice, c->stream));
        VMX_TRY(sync(c));
        K.have_win = true;
    }
    K.start_bit = (uint32_t)(*consumed_bits & 7); K.at_header = next_hdr;
    *n_text = total;
    return 0;
}

// comp[0, n) (host): a series of complete gzip members -> z.out[0, *n_text) on the device; waits for the result
int gzip_inflate_buffer(vm_ctx* c, GzipBufs& z, HostPinned& pin, const uint8_t* comp, int64_t n, GzipStats& S, int64_t* n_text) {
    S = GzipStats();
    *n_text = 0;
    if (n < 2 || comp[0] != 0x1f || comp[1] != 0x8b) { set_error("not a gzip member (bad magic) at file offset 0"); return VM_ERR_IO; }
    GzipCarry K;
    int64_t used = 0; bool done = false;
    return gzip_window_run(c, z, pin, comp, n, 0, true, INT64_MAX, K, S, n_text, &used, &done);
}

// The file half of a reader of plain gzip: beside BgzfIn, whose file, staging buffer, inflate buffers and carried tail it uses, with
// bgzf_in_window's contract: "d_inf[which] holds *avail bytes of text behind the carried tail". A window is the VMX_BAM_IN_CHUNK bytes of the
// file from the byte of the next block on; what links the windows is GzipCarry. READ-AHEAD: ch[0].stage (two chunks of room) holds the
// file's bytes [fpos, fpos + have). The next window begins somewhere inside this one, so what it needs beyond these bytes is known before this
// window's chain is linked: the chunk_bytes behind fpos + have. They are read into ch[1].stage on a thread of its own while the device
// works on this window, and appended when the next window is asked for; what this window consumed is then dropped from the front.
struct GzipIn { GzipBufs z; GzipCarry K; GzipStats S; int64_t fpos = 0, have = 0; bool eof = false; int64_t pre_want = 0; };

void gzip_in_free(GzipIn* g) { delete g; }

// bytes [at, at + want) of the file into k.stage; k.got: how many there were; k.rc / k.err on a read error
void gzip_read_into(BgzfIn* r, int slot, int64_t off_in_stage, int64_t at, int64_t want) {
    BamInChunk& k = r->ch[slot];
    const double t0 = now_s();
    k.got = 0; k.rc = 0; k.err.clear();
    while (k.got < want) {
        const ssize_t q = pread(r->fd, k.stage.p + off_in_stage + k.got, (size_t)(want - k.got), (off_t)(at + k.got));
        if (q < 0) { k.rc = VM_ERR_IO; k.err = "read error at file offset " + std::to_string((long long)(at + k.got)); break; }
        if (q == 0) break;
        k.got += q;
    }
    k.busy = now_s() - t0;
}

int gzip_in_window(BgzfIn* r, GzipIn* g, double* st, int64_t* avail_out) {
    vm_ctx* c = r->c;
    if (r->file_done) return 0;
    BamInChunk& k = r->ch[0];
    double t0 = now_s();
    VMX_TRY(k.stage.reserve((size_t)std::min<int64_t>(2 * r->chunk_bytes, std::max<int64_t>(r->fsize, 1))));      // (reserved once: the size does not change)
    if (r->pre_on) {                                                    // what was read ahead goes behind the bytes in hand
        r->pre.get(); r->pre_on = false;
        BamInChunk& a = r->ch[1];
        st[0] += a.busy;
        if (a.rc < 0) { set_error(a.err); return a.rc; }
        memcpy(k.stage.p + g->have, a.stage.p, (size_t)a.got);
        g->have += a.got;
        if (a.got < g->pre_want) g->eof = true;
    }
    if (g->have < r->chunk_bytes && !g->eof) {                          // the first window (nothing was read ahead yet)
        const int64_t want = r->chunk_bytes - g->have;
        gzip_read_into(r, 0, g->have, g->fpos + g->have, want);
        if (k.rc < 0) { set_error(k.err); return k.rc; }
        st[0] += k.busy;
        g->have += k.got;
        if (k.got < want) g->eof = true;
    }
    st[1] += now_s() - t0;
    if (g->have == 0) {                                                 // the file ended at a window's edge
        if (!g->K.at_header) { set_error("truncated gzip input: what begins at file offset " + std::to_string((long long)g->fpos) + " is not complete"); return VM_ERR_IO; }
        r->file_done = true;
        return 0;
    }
    k.got = std::min<int64_t>(g->have, r->chunk_bytes);
    const bool last = g->eof && k.got == g->have;
    if (!g->eof && g->have <= r->chunk_bytes) {                         // read ahead while the device works
        VMX_TRY(r->ch[1].stage.reserve((size_t)std::min<int64_t>(r->chunk_bytes, std::max<int64_t>(r->fsize, 1))));
        g->pre_want = r->chunk_bytes;
        r->pre_on = true;
        r->pre = std::async(std::launch::async, gzip_read_into, r, 1, (int64_t)0, g->fpos + g->have, g->pre_want);
    }
    t0 = now_s();
    int64_t text = 0, used = 0; bool done = false;
    VMX_TRY(gzip_window_run(c, g->z, r->pin, (const uint8_t*)k.stage.p, k.got, g->fpos, last, r->max_inf, g->K, g->S, &text, &used, &done));
    DevBuf& dst = r->d_inf[r->which ^ 1];
    const int64_t avail = r->carry + text;
    VMX_TRY(dst.reserve((size_t)avail + 64));
    if (r->carry) VMX_HIP(hipMemcpyAsync(dst.p, r->d_inf[r->which].as<uint8_t>() + r->tail_off, (size_t)r->carry, hipMemcpyDeviceToDevice, c->stream));
    if (text) VMX_HIP(hipMemcpyAsync(dst.as<uint8_t>() + r->carry, g->z.out.p, (size_t)text, hipMemcpyDeviceToDevice, c->stream));
    VMX_TRY(sync(c));
    r->which ^= 1;
    const int64_t eaten = used >> 3;                                    // whole bytes in front of the next window's first bit
    memmove(k.stage.p, k.stage.p + eaten, (size_t)(g->have - eaten));
    g->have -= eaten; g->fpos += eaten;
    if (done) r->file_done = true;
    st[2] += now_s() - t0; st[7] += 1; st[8] += (double)(used >> 3); st[9] += (double)text;
    *avail_out = avail;
    return 1;
}

double gzip_in_stat(const GzipIn* g, int i) { return g && i >= 0 && i < 8 ? g->S.v[i] : 0.0; }

GzipIn* gzip_in_new() { return new GzipIn(); }

}  // namespace

extern "C" {

int vm_gzip_decompress_stats(vm_ctx* c, const void* in, int64_t n, char** out, int64_t* n_out, double* stats, int n_stats) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || !n_out || n < 0 || (n > 0 && !in) || (n_stats > 0 && !stats)) return VM_ERR_ARG;
    GzipBufs z; HostPinned pin; GzipStats S;
    int64_t total = 0;
    int rc = 0;
    if (n > 0) rc = gzip_inflate_buffer(c, z, pin, (const uint8_t*)in, n, S, &total);
    for (int i = 0; i < n_stats; ++i) stats[i] = i < 8 ? S.v[i] : 0.0;
    char* res = nullptr;
    if (rc == 0 && !(res = (char*)malloc((size_t)total + 1))) { set_error("out of host memory"); rc = VM_ERR_OOM; }
    if (rc == 0 && total && hipMemcpy(res, z.out.p, (size_t)total, hipMemcpyDeviceToHost) != hipSuccess) { set_error("vm_gzip_decompress: download failed"); rc = VM_ERR_HIP; }
    (void)hipStreamSynchronize(c->stream);
    if (rc < 0) { free(res); return rc; }
    *out = res; *n_out = total;
    return 0;
}

int vm_gzip_decompress(vm_ctx* c, const void* in, int64_t n, char** out, int64_t* n_out) { return vm_gzip_decompress_stats(c, in, n, out, n_out, nullptr, 0); }

int vm_bgzf_decompress(vm_ctx* c, const void* in, int64_t n, char** out, int64_t* n_out) {
    if (out) *out = nullptr;
    if (n_out) *n_out = 0;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || !n_out || n < 0 || (n > 0 && !in)) return VM_ERR_ARG;
    MemberTab T; std::string err; bool nb = false;
    const int wrc = walk_members((const uint8_t*)in, n, 0, INT64_MAX, T, &err, &nb);
    if (wrc < 0) { set_error(err); return wrc; }
    if (T.consumed != n) { set_error("truncated input: the BGZF member at file offset " + std::to_string((long long)T.consumed) + " is not complete"); return VM_ERR_IO; }
    InflateBufs z; HostPinned pin; DevBuf d_out;
    int rc = d_out.reserve((size_t)T.inflated + 64);
    if (rc == 0) rc = inflate_run(c, z, pin, (const uint8_t*)in, n, T, d_out.as<uint8_t>());
    char* res = nullptr;
    if (rc == 0 && !(res = (char*)malloc((size_t)T.inflated + 1))) { set_error("out of host memory"); rc = VM_ERR_OOM; }
    if (rc == 0 && T.inflated && hipMemcpy(res, d_out.p, (size_t)T.inflated, hipMemcpyDeviceToHost) != hipSuccess) { set_error("vm_bgzf_decompress: download failed"); rc = VM_ERR_HIP; }
    (void)hipStreamSynchronize(c->stream);
    if (rc < 0) { free(res); return rc; }
    *out = res; *n_out = T.inflated;
    return 0;
}

void vm_bam_reader_close(vm_bam_reader* r) {
    if (!r) return;
    reader_close(r);
}

int vm_bam_reader_open(vm_ctx* c, const char* path, vm_bam_reader** out) { return vm_bam_reader_open_tags(c, path, nullptr, out); }

int vm_bam_reader_open_tags(vm_ctx* c, const char* path, const char* tags, vm_bam_reader** out) {
    if (out) *out = nullptr;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || !path) return VM_ERR_ARG;
    std::vector<uint16_t> sel;
    const bool all = tags && strcmp(tags, "*") == 0;
    if (tags && *tags && !all) {                                        // XX(,XX)*, each [A-Za-z][A-Za-z0-9] (SAMv1 1.5)
        for (const char* q = tags;; q += 3) {
            const bool ok = isalpha((unsigned char)q[0]) && isalnum((unsigned char)q[1]) && (q[2] == ',' || q[2] == 0);
            if (!ok) { set_error(std::string("vm_bam_reader_open_tags: the tag list is neither empty, \"*\" nor two-character tags separated by commas: ") + tags); return VM_ERR_ARG; }
            sel.push_back((uint16_t)((uint8_t)q[0] | (uint16_t)(uint8_t)q[1] << 8));
            if (q[2] == 0) break;
        }
    }
    vm_bam_reader* r = new vm_bam_reader();
    r->c = c;
    r->tags_on = all || !sel.empty(); r->tags_all = all ? 1 : 0; r->tags = sel;
    int rc = bgzf_in_open(&r->in, c, path);
    if (rc == 0 && r->tags_on) rc = r->d_sel.reserve(sel.size() * 2 + 8);
    if (rc == 0 && !sel.empty() && hipMemcpy(r->d_sel.p, sel.data(), sel.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { set_error("vm_bam_reader_open_tags: upload failed"); rc = VM_ERR_HIP; }
    if (rc == 0 && r->in.fsize == 0) { set_error(std::string("empty file: ") + path); rc = VM_ERR_IO; }
    while (rc == 0 && !r->hdr_done) {
        rc = reader_window(r, 0);
        if (rc == 0) { set_error("truncated file: the BAM header is not complete"); rc = VM_ERR_IO; }
        else if (rc > 0) rc = 0;
    }
    if (rc < 0) { vm_bam_reader_close(r); return rc; }
    r->h.cur = 0; r->h.at = 0;
    memcpy(r->pub, r->st, sizeof r->pub);
    r->h.prod_on = true;                                                // the second window is decoded while the caller takes the first
    r->h.prod = std::async(std::launch::async, reader_produce<vm_bam_reader>, r, 1);
    *out = r;
    return 0;
}

int64_t vm_bam_reader_read(vm_bam_reader* r, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs, int64_t** seq_off, char** quals,
                           int64_t** qual_off, char** comments, int64_t** com_off) {
    if (!r || !r->c) return VM_ERR_NO_CTX;
    if (!names || !name_off || !seqs || !seq_off || !quals || !qual_off || !comments || !com_off) return VM_ERR_ARG;
    return reader_read(r, r->tags_on, "vm_bam_reader_read", max_reads, max_bases, names, name_off, seqs, seq_off, quals, qual_off, comments, com_off);
}

int vm_bam_reader_stats(const vm_bam_reader* r, double* out, int n) {
    if (!r || !out) return VM_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = i == 6 ? r->h.handout_s : i < 13 ? r->pub[i] : 0.0;       // (both written by the caller's own thread)
    return 0;
}

/* ---- bgzipped FASTQ (include/vacmapx.h) ---- */

void vm_fastq_reader_close(vm_fastq_reader* r) {
    if (!r) return;
    reader_close(r);
}

int vm_fastq_reader_open(vm_ctx* c, const char* path, vm_fastq_reader** out) { return vm_fastq_reader_open_opts(c, path, 0, out); }

int vm_fastq_reader_open_opts(vm_ctx* c, const char* path, int flags, vm_fastq_reader** out) {
    if (out) *out = nullptr;
    if (!c) return VM_ERR_NO_CTX;
    if (!out || !path) return VM_ERR_ARG;
    if (flags & ~(VM_READER_GZIP_DEVICE | VM_READER_FASTA)) { set_error("vm_fastq_reader_open_opts: unknown flag bits " + std::to_string(flags & ~(VM_READER_GZIP_DEVICE | VM_READER_FASTA))); return VM_ERR_ARG; }
    vm_fastq_reader* r = new vm_fastq_reader();
    r->c = c;
    r->fasta = (flags & VM_READER_FASTA) != 0;
    int rc = bgzf_in_open(&r->in, c, path);
    if (rc == 0 && r->in.fsize == 0) { set_error(std::string("empty file: ") + path); rc = VM_ERR_IO; }
    if (rc == 0) {
        unsigned char magic[2] = {0, 0};
        const ssize_t got = pread(r->in.fd, magic, 2, 0);
        if (got < 0) { set_error(std::string("cannot read ") + path); rc = VM_ERR_IO; }
        else if (got < 2 || magic[0] != 0x1f || magic[1] != 0x8b) { set_error(std::string("not a gzip file (the device reader takes bgzipped FASTQ): ") + path); rc = VM_ERR_UNSUPPORTED; }
    }
    if (rc == 0 && (flags & VM_READER_GZIP_DEVICE)) {                   // plain gzip (no BGZF BC subfield in the first member) goes through GzipIn
        unsigned char h[18] = {0};
        const ssize_t got = pread(r->in.fd, h, 18, 0);
        const bool bgzf = got == 18 && h[3] == 4 && h[12] == 'B' && h[13] == 'C';
        if (!bgzf) r->gz = gzip_in_new();
    }
    // windows until one holds a record: the first record's header decides at once whether this is FASTQ
    int w = 1;
    while (rc == 0 && w == 1 && r->h.win[0].n == 0) { w = reader_window(r, 0); if (w < 0) rc = w; }
    if (rc < 0) { vm_fastq_reader_close(r); return rc; }
    r->h.cur = 0; r->h.at = 0;
    memcpy(r->pub, r->st, sizeof r->pub);
    if (w == 1) {                                                       // the second window is parsed while the caller takes the first
        r->h.prod_on = true;
        r->h.prod = std::async(std::launch::async, reader_produce<vm_fastq_reader>, r, 1);
    }
    *out = r;
    return 0;
}

int64_t vm_fastq_reader_read(vm_fastq_reader* r, int64_t max_reads, int64_t max_bases, char** names, int64_t** name_off, char** seqs, int64_t** seq_off, char** quals,
                             int64_t** qual_off, char** comments, int64_t** com_off) {
    if (!r || !r->c) return VM_ERR_NO_CTX;
    if (!names || !name_off || !seqs || !seq_off || !quals || !qual_off || !comments || !com_off) return VM_ERR_ARG;
    return reader_read(r, true, "vm_fastq_reader_read", max_reads, max_bases, names, name_off, seqs, seq_off, quals, qual_off, comments, com_off);
}

int vm_fastq_reader_stats(const vm_fastq_reader* r, double* out, int n) {
    if (!r || !out) return VM_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = i == 6 ? r->h.handout_s : i < 11 ? r->pub[i] : i < 19 ? gzip_in_stat(r->gz, i - 11) : 0.0;
    return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ the reference FASTA (kernels: k_fasta_in.hip)
// The text of a reference goes through the device window by window: plain files by read(2) into page-locked staging (read ahead on a thread),
// plain gzip through zlib on that thread into the same staging, BGZF through BgzfIn. What is carried from window to window: the bases so far,
// "a header has been seen", "at a line start", and as bytes the incomplete header line or the '\r' run the window was cut in front of.

namespace {

struct RefRaw {                                         // plain or plain-gzip input: two staging buffers, the next one filled while the device parses
    int fd = -1; gzFile gz = nullptr;
    int64_t win = 0;
    HostPinned stage[2]; int64_t got[2] = {0, 0}; int rc[2] = {0, 0}; bool eof[2] = {false, false}; std::string err[2]; double busy[2] = {0, 0};
    std::future<void> pre; bool pre_on = false; int slot = 0;
    ~RefRaw() { if (pre_on) pre.get(); if (gz) gzclose(gz); else if (fd >= 0) close(fd); }
};

void ref_raw_fill(RefRaw* s, int k) {
    const double t0 = now_s();
    s->got[k] = 0; s->rc[k] = 0; s->eof[k] = false; s->err[k].clear();
    while (s->got[k] < s->win) {
        const int64_t want = std::min<int64_t>(s->win - s->got[k], 1 << 30);
        const int64_t q = s->gz ? (int64_t)gzread(s->gz, s->stage[k].p + s->got[k], (unsigned)want) : (int64_t)read(s->fd, s->stage[k].p + s->got[k], (size_t)want);
        if (q < 0) { s->rc[k] = VM_ERR_IO; s->err[k] = s->gz ? std::string("gzip stream: ") + gzerror(s->gz, nullptr) : std::string("read error"); break; }
        if (q == 0) {
            s->eof[k] = true;
            int en = Z_OK;
            if (s->gz) { const char* msg = gzerror(s->gz, &en); if (en != Z_OK && en != Z_STREAM_END) { s->rc[k] = VM_ERR_IO; s->err[k] = std::string("gzip stream: ") + msg; } }
            break;
        }
        s->got[k] += q;
    }
    s->busy[k] = now_s() - t0;
}

struct RefParse {
    vm_ctx* c = nullptr; vm_index* mi = nullptr;
    DevBuf d_map, d_tile, d_state, d_res, d_cnt, d_coff, d_tmp, d_wout, d_hpos, d_hbase, d_hsz, d_hoff, d_blob, d_other;
    HostPinned pin;
    int64_t base = 0; int seen = 0, ls0 = 1;             // carried: bases so far, a header has been seen, the window begins at a line start
    std::vector<int64_t> starts;
    int64_t win = 0; std::string path;
    double* st = nullptr;
};

// the codes so far are kept when the buffer has to grow (compressed input: the total is not known in front)
int ref_codes_room(RefParse& R, int64_t need) {
    DevBuf& d = R.mi->d_codes;
    if (d.p && (size_t)need + 64 <= d.cap) return 0;
    if (!d.p || R.base == 0) return d.reserve((size_t)need + 64);
    DevBuf nb;
    VMX_TRY(nb.reserve(std::max((size_t)need + 64, d.cap + d.cap / 2)));
    VMX_HIP(hipMemcpyAsync(nb.p, d.p, (size_t)R.base, hipMemcpyDeviceToDevice, R.c->stream));
    VMX_TRY(sync(R.c));
    d = std::move(nb);
    return 0;
}

int ref_long_line(const RefParse& R) {
    set_error("reference FASTA " + R.path + ": a header line (or a run of '\\r') does not fit in one window of " + std::to_string((long long)R.win) + " bytes");
    return VM_ERR_UNSUPPORTED;
}

// one window buf[0, avail): its kept bytes to mi->bases and mi->d_codes, its headers to mi->names and R.starts; *end_out: where it was cut
int ref_window(RefParse& R, const uint8_t* buf, int64_t avail, bool closing, int64_t* end_out) {
    vm_ctx* c = R.c; vm_index* mi = R.mi;
    *end_out = avail;
    if (avail == 0) return 0;
    double t0 = now_s();
    const int64_t nch = (avail + VMX_FQ_CHUNK - 1) / VMX_FQ_CHUNK, ntile = (nch + VMX_FQ_LTILE) / VMX_FQ_LTILE;
    VMX_TRY(R.d_map.reserve((size_t)nch + 1)); VMX_TRY(R.d_tile.reserve((size_t)ntile)); VMX_TRY(R.d_state.reserve((size_t)nch + 1));
    VMX_TRY(R.d_res.reserve(sizeof(vmx_fa_result))); VMX_TRY(R.pin.reserve(256));
    vmx_fa_result* res = R.d_res.as<vmx_fa_result>();
    VMX_HIP(hipMemsetAsync(res, 0, sizeof(vmx_fa_result), c->stream));
    const unsigned gch = (unsigned)((nch + 3) / 4);
    hipLaunchKernelGGL(k_fa_maps, dim3(gch), dim3(256), 0, c->stream, buf, avail, nch, R.ls0, R.d_map.as<uint8_t>(), res);
    hipLaunchKernelGGL(k_fa_tile_tot, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, R.d_map.as<const uint8_t>(), nch, R.d_tile.as<uint8_t>());
    hipLaunchKernelGGL(k_fq_tile_scan, dim3(1), dim3(1024), 0, c->stream, R.d_tile.as<uint8_t>(), ntile);
    hipLaunchKernelGGL(k_fa_states, dim3((unsigned)ntile), dim3(VMX_FQ_LTILE), 0, c->stream, R.d_map.as<const uint8_t>(), R.d_tile.as<const uint8_t>(), nch, R.seen << 1, R.d_state.as<uint8_t>());
    hipLaunchKernelGGL(k_fa_result, dim3(1), dim3(64), 0, c->stream, buf, avail, nch, R.d_state.as<const uint8_t>(), R.ls0, closing ? 1 : 0, res);
    VMX_HIP(hipMemcpyAsync(R.pin.p, res, sizeof(vmx_fa_result), hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    vmx_fa_result F; memcpy(&F, R.pin.p, sizeof F);
    if (F.end < 0 || F.end > avail) { set_error("reference FASTA: the cut pass left an offset outside the window"); return VM_ERR_HIP; }
    const int64_t end = F.end;
    *end_out = end;
    if (end == 0) { R.st[2] += now_s() - t0; return 0; }
    const int64_t ne = (end + VMX_FQ_CHUNK - 1) / VMX_FQ_CHUNK;
    const unsigned ge = (unsigned)((ne + 3) / 4);
    VMX_TRY(R.d_cnt.reserve((size_t)(ne + 1) * 8)); VMX_TRY(R.d_coff.reserve((size_t)(ne + 1) * 8));
    hipLaunchKernelGGL(k_fa_count, dim3(ge), dim3(256), 0, c->stream, buf, end, ne, R.d_state.as<const uint8_t>(), R.ls0, R.d_cnt.as<int64_t>());
    VMX_TRY(vmx_scan64(c, R.d_tmp, R.d_cnt.as<const int64_t>(), R.d_coff.as<int64_t>(), (size_t)ne + 1));
    VMX_HIP(hipMemcpyAsync(R.pin.p, R.d_coff.as<int64_t>() + ne, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    int64_t tot; memcpy(&tot, R.pin.p, 8);
    const int64_t kept = tot & 0xffffffffll, nh = tot >> 32;
    if (kept > end || nh > end) { set_error("reference FASTA: the count pass left a total larger than the window"); return VM_ERR_HIP; }
    if (R.base + kept >= (1LL << 35)) { set_error("reference longer than 2^35 bases"); return VM_ERR_UNSUPPORTED; }
    if ((int64_t)mi->names.size() + nh > (1 << 24)) { set_error("reference with more than 2^24 contigs"); return VM_ERR_UNSUPPORTED; }
    VMX_TRY(ref_codes_room(R, R.base + kept));
    VMX_TRY(R.d_wout.reserve((size_t)kept + 32)); VMX_TRY(R.d_hpos.reserve((size_t)(nh + 1) * 8)); VMX_TRY(R.d_hbase.reserve((size_t)(nh + 1) * 8));
    hipLaunchKernelGGL(k_fa_write, dim3(ge), dim3(256), 0, c->stream, buf, end, ne, R.d_state.as<const uint8_t>(), R.ls0, R.d_coff.as<const int64_t>(), R.base, R.d_wout.as<uint8_t>(),
                       mi->d_codes.as<uint8_t>(), R.d_hpos.as<int64_t>(), R.d_hbase.as<int64_t>(), R.d_other.as<unsigned long long>());
    std::vector<int64_t> hoff, hbase; std::vector<char> blob;
    if (nh > 0) {
        VMX_TRY(R.d_hsz.reserve((size_t)(nh + 1) * 8)); VMX_TRY(R.d_hoff.reserve((size_t)(nh + 1) * 8));
        hipLaunchKernelGGL(k_fa_hdr_size, dim3((unsigned)((nh + 1 + 3) / 4)), dim3(256), 0, c->stream, buf, end, R.d_hpos.as<const int64_t>(), nh, R.d_hsz.as<int64_t>());
        VMX_TRY(vmx_scan64(c, R.d_tmp, R.d_hsz.as<const int64_t>(), R.d_hoff.as<int64_t>(), (size_t)nh + 1));
        hoff.resize((size_t)nh + 1); hbase.resize((size_t)nh);
        VMX_TRY(download(hoff.data(), R.d_hoff.p, (size_t)nh + 1, c->stream));
        VMX_TRY(download(hbase.data(), R.d_hbase.p, (size_t)nh, c->stream));
        VMX_TRY(sync(c));
        const int64_t hb = hoff[(size_t)nh];
        if (hb < 0 || hb > end) { set_error("reference FASTA: the header pass left a size larger than the window"); return VM_ERR_HIP; }
        VMX_TRY(R.d_blob.reserve((size_t)hb + 32));
        hipLaunchKernelGGL(k_fa_hdr_copy, dim3((unsigned)((nh + 3) / 4)), dim3(256), 0, c->stream, buf, R.d_hpos.as<const int64_t>(), R.d_hoff.as<const int64_t>(), nh, R.d_blob.as<uint8_t>());
        blob.resize((size_t)hb + 1);
        VMX_TRY(download(blob.data(), R.d_blob.p, (size_t)hb, c->stream));
    }
    VMX_TRY(sync(c));
    R.st[2] += now_s() - t0;
    for (int64_t h = 0; h < nh; ++h) {
        if (hoff[(size_t)h + 1] - hoff[(size_t)h] + 1 >= R.win) return ref_long_line(R);    // (one rule, wherever the line falls in its window)
        mi->names.push_back(fasta_header_name(blob.data() + hoff[(size_t)h], (size_t)(hoff[(size_t)h + 1] - hoff[(size_t)h])));
        R.starts.push_back(hbase[(size_t)h]);
    }
    t0 = now_s();
    if (kept > 0) {
        if ((int64_t)mi->bases.size() < R.base + kept) mi->bases.resize((size_t)(R.base + kept));      // (compressed input: the string grows, geometrically past what was reserved)
        VMX_HIP(hipMemcpyAsync(&mi->bases[(size_t)R.base], R.d_wout.as<uint8_t>() + (R.base & 15), (size_t)kept, hipMemcpyDeviceToHost, c->stream));
        VMX_TRY(sync(c));
    }
    R.st[3] += now_s() - t0;
    R.base += kept; R.seen |= nh > 0; R.ls0 = F.end_ls;
    return 0;
}

int ref_fasta_device_impl(vm_ctx* c, const char* path, vm_index* mi, double* st, int flags) {
    RefParse R; R.c = c; R.mi = mi; R.st = st;
    VMX_TRY(R.d_other.reserve(8)); VMX_HIP(hipMemsetAsync(R.d_other.p, 0, 8, c->stream));
    BgzfIn in;
    struct CloseIn { BgzfIn* r; ~CloseIn() { bgzf_in_close(r); } } close_in{&in};
    in.c = c;
    unsigned char mg[18]; ssize_t ng;
    {
        const int fd = open(path, O_RDONLY);
        if (fd < 0) { set_error(std::string("cannot open ") + path); return VM_ERR_IO; }
        ng = pread(fd, mg, 18, 0);
        close(fd);
    }
    const bool gz = ng >= 2 && mg[0] == 0x1f && mg[1] == 0x8b;
    const bool bgzf = gz && ng >= 18 && mg[2] == 8 && mg[3] == 4 && mg[12] == 'B' && mg[13] == 'C';
    // VM_READER_GZIP_DEVICE: plain gzip through GzipIn (inflated on the device in parallel chunks) in BgzfIn's place, window for window
    struct FreeGz { GzipIn* g; ~FreeGz() { gzip_in_free(g); } } gzdev{gz && !bgzf && (flags & VM_READER_GZIP_DEVICE) ? gzip_in_new() : nullptr};
    const bool dev_in = bgzf || gzdev.g;
    int64_t win = (int64_t)256 << 20;
    RefRaw raw;
    if (dev_in) { VMX_TRY(bgzf_in_open(&in, c, path)); win = in.max_inf; mi->bases.reserve((size_t)std::min<int64_t>(in.fsize * 5, (1LL << 35) - 1)); }
    else {
        // VMX_REF_IN_WINDOW: text bytes per window of plain and plain-gzip input (tests cross many windows with small files)
        if (const char* e = getenv("VMX_REF_IN_WINDOW")) win = std::min<int64_t>(std::max<int64_t>(atoll(e), 1 << 16), (int64_t)1 << 30);
        raw.fd = open(path, O_RDONLY);
        if (raw.fd < 0) { set_error(std::string("cannot open ") + path); return VM_ERR_IO; }
        const int64_t fsize = (int64_t)lseek(raw.fd, 0, SEEK_END);
        if (fsize < 0 || lseek(raw.fd, 0, SEEK_SET) != 0) { set_error(std::string("cannot seek in ") + path); return VM_ERR_IO; }
        if (gz) {
            mi->bases.reserve((size_t)std::min<int64_t>(fsize * 5, (1LL << 35) - 1));     // (address space for the usual 4 : 1 of DNA text: the string then grows in place)
            raw.gz = gzdopen(raw.fd, "rb");
            if (!raw.gz) { set_error(std::string("cannot open the gzip stream of ") + path); return VM_ERR_IO; }
            gzbuffer(raw.gz, 1 << 20);
        } else {
            // the file size bounds the bases of a plain file: too long a reference is refused, and the codes and the host copy are sized, before the first window
            win = std::min<int64_t>(win, std::max<int64_t>(fsize, 1 << 16));
            const int64_t bound = std::min<int64_t>(fsize, (1LL << 35) - 1);
            VMX_TRY(ref_codes_room(R, bound));
            mi->bases.resize((size_t)bound);
        }
        VMX_TRY(raw.stage[0].reserve((size_t)win)); VMX_TRY(raw.stage[1].reserve((size_t)win));
        raw.win = win;
        VMX_TRY(in.pin.reserve(256));
    }
    R.win = win; R.path = path;
    for (bool closing = false; !closing;) {
        int64_t avail = 0;
        if (dev_in) {
            double bst[13] = {0};
            const int irc = gzdev.g ? gzip_in_window(&in, gzdev.g, bst, &avail) : bgzf_in_window(&in, bst, &avail);
            st[0] += bst[0]; st[1] += bst[2]; st[5] += bst[9];
            if (irc < 0) return irc;
            closing = in.file_done;
            if (irc == 0) {                                                  // (the file ended behind a window that was not its last: what was carried closes it)
                DevBuf& dst = in.d_inf[in.which ^ 1];
                VMX_TRY(dst.reserve((size_t)in.carry + 64));
                if (in.carry) VMX_HIP(hipMemcpyAsync(dst.p, in.d_inf[in.which].as<uint8_t>() + in.tail_off, (size_t)in.carry, hipMemcpyDeviceToDevice, c->stream));
                in.which ^= 1; avail = in.carry; closing = true;
            }
        } else {
            double t0;
            if (raw.pre_on) { raw.pre.get(); raw.pre_on = false; } else ref_raw_fill(&raw, raw.slot);
            const int k = raw.slot;
            st[gz ? 1 : 0] += raw.busy[k];                                   // (zlib's time holds the file read of a gzip stream)
            if (raw.rc[k] < 0) { set_error(raw.err[k] + " in " + path); return raw.rc[k]; }
            closing = raw.eof[k];
            if (!closing) { raw.pre_on = true; raw.pre = std::async(std::launch::async, ref_raw_fill, &raw, k ^ 1); }
            raw.slot ^= 1;
            t0 = now_s();
            DevBuf& dst = in.d_inf[in.which ^ 1];
            avail = in.carry + raw.got[k];
            VMX_TRY(dst.reserve((size_t)avail + 64));
            if (in.carry) VMX_HIP(hipMemcpyAsync(dst.p, in.d_inf[in.which].as<uint8_t>() + in.tail_off, (size_t)in.carry, hipMemcpyDeviceToDevice, c->stream));
            if (raw.got[k]) VMX_HIP(hipMemcpyAsync(dst.as<uint8_t>() + in.carry, raw.stage[k].p, (size_t)raw.got[k], hipMemcpyHostToDevice, c->stream));
            VMX_TRY(sync(c));
            in.which ^= 1;
            st[0] += now_s() - t0;                                           // (the upload counts as reading the file)
            st[5] += (double)raw.got[k];
        }
        st[6] += 1;
        int64_t end = avail;
        VMX_TRY(ref_window(R, in.d_inf[in.which].as<const uint8_t>(), avail, closing, &end));
        in.tail_off = end; in.carry = avail - end;
        if (!closing && in.carry >= win) return ref_long_line(R);
    }
    mi->bases.resize((size_t)R.base);
    const size_t n = mi->names.size();
    for (size_t i = 0; i < n; ++i) { mi->offsets.push_back(R.starts[i]); mi->lens.push_back((i + 1 < n ? R.starts[i + 1] : R.base) - R.starts[i]); }
    mi->offsets.push_back(R.base);
    VMX_TRY(ref_codes_room(R, R.base));
    unsigned long long n_other = 0;
    VMX_HIP(hipMemcpyAsync(&n_other, R.d_other.p, 8, hipMemcpyDeviceToHost, c->stream));
    VMX_TRY(sync(c));
    mi->n_other_letters = (int64_t)n_other;
    st[7] = (double)n;
    return 0;
}

}  // namespace

// path -> mi->names, lens, offsets, bases, d_codes (without the tail padding) and n_other_letters, parsed on the device. st[0 .. 8): seconds of file
// read, inflate, parse kernels, download of the bases, (index build: the caller's), then text bytes, windows, contigs.
int vmx_ref_fasta_device(vm_ctx* c, const char* path, vm_index* mi, double* st, int flags) {
    try { return ref_fasta_device_impl(c, path, mi, st, flags); }
    catch (const std::bad_alloc&) { set_error("reference FASTA: out of host memory"); return VM_ERR_OOM; }
}
