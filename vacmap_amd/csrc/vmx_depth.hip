// vmx_depth.hip — host side of the depth-of-coverage accumulator (vmx_depth.h; the rule: vacmapx.h at vm_depth_add): create / free, merge, the host
// copies of the counts and the two texts. A host accumulator's text is made here (depth_text); a device accumulator's by k_depth_sums and
// k_depth_lines (k_depth.hip), byte for byte the same. The adds: vm_depth_add in vmx_sam.hip, the device ones in vmx_sam_dev.hip.
#include "vmx_depth.h"
#include "vmx_index_priv.h"

using namespace vmx;

namespace {

int wait(vm_ctx* c) {
    const hipError_t e = vmx_stream_sync(c);
    if (e != hipSuccess) return hip_fail(e, "stream wait", __FILE__, __LINE__);
    return 0;
}
int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, what, __FILE__, __LINE__);
    return 0;
}

void put_u(std::string& s, unsigned long long u) { char b[24]; int n = 0; do { b[n++] = (char)('0' + u % 10); u /= 10; } while (u); while (n) s.push_back(b[--n]); }
void put_mean(std::string& s, unsigned long long count, unsigned long long len) {
    const unsigned long long h = vmx_depth_hundredths(count, len);
    put_u(s, h / 100); s.push_back('.'); s.push_back((char)('0' + (h % 100) / 10)); s.push_back((char)('0' + h % 10));
}

// the text of the rule from host counts
std::string depth_text(const vm_depth* d, const int64_t* counts, int which) {
    std::string s;
    const size_t nseq = d->lens.size();
    if (which == VM_DEPTH_REGIONS) {
        for (size_t c = 0; c < nseq; ++c)
            for (int64_t w = d->win_off[c]; w < d->win_off[c + 1]; ++w) {
                const int64_t start = (w - d->win_off[c]) * d->window, end = std::min(start + d->window, d->lens[c]);
                s += d->names[c]; s.push_back('\t'); put_u(s, (unsigned long long)start); s.push_back('\t'); put_u(s, (unsigned long long)end); s.push_back('\t');
                put_mean(s, (unsigned long long)counts[w], (unsigned long long)(end - start)); s.push_back('\n');
            }
        return s;
    }
    unsigned long long all = 0, all_len = 0;
    for (size_t c = 0; c <= nseq; ++c) {
        unsigned long long sum = 0;
        if (c < nseq) { for (int64_t w = d->win_off[c]; w < d->win_off[c + 1]; ++w) sum += (unsigned long long)counts[w]; all += sum; all_len += (unsigned long long)d->lens[c]; }
        const unsigned long long len = c < nseq ? (unsigned long long)d->lens[c] : all_len, v = c < nseq ? sum : all;
        s += c < nseq ? d->names[c] : std::string("total"); s.push_back('\t'); put_u(s, len); s.push_back('\t'); put_u(s, v); s.push_back('\t'); put_mean(s, v, len); s.push_back('\n');
    }
    return s;
}

// a host copy of the counts of any accumulator (a device one: one wait on its context)
int host_counts(vm_depth* d, std::vector<int64_t>& out) {
    if (!d->ctx) { out = d->h_counts; return 0; }
    out.assign((size_t)d->n_win, 0);
    VMX_HIP(hipSetDevice(d->ctx->device));
    vmx_fetch_scope fs(d->ctx);
    VMX_TRY(vmx_fetch(d->ctx, out.data(), d->d_counts.p, (size_t)d->n_win));
    return wait(d->ctx);
}

int device_text(vm_depth* d, int which, char** text, int64_t* n) {
    vm_ctx* c = d->ctx;
    VMX_HIP(hipSetDevice(c->device));
    vmx_fetch_scope fs(c);
    hipStream_t st = c->stream;
    const int32_t nseq = (int32_t)d->lens.size();
    const int64_t items = which == VM_DEPTH_REGIONS ? d->n_win : (int64_t)nseq + 1;
    int64_t total_len = 0; for (int64_t l : d->lens) total_len += l;
    VMX_TRY(d->d_sums.reserve(8 * ((size_t)nseq + 1))); VMX_TRY(d->d_lsz.reserve(8 * ((size_t)items + 1))); VMX_TRY(d->d_loff.reserve(8 * ((size_t)items + 1)));
    VMX_TRY(d->d_text.reserve(16));
    const unsigned long long* counts = d->d_counts.as<const unsigned long long>();
    unsigned long long* sums = d->d_sums.as<unsigned long long>();
    VMX_HIP(hipMemsetAsync(sums, 0, 8 * ((size_t)nseq + 1), st)); VMX_HIP(hipMemsetAsync(d->d_lsz.p, 0, 8 * ((size_t)items + 1), st));
    if (which == VM_DEPTH_SUMMARY && nseq) hipLaunchKernelGGL(k_depth_sums, dim3((unsigned)nseq, 32), dim3(64), 0, st, counts, d->d_win_off.as<const int64_t>(), nseq, sums);
    const unsigned grid = (unsigned)((items + 255) / 256);
    auto lines = [&](int write) {
        if (items) hipLaunchKernelGGL(k_depth_lines, dim3(grid), dim3(256), 0, st, counts, d->d_win_off.as<const int64_t>(), d->d_lens.as<const int64_t>(), d->d_cnames.as<const char>(),
                                      d->d_cname_off.as<const int64_t>(), nseq, d->window, (const unsigned long long*)sums, which, total_len, items, d->d_lsz.as<int64_t>(),
                                      d->d_loff.as<const int64_t>(), d->d_text.as<char>(), write);
    };
    lines(0);
    VMX_TRY(launched("k_depth_lines (sizes)"));
    VMX_TRY(vmx_scan64(c, d->d_tmp, d->d_lsz.as<const int64_t>(), d->d_loff.as<int64_t>(), (size_t)items + 1));
    int64_t h_tot = 0;
    VMX_TRY(vmx_fetch(c, &h_tot, d->d_loff.as<int64_t>() + items, 1));
    VMX_TRY(wait(c));
    VMX_TRY(d->d_text.reserve((size_t)h_tot + 16));
    lines(1);
    VMX_TRY(launched("k_depth_lines"));
    char* h = (char*)malloc((size_t)h_tot + 1);
    if (!h) { set_error("out of host memory"); return VM_ERR_OOM; }
    int rc = vmx_fetch(c, h, d->d_text.p, (size_t)h_tot);
    if (rc >= 0) rc = wait(c);
    if (rc < 0) { free(h); return rc; }
    h[h_tot] = 0;
    *text = h; *n = h_tot;
    return VM_OK;
}

}  // namespace

extern "C" {

int vm_depth_create(vm_ctx* c, const vm_index* mi, int64_t window, int min_mapq, vm_depth** out) {
    if (out) *out = nullptr;
    if (!mi || !out) { set_error("vm_depth_create: bad arguments"); return VM_ERR_ARG; }
    if (window < 1) { set_error("vm_depth_create: the window must be at least 1"); return VM_ERR_ARG; }
    if (min_mapq < 0 || min_mapq > 255) { set_error("vm_depth_create: the MAPQ threshold must lie in 0 .. 255"); return VM_ERR_ARG; }
    const size_t nseq = mi->names.size();
    std::vector<int64_t> win_off(nseq + 1, 0);
    for (size_t i = 0; i < nseq; ++i) {
        const int64_t L = mi->lens[i] > 0 ? mi->lens[i] : 0;
        win_off[i + 1] = win_off[i] + (L / window + (L % window ? 1 : 0));
        if (win_off[i + 1] > ((int64_t)1 << 28)) { set_error("vm_depth_create: more than 2^28 windows; choose a larger window"); return VM_ERR_ARG; }
    }
    vm_depth* d = nullptr;
    try {
        d = new vm_depth();
        d->ctx = c; d->index_serial = mi->serial; d->window = window; d->min_mapq = min_mapq;
        d->names = mi->names; d->lens = mi->lens; d->win_off = win_off; d->n_win = win_off[nseq];
        if (!c) d->h_counts.assign((size_t)d->n_win, 0);
    } catch (const std::bad_alloc&) { delete d; set_error("vm_depth_create: out of host memory"); return VM_ERR_OOM; }
    if (c) {
        auto make = [&]() -> int {
            VMX_HIP(hipSetDevice(c->device));
            std::string cn; std::vector<int64_t> co(1, 0);
            for (const std::string& s : d->names) { cn += s; co.push_back((int64_t)cn.size()); }
            VMX_TRY(d->d_counts.reserve(8 * (size_t)(d->n_win + 1)));
            VMX_HIP(hipMemsetAsync(d->d_counts.p, 0, 8 * (size_t)(d->n_win + 1), c->stream));
            VMX_TRY(upload(d->d_win_off, d->win_off.data(), d->win_off.size(), c->stream));
            VMX_TRY(upload(d->d_lens, d->lens.data(), d->lens.size(), c->stream));
            VMX_TRY(upload(d->d_cnames, cn.data(), cn.size(), c->stream));
            VMX_TRY(upload(d->d_cname_off, co.data(), co.size(), c->stream));
            return wait(c);                                              // (the host sources die here)
        };
        const int rc = make();
        if (rc < 0) { delete d; return rc; }
    }
    *out = d;
    return VM_OK;
}

void vm_depth_free(vm_depth* d) {
    if (!d) return;
    if (d->ctx) {
        if (d->ctx->depth == d) d->ctx->depth = nullptr;
        (void)hipSetDevice(d->ctx->device);
        if (d->ctx->stream) (void)hipStreamSynchronize(d->ctx->stream);   // (a queued k_depth_add still adds to the table)
    }
    delete d;
}

// dst += counts[n_win] (host memory)
static int add_counts(vm_depth* dst, const int64_t* h) {
    if (!dst->ctx) {                                                     // (atomic: a vm_depth_add on dst may be running in another thread)
        for (int64_t i = 0; i < dst->n_win; ++i) if (h[i]) __atomic_fetch_add(&dst->h_counts[(size_t)i], h[i], __ATOMIC_RELAXED);
        return VM_OK;
    }
    vm_ctx* c = dst->ctx;
    VMX_HIP(hipSetDevice(c->device));
    VMX_TRY(upload(dst->d_tmp, h, (size_t)dst->n_win, c->stream));
    if (dst->n_win) hipLaunchKernelGGL(k_depth_merge, dim3(grid1d(dst->n_win, 4096)), dim3(256), 0, c->stream, dst->d_counts.as<unsigned long long>(),
                                       dst->d_tmp.as<const unsigned long long>(), dst->n_win);
    VMX_TRY(launched("k_depth_merge"));
    return wait(c);                                                      // (the host source may die here)
}

int vm_depth_merge(vm_depth* dst, vm_depth* src) {
    if (!dst || !src) { set_error("vm_depth_merge: bad arguments"); return VM_ERR_ARG; }
    if (dst->window != src->window || dst->lens != src->lens) { set_error("vm_depth_merge: the accumulators differ in their contig lengths or their window"); return VM_ERR_ARG; }
    if (dst == src) { set_error("vm_depth_merge: dst and src are the same accumulator"); return VM_ERR_ARG; }
    std::vector<int64_t> h;
    try { VMX_TRY(host_counts(src, h)); } catch (const std::bad_alloc&) { set_error("vm_depth_merge: out of host memory"); return VM_ERR_OOM; }
    return add_counts(dst, h.data());
}

int vm_depth_add_counts(vm_depth* dst, const int64_t* counts, int64_t n_windows) {
    if (!dst || (n_windows && !counts) || n_windows != dst->n_win) { set_error("vm_depth_add_counts: the table does not have the accumulator's number of windows"); return VM_ERR_ARG; }
    return add_counts(dst, counts);
}

int vm_depth_counts(vm_depth* d, int64_t** counts, int64_t** win_off, int64_t* n_windows) {
    if (counts) *counts = nullptr;
    if (win_off) *win_off = nullptr;
    if (!d || !counts || !win_off || !n_windows) { set_error("vm_depth_counts: bad arguments"); return VM_ERR_ARG; }
    std::vector<int64_t> h;
    try { VMX_TRY(host_counts(d, h)); } catch (const std::bad_alloc&) { set_error("vm_depth_counts: out of host memory"); return VM_ERR_OOM; }
    int64_t* a = (int64_t*)malloc(8 * (h.size() + 1)); int64_t* b = (int64_t*)malloc(8 * d->win_off.size());
    if (!a || !b) { free(a); free(b); set_error("out of host memory"); return VM_ERR_OOM; }
    if (!h.empty()) memcpy(a, h.data(), 8 * h.size());
    memcpy(b, d->win_off.data(), 8 * d->win_off.size());
    *counts = a; *win_off = b; *n_windows = d->n_win;
    return VM_OK;
}

int vm_depth_text(vm_depth* d, int which, char** text, int64_t* n) {
    if (text) *text = nullptr;
    if (n) *n = 0;
    if (!d || !text || !n || (which != VM_DEPTH_REGIONS && which != VM_DEPTH_SUMMARY)) { set_error("vm_depth_text: bad arguments"); return VM_ERR_ARG; }
    if (d->ctx) return device_text(d, which, text, n);
    try {
        const std::string s = depth_text(d, d->h_counts.data(), which);
        char* h = (char*)malloc(s.size() + 1);
        if (!h) { set_error("out of host memory"); return VM_ERR_OOM; }
        memcpy(h, s.data(), s.size()); h[s.size()] = 0;
        *text = h; *n = (int64_t)s.size();
        return VM_OK;
    } catch (const std::bad_alloc&) { set_error("vm_depth_text: out of host memory"); return VM_ERR_OOM; }
}

}  // extern "C"
