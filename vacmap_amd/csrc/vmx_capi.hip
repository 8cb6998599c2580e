// vmx_capi.hip — C-ABI entry points of libvacmapx.so (include/vacmapx.h): context, tables, DP and chain stage entries.
// Everything that computes runs the HIP kernels of this directory on the context's stream; there is no CPU path.
#include "vmx_host.h"
#include <time.h>
#include "vmx_select.h"
#include "vmx_stage.h"
#include "vmx_sam_dev.h"
#include "vmx_round.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>

namespace vmx {
static thread_local std::string g_err;
void set_error(const std::string& s) { g_err = s; }
int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    g_err = std::string("HIP error: ") + hipGetErrorString(e) + " at " + what + " (" + file + ":" + std::to_string(line) + ")";
    return e == hipErrorOutOfMemory ? VM_ERR_OOM : VM_ERR_HIP;
}
}  // namespace vmx
using namespace vmx;


static inline int grid_for(const vm_ctx* c, int64_t n_items, int per_cu = 8) {
    int64_t g = std::min<int64_t>(n_items, (int64_t)c->num_cu * per_cu);
    return (int)std::max<int64_t>(g, 1);
}
template <class T> static T* host_alloc(size_t n) { return (T*)malloc(sizeof(T) * (n ? n : 1)); }

extern "C" {

const char* vm_last_error(void) { return g_err.c_str(); }
const char* vm_version(void) { return "vacmapx 0.1 (gfx950)"; }
void vm_free(void* p) { free(p); }

void vm_params_default(vm_params* p, int mode) {
    memset(p, 0, sizeof(*p));
    p->mode = mode; p->check_num = 100; p->mid_occ = -1;
    p->global_maxdiff = 50; p->local_maxdiff = 30; p->local_kmersize = 9;
    if (mode == VM_MODE_L) { p->local_skipcost = 59.; p->global_skipcost = 40.; p->maxdivergence = 0.1; }
    else if (mode == VM_MODE_H) { p->local_skipcost = 40.; p->global_skipcost = 40.; p->maxdivergence = 0.2; }
    else { p->local_skipcost = 30.; p->global_skipcost = 30.; p->maxdivergence = 0.5; }
    p->nodiscard = !(mode == VM_MODE_L || mode == VM_MODE_H);
    // -mode asm: --eqx forced (src/vacmap/vacmap:246), maxdivergence forced to 1 by the worker (mammap_asm.py:23483), check_num = -1 (:23206)
    if (mode == VM_MODE_ASM) { p->eqx = 1; p->maxdivergence = 1.0; p->check_num = -1; }
}

}  // extern "C"
// ---- the mailbox (vmx_host.h)
__global__ void k_signal(unsigned long long* word, unsigned long long v) {
#ifdef VMX_EMU
    *word = v;
#else
    __hip_atomic_store(word, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
}
// every piece is cut into 16 KB slices dealt round-robin to the workgroups; the last workgroup to finish publishes the sequence word (system scope: the host polls it)
__global__ void __launch_bounds__(256) k_export(vmx_export_args A) {
    __shared__ int s_last;
    const unsigned G = gridDim.x, b = blockIdx.x;
    unsigned long long slice0 = 0;
    for (int p = 0; p < A.n; ++p) {
        const unsigned long long nb = A.bytes[p], ns = (nb + 16383ULL) >> 14;
        for (unsigned long long sl = (b + G - (unsigned)(slice0 % G)) % G; sl < ns; sl += G) {
            const unsigned long long lo = sl << 14, hi = lo + 16384ULL < nb ? lo + 16384ULL : nb;
            const char* s = A.src[p] + lo; char* d = A.dst[p] + lo;
            const unsigned long long n = hi - lo;
            if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0) {
                const unsigned long long nv = n >> 4;
                struct b16 { unsigned long long x, y; };
                for (unsigned long long i = threadIdx.x; i < nv; i += blockDim.x) ((b16*)d)[i] = ((const b16*)s)[i];
                for (unsigned long long i = (nv << 4) + threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
            } else for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
        }
        slice0 += ns;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#ifdef VMX_EMU
        const unsigned long long old = __atomic_fetch_add(A.done, 1ULL, __ATOMIC_ACQ_REL);
#else
        __threadfence_system();
        const unsigned long long old = __hip_atomic_fetch_add(A.done, 1ULL, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
#endif
        s_last = old + 1ULL == (unsigned long long)G;
        if (s_last) {
#ifdef VMX_EMU
            *A.done = 0ULL; *A.word = A.seq;
#else
            __hip_atomic_store(A.done, 0ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(A.word, A.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
#endif
        }
    }
}
// the pieces of an upload group out of the ring (device-mapped host memory) into their places, 16 KB slices dealt round-robin to the workgroups
__global__ void __launch_bounds__(256) k_import(vmx_import_args A) {
    const unsigned G = gridDim.x, b = blockIdx.x;
    unsigned long long slice0 = 0;
    for (int p = 0; p < A.n; ++p) {
        const unsigned long long nb = A.bytes[p], ns = (nb + 16383ULL) >> 14;
        for (unsigned long long sl = (b + G - (unsigned)(slice0 % G)) % G; sl < ns; sl += G) {
            const unsigned long long lo = sl << 14, hi = lo + 16384ULL < nb ? lo + 16384ULL : nb, n = hi - lo;
            const char* s = A.src[p] + lo; char* d = A.dst[p] + lo;
            if ((((uintptr_t)s | (uintptr_t)d) & 7) == 0) {
                const unsigned long long nv = n >> 3;
                for (unsigned long long i = threadIdx.x; i < nv; i += blockDim.x) ((unsigned long long*)d)[i] = ((const unsigned long long*)s)[i];
                for (unsigned long long i = (nv << 3) + threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
            } else for (unsigned long long i = threadIdx.x; i < n; i += blockDim.x) d[i] = s[i];
        }
        slice0 += ns;
    }
}
static int mailbox_create(vm_ctx* c) {
    vmx_mailbox& m = c->mb;
    const char* mode = getenv("VMX_WAIT_MODE");
    if (mode && !strcmp(mode, "spin")) { m.on = false; return 0; }
    if (const char* e = getenv("VMX_POLL_US")) { const long long v = atoll(e); if (v >= 1 && v <= 100000) m.poll_ns = v * 1000; }
    const size_t up = (size_t)8 << 20, dn = (size_t)8 << 20, tot = 4096 + up + dn;
    void* hp = nullptr;
    if (hipHostMalloc(&hp, tot, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); m.on = false; return 0; }       // no page-locked memory: the legacy waits
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(hp); m.on = false; return 0; }
    memset(hp, 0, 4096);
    m.h = (char*)hp; m.d = (char*)dp; m.up_off = 4096; m.up_cap = up; m.dn_off = 4096 + up; m.dn_cap = dn; m.on = true;
    void* dc = nullptr;
    if (hipMalloc(&dc, 64) == hipSuccess) { (void)hipMemset(dc, 0, 64); m.done_ctr = (unsigned long long*)dc; } else (void)hipGetLastError();      // (without it: copies + k_signal)
    return 0;
}
static void mailbox_destroy(vm_ctx* c) {
    vmx_mailbox& m = c->mb;
    if (m.h) (void)hipHostFree(m.h);
    if (m.big) (void)hipHostFree(m.big);
    if (m.done_ctr) (void)hipFree(m.done_ctr);
    m = vmx_mailbox();
}
#ifdef VMX_CF_TICKS
extern "C" void vmx_cf_ticks_dump();
#endif
// The one way a context ends (vm_ctx_destroy, and vm_ctx_create when it fails half way: what was not created yet is null), in this order: the stream is drained,
// every buffer of the context goes back, the parked allocations follow, and only then the events, the streams and the mailbox go.
static void ctx_teardown(vm_ctx* c) {
    if (c->stream) (void)hipStreamSynchronize(c->stream);
#ifdef VMX_CF_TICKS
    vmx_cf_ticks_dump();
#endif
    delete c->xbufs; delete c->lbufs; delete c->bbufs; delete c->sbufs;
    c->tab_buf.release();
    vmx::devbuf_retired().flush();
    for (hipEvent_t e : c->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->gev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->kev) if (e) (void)hipEventDestroy(e);
    for (int i = 0; i < 4; ++i) { if (c->aux[i]) { (void)hipStreamSynchronize(c->aux[i]); (void)hipStreamDestroy(c->aux[i]); } if (c->join_ev[i]) (void)hipEventDestroy(c->join_ev[i]); }
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->low) { (void)hipStreamSynchronize(c->low); (void)hipStreamDestroy(c->low); (void)hipEventDestroy(c->low_ev[0]); (void)hipEventDestroy(c->low_ev[1]); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    mailbox_destroy(c);
    delete c;
}
int vmx_mailbox_wait(vm_ctx* c) {
    vmx_mailbox& m = c->mb;
    const unsigned long long want = ++m.seq;
    {   // the noted downloads: one kernel per VMX_EXPORT_MAX pieces, the last of them carries the sequence word (no piece: the bare signal)
        vmx_export_args E; memset(&E, 0, sizeof E);
        unsigned long long tot = 0; bool signalled = false;
        auto flush = [&](bool last) {
            if (!E.n && !last) return;
            if (!E.n) { hipLaunchKernelGGL(k_signal, dim3(1), dim3(1), 0, c->stream, (unsigned long long*)m.d, want); signalled = true; return; }
            // the word of a kernel that is not the last one of this wait is a scratch word of the mailbox (offset 64): only the last launch moves the real one
            E.word = (unsigned long long*)(m.d + (last ? 0 : 64)); E.seq = want; E.done = m.done_ctr;
            const unsigned G = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>((tot + 16383ULL) >> 14, 64ULL));
            hipLaunchKernelGGL(k_export, dim3(G), dim3(256), 0, c->stream, E);
            if (last) signalled = true;
            memset(&E, 0, sizeof E); tot = 0;
        };
        size_t left = 0; for (const vmx_mailbox::Pending& p : m.pend) left += p.dev ? 1 : 0;
        for (const vmx_mailbox::Pending& p : m.pend) {
            if (!p.dev) continue;
            const char* land_d = (p.src >= m.h && p.src < m.h + m.dn_off + m.dn_cap) ? m.d + (p.src - m.h) : m.big_d + (p.src - m.big);
            E.src[E.n] = (const char*)p.dev; E.dst[E.n] = (char*)land_d; E.bytes[E.n] = p.bytes; ++E.n; tot += p.bytes; --left;
            if (E.n == VMX_EXPORT_MAX) flush(left == 0);
        }
        if (!signalled) flush(true);
    }
    volatile unsigned long long* w = (volatile unsigned long long*)m.h;
    struct timespec ts; ts.tv_sec = 0; ts.tv_nsec = (long)m.poll_ns;
    long long slept = 0, next_query = 500000000LL;
    while (__atomic_load_n(w, __ATOMIC_ACQUIRE) < want) {
        nanosleep(&ts, nullptr);
        slept += m.poll_ns;
        if (slept >= next_query) {                                    // a stream that died (a faulting kernel) never delivers the word
            next_query += 500000000LL;
            const hipError_t q = hipStreamQuery(c->stream);
            if (q != hipSuccess && q != hipErrorNotReady) { m.pend.clear(); m.dn_used = 0; m.big_used = 0; m.up_used = 0; return vmx::hip_fail(q, "hipStreamQuery (mailbox wait)", __FILE__, __LINE__); }
        }
    }
    for (const vmx_mailbox::Pending& p : m.pend) memcpy(p.dst, p.src, p.bytes);
    m.pend.clear(); m.dn_used = 0; m.big_used = 0; m.up_used = 0;
    return 0;
}
int vmx_fetch_bytes(vm_ctx* c, void* host, const void* dev, size_t bytes) {
    vmx_mailbox& m = c->mb;
    char* land = nullptr;
    const size_t at = (m.dn_used + 63) & ~(size_t)63;
    if (at + bytes <= m.dn_cap) { land = m.h + m.dn_off + at; m.dn_used = at + bytes; }
    else {
        const size_t bat = (m.big_used + 63) & ~(size_t)63;
        if (bat + bytes > m.big_cap && m.big_used == 0) {             // grow the landing block while nothing is on its way into it
            if (m.big) { (void)hipHostFree(m.big); m.big = nullptr; m.big_cap = 0; m.big_d = nullptr; }
            const size_t want = bytes + bytes / 2 + ((size_t)4 << 20);
            void* hp = nullptr; void* dp = nullptr;
            if (hipHostMalloc(&hp, want, hipHostMallocMapped) == hipSuccess) {
                if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) { m.big = (char*)hp; m.big_d = (char*)dp; m.big_cap = want; }
                else { (void)hipGetLastError(); (void)hipHostFree(hp); }
            } else (void)hipGetLastError();
        }
        if (bat + bytes <= m.big_cap) { land = m.big + bat; m.big_used = bat + bytes; }
    }
    if (!land) {                                                      // no page-locked room: the plain copy (waits inside the call)
        VMX_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
        return 0;
    }
    static const bool by_copy = getenv("VMX_FETCH_COPIES") != nullptr;      // A/B knob: a runtime copy per piece + k_signal (the first form of the mailbox)
    if (by_copy || !m.done_ctr) { VMX_HIP(hipMemcpyAsync(land, dev, bytes, hipMemcpyDeviceToHost, c->stream)); m.pend.push_back(vmx_mailbox::Pending{host, land, bytes, nullptr}); }
    else m.pend.push_back(vmx_mailbox::Pending{host, land, bytes, dev});
    return 0;
}
// ---- counters of the row chain kernels (vmx_host.h)
static unsigned long long* g_chain_dbg = nullptr;
static std::mutex g_chain_dbg_m;
static int chain_dbg_enable() {
    std::lock_guard<std::mutex> g(g_chain_dbg_m);
    if (g_chain_dbg) return 0;
    unsigned long long* q = nullptr;
    if (hipMalloc((void**)&q, 64) != hipSuccess) { (void)hipGetLastError(); return -1; }
    (void)hipMemset(q, 0, 64);
    g_chain_dbg = q;
    return 0;
}
unsigned long long* vmx_chain_dbg() {
    static const bool env = [] { if (getenv("VMX_DBG_CHAIN")) (void)chain_dbg_enable(); return true; }(); (void)env;
    return g_chain_dbg;
}
void vmx_chain_dbg_report(hipStream_t st) {
    static const bool print = getenv("VMX_DBG_CHAIN") != nullptr;
    unsigned long long* p = vmx_chain_dbg(); if (!p || !print) return;
    unsigned long long h[8]; (void)hipStreamSynchronize(st); (void)hipMemcpy(h, p, 64, hipMemcpyDeviceToHost);
    fprintf(stderr, "[chain rows] global: anchors %llu scans past the window %llu insertions through HBM %llu opcount %llu | local: %llu %llu %llu %llu\n", h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7]);
}
extern "C" {
int vm_debug_chain_counters(int enable, unsigned long long* out8) {
    if (enable > 0 && chain_dbg_enable() < 0) { vmx::set_error("vm_debug_chain_counters: no device memory"); return VM_ERR_OOM; }
    unsigned long long* p = g_chain_dbg;
    if (out8) { memset(out8, 0, 64); if (p) { VMX_HIP(hipDeviceSynchronize()); VMX_HIP(hipMemcpy(out8, p, 64, hipMemcpyDeviceToHost)); } }
    if (enable < 0 && p) { VMX_HIP(hipDeviceSynchronize()); VMX_HIP(hipMemset(p, 0, 64)); }           // -1: read and reset
    return VM_OK;
}

int vm_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int vm_ctx_create(int device_id, vm_ctx** out) {
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device: libvacmapx has no CPU fallback"); return VM_ERR_NO_DEVICE; }
    if (device_id < 0 || device_id >= n) { set_error("bad device id"); return VM_ERR_ARG; }
    VMX_HIP(hipSetDevice(device_id));
    vm_ctx* c = new vm_ctx();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0) c->num_cu = prop.multiProcessorCount;
    int prio_least = 0, prio_greatest = 0;
    const bool prio = vmx_stream_prio_on() && hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) == hipSuccess && prio_least != prio_greatest;
    if ((prio ? hipStreamCreateWithPriority(&c->stream, hipStreamDefault, prio_greatest) : hipStreamCreate(&c->stream)) != hipSuccess) { ctx_teardown(c); set_error("hipStreamCreate failed"); return VM_ERR_HIP; }
    if (prio && hipStreamCreateWithPriority(&c->low, hipStreamDefault, prio_least) == hipSuccess) { (void)hipEventCreateWithFlags(&c->low_ev[0], hipEventDisableTiming); (void)hipEventCreateWithFlags(&c->low_ev[1], hipEventDisableTiming); }
    else c->low = nullptr;
    for (int i = 0; i < 24; ++i) (void)hipEventCreate(&c->ev[i]);
    for (int i = 0; i < 48; ++i) (void)hipEventCreate(&c->gev[i]);
    for (int i = 0; i < 4; ++i) (void)hipEventCreate(&c->kev[i]);
    for (int i = 0; i < 4; ++i) { if (prio) (void)hipStreamCreateWithPriority(&c->aux[i], hipStreamDefault, prio_greatest); else (void)hipStreamCreate(&c->aux[i]); (void)hipEventCreate(&c->join_ev[i]); }
    (void)hipEventCreate(&c->fork_ev);
    (void)mailbox_create(c);
    // cost tables -> one device blob
    const HostTables& T = host_tables();
    size_t o_extra = 0, o_rh = o_extra + T.extra.size() * 4, o_rr = o_rh + 400, o_lr = o_rr + 400;
    size_t o_l2c = (o_lr + 400 + 15) & ~(size_t)15, o_l2i = o_l2c + T.log2cache.size() * 8, tot = o_l2i + T.log2int.size() * 8;
    std::vector<char> blob(tot);
    memcpy(&blob[o_extra], T.extra.data(), T.extra.size() * 4);
    memcpy(&blob[o_rh], T.readgap_h.data(), 400); memcpy(&blob[o_rr], T.readgap_r.data(), 400); memcpy(&blob[o_lr], T.large_readgap.data(), 400);
    memcpy(&blob[o_l2c], T.log2cache.data(), T.log2cache.size() * 8); memcpy(&blob[o_l2i], T.log2int.data(), T.log2int.size() * 8);
    if (c->tab_buf.reserve(tot) < 0) { ctx_teardown(c); return VM_ERR_OOM; }
    if (hipMemcpy(c->tab_buf.p, blob.data(), tot, hipMemcpyHostToDevice) != hipSuccess) { ctx_teardown(c); set_error("table upload failed"); return VM_ERR_HIP; }
    char* base = (char*)c->tab_buf.p;
    c->tables.extra = (const float*)(base + o_extra); c->tables.extra_n = (int)T.extra.size();
    c->tables.readgap_h = (const float*)(base + o_rh); c->tables.readgap_r = (const float*)(base + o_rr);
    c->tables.large_readgap = (const float*)(base + o_lr);
    c->tables.log2cache = (const double*)(base + o_l2c); c->tables.log2cache_n = (int)T.log2cache.size();
    c->tables.log2int = (const double*)(base + o_l2i);
    // closed-form prefix of `extra` (vmx_extra_cost, vmx_kernels.h): the same two multiplies the kernels do, compared entry by entry
    {
        int an = 0; const int lim = std::min<int>(20000, (int)T.extra.size() - 1);
        for (; an < lim; ++an) {
            const double dg = (double)an; const double a = dg * 0.01;
            const float v = (float)((a < 10.0 ? a : 10.0) + dg * 0.001);
            if (memcmp(&v, &T.extra[an], 4) != 0) break;
        }
        c->tables.extra_arith_n = an;
        if (T.extra.back() != 36.0f) { ctx_teardown(c); set_error("cost table `extra` does not end at 36.0"); return VM_ERR_UNSUPPORTED; }
    }
    *out = c;
    return VM_OK;
}

void vm_ctx_destroy(vm_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    ctx_teardown(c);
}

int vm_ctx_set_inflight(vm_ctx* c, int n_contexts) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (n_contexts < 1) { set_error("n_contexts must be >= 1"); return VM_ERR_ARG; }
    c->inflight = n_contexts;
    return VM_OK;
}

int vm_ctx_mem_info(vm_ctx* c, int64_t* free_bytes, int64_t* total_bytes) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    size_t f = 0, t = 0;
#ifndef VMX_EMU
    VMX_HIP(hipSetDevice(c->device));
    VMX_HIP(hipMemGetInfo(&f, &t));
#else
    f = (size_t)1 << 34; t = (size_t)1 << 34;
#endif
    *free_bytes = (int64_t)f; *total_bytes = (int64_t)t;
    return VM_OK;
}

int vm_ctx_set_blocking_sync(vm_ctx* c, int on) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    // round 6: sleeping waits are the default (the mailbox of vmx_host.h); on == 0 switches this context to the legacy spinning waits (A/B runs)
    if (on && !c->mb.h) { VMX_HIP(hipSetDevice(c->device)); (void)mailbox_create(c); }
    c->mb.on = on != 0 && c->mb.h != nullptr;
    return VM_OK;
}

int64_t vm_table(vm_ctx* c, int which, void** data) {
    if (!c) return VM_ERR_NO_CTX;
    const vmx_tables& t = c->tables;
    const void* src; size_t n, es;
    switch (which) {
        case 0: src = t.extra; n = t.extra_n; es = 4; break;
        case 1: src = t.readgap_h; n = 100; es = 4; break;
        case 2: src = t.readgap_r; n = 100; es = 4; break;
        case 3: src = t.large_readgap; n = 100; es = 4; break;
        case 4: src = t.log2cache; n = t.log2cache_n; es = 8; break;
        case 5: src = t.log2int; n = 1025; es = 8; break;
        default: return VM_ERR_ARG;
    }
    *data = malloc(n * es);
    VMX_HIP(hipMemcpy(*data, src, n * es, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

}  // extern "C"

vmx_entry_bufs* vmx_ctx_entry_bufs(vm_ctx* c) { if (!c->xbufs) c->xbufs = new vmx_entry_bufs(); return c->xbufs; }

// upload concatenated ASCII + encode to codes in buf_codes; offsets uploaded to buf_off
static int upload_encode(vm_ctx* c, const char* s, const int64_t* off, int64_t n, DevBuf& raw, DevBuf& codes, DevBuf& doff) {
    const int64_t tot = off[n];
    VMX_TRY(upload(raw, s, (size_t)tot, c->stream));
    VMX_TRY(codes.reserve((size_t)tot + 64));
    VMX_TRY(upload(doff, off, (size_t)n + 1, c->stream));
    if (tot) hipLaunchKernelGGL(k_encode, dim3(grid_for(c, (tot + 255) / 256)), dim3(256), 0, c->stream, raw.as<char>(), codes.as<uint8_t>(), tot);
    return 0;
}

extern "C" {

int vm_edit_distance_batch(vm_ctx* c, int64_t n, const char* q, const int64_t* q_off, const char* t, const int64_t* t_off, int64_t** dist) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    *dist = nullptr;
    VMX_HIP(hipSetDevice(c->device));
    vmx_entry_bufs& X = *vmx_ctx_entry_bufs(c);
    VMX_TRY(upload_encode(c, q, q_off, n, X.a.raw, X.a.codes, X.a.off));
    VMX_TRY(upload_encode(c, t, t_off, n, X.b.raw, X.b.codes, X.b.off));
    VMX_TRY(X.pool.reserve((size_t)VMX_ED_WAVES * (size_t)t_off[n] + 64));     // carry ring: VMX_ED_WAVES x one int8 per text column
    VMX_TRY(X.out.reserve(sizeof(int64_t) * (size_t)(n + 1)));
    if (n) {
        // longest-first device work queue; long patterns (> 4 passes) on 16-wave workgroups, the rest on 4-wave workgroups
        std::vector<int64_t> sz((size_t)n); for (int64_t i = 0; i < n; ++i) sz[i] = q_off[i + 1] - q_off[i];
        int32_t nn = (int32_t)n;
        VMX_TRY(upload(X.sizes, sz.data(), (size_t)n, c->stream)); VMX_TRY(upload(X.count, &nn, 1, c->stream));
        VMX_TRY(X.order.reserve(4 * (size_t)(n + 1))); VMX_TRY(X.range.reserve(64));
        int32_t* d_range = X.range.as<int32_t>(); int32_t* d_cnt = d_range + 4;
        int64_t thresh = VMX_ED_LONG;
        if (const char* e = getenv("VMX_ED_LONG")) thresh = atoll(e);      // test knob: exercise the 16-wave launch with short patterns
        hipLaunchKernelGGL(k_size_order, dim3(1), dim3(1024), 0, c->stream, X.sizes.as<int64_t>(), X.count.as<int32_t>(), thresh, X.order.as<int32_t>(), d_range, d_cnt);
        for (int which = 0; which < 2; ++which)
            hipLaunchKernelGGL(k_edit_distance, dim3(grid_for(c, n, which == 0 ? 2 : 8)), dim3(which == 0 ? 64 * VMX_ED_WAVES : 256), 0, c->stream, X.a.codes.as<uint8_t>(),
                               X.a.off.as<int64_t>(), X.b.codes.as<uint8_t>(), X.b.off.as<int64_t>(), X.pool.as<int8_t>(), X.order.as<int32_t>(), d_range, d_cnt, which,
                               X.out.as<int64_t>(), (int64_t)0, (int32_t*)nullptr);
    }
    *dist = host_alloc<int64_t>((size_t)n);
    VMX_TRY(download(*dist, X.out.p, (size_t)n, c->stream));
    VMX_HIP(hipStreamSynchronize(c->stream));
    VMX_HIP(hipGetLastError());
    return VM_OK;
}

int vm_edit_distance_bound_batch(vm_ctx* c, int tier, int64_t n, const char* q, const int64_t* q_off, const char* t, const int64_t* t_off, int64_t** bound) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    *bound = nullptr;
    VMX_HIP(hipSetDevice(c->device));
    vmx_entry_bufs& X = *vmx_ctx_entry_bufs(c);
    VMX_TRY(upload_encode(c, q, q_off, n, X.a.raw, X.a.codes, X.a.off));
    VMX_TRY(upload_encode(c, t, t_off, n, X.b.raw, X.b.codes, X.b.off));
    VMX_TRY(X.out.reserve(sizeof(int64_t) * (size_t)(n + 1)));
    if (n) {
        std::vector<int64_t> sz((size_t)n); for (int64_t i = 0; i < n; ++i) sz[i] = q_off[i + 1] - q_off[i];
        int32_t nn = (int32_t)n;
        VMX_TRY(upload(X.sizes, sz.data(), (size_t)n, c->stream)); VMX_TRY(upload(X.count, &nn, 1, c->stream));
        VMX_TRY(X.order.reserve(4 * (size_t)(n + 1))); VMX_TRY(X.range.reserve(64));
        int32_t* d_range = X.range.as<int32_t>(); int32_t* d_cnt = d_range + 4;
        hipLaunchKernelGGL(k_size_order, dim3(1), dim3(1024), 0, c->stream, X.sizes.as<int64_t>(), X.count.as<int32_t>(), (int64_t)0, X.order.as<int32_t>(), d_range, d_cnt);
        if (tier == 1)
            hipLaunchKernelGGL(k_ed_banded4, dim3(grid_for(c, (n + 3) / 4, 16)), dim3(64), 0, c->stream, X.a.codes.as<uint8_t>(), X.a.off.as<int64_t>(), X.b.codes.as<uint8_t>(),
                               X.b.off.as<int64_t>(), X.order.as<int32_t>(), d_range, d_cnt, X.out.as<int64_t>());
        else
            hipLaunchKernelGGL(k_ed_banded, dim3(grid_for(c, n, 16)), dim3(64), 0, c->stream, X.a.codes.as<uint8_t>(), X.a.off.as<int64_t>(), X.b.codes.as<uint8_t>(), X.b.off.as<int64_t>(),
                               X.order.as<int32_t>(), d_range, d_cnt, X.out.as<int64_t>());
    }
    *bound = host_alloc<int64_t>((size_t)n);
    VMX_TRY(download(*bound, X.out.p, (size_t)n, c->stream));
    VMX_HIP(hipStreamSynchronize(c->stream));
    VMX_HIP(hipGetLastError());
    return VM_OK;
}

int64_t vm_edit_distance(vm_ctx* c, const char* q, int64_t ql, const char* t, int64_t tl) {
    int64_t qo[2] = {0, ql}, to[2] = {0, tl};
    int64_t* d = nullptr;
    int rc = vm_edit_distance_batch(c, 1, q, qo, t, to, &d);
    if (rc < 0) return rc;
    int64_t v = d[0]; free(d);
    return v;
}

int vm_k_extend_batch(vm_ctx* c, int match, int mismatch, int o, int e, int bw, int zdrop, int64_t n, const char* t, const int64_t* t_off,
                      const char* q, const int64_t* q_off, int32_t** t_e, int32_t** q_e, int32_t** score) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (bw > 496) { set_error("vm_k_extend_batch: band wider than 496 unsupported"); return VM_ERR_UNSUPPORTED; }
    if (bw < 0)      // no band: k_extend's LDS ring holds diagonals of up to 497 cells, min(tl, ql) + 1 without a band
        for (int64_t p = 0; p < n; ++p)
            if (std::min(t_off[p + 1] - t_off[p], q_off[p + 1] - q_off[p]) > 496) {
                set_error("vm_k_extend_batch: no band (bw < 0) with both sides longer than 496 unsupported"); return VM_ERR_UNSUPPORTED;
            }
    VMX_HIP(hipSetDevice(c->device));
    vmx_entry_bufs& X = *vmx_ctx_entry_bufs(c);
    VMX_TRY(upload_encode(c, t, t_off, n, X.a.raw, X.a.codes, X.a.off));
    VMX_TRY(upload_encode(c, q, q_off, n, X.b.raw, X.b.codes, X.b.off));
    VMX_TRY(X.out.reserve(sizeof(int32_t) * 3 * (size_t)(n + 1)));
    int32_t* d_te = X.out.as<int32_t>(); int32_t* d_qe = d_te + n; int32_t* d_sc = d_qe + n;
    if (n) hipLaunchKernelGGL(k_extend, dim3(grid_for(c, n, 16)), dim3(64), 0, c->stream, X.a.codes.as<uint8_t>(), X.a.off.as<int64_t>(),
                              X.b.codes.as<uint8_t>(), X.b.off.as<int64_t>(), (int)n, match, mismatch, o, e, bw, zdrop, d_te, d_qe, d_sc, (const int32_t*)nullptr);
    *t_e = host_alloc<int32_t>((size_t)n); *q_e = host_alloc<int32_t>((size_t)n); *score = host_alloc<int32_t>((size_t)n);
    VMX_TRY(download(*t_e, d_te, (size_t)n, c->stream)); VMX_TRY(download(*q_e, d_qe, (size_t)n, c->stream));
    VMX_TRY(download(*score, d_sc, (size_t)n, c->stream));
    VMX_HIP(hipStreamSynchronize(c->stream));
    VMX_HIP(hipGetLastError());
    return VM_OK;
}

// the CIGARs of n problems (problem i's at probs[i].cig_off of the pool, len[i] bytes) as NUL-terminated strings one after the other
static void cigar_strings(int64_t n, const vmx_dp_prob* probs, const char* pool, const int32_t* len, char** cigars, int64_t** cigar_off) {
    *cigar_off = host_alloc<int64_t>((size_t)n + 1);
    int64_t tot = 0;
    for (int64_t i = 0; i < n; ++i) { (*cigar_off)[i] = tot; tot += len[i] + 1; }
    (*cigar_off)[n] = tot;
    *cigars = host_alloc<char>((size_t)tot + 1);
    for (int64_t i = 0; i < n; ++i) { memcpy(*cigars + (*cigar_off)[i], pool + probs[i].cig_off, (size_t)len[i]); (*cigars)[(*cigar_off)[i] + len[i]] = 0; }
}

// k_gapfill_fill: the full matrix, scores captured (the reference's k_cigar call shape)
int vm_k_cigar_batch(vm_ctx* c, const vm_score* sc, int eqx, int64_t n, const char* t, const int64_t* t_off, const char* q,
                     const int64_t* q_off, char** cigars, int64_t** cigar_off, int32_t** scores) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (n > 0x7fffffff) { set_error("too many problems"); return VM_ERR_ARG; }
    VMX_HIP(hipSetDevice(c->device));
    vmx_entry_bufs& X = *vmx_ctx_entry_bufs(c);
    VMX_TRY(upload_encode(c, t, t_off, n, X.a.raw, X.a.codes, X.a.off));
    VMX_TRY(upload_encode(c, q, q_off, n, X.b.raw, X.b.codes, X.b.off));
    std::vector<vmx_dp_prob> probs((size_t)n);
    int64_t tb = 0, bnd = 0, run = 0, cig = 0;
    for (int64_t i = 0; i < n; ++i) {
        vmx_dp_prob& p = probs[i];
        p.t_off = t_off[i]; p.q_off = q_off[i]; p.tl = (int32_t)(t_off[i + 1] - t_off[i]); p.ql = (int32_t)(q_off[i + 1] - q_off[i]);
        p.tb_off = tb; p.bnd_off = bnd; p.run_off = run; p.cig_off = cig;
        tb += vmx_gf_tb_bytes_full(p.tl, p.ql);
        const vmx_gf_pool_sizes ps = vmx_gf_pools(p.tl, p.ql);
        bnd += ps.bnd; run += ps.run; cig += ps.cig;
    }
    VMX_TRY(upload(X.probs, probs.data(), (size_t)n, c->stream));
    VMX_TRY(X.pool.reserve((size_t)tb + 64)); VMX_TRY(X.bnd.reserve(sizeof(int32_t) * (size_t)(bnd + 4)));
    VMX_TRY(X.run.reserve(sizeof(uint32_t) * (size_t)(run + 4))); VMX_TRY(X.cig.reserve((size_t)cig + 16));
    VMX_TRY(X.out.reserve(sizeof(int32_t) * 2 * (size_t)(n + 1)));
    int32_t* d_score = X.out.as<int32_t>(); int32_t* d_len = d_score + n;
    if (n) {
        hipLaunchKernelGGL(k_gapfill_fill, dim3(grid_for(c, n, 16)), dim3(64), 0, c->stream, X.a.codes.as<uint8_t>(), X.b.codes.as<uint8_t>(),
                           X.probs.as<vmx_dp_prob>(), (int)n, sc->match, sc->mismatch, sc->o1, sc->e1, sc->o2, sc->e2, X.pool.as<uint8_t>(),
                           X.bnd.as<int32_t>(), d_score, (const int32_t*)nullptr, (int32_t*)nullptr);
        hipLaunchKernelGGL(k_gapfill_trace, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, X.a.codes.as<uint8_t>(), X.b.codes.as<uint8_t>(),
                           X.probs.as<vmx_dp_prob>(), (int)n, eqx, X.pool.as<uint8_t>(), X.run.as<uint32_t>(), X.cig.as<char>(), d_len, (const int32_t*)nullptr, (const uint8_t*)nullptr, 1, (int32_t*)nullptr);
    }
    std::vector<char> hc((size_t)cig + 16); std::vector<int32_t> hl((size_t)n);
    *scores = host_alloc<int32_t>((size_t)n);
    VMX_TRY(download(hc.data(), X.cig.p, (size_t)cig, c->stream));
    VMX_TRY(download(hl.data(), d_len, (size_t)n, c->stream));
    VMX_TRY(download(*scores, d_score, (size_t)n, c->stream));
    VMX_HIP(hipStreamSynchronize(c->stream));
    VMX_HIP(hipGetLastError());
    cigar_strings(n, probs.data(), hc.data(), hl.data(), cigars, cigar_off);
    return VM_OK;
}

// the gap fill of vm_align_batch (vmx_gapfill_chunk) on n problems as one chunk: the problem table is built here with the batch's traceback sizes and queue keys
// (vmx_round.h), the second launch's pool is sized for its worst case (every small problem filled again in full). stats: small problems tried in a band, kept
// (proven), queued for the second launch (incl. the small ones never tried), problems outside the small class, then the second launch's larger problems: kept from a
// wave-wide band, filled in full (stats: six values).
int vm_k_cigar_batch_banded(vm_ctx* c, const vm_score* sc, int eqx, int64_t n, const char* t, const int64_t* t_off, const char* q,
                            const int64_t* q_off, char** cigars, int64_t** cigar_off, int32_t** band_flag, int64_t* stats) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (n > 0x7fffffff) { set_error("too many problems"); return VM_ERR_ARG; }
    VMX_HIP(hipSetDevice(c->device));
    vmx_fetch_scope fetch_scope(c);
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    vmx_entry_bufs& X = *vmx_ctx_entry_bufs(c);
    VMX_TRY(upload_encode(c, t, t_off, n, X.a.raw, B.tpool, X.a.off));
    VMX_TRY(upload_encode(c, q, q_off, n, X.b.raw, B.qpool, X.b.off));
    const int ad_pct = vmx_ad_pct_env();
    vmx_round_args R; memset(&R, 0, sizeof R);
    R.ad_on = 1; R.ad_match = sc->match; R.ad_o1 = sc->o1; R.ad_e1 = sc->e1; R.ad_o2 = sc->o2; R.ad_e2 = sc->e2; R.ad_pct = ad_pct;
    std::vector<vmx_dp_prob> probs((size_t)n);
    std::vector<int64_t> keys((size_t)n);
    int64_t tb = 0, bnd = 0, run = 0, cig = 0, redo = 0;
    for (int64_t i = 0; i < n; ++i) {
        vmx_dp_prob& p = probs[i];
        p.t_off = t_off[i]; p.q_off = q_off[i]; p.tl = (int32_t)(t_off[i + 1] - t_off[i]); p.ql = (int32_t)(q_off[i + 1] - q_off[i]);
        p.tb_off = tb; p.bnd_off = bnd; p.run_off = run; p.cig_off = cig;
        tb += vmx_round_tb_bytes(R, p.tl, p.ql); keys[i] = vmx_round_key(R, p.tl, p.ql);
        if (vmx_gf_small(p.tl, p.ql)) redo += vmx_gf_tb_bytes_redo(p.tl, p.ql);
        const vmx_gf_pool_sizes ps = vmx_gf_pools(p.tl, p.ql);
        bnd += ps.bnd; run += ps.run; cig += ps.cig;
    }
    const int32_t nn = (int32_t)n;
    VMX_TRY(upload(B.dptab, probs.data(), (size_t)n, c->stream)); VMX_TRY(upload(B.dpsz[0], keys.data(), (size_t)n, c->stream)); VMX_TRY(upload(B.chunkn, &nn, 1, c->stream));
    VMX_TRY(B.tb.reserve((size_t)tb + 64)); VMX_TRY(B.tbredo.reserve((size_t)redo + 64)); VMX_TRY(B.bnd.reserve(sizeof(int32_t) * (size_t)(bnd + 4)));
    VMX_TRY(B.run.reserve(sizeof(uint32_t) * (size_t)(run + 4))); VMX_TRY(B.cig.reserve((size_t)cig + 16));
    VMX_TRY(B.ciglen.reserve(4 * (size_t)(n + 1))); VMX_TRY(B.cigq.reserve(4 * (size_t)(n + 1))); VMX_TRY(B.dpscore.reserve(4 * (size_t)(n + 1)));
    VMX_TRY(B.order.reserve(4 * (size_t)(2 * n + 64)));
    VMX_TRY(B.gfctl.reserve(sizeof(vmx_gf_ctl))); VMX_HIP(hipMemsetAsync(B.gfctl.p, 0, sizeof(vmx_gf_ctl), c->stream));
    if (!vmx_tb_base_ok(B.tb.p, 0)) { set_error("gap fill: the traceback space does not start on a 64-byte line"); return VM_ERR_ARG; }
    if (n) vmx_gapfill_chunk(c, B, *sc, ad_pct, eqx, 0, n, B.chunkn.as<int32_t>(), 0, B.gfctl.as<vmx_gf_ctl>(), B.order.as<int32_t>() + n + 32, redo, nullptr);
    std::vector<char> hc((size_t)cig + 16); std::vector<int32_t> hl((size_t)n), flag((size_t)n);
    vmx_gf_ctl ctl;                                                  // its counters; the size-order scratch behind them is not fetched
    VMX_TRY(download(hc.data(), B.cig.p, (size_t)cig, c->stream));
    VMX_TRY(download(hl.data(), B.ciglen.p, (size_t)n, c->stream));
    VMX_TRY(download(flag.data(), B.dpscore.p, (size_t)n, c->stream));          // the _ns form leaves the layout flag where the score would be (it never captures scores)
    VMX_TRY(download((char*)&ctl, B.gfctl.p, offsetof(vmx_gf_ctl, scratch), c->stream));
    VMX_HIP(vmx_stream_sync(c));
    VMX_HIP(hipGetLastError());
    int64_t nb = 0, eligible = 0, small = 0;
    for (int64_t i = 0; i < n; ++i) {
        const bool sm = vmx_gf_small(probs[i].tl, probs[i].ql);
        if (!sm) flag[i] = 0;                                     // (the larger forms leave their score there)
        small += sm; nb += sm && flag[i] > VMX_AD_FLAG;
        eligible += sm && vmx_ad_ns(probs[i].tl, probs[i].ql, sc->match, sc->o1, sc->e1, sc->o2, sc->e2, ad_pct & 0xffff, (ad_pct >> 16) & 0xffff) > 0;
    }
    if (stats) { stats[0] = eligible; stats[1] = nb; stats[2] = ctl.redo_n; stats[3] = n - small; stats[4] = ctl.redo_kept; stats[5] = ctl.redo_full; }
    if (band_flag) { *band_flag = host_alloc<int32_t>((size_t)n); memcpy(*band_flag, flag.data(), sizeof(int32_t) * (size_t)n); }
    cigar_strings(n, probs.data(), hc.data(), hl.data(), cigars, cigar_off);
    return VM_OK;
}

int vm_k_cigar(vm_ctx* c, const char* t, int64_t tl, const char* q, int64_t ql, const vm_score* sc, int bw, int zdrop, int eqx, vm_cigar_out* out) {
    memset(out, 0, sizeof(*out));
    int64_t to[2] = {0, tl}, qo[2] = {0, ql};
    if (zdrop < 0) {   // global end-to-end (:21554)
        char* cg = nullptr; int64_t* co = nullptr; int32_t* s = nullptr;
        int rc = vm_k_cigar_batch(c, sc, eqx, 1, t, to, q, qo, &cg, &co, &s);
        if (rc < 0) return rc;
        out->cigar = cg; out->q_e = (int32_t)ql; out->t_e = (int32_t)tl; out->score = s[0];
        free(co); free(s);
        return VM_OK;
    }
    if (sc->o1 != sc->o2 || sc->e1 != sc->e2) { set_error("vm_k_cigar: z-drop extension needs identical gap pieces (the reference calls it with 4,4,4,4)"); return VM_ERR_UNSUPPORTED; }
    int32_t *te = nullptr, *qe = nullptr, *s = nullptr;
    int rc = vm_k_extend_batch(c, sc->match, sc->mismatch, sc->o1, sc->e1, bw, zdrop, 1, t, to, q, qo, &te, &qe, &s);
    if (rc < 0) return rc;
    out->cigar = (char*)calloc(1, 1); out->t_e = te[0]; out->q_e = qe[0]; out->score = s[0];
    free(te); free(qe); free(s);
    return VM_OK;
}

// ------------------------------------------------------------------------------------------------ global chain stage
void vm_chains_out_free(vm_chains_out* o) {
    free(o->need_reverse); free(o->mapq); free(o->score); free(o->fast_used); free(o->read_path_off); free(o->path_off);
    free(o->path_anchors); free(o->S); free(o->P); free(o->S_arg); free(o->gmax); free(o->opcount);
    memset(o, 0, sizeof(*o));
}

int vm_chain_global_batch(vm_ctx* c, const vm_params* prm, int kmersize, int64_t n, const int64_t* anchors, const int64_t* aoff,
                          const int64_t* readlens, int want_raw, vm_chains_out* out) {
    memset(out, 0, sizeof(*out));
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (prm->global_maxdiff > 62) { set_error("global_maxdiff > 62 unsupported"); return VM_ERR_UNSUPPORTED; }
    const int64_t tot = aoff[n];
    if (const int64_t bad = vmx_rows_misfit(anchors, tot); bad >= 0) {
        char msg[192]; snprintf(msg, sizeof msg, "vm_chain_global_batch: anchor row %lld does not fit the device row (l in 0 ... 65535, q and q + l in int32, s in int16)", (long long)bad);
        set_error(msg); return VM_ERR_UNSUPPORTED;
    }
    VMX_HIP(hipSetDevice(c->device));
    vmx_fetch_scope fetch_scope(c);
    vmx_batch_bufs& B = *vmx_ctx_batch_bufs(c);
    const std::vector<int64_t> h_aoff(aoff, aoff + n + 1);
    std::vector<int64_t> h_roff((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) h_roff[(size_t)r + 1] = h_roff[(size_t)r] + readlens[r];
    VMX_TRY(upload(B.rows, anchors, (size_t)tot * 4, c->stream)); VMX_TRY(upload(B.aoff, aoff, (size_t)n + 1, c->stream));
    VMX_TRY(upload(B.lens, readlens, (size_t)n, c->stream)); VMX_TRY(upload(B.off, h_roff.data(), (size_t)n + 1, c->stream));
    DevBuf& d_ran = vmx_ctx_entry_bufs(c)->out;                       // GC-fast's flags: fast_used
    VMX_TRY(d_ran.reserve(4 * (size_t)(n + 1))); VMX_HIP(hipMemsetAsync(d_ran.p, 0, 4 * (size_t)n, c->stream));
    const int rmode = prm->mode == VM_MODE_R ? 1 : (prm->mode == VM_MODE_ASM ? 2 : 0);
    double* d_score = nullptr; int32_t* d_mapq = nullptr; int32_t* d_np = nullptr;
    if (n) {
        VMX_TRY(vmx_global_stage(c, B, prm, kmersize, n, B.off.as<int64_t>(), h_roff, h_aoff, rmode, d_ran.as<int32_t>()));
        vmx_res_ptrs(B, n, &d_score, &d_mapq, &d_np);
    }
    // download
    std::vector<int32_t> h_np((size_t)n), h_plen((size_t)tot);
    std::vector<vmx_anchor> h_prow((size_t)tot);
    out->need_reverse = host_alloc<int32_t>((size_t)n); out->mapq = host_alloc<int32_t>((size_t)n); out->score = host_alloc<double>((size_t)n);
    out->fast_used = host_alloc<int32_t>((size_t)n); out->gmax = host_alloc<int64_t>((size_t)n); out->opcount = host_alloc<int64_t>((size_t)n);
    VMX_TRY(download(out->need_reverse, B.flip.p, (size_t)n, c->stream)); VMX_TRY(download(out->mapq, d_mapq, (size_t)n, c->stream));
    VMX_TRY(download(out->score, d_score, (size_t)n, c->stream)); VMX_TRY(download(h_np.data(), d_np, (size_t)n, c->stream));
    VMX_TRY(download(h_plen.data(), B.plen.p, (size_t)tot, c->stream)); VMX_TRY(download(h_prow.data(), B.prow.p, (size_t)tot, c->stream));
    VMX_TRY(download(out->gmax, B.gmax.p, (size_t)n, c->stream)); VMX_TRY(download(out->opcount, B.opc.p, (size_t)n, c->stream));
    VMX_TRY(download(out->fast_used, d_ran.p, (size_t)n, c->stream));
    std::vector<int32_t> hP, hSA;
    if (want_raw) {
        out->S = host_alloc<double>((size_t)tot); out->P = host_alloc<int64_t>((size_t)tot); out->S_arg = host_alloc<int64_t>((size_t)tot);
        hP.resize((size_t)tot); hSA.resize((size_t)tot);
        VMX_TRY(download(out->S, B.S.p, (size_t)tot, c->stream)); VMX_TRY(download(hP.data(), B.P.p, (size_t)tot, c->stream));
        VMX_TRY(download(hSA.data(), B.SA.p, (size_t)tot, c->stream));
    }
    VMX_HIP(vmx_stream_sync(c));
    VMX_HIP(hipGetLastError());
    if (want_raw) for (int64_t i = 0; i < tot; ++i) { out->P[i] = hP[i]; out->S_arg[i] = hSA[i]; }
    for (int64_t r = 0; r < n; ++r) if (h_np[r] < 0) h_np[r] = 0;      // -mode asm: a contig waiting for decode_hit's edlib tie-break (made inside vm_align_batch) has no path at this stage entry
    int64_t npaths = 0, nrows = 0;
    for (int64_t r = 0; r < n; ++r) { npaths += h_np[r]; for (int p = 0; p < h_np[r]; ++p) nrows += h_plen[aoff[r] + p]; }
    out->read_path_off = host_alloc<int64_t>((size_t)n + 1); out->path_off = host_alloc<int64_t>((size_t)npaths + 1);
    out->path_anchors = host_alloc<int64_t>((size_t)nrows * 4);
    int64_t pi = 0, ro = 0;
    for (int64_t r = 0; r < n; ++r) {
        out->read_path_off[r] = pi;
        int64_t src = aoff[r];
        for (int p = 0; p < h_np[r]; ++p) {
            out->path_off[pi++] = ro;
            for (int x = 0; x < h_plen[aoff[r] + p]; ++x) {
                const vmx_anchor& a = h_prow[src++];
                int64_t* o = out->path_anchors + 4 * ro++;
                o[0] = a.q; o[1] = a.r; o[2] = a.s; o[3] = (uint16_t)a.l;      // (the length is an unsigned 16-bit field: 32768 ... 65535 read back as such)
            }
        }
    }
    out->read_path_off[n] = pi; out->path_off[pi] = ro;
    return VM_OK;
}

}  // extern "C"
