// vmx_devbuf.h — who owns memory the device reads and writes: DevBuf (device), HostPinned (page-locked host), and DevView, a slice of someone else's DevBuf.
// A DevBuf frees its allocation when it dies, so a struct of buffers needs no release list and a local needs no guard; it moves and does not copy.
// No DevBuf or HostPinned has static storage duration: its destructor would call into the HIP runtime during process exit, after the runtime may be gone.
// Needs the HIP runtime (hip_emu.h under VMX_EMU), the status codes of vacmapx.h and the two error reporters declared below: a plain g++ builds it alone.
#ifndef VMX_DEVBUF_H
#define VMX_DEVBUF_H
#ifdef VMX_EMU
#include "hip_emu.h"
#else
#include <hip/hip_runtime.h>
#endif
#include "../../include/vacmapx.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>
#include <execinfo.h>

namespace vmx {

void set_error(const std::string& s);
int hip_fail(hipError_t e, const char* what, const char* file, int line);

// growth statistics of the grow-only pools (tuning aid, printed with VMX_DBG_POOLS): a growth is a hipFree — which waits for the whole
// device, every other context's batch included — plus a hipMalloc
struct DevBufStats { std::atomic<long long> grows{0}, first{0}, ns{0}; };
inline DevBufStats& devbuf_stats() { static DevBufStats s; return s; }

// A buffer that has to grow is not freed on the spot: hipFree waits for the WHOLE device — every other context's batch in flight — and a
// run's first windows grow a few hundred buffers (each new longest read resizes the per-slot pools). The outgrown allocations are parked
// here and freed together once they add up to VMX_RETIRE_BYTES (one device-wide wait instead of hundreds), when an allocation fails, or
// when a context is destroyed.
struct DevBufRetired {
    std::mutex m; std::vector<void*> v; size_t bytes = 0;
    void flush_locked() { for (void* q : v) (void)hipFree(q); v.clear(); bytes = 0; }
    void flush() { std::lock_guard<std::mutex> g(m); flush_locked(); }
    void park(void* q, size_t cap) {
        std::lock_guard<std::mutex> g(m);
        v.push_back(q); bytes += cap;
        if (bytes > ((size_t)6 << 30) || v.size() >= 512) flush_locked();
    }
};
inline DevBufRetired& devbuf_retired() { static DevBufRetired r; return r; }

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default; DevBuf(const DevBuf&) = delete; DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    // grows with head-room so that slightly larger batches do not reallocate: 1/8 on the first allocation, 1/2 (at most 2 GB) when the
    // buffer has to grow again — the input has shown that it varies
    int reserve(size_t bytes) {
        if (bytes <= cap && p) return 0;
        const auto t0 = std::chrono::steady_clock::now();
        const bool regrow = p != nullptr;
        if (p) { devbuf_retired().park(p, cap); p = nullptr; cap = 0; }
        size_t want = bytes + (regrow ? std::min<size_t>(bytes / 2, (size_t)2 << 30) : std::min<size_t>(bytes / 8, (size_t)1 << 30)) + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) { (void)hipGetLastError(); devbuf_retired().flush(); e = hipMalloc(&p, want); }                // give the parked memory back first
        if (e != hipSuccess && regrow) { (void)hipGetLastError(); want = bytes + 256; e = hipMalloc(&p, want); }          // no room for the head-room: exact size
        if (e != hipSuccess) { p = nullptr; if (getenv("VMX_DBG_POOLS")) { fprintf(stderr, "[pools] hipMalloc of %.3f GB (asked: %.3f GB) failed\n", want / 1e9, bytes / 1e9); void* bt[24]; const int nb = backtrace(bt, 24); backtrace_symbols_fd(bt, nb, 2); } return hip_fail(e, "hipMalloc", __FILE__, __LINE__); }
        cap = want;
        DevBufStats& st = devbuf_stats(); (regrow ? st.grows : st.first)++;
        const long long ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        st.ns += ns;
        static const bool verbose = getenv("VMX_DBG_POOLS") && atoi(getenv("VMX_DBG_POOLS")) >= 2;
        if (verbose && ns > 2000000) fprintf(stderr, "[pools] %s of %.3f GB took %.1f ms\n", regrow ? "re-allocation" : "allocation", want / 1e9, ns * 1e-6);
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// cap bytes at p inside a DevBuf that someone else owns (or all of it): frees nothing, reserves nothing, copies freely. Valid until its owner grows or dies.
struct DevView {
    void* p = nullptr; size_t cap = 0;
    DevView() = default; DevView(void* q, size_t n) : p(q), cap(n) {} DevView(const DevBuf& b) : p(b.p), cap(b.cap) {}
    template <class T> T* as() const { return (T*)p; }
};

// grow-only page-locked buffer with head-room. An outgrown buffer is parked, not freed: hipHostFree waits for the whole device (the aligner
// contexts' batches included), so the parked ones go when their owner does, as DevBuf parks its outgrown device buffers
struct HostPinned {
    char* p = nullptr; size_t cap = 0;
    std::vector<char*> parked;
    HostPinned() = default; HostPinned(const HostPinned&) = delete; HostPinned& operator=(const HostPinned&) = delete;
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

}  // namespace vmx
#endif
