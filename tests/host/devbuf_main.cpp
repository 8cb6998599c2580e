// TEST-ONLY: drives vacmap_amd/csrc/vmx_devbuf.h (DevBuf, DevView, HostPinned, the parking list) against the emulator's allocator from a plain C++ program and
// prints one JSON row per case; tests/test_devbuf.py builds it with g++ -fsanitize=address,undefined, runs it and checks every row. The emulator counts its live
// allocations (hip_emu.h), AddressSanitizer sees a block freed twice, and LeakSanitizer, at exit, one that nobody freed.
#include "vmx_devbuf.h"
#include <type_traits>
#include <utility>

namespace vmx {
static std::string g_err;
void set_error(const std::string& s) { g_err = s; }
int hip_fail(hipError_t e, const char* what, const char*, int) { g_err = std::string(what) + " failed: " + std::to_string(e); return -1; }
}
using namespace vmx;

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "a DevBuf owns its allocation: it must not copy");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "a DevBuf moves");
static_assert(std::is_trivially_copyable<DevView>::value && std::is_trivially_destructible<DevView>::value, "a view owns nothing");
static_assert(!std::is_copy_constructible<HostPinned>::value, "a HostPinned owns its blocks: it must not copy");

static long long dev() { return hipemu::live_allocs(0).load(); }
static long long host() { return hipemu::live_allocs(1).load(); }
static size_t parked() { std::lock_guard<std::mutex> g(devbuf_retired().m); return devbuf_retired().v.size(); }
static int n_rows = 0;
#define ROW(...) do { printf(n_rows++ ? ",\n" : "[\n"); printf(__VA_ARGS__); } while (0)

struct Bundle { DevBuf a, b[2]; struct Inner { DevBuf x, y; } in; HostPinned pin; };

int main() {
    for (size_t b : {(size_t)1, (size_t)300, (size_t)1000, (size_t)4096}) {                  // first reserve
        DevBuf d; const int rc = d.reserve(b);
        ROW("{\"case\":\"first\",\"bytes\":%zu,\"rc\":%d,\"cap\":%zu,\"live\":%lld}", b, rc, d.cap, dev());
    }
    ROW("{\"case\":\"first_gone\",\"live\":%lld,\"parked\":%zu}", dev(), parked());
    for (size_t b : {(size_t)594, (size_t)1001, (size_t)5000}) {                             // growing: the old block is parked, not freed
        DevBuf d; d.reserve(300); void* p0 = d.p; const size_t park0 = parked(); const long long live0 = dev();
        const int rc = d.reserve(b);
        ROW("{\"case\":\"grow\",\"bytes\":%zu,\"rc\":%d,\"cap\":%zu,\"moved\":%d,\"parked_more\":%zu,\"live_more\":%lld,\"parked_bytes\":%zu}", b, rc, d.cap, (int)(d.p != p0),
            parked() - park0, dev() - live0, devbuf_retired().bytes);
        devbuf_retired().flush();
    }
    {                                                                                        // within capacity: nothing moves
        DevBuf d; d.reserve(300); void* p0 = d.p; const size_t c0 = d.cap; const long long live0 = dev();
        const int r1 = d.reserve(10), r2 = d.reserve(c0);
        ROW("{\"case\":\"within\",\"rc\":[%d,%d],\"same_p\":%d,\"same_cap\":%d,\"live_more\":%lld,\"parked\":%zu}", r1, r2, (int)(d.p == p0), (int)(d.cap == c0), dev() - live0, parked());
    }
    {                                                                                        // the 512th parked block empties the list
        devbuf_retired().flush();
        size_t at511 = 0; long long live511 = 0;
        for (int i = 0; i < 512; ++i) {
            DevBuf d; d.reserve(64); d.reserve(d.cap + 1);
            if (i == 510) { at511 = parked(); live511 = dev(); }
        }
        ROW("{\"case\":\"park512\",\"parked_after_511\":%zu,\"live_after_511\":%lld,\"parked_after_512\":%zu,\"live_after_512\":%lld}", at511, live511, parked(), dev());
    }
    {                                                                                        // flush
        DevBuf d; d.reserve(64); d.reserve(d.cap + 1); d.reserve(d.cap + 1);
        const size_t before = parked(); const long long live0 = dev();
        devbuf_retired().flush();
        ROW("{\"case\":\"flush\",\"parked_before\":%zu,\"parked_after\":%zu,\"bytes_after\":%zu,\"freed\":%lld}", before, parked(), devbuf_retired().bytes, live0 - dev());
    }
    {                                                                                        // move construction
        DevBuf a; a.reserve(500); void* p0 = a.p; const size_t c0 = a.cap; const long long live0 = dev();
        DevBuf b(std::move(a));
        ROW("{\"case\":\"move_ctor\",\"src_empty\":%d,\"dst_has\":%d,\"live_more\":%lld}", (int)(a.p == nullptr && a.cap == 0), (int)(b.p == p0 && b.cap == c0), dev() - live0);
    }
    {                                                                                        // move assignment: what the target held is freed once, the source is empty
        DevBuf a, b; a.reserve(500); b.reserve(700); void* p0 = a.p; const size_t c0 = a.cap; const long long live0 = dev();
        b = std::move(a);
        const long long freed = live0 - dev();
        DevBuf& self = b; b = std::move(self);                                               // onto itself: nothing happens
        ROW("{\"case\":\"move_assign\",\"src_empty\":%d,\"dst_has\":%d,\"freed\":%lld,\"freed_after_self\":%lld}", (int)(a.p == nullptr && a.cap == 0), (int)(b.p == p0 && b.cap == c0), freed, live0 - dev());
    }
    ROW("{\"case\":\"moves_gone\",\"live\":%lld}", dev());
    {                                                                                        // a view frees nothing
        DevBuf d; d.reserve(1000); const long long live0 = dev(); int ok = 0;
        {
            DevView whole(d), part((char*)d.p + 256, 128), copy = part;
            ok = whole.p == d.p && whole.cap == d.cap && part.as<char>() == d.as<char>() + 256 && copy.cap == 128;
        }
        d.as<char>()[999] = 1;                                                               // (still there: AddressSanitizer would say otherwise)
        ROW("{\"case\":\"view\",\"ok\":%d,\"freed\":%lld}", ok, live0 - dev());
    }
    {                                                                                        // HostPinned: grow, park, destroy
        long long live_grown = 0; size_t cap1 = 0, cap2 = 0, np = 0; int same = 0;
        {
            HostPinned h; h.reserve(100); cap1 = h.cap; char* p0 = h.p; h.reserve(50); same = h.p == p0 && h.cap == cap1;
            h.reserve(10000); cap2 = h.cap; np = h.parked.size(); live_grown = host();
            h.p[9999] = 1;
        }
        ROW("{\"case\":\"pinned\",\"cap\":[%zu,%zu],\"same_within\":%d,\"parked\":%zu,\"live_grown\":%lld,\"live_after\":%lld,\"dev_live\":%lld}", cap1, cap2, same, np, live_grown, host(), dev());
    }
    {                                                                                        // a bundle of buffers, used and destroyed
        long long live_in = 0, host_in = 0;
        {
            Bundle B; B.a.reserve(100); B.b[1].reserve(2000); B.in.x.reserve(1); B.in.x.reserve(5000); B.pin.reserve(64);
            B.in.y = std::move(B.b[1]); B.b[0].reserve(10);
            live_in = dev(); host_in = host();
        }
        devbuf_retired().flush();
        ROW("{\"case\":\"bundle\",\"live_in\":%lld,\"host_in\":%lld,\"live_after\":%lld,\"host_after\":%lld}", live_in, host_in, dev(), host());
    }
    ROW("{\"case\":\"stats\",\"first\":%lld,\"grows\":%lld}", devbuf_stats().first.load(), devbuf_stats().grows.load());
    printf("\n]\n");
    return (dev() == 0 && host() == 0 && vmx::g_err.empty()) ? 0 : 1;
}
