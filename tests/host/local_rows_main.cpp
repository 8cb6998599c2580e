// TEST-ONLY: the host's check of the rows given to vm_local_dp_batch (vacmap_amd/csrc/vmx_local_rows.h) alone, built with plain g++ under AddressSanitizer
// and UBSan (tests/test_local_rows_host.py). Usage: local_rows <file> ...: every file holds one batch as whitespace-separated integers — n, by_start, then
// n + 1 row offsets, n guide counts, n read lengths and 4 integers per row. Every array is a heap block of exactly its size (a read past one is a sanitizer
// report). One output line per file: code, read, row, and the reason.
#include "vmx_local_rows.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "r");
        if (!f) return 2;
        std::vector<long long> v;
        for (long long x; fscanf(f, "%lld", &x) == 1;) v.push_back(x);
        fclose(f);
        if (v.size() < 2) return 2;
        const int64_t n = v[0]; const bool by_start = v[1] != 0;
        size_t at = 2;
        if (n < 0 || v.size() < at + (size_t)(3 * n + 1)) return 2;
        std::unique_ptr<int64_t[]> off(new int64_t[(size_t)n + 1]);
        for (int64_t i = 0; i <= n; ++i) off[(size_t)i] = v[at++];
        std::unique_ptr<int32_t[]> ng(new int32_t[(size_t)(n ? n : 1)]);
        for (int64_t i = 0; i < n; ++i) ng[(size_t)i] = (int32_t)v[at++];
        std::unique_ptr<int64_t[]> rl(new int64_t[(size_t)(n ? n : 1)]);
        for (int64_t i = 0; i < n; ++i) rl[(size_t)i] = v[at++];
        const size_t nrow = (v.size() - at) / 4;
        std::unique_ptr<int64_t[]> rows(new int64_t[nrow ? 4 * nrow : 1]);
        for (size_t i = 0; i < 4 * nrow; ++i) rows[i] = v[at++];
        // (the offsets of a well-formed file end at its row count; a file whose offsets point past its rows is the test's mistake, not a case)
        int64_t top = 0; for (int64_t i = 0; i <= n; ++i) top = off[(size_t)i] > top ? off[(size_t)i] : top;
        if ((size_t)top > nrow) return 3;
        const vmx_rows_verdict r = vmx_local_rows_check(rows.get(), off.get(), n, ng.get(), rl.get(), by_start);
        printf("%d %lld %lld %s\n", r.code, (long long)r.read, (long long)r.row, r.what);
    }
    return 0;
}
