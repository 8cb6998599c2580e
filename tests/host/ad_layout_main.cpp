// TEST-ONLY: prints the anti-diagonal traceback layout of vacmap_amd/csrc/vmx_gapfill.h (vmx_ad_tb_off, vmx_ad_tb_bytes, and the reader's split of a cell's offset
// into a lane part and an anti-diagonal part) from a plain C++ program as one JSON object; tests/test_emu_ad_block_store.py builds it with g++ under
// AddressSanitizer and UBSan, runs it and compares every offset with a NumPy statement of the layout. The header's own build-time checks are compiled in.
#define __host__
#define __device__
#define __forceinline__ inline
#define VMX_GAPFILL_CHECKS
#include "vmx_gapfill.h"
#include <cstdio>

int main() {
    const int S = 24, LN = 16;          // six blocks of four anti-diagonals x the 16 lanes of a row
    printf("{\"AB\":%d,\"S\":%d,\"L\":%d,\"off\":{", VMX_AD_AB, S, LN);
    const int Ws[3] = {1, 2, 4};
    for (int w = 0; w < 3; ++w) {
        printf("%s\"%d\":[", w ? "," : "", Ws[w]);
        for (int s = 0; s < S; ++s)
            for (int l = 0; l < LN; ++l) printf("%s%zu", (s || l) ? "," : "", vmx_ad_tb_off((size_t)s, (size_t)l, Ws[w]));
        printf("]");
    }
    // the space of a problem, per slot width: [tl, ql, W, bytes]
    printf("},\"bytes\":[");
    bool first = true;
    for (int tl = 1; tl <= 9; ++tl)
        for (int ql = 1; ql <= 160 - tl; ql += (ql < 8 ? 1 : 37))
            for (int w = 0; w < 3; ++w) { printf("%s[%d,%d,%d,%lld]", first ? "" : ",", tl, ql, Ws[w], (long long)vmx_ad_tb_bytes(tl, ql, Ws[w])); first = false; }
    // the walk's view of a proven problem: [tl, ql, ns, i, j, cell_off, lane_off, step_off] for cells down the diagonals the band holds
    printf("],\"cells\":[");
    first = true;
    for (int ns = 1; ns <= VMX_AD_NS_MAX; ++ns) {
        const int tl = 21, ql = 24;
        const vmx_tb_layout L = vmx_tb_layout_of(tl, ql, VMX_AD_FLAG + ns);
        for (int i = 1; i <= tl; i += 3)
            for (int j = 1; j <= ql; j += 2) {
                const int x = (j - i) - L.dlo;
                if (x < 0 || x >= 32 * ns) continue;
                printf("%s[%d,%d,%d,%d,%d,%zu,%zu,%zu,%d,%d]", first ? "" : ",", tl, ql, ns, i, j, vmx_tb_cell_off(L, i, j), vmx_tb_ad_lane_off(L, i, j), vmx_tb_ad_step_off(L, i + j - 1), L.dlo,
                       1 << L.w);
                first = false;
            }
    }
    printf("]}\n");
    return 0;
}
