// vmx_local_rows.h — what the host checks of the anchor rows handed to vm_local_dp_batch before anything reaches the device. Plain C++ (no HIP), so that
// tests/host/local_rows_main.cpp builds it alone under AddressSanitizer and UBSan.
// The device row (vmx_anchor) keeps q in 32 bits, l as an unsigned 16-bit length and the strand in 16: a batch with a row that does not fit is refused as a
// whole (UNSUPPORTED, as vm_chain_global_batch does), and so is a strand other than +1 / -1. The DPs take their rows in the order the seeding leaves them in
// — stable by read end q + l (:28585), by read start q in mode R — and the `_fast` twins size their score buckets from the read length: rows out of order,
// a negative read position, a row that ends behind its read or a guide count below 1 are the caller's mistake (ARG).
#ifndef VMX_LOCAL_ROWS_H
#define VMX_LOCAL_ROWS_H
#include <stdint.h>

#define VMX_ROWS_OK 0
#define VMX_ROWS_ARG (-1)              /* = VM_ERR_ARG */
#define VMX_ROWS_UNSUPPORTED (-7)      /* = VM_ERR_UNSUPPORTED */

struct vmx_rows_verdict { int code; int64_t read, row; const char* what; };       // row: index into the batch's rows (-1: the read as a whole)

// rows: 4 int64 per row (q, r, s, l); off[n + 1]: first row of every read; by_start: mode R
static inline vmx_rows_verdict vmx_local_rows_check(const int64_t* rows, const int64_t* off, int64_t n, const int32_t* n_guides_total, const int64_t* readlens, bool by_start) {
    if (off[0] != 0) return vmx_rows_verdict{VMX_ROWS_ARG, 0, -1, "row offsets do not start at 0"};
    for (int64_t r = 0; r < n; ++r) if (off[r + 1] < off[r]) return vmx_rows_verdict{VMX_ROWS_ARG, r, -1, "row offsets decrease"};
    // what the device's fields cannot carry first: the refusal does not depend on anything else being right
    for (int64_t r = 0; r < n; ++r)
        for (int64_t i = off[r]; i < off[r + 1]; ++i) {
            const int64_t q = rows[4 * i], s = rows[4 * i + 2], l = rows[4 * i + 3];
            if (l < 0 || l > 65535) return vmx_rows_verdict{VMX_ROWS_UNSUPPORTED, r, i, "l outside 0 ... 65535"};
            if (q < INT32_MIN || q > INT32_MAX || q + l > INT32_MAX) return vmx_rows_verdict{VMX_ROWS_UNSUPPORTED, r, i, "q or q + l outside int32"};
            if (s != 1 && s != -1) return vmx_rows_verdict{VMX_ROWS_UNSUPPORTED, r, i, "s is neither +1 nor -1"};
        }
    for (int64_t r = 0; r < n; ++r) {
        if (n_guides_total[r] < 1) return vmx_rows_verdict{VMX_ROWS_ARG, r, -1, "n_guides_total below 1"};
        if (readlens[r] < 0 || readlens[r] > INT32_MAX) return vmx_rows_verdict{VMX_ROWS_ARG, r, -1, "read length outside 0 ... 2^31 - 1"};
        if (off[r + 1] - off[r] > INT32_MAX) return vmx_rows_verdict{VMX_ROWS_ARG, r, -1, "more than 2^31 - 1 rows"};
        int64_t prev = INT64_MIN;
        for (int64_t i = off[r]; i < off[r + 1]; ++i) {
            const int64_t q = rows[4 * i], l = rows[4 * i + 3];
            if (q < 0) return vmx_rows_verdict{VMX_ROWS_ARG, r, i, "negative read position"};
            if (q + l > readlens[r]) return vmx_rows_verdict{VMX_ROWS_ARG, r, i, "row ends behind its read"};
            const int64_t key = by_start ? q : q + l;
            if (key < prev) return vmx_rows_verdict{VMX_ROWS_ARG, r, i, by_start ? "rows are not in order of read start" : "rows are not in order of read end"};
            prev = key;
        }
    }
    return vmx_rows_verdict{VMX_ROWS_OK, -1, -1, ""};
}

#endif
