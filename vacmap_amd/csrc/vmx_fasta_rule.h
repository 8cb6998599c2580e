// vmx_fasta_rule.h — the line rule of a reference FASTA over a byte stream (the rule: include/vacmapx.h, vm_index_build_fasta). No HIP: a plain
// g++ builds it alone (tests/host/fasta_rule_main.cpp). The host parser feeds it the pieces of a plain file or of a zlib stream; the device
// parser (k_fasta_in.hip) implements the same rule per chunk of text and hands its header lines to fasta_header_name.
#ifndef VMX_FASTA_RULE_H
#define VMX_FASTA_RULE_H
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace vmx {

// the name of a header line: the bytes behind '>' (s[0, n), trailing '\r' already removed or not) up to the first blank or tab; may be empty
inline std::string fasta_header_name(const char* s, size_t n) {
    while (n && s[n - 1] == '\r') --n;
    size_t e = 0;
    while (e < n && s[e] != ' ' && s[e] != '\t') ++e;
    return std::string(s, e);
}

struct FastaRule {
    std::vector<std::string> names, seqs;
    std::string cur;                        // the bytes of a line whose newline has not arrived

    // a line without its newline
    void line(const char* s, size_t n) {
        while (n && s[n - 1] == '\r') --n;
        if (n == 0) return;
        if (s[0] == '>') { names.push_back(fasta_header_name(s + 1, n - 1)); seqs.emplace_back(); }
        else if (!seqs.empty()) seqs.back().append(s, n);
    }
    // the next n bytes of the stream, cut anywhere
    void feed(const char* p, size_t n) {
        while (n) {
            const char* nl = (const char*)memchr(p, '\n', n);
            if (!nl) { cur.append(p, n); return; }
            const size_t k = (size_t)(nl - p);
            if (cur.empty()) line(p, k);
            else { cur.append(p, k); line(cur.data(), cur.size()); cur.clear(); }
            p += k + 1; n -= k + 1;
        }
    }
    // the end of the stream: the bytes behind the last newline are a line as well
    void finish() { line(cur.data(), cur.size()); cur.clear(); }
};

}  // namespace vmx
#endif
