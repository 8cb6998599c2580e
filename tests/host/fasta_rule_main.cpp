// TEST-ONLY: the line rule of a reference FASTA (vacmap_amd/csrc/vmx_fasta_rule.h) alone, built with plain g++ under AddressSanitizer and UBSan
// (tests/test_fasta_rule_host.py). Usage: fasta_rule <file> <piece bytes> ...: for every piece size the file goes through FastaRule::feed in
// pieces of that many bytes, each piece a heap block of exactly its size (a read past a piece is a sanitizer report); one output line
// per contig: piece size, name and letters in hex.
#include "vmx_fasta_rule.h"
#include <cstdio>
#include <cstdlib>
#include <memory>

static void hex(const std::string& s) { for (unsigned char c : s) printf("%02x", c); }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::string text;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) text.append(buf, n);
    fclose(f);
    for (int a = 2; a < argc; ++a) {
        const size_t piece = (size_t)atoll(argv[a]);
        if (piece == 0) return 2;
        vmx::FastaRule R;
        for (size_t at = 0; at < text.size(); at += piece) {
            const size_t n = std::min(piece, text.size() - at);
            std::unique_ptr<char[]> p(new char[n]);
            memcpy(p.get(), text.data() + at, n);
            R.feed(p.get(), n);
        }
        R.finish();
        if (R.names.size() != R.seqs.size()) return 3;
        for (size_t i = 0; i < R.names.size(); ++i) { printf("%zu ", piece); hex(R.names[i]); printf(" "); hex(R.seqs[i]); printf("\n"); }
        printf("%zu end\n", piece);
    }
    return 0;
}
