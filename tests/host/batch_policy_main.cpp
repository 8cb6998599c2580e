// TEST-ONLY: drives vacmap_amd/csrc/vmx_batch_policy.h (the batched path's host decisions) from a plain C++ program and prints what it decided as one JSON object;
// tests/test_batch_policy.py builds it with g++ -fsanitize=address,undefined, runs it and compares every row with a Python restatement of the rules.
// Each row carries its own inputs ("in") next to the result ("out"), so the Python side needs no second copy of the case list.
#include "vmx_batch_policy.h"
#include <cstdio>
#include <cstring>

static void p_geo(bool first, long long cl, long long len, int mul, int tmask, long long tdiv) {
    const vmx_read_geo g = vmx_read_geometry(cl, len, mul, tmask, tdiv);
    printf("%s{\"in\":[%lld,%lld,%d,%d,%lld],\"out\":[%lld,%lld,%lld,%lld]}", first ? "" : ",", cl, len, mul, tmask, tdiv, g.anchors, g.segs, g.blob, g.full);
}
static void p_pool(bool first, int bit, long long x, int mul, int tmask, long long tdiv) {
    printf("%s{\"in\":[%d,%lld,%d,%d,%lld],\"out\":%lld}", first ? "" : ",", bit, x, mul, tmask, tdiv, vmx_pool_scaled(bit, x, mul, tmask, tdiv));
}

struct vote_t { int ad_cur; long long not_proven, problems; };
// one rule from a start state through a list of votes: the state after every vote
static void p_rule(bool first, const char* name, vmx_ad_rule r, const std::vector<vote_t>& votes) {
    printf("%s{\"name\":\"%s\",\"start\":[%d,%d,%d],\"steps\":[", first ? "" : ",", name, r.pct, r.floor, r.hold);
    for (size_t i = 0; i < votes.size(); ++i) {
        r.vote(votes[i].ad_cur, votes[i].not_proven, votes[i].problems);
        printf("%s{\"in\":[%d,%lld,%lld],\"out\":[%d,%d,%d]}", i ? "," : "", votes[i].ad_cur, votes[i].not_proven, votes[i].problems, r.pct, r.floor, r.hold);
    }
    printf("]}");
}

static void p_status(bool first, const vmx_status_in& s) {
    const vmx_read_outcome o = vmx_read_status(s);
    printf("%s{\"in\":{\"er_status\":%d,\"er_active\":%d,\"er_redo\":%d,\"er_pass\":%d,\"er_nrec\":%d,\"fast_local\":%d,\"do_pass1\":%d,\"force_exact\":%d,\"test_side_every\":%lld,\"r\":%lld,"
           "\"gmax\":%lld,\"n_anchors\":%lld,\"rmode\":%d,\"asm_override\":%d},\"out\":[%d,%d]}",
           first ? "" : ",", s.er_status, s.er_active, s.er_redo, s.er_pass, s.er_nrec, (int)s.fast_local, (int)s.do_pass1, (int)s.force_exact, s.test_side_every, s.r, s.gmax, s.n_anchors, s.rmode,
           s.asm_override, o.status, (int)o.unmapped);
}
static vmx_status_in clean() { vmx_status_in s; memset(&s, 0, sizeof s); s.er_active = 1; s.er_nrec = 1; s.n_anchors = 50; s.r = 3; return s; }

// ---- splice: a result is (records, blob); CIGAR strings are NUL-terminated in the blob
struct result_t { std::vector<vm_record> recs; std::string blob; };
static void add_rec(result_t& R, int read, const char* cigar, int64_t q_st, int64_t q_en) {
    vm_record x; memset(&x, 0, sizeof x);
    x.read_idx = read; x.contig = 0; x.strand = 1; x.mapq = 60; x.q_st = q_st; x.q_en = q_en; x.r_st = 100 + q_st; x.r_en = 100 + q_en;
    x.cigar_off = (int64_t)R.blob.size(); x.cigar_len = (int64_t)strlen(cigar);
    R.blob.append(cigar); R.blob.push_back('\0');
    R.recs.push_back(x);
}
static void p_result(const char* key, const std::vector<vm_record>& recs, const std::string& blob) {
    printf("\"%s\":{\"recs\":[", key);
    for (size_t i = 0; i < recs.size(); ++i)
        printf("%s[%d,%lld,%lld,%lld,%lld]", i ? "," : "", recs[i].read_idx, (long long)recs[i].q_st, (long long)recs[i].q_en, (long long)recs[i].cigar_off, (long long)recs[i].cigar_len);
    printf("],\"blob\":\"");
    for (unsigned char ch : blob) printf("%02x", ch);
    printf("\"}");
}
struct side_t { std::vector<int32_t> sub; result_t res; std::vector<int32_t> status; };      // one side round: the reads it ran, what came back, their statuses
static void p_splice(bool first, const char* name, int64_t n, const result_t& main_res, std::vector<int32_t> status, const std::vector<side_t>& rounds, const std::vector<int32_t>& given_up) {
    printf("%s{\"name\":\"%s\",\"n\":%lld,\"status_in\":[", first ? "" : ",", name, (long long)n);
    for (int64_t r = 0; r < n; ++r) printf("%s%d", r ? "," : "", status[(size_t)r]);
    printf("],"); p_result("main", main_res.recs, main_res.blob);
    vmx_splice sp; sp.begin(main_res.recs.data(), (int64_t)main_res.recs.size(), main_res.blob.data(), n, rounds.empty() ? given_up : rounds[0].sub);
    printf(",\"rounds\":[");
    for (size_t k = 0; k < rounds.size(); ++k) {
        const side_t& s = rounds[k];
        printf("%s{\"sub\":[", k ? "," : "");
        for (size_t j = 0; j < s.sub.size(); ++j) { printf("%s%d", j ? "," : "", s.sub[j]); status[(size_t)s.sub[j]] = s.status[j]; }
        printf("],\"status\":[");
        for (size_t j = 0; j < s.status.size(); ++j) printf("%s%d", j ? "," : "", s.status[j]);
        printf("],"); p_result("res", s.res.recs, s.res.blob); printf("}");
        sp.add_side(s.res.recs.data(), (int64_t)s.res.recs.size(), s.res.blob.data(), s.sub);
    }
    printf("],\"given_up\":[");
    for (size_t j = 0; j < given_up.size(); ++j) { printf("%s%d", j ? "," : "", given_up[j]); status[(size_t)given_up[j]] = VM_READ_CAPACITY; }
    printf("],");
    sp.finish();
    vm_batch_stats st; memset(&st, 0, sizeof st); st.n_records = 777; st.n_failed = 5; st.n_unmapped = 6; st.aligned_bases = 9; st.cigar_bytes = 11;      // stale values: counters() replaces them
    sp.counters(status, n, st);
    p_result("out", sp.all, sp.blob);
    printf(",\"counters\":{\"n_records\":%lld,\"aligned_bases\":%lld,\"cigar_bytes\":%lld,\"n_failed\":%lld,\"n_unmapped\":%lld}}", (long long)st.n_records, (long long)st.aligned_bases,
           (long long)st.cigar_bytes, (long long)st.n_failed, (long long)st.n_unmapped);
}

static void p_stats(const char* key, const vm_batch_stats& s) {
    printf("\"%s\":{\"ms_total\":%.17g,\"ms_stage\":[", key, s.ms_total);
    for (int i = 0; i < 16; ++i) printf("%s%.17g", i ? "," : "", s.ms_stage[i]);
    printf("],\"n_host_syncs\":%lld,\"n_ed_tier2\":%lld,\"n_ed_full\":%lld,\"n_local_anchors\":%lld,\"n_local_general\":%lld,\"n_ed_tier1\":%lld,\"n_dp_problems\":%lld,\"dp_cells\":%lld,\"n_dp_redo\":%lld,"
           "\"n_records\":%lld,\"ms_gapfill_fill\":%.17g,\"ms_gapfill_trace\":%.17g,\"n_gapfill_launches\":%lld,\"n_reads\":%lld}",
           (long long)s.n_host_syncs, (long long)s.n_ed_tier2, (long long)s.n_ed_full, (long long)s.n_local_anchors, (long long)s.n_local_general, (long long)s.n_ed_tier1, (long long)s.n_dp_problems,
           (long long)s.dp_cells, (long long)s.n_dp_redo, (long long)s.n_records, s.ms_gapfill_fill, s.ms_gapfill_trace, (long long)s.n_gapfill_launches, (long long)s.n_reads);
}
static vm_batch_stats stats_filled(int base) {      // every field named above gets a value of its own
    vm_batch_stats s; memset(&s, 0, sizeof s);
    s.ms_total = base + 0.5; for (int i = 0; i < 16; ++i) s.ms_stage[i] = base + i + 0.25;
    s.n_host_syncs = base + 1; s.n_ed_tier2 = base + 2; s.n_ed_full = base + 3; s.n_local_anchors = base + 4; s.n_local_general = base + 5; s.n_ed_tier1 = base + 6; s.n_dp_problems = base + 7;
    s.dp_cells = base + 8; s.n_dp_redo = base + 9; s.n_records = base + 10; s.ms_gapfill_fill = base + 11.5; s.ms_gapfill_trace = base + 12.5; s.n_gapfill_launches = base + 13; s.n_reads = base + 14;
    return s;
}

int main() {
    // ---- pool geometry
    printf("{\"geometry\":[");
    p_geo(true, 0, 1000, 1, 0, 1);                       // no local anchors: nothing
    p_geo(false, 0, 1000, 4, 7, 3);
    p_geo(false, 1, 100, 1, 0, 1);
    p_geo(false, 2, 100, 1, 0, 1); p_geo(false, 3, 100, 1, 0, 1);      // cl / 2 rounds down
    for (long long len : {0LL, 1LL, 3LL, 5LL, 7LL, 8LL, 9LL, 15LL, 16LL}) p_geo(false, 5, len, 1, 0, 1);      // the blob slice's 8-byte rounding: 3 len is 0, 1 and 7 mod 8 at len 0 / 8 / 16, 3, 5; len itself at 8, 9, 15
    for (int bit : {1, 2, 4}) { p_geo(false, 40, 5000, 1, bit, 1000000000LL); p_geo(false, 40, 5000, 1, bit, 7); }      // every mask bit, at the floor of 1 and above it
    p_geo(false, 40, 5000, 1, 7, 1000000000LL);
    p_geo(false, 40, 5000, 1, 8 | 16, 7);                // bits of the other pools leave a read's slices alone
    p_geo(false, 40, 5000, 4, 0, 1); p_geo(false, 40, 5000, 1024, 0, 1); p_geo(false, 40, 5000, 16, 4, 5);
    p_geo(false, 13056, 100000000, 1024, 0, 1);          // no 32-bit intermediate
    printf("],\"pool\":[");
    p_pool(true, 8, 1000 + 16, 1, 0, 1); p_pool(false, 8, 1000 + 16, 1, 8, 1000000000LL); p_pool(false, 8, 1000 + 16, 4, 8, 3); p_pool(false, 8, 1016, 1, 16, 3);
    p_pool(false, 16, 6 * 60000000LL + (1 << 20), 1, 0, 1); p_pool(false, 16, 6 * 60000000LL + (1 << 20), 1024, 16, 1000); p_pool(false, 16, 1 << 20, 1, 16, 1LL << 40);

    // ---- band-width rule
    printf("],\"start_pct\":[%d,%d,%d,%d,%d],\"packed\":[", vmx_ad_rule::start_pct(VM_MODE_H), vmx_ad_rule::start_pct(VM_MODE_L), vmx_ad_rule::start_pct(VM_MODE_S), vmx_ad_rule::start_pct(VM_MODE_R),
           vmx_ad_rule::start_pct(VM_MODE_ASM));
    { bool f = true; for (int p : {20, 40, 44, 45, 46, 90, 100}) { printf("%s[%d,%d]", f ? "" : ",", p, vmx_ad_rule::packed(p)); f = false; } }
    printf("],\"rule\":[");
    vmx_ad_rule r90; r90.pct = 90;
    p_rule(true, "too few problems to vote", r90, {{90, 1999, 1999}, {90, 0, 1999}});
    p_rule(false, "2000 problems vote", r90, {{90, 0, 2000}});
    p_rule(false, "f just below 0.01", r90, {{90, 99, 10000}});
    p_rule(false, "f at 0.01", r90, {{90, 100, 10000}});
    p_rule(false, "f just below 0.025", r90, {{90, 249, 10000}});
    p_rule(false, "f at 0.025", r90, {{90, 250, 10000}});
    p_rule(false, "f at 0.03", r90, {{90, 300, 10000}});
    p_rule(false, "f just above 0.03", r90, {{90, 301, 10000}});
    p_rule(false, "a stale vote", r90, {{80, 5000, 10000}, {100, 0, 10000}, {90, 0, 10000}, {90, 0, 10000}});
    vmx_ad_rule r95; r95.pct = 95;
    p_rule(false, "up stops at 100", r95, {{95, 5000, 10000}, {100, 5000, 10000}});
    vmx_ad_rule r100; r100.pct = 100;
    p_rule(false, "pinned at 100", r100, {{100, 5000, 10000}, {100, 5000, 10000}});
    vmx_ad_rule r100h; r100h.pct = 100; r100h.floor = 100; r100h.hold = 2;
    p_rule(false, "at 100 the hold still counts down", r100h, {{100, 5000, 10000}, {100, 5000, 10000}, {100, 5000, 10000}});
    vmx_ad_rule rf; rf.pct = 60; rf.floor = 60;
    p_rule(false, "at the floor", rf, {{60, 0, 10000}});
    vmx_ad_rule rf2; rf2.pct = 70; rf2.floor = 60;
    p_rule(false, "down stops at the floor", rf2, {{70, 0, 10000}, {60, 0, 10000}});
    vmx_ad_rule r30; r30.pct = 30;
    p_rule(false, "down stops at 20", r30, {{30, 0, 10000}, {20, 0, 10000}});
    {   // up at 50, then 256 quiet batches: the floor holds, comes back to 20 at the 256th, and the 257th steps down
        std::vector<vote_t> v; v.push_back({50, 400, 10000});
        for (int i = 0; i < 257; ++i) v.push_back({60, 0, 10000});
        vmx_ad_rule r50; r50.pct = 50;
        p_rule(false, "the 256-batch hold", r50, v);
    }
    {   // a second step up inside the hold starts it again
        vmx_ad_rule r50; r50.pct = 50;
        p_rule(false, "up inside the hold", r50, {{50, 400, 10000}, {60, 0, 10000}, {60, 400, 10000}, {70, 0, 10000}});
    }

    // ---- per-read status: pairs that differ in one input
    printf("],\"status\":[");
    vmx_status_in s = clean(); p_status(true, s);
    s = clean(); s.er_nrec = 0; p_status(false, s);                                                        // unmapped
    s = clean(); s.er_status = VM_READ_RAISED; s.er_nrec = 0; p_status(false, s);                          // failed, not unmapped
    s = clean(); s.er_status = VMX_POL_EXT_CAPACITY_DEV; p_status(false, s);
    s = clean(); s.er_status = VMX_POL_EXT_NEED_EXACT_DEV; p_status(false, s);
    for (int code : {(int)VMX_POL_READ_CAPACITY_DEV, (int)VMX_POL_READ_BANDFALL_DEV}) for (int fast = 0; fast < 2; ++fast) { s = clean(); s.er_status = code; s.fast_local = fast; p_status(false, s); }
    s = clean(); s.er_status = VMX_POL_EXT_CAPACITY_DEV; s.fast_local = true; p_status(false, s);          // the fast path leaves the extend stage's own codes alone
    for (int dp1 = 0; dp1 < 2; ++dp1) { s = clean(); s.er_redo = 1; s.er_pass = 1; s.do_pass1 = dp1; p_status(false, s); }      // asks for pass 1
    s = clean(); s.er_redo = 1; s.er_pass = 0; p_status(false, s); s = clean(); s.er_redo = 1; s.er_pass = 1; s.er_active = 0; p_status(false, s);
    s = clean(); s.er_redo = 1; s.er_pass = 1; s.er_status = VM_READ_RAISED; p_status(false, s);           // a status is not overwritten by the pass-1 ask
    for (long long r : {3LL, 4LL, 0LL}) { s = clean(); s.test_side_every = 2; s.r = r; p_status(false, s); }                     // the test hook
    s = clean(); s.test_side_every = 2; s.r = 4; s.force_exact = true; p_status(false, s);
    s = clean(); s.test_side_every = 2; s.r = 4; s.er_status = VM_READ_RAISED; p_status(false, s);
    for (long long na : {2LL, 3LL}) { s = clean(); s.gmax = -2; s.n_anchors = na; s.test_side_every = 1; p_status(false, s); }   // GC-fast's raise beats "run again"
    s = clean(); s.gmax = -4; s.er_status = VMX_POL_EXT_CAPACITY_DEV; p_status(false, s);                  // unsupported beats a short pool
    s = clean(); s.gmax = -4; s.asm_override = VM_READ_CAPACITY; p_status(false, s);                       // the tie-break's status beats unsupported
    s = clean(); s.gmax = -2; s.n_anchors = 3; s.asm_override = VM_READ_CAPACITY; p_status(false, s);
    for (int rm = 0; rm < 3; ++rm) for (long long na : {2LL, 3LL}) { s = clean(); s.rmode = rm; s.n_anchors = na; s.asm_override = rm == 1 ? (int)VM_READ_CAPACITY : 0; p_status(false, s); }      // mode R's raise beats everything

    // ---- splice of side batches
    printf("],\"splice\":[");
    {   // 3 reads, the middle one run again: its own record is dropped, its two side records take its place
        result_t m; add_rec(m, 0, "10M", 0, 10); add_rec(m, 0, "5M2D3M", 20, 28); add_rec(m, 1, "7M", 0, 7); add_rec(m, 2, "3M1I3M", 5, 12);
        side_t a; a.sub = {1}; a.status = {0}; add_rec(a.res, 0, "4M", 0, 4); add_rec(a.res, 0, "6M1I", 10, 17);
        p_splice(true, "middle read again", 3, m, {0, VMX_EXT_SHORT_INTERNAL, 0}, {a}, {});
    }
    {   // a side batch with zero records: the read is unmapped; another read of the batch failed
        result_t m; add_rec(m, 0, "10M", 0, 10);
        side_t a; a.sub = {1}; a.status = {0};
        p_splice(false, "side batch without records", 4, m, {0, VMX_EXT_EXACT_INTERNAL, VM_READ_RAISED, 0}, {a}, {});
    }
    {   // two side rounds: read 2 is still short after the first and delivers in the second; the main batch keeps nothing
        result_t m; add_rec(m, 0, "1M", 0, 1); add_rec(m, 2, "2M", 0, 2);
        side_t a; a.sub = {0, 2}; a.status = {0, VMX_EXT_SHORT_INTERNAL}; add_rec(a.res, 0, "11M", 0, 11); add_rec(a.res, 1, "9M", 0, 9);
        side_t b; b.sub = {2}; b.status = {0}; add_rec(b.res, 0, "12M", 1, 13); add_rec(b.res, 0, "13M", 20, 33);
        p_splice(false, "two side rounds", 3, m, {VMX_EXT_SHORT_INTERNAL, 0, VMX_EXT_SHORT_INTERNAL}, {a, b}, {});
    }
    {   // a read that could not be helped: no side round ran, the read is reported as VM_READ_CAPACITY
        result_t m; add_rec(m, 0, "10M", 0, 10); add_rec(m, 1, "8M", 0, 8);
        p_splice(false, "given up", 2, m, {0, VMX_EXT_SHORT_INTERNAL}, {}, {1});
    }

    // ---- statistics of a side batch, result-size guess
    printf("],\"stats_add\":{");
    { vm_batch_stats a = stats_filled(100), b = stats_filled(1000); p_stats("st", a); printf(","); p_stats("st2", b); vmx_stats_add_side(a, b); printf(","); p_stats("out", a); }
    printf("},\"guess\":[");
    struct { double rpr, bpb; int64_t n, bases, cS, cB; } G[] = {{0.0, 0.0, 100, 100000, 5000, 700000}, {0.0, 0.7, 100, 100000, 5000, 700000}, {1.25, 0.31, 100, 100000, 5000, 700000}, {1.25, 0.31, 100, 100000, 300, 700000},
                                                                 {1.25, 0.31, 100, 100000, 5000, 80000}, {3.0, 2.0, 4096, 60000000, 1LL << 40, 1LL << 40}};
    for (size_t i = 0; i < sizeof G / sizeof G[0]; ++i) {
        const vmx_res_guess g = vmx_result_guess(G[i].rpr, G[i].bpb, G[i].n, G[i].bases, G[i].cS, G[i].cB);
        printf("%s{\"in\":[%.17g,%.17g,%lld,%lld,%lld,%lld],\"out\":[%lld,%lld]}", i ? "," : "", G[i].rpr, G[i].bpb, (long long)G[i].n, (long long)G[i].bases, (long long)G[i].cS, (long long)G[i].cB, (long long)g.nr, (long long)g.nb);
    }
    printf("],\"learn\":[");
    struct { double rpr, bpb; int64_t nr, nb, n, bases; } Lr[] = {{0.0, 0.0, 120, 31000, 100, 100000}, {2.0, 0.5, 120, 31000, 100, 100000}, {1.0, 0.5, 120, 31000, 100, 100000}, {1.0, 0.2, 120, 31000, 0, 0}, {1.0, 0.2, 0, 0, 5, 0}};
    for (size_t i = 0; i < sizeof Lr / sizeof Lr[0]; ++i) {
        double a = Lr[i].rpr, b = Lr[i].bpb; vmx_result_learn(a, b, Lr[i].nr, Lr[i].nb, Lr[i].n, Lr[i].bases);
        printf("%s{\"in\":[%.17g,%.17g,%lld,%lld,%lld,%lld],\"out\":[%.17g,%.17g]}", i ? "," : "", Lr[i].rpr, Lr[i].bpb, (long long)Lr[i].nr, (long long)Lr[i].nb, (long long)Lr[i].n, (long long)Lr[i].bases, a, b);
    }
    printf("]}\n");
    return 0;
}
