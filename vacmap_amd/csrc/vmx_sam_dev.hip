// vmx_sam_dev.hip — host side of the device SAM emitter (kernels: k_sam.hip): vmx_sam_emit_dev works on device pointers only, vm_sam_emit_device_comments
// (and vm_sam_emit_device, the same without comments) is the C-ABI around it (validation, uploads through the context's upload helpers, the text's way back through the mailbox's page-locked landing
// block). Three host waits per call: the operator pass's sizes, the lines' sizes, the text. Under vm_sam_opts.keep_unmapped the per-read pass
// (k_sam_unmapped) runs beside k_sam_lines on both sides of wait 2 and adds no wait; it runs in a batch without records too.
// vm_paf_emit_device is the same call with k_paf_lines (k_paf.hip) in the place of k_sam_lines and k_sam_unmapped: the same three waits.
// Depth of coverage (vmx_depth.h): while an accumulator is attached to the context, each of these calls launches k_depth_add behind the write pass of
// k_sam_ops (no wait, no upload of its own); vm_depth_add_device is the call without line kernels and without text: two waits.
#include "vmx_depth.h"
#include "vmx_index_priv.h"

using namespace vmx;

vmx_sam_bufs* vmx_ctx_sam_bufs(vm_ctx* c) {
    if (!c->sbufs) c->sbufs = new vmx_sam_bufs();
    return c->sbufs;
}

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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

// the contig names of `mi` as one device blob, kept until the context meets another index
int contig_names(vm_ctx* c, vmx_sam_bufs* S, const vm_index* mi) {
    if (S->names_of == mi->serial && S->cnames.p) return 0;      // (by serial, not by address: a closed index's address is reused by the next one, with other names)
    S->h_cnames.clear(); S->h_cname_off.assign(1, 0);                    // (the host sources of the copies live as long as the device blob)
    for (const std::string& s : mi->names) { S->h_cnames += s; S->h_cname_off.push_back((int64_t)S->h_cnames.size()); }
    VMX_TRY(upload(S->cnames, S->h_cnames.data(), S->h_cnames.size(), c->stream));
    VMX_TRY(upload(S->cname_off, S->h_cname_off.data(), S->h_cname_off.size(), c->stream));
    S->names_of = mi->serial;
    return 0;
}

}  // namespace

int vmx_sam_emit_dev(vm_ctx* c, const vm_index* mi, vmx_sam_in A, vmx_sam_totals* tot, bool paf, vm_depth* dep, bool lines) {
    vmx_sam_bufs* S = vmx_ctx_sam_bufs(c);
    tot->text_bytes = 0; tot->n_lines = 0; tot->n_skipped = 0;
    const int64_t n = A.n_reads, m = A.n_recs, ns = vmx_sam_slots(A);    // reads, records, line slots
    const bool unm = A.keep_unmapped && n > 0;
    VMX_TRY(contig_names(c, S, mi));
    A.codes = mi->d_codes.as<const uint8_t>(); A.coff = mi->d_off.as<const int64_t>(); A.nseq = (int32_t)mi->names.size();
    A.cnames = S->cnames.as<const char>(); A.cname_off = S->cname_off.as<const int64_t>();
    VMX_TRY(S->cnt.reserve(8 * (size_t)(n + 1))); VMX_TRY(S->first.reserve(8 * (size_t)(n + 1))); VMX_TRY(S->rflag.reserve(4 * (size_t)(n + 1)));
    VMX_TRY(S->keep.reserve(4 * (size_t)(m + 1))); VMX_TRY(S->ord.reserve(4 * (size_t)(m + 1))); VMX_TRY(S->mq.reserve(4 * (size_t)(m + 1))); VMX_TRY(S->flag.reserve(4 * (size_t)(m + 1)));
    VMX_TRY(S->ri.reserve(sizeof(vmx_sam_rinfo) * (size_t)(m + 1)));
    VMX_TRY(S->tsz.reserve(8 * (size_t)(m + 1))); VMX_TRY(S->toff.reserve(8 * (size_t)(m + 1))); VMX_TRY(S->lsz.reserve(8 * (size_t)(ns + 1))); VMX_TRY(S->loff.reserve(8 * (size_t)(ns + 1)));
    VMX_TRY(S->res.reserve(64)); VMX_TRY(S->text_off.reserve(8 * (size_t)(n + 1))); VMX_TRY(S->scratch.reserve(16));
    if (paf) VMX_TRY(S->pinfo.reserve(24 * (size_t)(m + 1)));
    int64_t* pinfo = paf ? S->pinfo.as<int64_t>() : nullptr;
    const unsigned paf_grid = (unsigned)(m + (unm ? n : 0));                // PAF: record lines, then (keep_unmapped) the reads' own slots
    vmx_sam_work K{};
    K.cnt = S->cnt.as<int64_t>(); K.first = S->first.as<int64_t>(); K.keep = S->keep.as<int32_t>(); K.ord = S->ord.as<int32_t>(); K.mq = S->mq.as<int32_t>();
    K.flag = S->flag.as<int32_t>(); K.rflag = S->rflag.as<int32_t>(); K.ri = S->ri.as<vmx_sam_rinfo>(); K.tsz = S->tsz.as<int64_t>(); K.toff = S->toff.as<int64_t>();
    K.scratch = S->scratch.as<char>(); K.lsz = S->lsz.as<int64_t>(); K.loff = S->loff.as<int64_t>(); K.res = S->res.as<unsigned long long>();
    hipStream_t st = c->stream;
    VMX_HIP(hipMemsetAsync(K.cnt, 0, 8 * (size_t)(n + 1), st)); VMX_HIP(hipMemsetAsync(K.rflag, 0, 4 * (size_t)(n + 1), st)); VMX_HIP(hipMemsetAsync(K.res, 0, 64, st));
    VMX_HIP(hipMemsetAsync(K.tsz, 0, 8 * (size_t)(m + 1), st)); VMX_HIP(hipMemsetAsync(K.lsz, 0, 8 * (size_t)(ns + 1), st));
    if (m) hipLaunchKernelGGL(k_sam_count, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, A, K);
    VMX_TRY(vmx_scan64(c, S->tmp, K.cnt, K.first, (size_t)n + 1));
    unsigned long long h_res[3] = {0, 0, 0}; int64_t h_tot = 0;
    // (a record that names no read or no contig is found by k_sam_count; the kernels below see its flag and do nothing)
    if (m) hipLaunchKernelGGL(k_sam_order, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, A, K);
    if (m) hipLaunchKernelGGL(k_sam_ops, dim3((unsigned)m), dim3(64), 0, st, A, K, 0);
    VMX_TRY(launched("k_sam_ops (sizes)"));
    VMX_TRY(vmx_scan64(c, S->tmp, K.tsz, K.toff, (size_t)m + 1));
    VMX_TRY(vmx_fetch(c, &h_tot, K.toff + m, 1)); VMX_TRY(vmx_fetch(c, h_res, K.res, 1));
    VMX_TRY(wait(c));                                                    // wait 1: the operator pass's sizes
    if (h_res[0] & VMX_SAM_E_RECORD) { set_error(std::string(!lines ? "vm_depth_add_device" : paf ? "vm_paf_emit_device" : "vm_sam_emit_device") + ": a record names no read or no contig, lies outside the CIGAR blob, or the records are not ordered by read"); return VM_ERR_ARG; }
    if (h_res[0] & VMX_SAM_E_COUNT) { set_error(std::string(!lines ? "vm_depth_add_device" : paf ? "vm_paf_emit_device" : "vm_sam_emit_device") + ": a CIGAR operator count of 2^31 or more"); return VM_ERR_ARG; }
    VMX_TRY(S->scratch.reserve((size_t)h_tot + 16));
    K.scratch = S->scratch.as<char>();
    if (m) hipLaunchKernelGGL(k_sam_ops, dim3((unsigned)m), dim3(64), 0, st, A, K, 1);
    if (!lines) {}
    else if (paf) { if (paf_grid) hipLaunchKernelGGL(k_paf_lines, dim3(paf_grid), dim3(64), 0, st, A, K, pinfo, (char*)nullptr, 0); }
    else {
        if (m) hipLaunchKernelGGL(k_sam_lines, dim3((unsigned)m), dim3(64), 0, st, A, K, (char*)nullptr, 0);
        if (unm) hipLaunchKernelGGL(k_sam_unmapped, dim3((unsigned)n), dim3(64), 0, st, A, K, (char*)nullptr, 0);      // (rflag: the size pass of k_sam_ops, before wait 1)
    }
    VMX_TRY(launched("k_sam_lines (sizes)"));
    VMX_TRY(vmx_scan64(c, S->tmp, K.lsz, K.loff, (size_t)ns + 1));
    hipLaunchKernelGGL(k_sam_text_off, dim3((unsigned)((n + 1 + 255) / 256)), dim3(256), 0, st, A, K, S->text_off.as<int64_t>());
    VMX_TRY(vmx_fetch(c, &h_tot, K.loff + ns, 1)); VMX_TRY(vmx_fetch(c, h_res, K.res, 3));
    VMX_TRY(wait(c));                                                    // wait 2: the lines' sizes
    VMX_TRY(S->text.reserve((size_t)h_tot + 16));
    // depth: queued once nothing but the runtime can fail the call any more; it reads what k_sam_order and both passes of k_sam_ops stored
    if (dep && m) hipLaunchKernelGGL(k_depth_add, dim3((unsigned)m), dim3(64), 0, st, A, K, dep->dev());
    if (!lines) {}
    else if (paf) { if (paf_grid) hipLaunchKernelGGL(k_paf_lines, dim3(paf_grid), dim3(64), 0, st, A, K, pinfo, S->text.as<char>(), 1); }
    else {
        if (m) hipLaunchKernelGGL(k_sam_lines, dim3((unsigned)m), dim3(64), 0, st, A, K, S->text.as<char>(), 1);
        if (unm) hipLaunchKernelGGL(k_sam_unmapped, dim3((unsigned)n), dim3(64), 0, st, A, K, S->text.as<char>(), 1);
    }
    VMX_TRY(launched("k_sam_lines"));
    tot->text_bytes = h_tot; tot->n_lines = (int64_t)h_res[1]; tot->n_skipped = (int64_t)h_res[2];
    return 0;
}

// vm_sam_emit_device_comments (kind 0), vm_paf_emit_device (kind 1: no qualities, no comments, no RG) and vm_depth_add_device (kind 2: as kind 1, adds
// to dep, no lines and no text): validation, uploads, the passes, the text's way back. Kinds 0 and 1 add to the context's attached accumulator.
static int emit_device(const int kind, vm_depth* dep, vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const char* quals, const int64_t* qual_off, const char* comments, const int64_t* com_off, const vm_record* recs,
                       int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped);

extern "C" {

int vm_paf_emit_device(vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text, int64_t** text_off,
                       int64_t* n_lines, int64_t* n_skipped) {
    return emit_device(1, nullptr, c, mi, o, n_reads, names, name_off, seqs, seq_off, nullptr, nullptr, nullptr, nullptr, recs, n_recs, cigar_blob, status, text, text_off, n_lines,
                       n_skipped);
}

int vm_depth_add_device(vm_depth* d, vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                        const int64_t* seq_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob, const int32_t* status, int64_t* n_lines, int64_t* n_skipped) {
    if (!d) { set_error("vm_depth_add_device: no accumulator"); return VM_ERR_ARG; }
    return emit_device(2, d, c, mi, o, n_reads, names, name_off, seqs, seq_off, nullptr, nullptr, nullptr, nullptr, recs, n_recs, cigar_blob, status, nullptr, nullptr, n_lines,
                       n_skipped);
}

int vm_ctx_attach_depth(vm_ctx* c, vm_depth* d) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (d && d->ctx != c) { set_error("vm_ctx_attach_depth: the accumulator was not made on this context"); return VM_ERR_ARG; }
    c->depth = d;
    return VM_OK;
}

int vm_sam_emit_device(vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const char* quals, const int64_t* qual_off, const vm_record* recs, int64_t n_recs, const char* cigar_blob,
                       const int32_t* status, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped) {
    return vm_sam_emit_device_comments(c, mi, o, n_reads, names, name_off, seqs, seq_off, quals, qual_off, nullptr, nullptr, recs, n_recs, cigar_blob, status, text, text_off,
                                       n_lines, n_skipped);
}

int vm_sam_emit_device_comments(vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                                const int64_t* seq_off, const char* quals, const int64_t* qual_off, const char* comments, const int64_t* com_off, const vm_record* recs,
                                int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped) {
    return emit_device(0, nullptr, c, mi, o, n_reads, names, name_off, seqs, seq_off, quals, qual_off, comments, com_off, recs, n_recs, cigar_blob, status, text, text_off, n_lines,
                       n_skipped);
}

}  // extern "C"

static int emit_device(const int kind, vm_depth* dep, vm_ctx* c, const vm_index* mi, const vm_sam_opts* o, int64_t n_reads, const char* names, const int64_t* name_off, const char* seqs,
                       const int64_t* seq_off, const char* quals, const int64_t* qual_off, const char* comments, const int64_t* com_off, const vm_record* recs,
                       int64_t n_recs, const char* cigar_blob, const int32_t* status, char** text, int64_t** text_off, int64_t* n_lines, int64_t* n_skipped) {
    const bool paf = kind != 0, lines = kind != 2;
    const std::string who = kind == 2 ? "vm_depth_add_device" : paf ? "vm_paf_emit_device" : "vm_sam_emit_device";
    char* no_text = nullptr; int64_t* no_off = nullptr;
    if (!lines) { text = &no_text; text_off = &no_off; }
    if (text) *text = nullptr;
    if (text_off) *text_off = nullptr;
    if (n_lines) *n_lines = 0;
    if (n_skipped) *n_skipped = 0;
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (lines) dep = c->depth;
    if (!mi || !o || !text || !text_off || !n_lines || !n_skipped || n_reads < 0 || n_recs < 0 || !name_off || !seq_off || (n_recs && (!recs || !cigar_blob))) { set_error(who + ": bad arguments"); return VM_ERR_ARG; }
    if (mi->has_host_seq && mi->n_other_letters > 0) {
        set_error(who + ": the reference holds " + std::to_string(mi->n_other_letters) + " letters other than ACGTN, which only the host emitter (" + (paf ? "vm_paf_emit" : "vm_sam_emit") + ") prints");
        return VM_ERR_UNSUPPORTED;
    }
    if (dep && (dep->ctx != c || dep->index_serial != mi->serial)) {
        set_error(who + ": the depth accumulator was made " + (dep->ctx != c ? "on another context (or in host memory)" : "for another index")); return VM_ERR_ARG;
    }
    // recs as vm_sam_emit validates them, and what keeps the kernels inside the blobs
    int64_t cig_len = 0;
    for (int64_t i = 0; i < n_recs; ++i) {
        const vm_record& r = recs[i];
        if (r.read_idx < 0 || r.read_idx >= n_reads) { set_error("vm_sam_emit: record of an unknown read"); return VM_ERR_ARG; }
        if (i && r.read_idx < recs[i - 1].read_idx) { set_error("vm_sam_emit: records must be ordered by read"); return VM_ERR_ARG; }
        if (r.contig < 0 || r.contig >= (int64_t)mi->names.size() || r.cigar_off < 0 || r.cigar_len < 0) { set_error(who + ": record of an unknown contig or with a negative CIGAR range"); return VM_ERR_ARG; }
        cig_len = std::max(cig_len, r.cigar_off + r.cigar_len);
    }
    auto range = [&](const int64_t* off, int64_t* lo, int64_t* hi) -> bool {      // the bytes of a blob its offsets use
        *lo = n_reads ? off[0] : 0; *hi = *lo;
        for (int64_t r = 0; r < n_reads; ++r) { if (off[r] < 0 || off[r + 1] < off[r]) return false; *lo = std::min(*lo, off[r]); *hi = std::max(*hi, off[r + 1]); }
        return true;
    };
    int64_t nlo, nhi, slo, shi, qlo = 0, qhi = 0, clo = 0, chi = 0;
    const bool with_q = quals && qual_off;
    if (!range(name_off, &nlo, &nhi) || !range(seq_off, &slo, &shi) || (with_q && !range(qual_off, &qlo, &qhi)) || (com_off && !range(com_off, &clo, &chi))) { set_error(who + ": offsets must not decrease"); return VM_ERR_ARG; }
    if ((nhi > nlo && !names) || (shi > slo && !seqs) || (chi > clo && !comments)) { set_error(who + ": bad arguments"); return VM_ERR_ARG; }
    const bool with_c = comments && com_off && chi > clo;                // (no comment byte at all: the run is the one without comments)
    VMX_HIP(hipSetDevice(c->device));
    vmx_fetch_scope fs(c);
    vmx_sam_bufs* S = vmx_ctx_sam_bufs(c);
    const double t0 = now_s();
    hipStream_t st = c->stream;
    VMX_TRY(upload(S->names, names ? names + nlo : names, (size_t)(nhi - nlo), st)); VMX_TRY(upload(S->name_off, name_off, (size_t)n_reads + 1, st));
    VMX_TRY(upload(S->seqs, seqs ? seqs + slo : seqs, (size_t)(shi - slo), st)); VMX_TRY(upload(S->seq_off, seq_off, (size_t)n_reads + 1, st));
    if (with_q) { VMX_TRY(upload(S->quals, quals + qlo, (size_t)(qhi - qlo), st)); VMX_TRY(upload(S->qual_off, qual_off, (size_t)n_reads + 1, st)); }
    if (with_c) { VMX_TRY(upload(S->comments, comments + clo, (size_t)(chi - clo), st)); VMX_TRY(upload(S->com_off, com_off, (size_t)n_reads + 1, st)); }
    VMX_TRY(upload(S->recs, recs, (size_t)n_recs, st)); VMX_TRY(upload(S->cigars, cigar_blob, (size_t)cig_len, st));
    if (status) VMX_TRY(upload(S->status, status, (size_t)n_reads, st));
    const size_t rg_len = (o->rg_id && !paf) ? strlen(o->rg_id) : 0;                  // (a PAF line carries no RG)
    if (o->rg_id && !paf) VMX_TRY(upload(S->rg, o->rg_id, rg_len, st));
    vmx_sam_in A{};
    A.n_reads = n_reads; A.n_recs = n_recs;
    A.names = S->names.as<const char>(); A.name_off = S->name_off.as<const int64_t>(); A.name_base = nlo;
    A.seqs = S->seqs.as<const char>(); A.seq_off = S->seq_off.as<const int64_t>(); A.seq_base = slo;
    A.quals = with_q ? S->quals.as<const char>() : nullptr; A.qual_off = with_q ? S->qual_off.as<const int64_t>() : nullptr; A.qual_base = qlo;
    A.comments = with_c ? S->comments.as<const char>() : nullptr; A.com_off = with_c ? S->com_off.as<const int64_t>() : nullptr; A.com_base = clo;
    A.recs = S->recs.as<const vm_record>(); A.cigars = S->cigars.as<const char>(); A.cigars_len = cig_len;
    A.status = status ? S->status.as<const int32_t>() : nullptr;
    A.md = o->md; A.shortcs = o->shortcs; A.cigar2cg = o->cigar2cg; A.markunbalancetra = o->markunbalancetra; A.hardclip = o->hardclip; A.fakecigar = o->fakecigar; A.asm_mode = o->asm_mode; A.keep_unmapped = o->keep_unmapped ? 1 : 0;
    A.rg = (o->rg_id && !paf) ? S->rg.as<const char>() : nullptr; A.rg_len = (int32_t)rg_len;
    const double t1 = now_s();
    vmx_sam_totals tot;
    VMX_TRY(vmx_sam_emit_dev(c, mi, A, &tot, paf, dep, lines));
    if (!lines) { *n_lines = tot.n_lines; *n_skipped = tot.n_skipped; return VM_OK; }      // (the counts stay on the device; nothing to fetch)
    char* h_text = (char*)malloc((size_t)tot.text_bytes + 1); int64_t* h_off = (int64_t*)malloc(8 * ((size_t)n_reads + 1));
    if (!h_text || !h_off) { free(h_text); free(h_off); set_error("out of host memory"); return VM_ERR_OOM; }
    int rc = vmx_fetch(c, h_off, S->text_off.p, (size_t)n_reads + 1);
    if (rc >= 0) rc = vmx_fetch(c, h_text, S->text.p, (size_t)tot.text_bytes);
    const double t2 = now_s();
    if (rc >= 0) rc = wait(c);                                           // wait 3: the text
    if (rc < 0) { free(h_text); free(h_off); return rc; }
    h_text[tot.text_bytes] = 0;
    S->s_upload = t1 - t0; S->s_kernel = t2 - t1; S->s_download = now_s() - t2;
    *text = h_text; *text_off = h_off; *n_lines = tot.n_lines; *n_skipped = tot.n_skipped;
    return VM_OK;
}

extern "C" {

// wall seconds of the context's last vm_sam_emit_device call: upload (validation included), the passes up to the last launch (two waits), the text's way back
int vm_sam_emit_device_times(vm_ctx* c, double* out3) {
    if (!c) { set_error("no context"); return VM_ERR_NO_CTX; }
    if (!out3) return VM_ERR_ARG;
    vmx_sam_bufs* S = vmx_ctx_sam_bufs(c);
    out3[0] = S->s_upload; out3[1] = S->s_kernel; out3[2] = S->s_download;
    return VM_OK;
}

}  // extern "C"
