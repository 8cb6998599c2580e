"""ctypes binding of libvacmapx.so (include/vacmapx.h) — the reference-side binding a VACmap maintainer would add.

`load()` opens the in-tree HIP library (built by vacmap_amd/build.py for gfx950). There is no fallback: a missing library
raises, and without a GPU `Context()` raises VmxError(VM_ERR_NO_DEVICE).
"""
import ctypes as C
import os
import weakref
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_SO = os.environ.get('VACMAPX_LIB') or os.path.join(_HERE, 'libvacmapx.so')     # VACMAPX_LIB: another build of the same library (tuning variants)

VM_ERR_NO_DEVICE = -2
MODES = {'H': 0, 'L': 1, 'S': 2, 'R': 3, 'asm': 4}


class VmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('vacmapx error %d: %s' % (code, msg))
        self.code = code


class Params(C.Structure):
    _fields_ = [('mode', C.c_int32), ('check_num', C.c_int32), ('mid_occ', C.c_int32), ('global_maxdiff', C.c_int32),
                ('local_maxdiff', C.c_int32), ('local_kmersize', C.c_int32), ('eqx', C.c_int32), ('hardclip', C.c_int32),
                ('nodiscard', C.c_int32), ('reserved', C.c_int32), ('global_skipcost', C.c_double),
                ('local_skipcost', C.c_double), ('maxdivergence', C.c_double)]


class Score(C.Structure):
    _fields_ = [('match', C.c_int32), ('mismatch', C.c_int32), ('o1', C.c_int32), ('e1', C.c_int32), ('o2', C.c_int32), ('e2', C.c_int32)]


class CigarOut(C.Structure):
    _fields_ = [('cigar', C.c_void_p), ('q_e', C.c_int32), ('t_e', C.c_int32), ('score', C.c_int32)]


class ChainsOut(C.Structure):
    _fields_ = [('need_reverse', C.POINTER(C.c_int32)), ('mapq', C.POINTER(C.c_int32)), ('score', C.POINTER(C.c_double)),
                ('fast_used', C.POINTER(C.c_int32)), ('read_path_off', C.POINTER(C.c_int64)), ('path_off', C.POINTER(C.c_int64)),
                ('path_anchors', C.POINTER(C.c_int64)), ('S', C.POINTER(C.c_double)), ('P', C.POINTER(C.c_int64)),
                ('S_arg', C.POINTER(C.c_int64)), ('gmax', C.POINTER(C.c_int64)), ('opcount', C.POINTER(C.c_int64))]


class LinkedOut(C.Structure):
    _fields_ = [('gmax', C.c_int64), ('n_hot', C.c_int64), ('n_cold', C.c_int64), ('opcount', C.c_int64), ('cold_max', C.c_double),
                ('S', C.POINTER(C.c_double)), ('P', C.POINTER(C.c_int64)), ('S_arg_hot', C.POINTER(C.c_int64)),
                ('carry_status', C.c_int32), ('saved', C.c_int32), ('n_carry', C.c_int64), ('carry_S', C.POINTER(C.c_double)),
                ('carry_P', C.POINTER(C.c_int64)), ('carry_rows', C.POINTER(C.c_int64)), ('carry_g_max_scores', C.c_double), ('carry_prereadloc', C.c_int64)]


class LocalOut(C.Structure):
    _fields_ = [('status', C.POINTER(C.c_int32)), ('variant', C.POINTER(C.c_int32)), ('score', C.POINTER(C.c_double)),
                ('chain_off', C.POINTER(C.c_int64)), ('chain', C.POINTER(C.c_int64)), ('raw_off', C.POINTER(C.c_int64)),
                ('raw', C.POINTER(C.c_int64))]


class LocalDpOut(C.Structure):
    _fields_ = [('status', C.POINTER(C.c_int32)), ('variant', C.POINTER(C.c_int32)), ('fast_used', C.POINTER(C.c_int32)), ('sp_valid', C.POINTER(C.c_int32)),
                ('score', C.POINTER(C.c_double)), ('chain_off', C.POINTER(C.c_int64)), ('chain', C.POINTER(C.c_int64)), ('S', C.POINTER(C.c_double)),
                ('P', C.POINTER(C.c_int64))]


LOCAL_DP_WANT_SP, LOCAL_DP_DEVICE_LIST = 1, 2          # vm_local_dp_batch's flag bits


class Record(C.Structure):
    _fields_ = [('read_idx', C.c_int32), ('contig', C.c_int32), ('strand', C.c_int32), ('mapq', C.c_int32),
                ('q_st', C.c_int64), ('q_en', C.c_int64), ('r_st', C.c_int64), ('r_en', C.c_int64),
                ('cigar_off', C.c_int64), ('cigar_len', C.c_int64)]


class SamOpts(C.Structure):
    _fields_ = [('md', C.c_int32), ('shortcs', C.c_int32), ('cigar2cg', C.c_int32), ('markunbalancetra', C.c_int32), ('hardclip', C.c_int32),
                ('fakecigar', C.c_int32), ('rg_id', C.c_char_p), ('asm_mode', C.c_int32), ('keep_unmapped', C.c_int32)]


class BatchStats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ('n_reads', 'read_bases', 'n_minimizers', 'n_hits', 'n_anchors', 'n_local_hits', 'n_local_anchors',
                                          'n_segments', 'n_ed_problems', 'ed_cells', 'n_ext_problems', 'ext_cells', 'n_dp_problems',
                                          'dp_cells', 'n_records', 'cigar_bytes', 'aligned_bases', 'n_unmapped', 'n_failed',
                                          'dp_string_bytes')] + \
               [('ms_total', C.c_double), ('ms_stage', C.c_double * 16), ('ms_gapfill_fill', C.c_double), ('ms_gapfill_trace', C.c_double),
                ('n_gapfill_launches', C.c_int64), ('n_ed_full', C.c_int64), ('n_ed_tier2', C.c_int64), ('n_ed_tier1', C.c_int64),
                ('n_dp_redo', C.c_int64), ('dp_redo_tb_bytes', C.c_int64), ('ms_local_seed', C.c_double), ('ms_cluster', C.c_double), ('n_host_syncs', C.c_int64), ('n_local_general', C.c_int64), ('n_ext_retries', C.c_int64), ('n_batch_retries', C.c_int64),
                ('n_dp_redo_wide', C.c_int64), ('n_dp_redo_full', C.c_int64)]


def _b(s):
    return s if isinstance(s, (bytes, bytearray)) else s.encode()


def _cat(seqs):
    bs = [_b(s) for s in seqs]
    off = np.zeros(len(bs) + 1, np.int64)
    if bs:
        off[1:] = np.cumsum([len(b) for b in bs])
    return b''.join(bs), off


def _seq_ptrs(seqs):
    """contig sequences as (keep-alive objects, char** argument, int64 lengths) without copying uint8 NumPy arrays (a 3.1 Gb
    reference is handed over in place); str / bytes are accepted too"""
    keep, ptrs, lens = [], [], []
    for x in seqs:
        if isinstance(x, np.ndarray):
            a = np.ascontiguousarray(x, dtype=np.uint8)
            keep.append(a); ptrs.append(a.ctypes.data); lens.append(a.size)
        else:
            b = C.create_string_buffer(_b(x), len(x)) if len(x) else C.create_string_buffer(1)
            keep.append(b); ptrs.append(C.addressof(b)); lens.append(len(x))
    n = len(ptrs)
    arr = (C.c_void_p * max(n, 1))(*ptrs)
    return keep, C.cast(arr, C.POINTER(C.c_char_p)), (C.c_int64 * max(n, 1))(*lens)


class VmxLib:
    """Thin typed view of the C-ABI. `path` defaults to the in-tree libvacmapx.so."""

    def __init__(self, path=None):
        path = path or DEFAULT_SO
        try:        # one HIP runtime per process: torch bundles its own libamdhip64, and whichever copy is loaded first serves both. Load
            if os.environ.get('VACMAPX_SKIP_TORCH') == '1' and 'torch' not in __import__('sys').modules:
                raise ImportError('single-GPU command line: no torch, the library brings the system HIP runtime (saves ~1.5 s of start-up)')
            import torch  # noqa: F401   torch's before this library so that vacmap_amd.dist (RCCL broadcast of the HBM-resident index) works
        except ImportError:               # whatever the import order of the caller; without torch there is simply no multi-GPU plumbing
            pass
        if not os.path.exists(path):
            raise FileNotFoundError('%s not built: run `python -m vacmap_amd.build` (hipcc, gfx950). No fallback exists.' % path)
        L = self.L = C.CDLL(path)
        vp, i32, i64, dbl, cp, P = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_char_p, C.POINTER
        L.vm_last_error.restype = cp
        L.vm_version.restype = cp
        L.vm_free.argtypes = [vp]
        L.vm_params_default.argtypes = [P(Params), C.c_int]
        L.vm_ctx_create.argtypes = [C.c_int, P(vp)]
        L.vm_ctx_destroy.argtypes = [vp]
        L.vm_ctx_set_inflight.argtypes = [vp, C.c_int]
        L.vm_ctx_set_blocking_sync.argtypes = [vp, C.c_int]
        L.vm_debug_chain_counters.argtypes = [C.c_int, C.POINTER(C.c_ulonglong)]
        L.vm_ctx_mem_info.argtypes = [vp, P(i64), P(i64)]
        L.vm_table.argtypes = [vp, C.c_int, P(vp)]; L.vm_table.restype = i64
        L.vm_edit_distance_batch.argtypes = [vp, i64, cp, vp, cp, vp, P(P(i64))]
        L.vm_edit_distance_bound_batch.argtypes = [vp, C.c_int, i64, cp, vp, cp, vp, P(P(i64))]
        L.vm_edit_distance.argtypes = [vp, cp, i64, cp, i64]; L.vm_edit_distance.restype = i64
        L.vm_k_extend_batch.argtypes = [vp] + [C.c_int] * 6 + [i64, cp, vp, cp, vp, P(P(i32)), P(P(i32)), P(P(i32))]
        L.vm_k_cigar_batch.argtypes = [vp, P(Score), C.c_int, i64, cp, vp, cp, vp, P(vp), P(P(i64)), P(P(i32))]
        L.vm_k_cigar.argtypes = [vp, cp, i64, cp, i64, P(Score), C.c_int, C.c_int, C.c_int, P(CigarOut)]
        L.vm_k_cigar_batch_banded.argtypes = [vp, P(Score), C.c_int, i64, cp, vp, cp, vp, P(vp), P(P(i64)), P(P(i32)), vp]
        L.vm_chain_global_batch.argtypes = [vp, P(Params), C.c_int, i64, vp, vp, vp, C.c_int, P(ChainsOut)]
        L.vm_chain_linked.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, i64, vp, i64, vp, vp, C.c_double, i64, i64, P(LinkedOut)]
        L.vm_linked_out_free.argtypes = [P(LinkedOut)]
        L.vm_align_asm.argtypes = [vp, vp, P(Params), C.c_char_p, i64, i64, i64, i64, P(P(Record)), P(i64), P(vp), P(C.c_int32)]
        L.vm_chains_out_free.argtypes = [P(ChainsOut)]
        L.vm_index_build_fasta.argtypes = [vp, cp, C.c_int, C.c_int, P(vp)]
        L.vm_index_build_fasta_device.argtypes = [vp, cp, C.c_int, C.c_int, P(vp), P(dbl), C.c_int]
        L.vm_index_build_fasta_device_opts.argtypes = [vp, cp, C.c_int, C.c_int, C.c_int, P(vp), P(dbl), C.c_int]
        L.vm_index_build_mem.argtypes = [vp, C.c_int, P(cp), P(cp), P(i64), C.c_int, C.c_int, P(vp)]
        L.vm_index_save.argtypes = [vp, cp]; L.vm_index_load.argtypes = [vp, cp, P(vp)]
        L.vm_index_save_mmi.argtypes = [vp, cp, C.c_int]; L.vm_index_load_mmi.argtypes = [vp, cp, P(vp)]
        L.vm_index_free.argtypes = [vp]
        for f in ('vm_index_k', 'vm_index_w', 'vm_index_nseq', 'vm_index_mid_occ', 'vm_index_blob_count'):
            getattr(L, f).argtypes = [vp]
        L.vm_index_n_minimizers.argtypes = [vp]; L.vm_index_n_minimizers.restype = i64
        L.vm_index_n_distinct.argtypes = [vp]; L.vm_index_n_distinct.restype = i64
        L.vm_index_seq_info.argtypes = [vp, C.c_int, P(cp), P(i64), P(i64)]
        L.vm_index_seq.argtypes = [vp, C.c_int, i64, i64, vp]; L.vm_index_seq.restype = i64
        L.vm_index_minimizers.argtypes = [vp, P(P(C.c_uint64)), P(P(C.c_uint64)), P(i64)]
        L.vm_index_blob.argtypes = [vp, C.c_int, P(vp), P(i64)]
        L.vm_index_meta_size.argtypes = [vp, P(i64)]; L.vm_index_meta_get.argtypes = [vp, vp, i64]
        L.vm_index_from_meta.argtypes = [vp, vp, i64, P(vp)]
        L.vm_sketch_batch.argtypes = [vp, C.c_int, C.c_int, i64, cp, vp, P(P(C.c_uint64)), P(P(i32)), P(P(C.c_int8)), P(P(i64))]
        L.vm_map_batch.argtypes = [vp, vp, C.c_int, C.c_int, i64, cp, vp, P(P(i64)), P(P(i64))]
        L.vm_map.argtypes = [vp, vp, cp, i64, C.c_int, C.c_int, P(P(i64)), P(i64)]
        L.vm_local_chain_batch.argtypes = [vp, vp, P(Params), i64, cp, vp, vp, vp, vp, P(LocalOut)]
        L.vm_local_out_free.argtypes = [P(LocalOut)]
        L.vm_local_dp_batch.argtypes = [vp, P(Params), i64, vp, vp, vp, vp, C.c_int, P(LocalDpOut)]
        L.vm_local_dp_out_free.argtypes = [P(LocalDpOut)]
        L.vm_align_batch.argtypes = [vp, vp, P(Params), i64, cp, vp, P(P(Record)), P(i64), P(vp), vp, P(BatchStats)]
        L.vm_align_trace.argtypes = [vp, vp, P(Params), i64, cp, vp, C.c_int, P(P(i64)), P(P(i64))]
        L.vm_sam_emit.argtypes = [vp, P(SamOpts), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, C.c_int, P(vp), P(P(i64)), P(i64), P(i64)]
        L.vm_sam_emit_device.argtypes = [vp, vp, P(SamOpts), i64, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, P(vp), P(P(i64)), P(i64), P(i64)]
        L.vm_sam_emit_device_comments.argtypes = [vp, vp, P(SamOpts), i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, P(vp), P(P(i64)), P(i64), P(i64)]
        L.vm_sam_emit_device_times.argtypes = [vp, P(dbl)]
        L.vm_paf_emit.argtypes = [vp, P(SamOpts), i64, vp, vp, vp, vp, vp, i64, vp, vp, C.c_int, P(vp), P(P(i64)), P(i64), P(i64)]
        L.vm_paf_emit_device.argtypes = [vp, vp, P(SamOpts), i64, vp, vp, vp, vp, vp, i64, vp, vp, P(vp), P(P(i64)), P(i64), P(i64)]
        L.vm_depth_create.argtypes = [vp, vp, i64, C.c_int, P(vp)]
        L.vm_depth_free.argtypes = [vp]; L.vm_depth_free.restype = None
        L.vm_depth_add.argtypes = [vp, vp, P(SamOpts), i64, vp, vp, vp, vp, vp, i64, vp, vp, C.c_int, P(i64), P(i64)]
        L.vm_depth_add_device.argtypes = [vp, vp, vp, P(SamOpts), i64, vp, vp, vp, vp, vp, i64, vp, vp, P(i64), P(i64)]
        L.vm_ctx_attach_depth.argtypes = [vp, vp]
        L.vm_depth_merge.argtypes = [vp, vp]
        L.vm_depth_add_counts.argtypes = [vp, vp, i64]
        L.vm_depth_counts.argtypes = [vp, P(P(i64)), P(P(i64)), P(i64)]
        L.vm_depth_text.argtypes = [vp, C.c_int, P(vp), P(i64)]
        L.vm_blob_gather.argtypes = [vp, vp, vp, i64, vp, vp]; L.vm_blob_gather.restype = i64
        L.vm_blob_write_parts.argtypes = [C.c_int, vp, vp, vp, vp, i64]; L.vm_blob_write_parts.restype = i64
        L.vm_pinned_alloc.argtypes = [i64, C.c_int]; L.vm_pinned_alloc.restype = vp
        L.vm_pinned_free.argtypes = [vp]; L.vm_pinned_free.restype = None
        L.vm_blob_gather_parts.argtypes = [vp, vp, vp, vp, i64, vp]; L.vm_blob_gather_parts.restype = i64
        L.vm_blob_write_parts_mmap.argtypes = [C.c_int, i64, vp, vp, vp, vp, i64, C.c_int]; L.vm_blob_write_parts_mmap.restype = i64
        L.vm_fastx_open.argtypes = [cp, P(vp)]; L.vm_fastx_close.argtypes = [vp]; L.vm_fastx_open_range.argtypes = [cp, i64, i64, P(vp)]
        L.vm_fastx_read.argtypes = [vp, i64, i64] + [P(vp), P(P(i64))] * 4; L.vm_fastx_read.restype = i64
        L.vm_reads_upload.argtypes = [vp, i64, cp, vp, P(vp)]
        L.vm_reads_free.argtypes = [vp]
        L.vm_reads_reupload.argtypes = [vp, vp, i64, vp, vp]
        L.vm_align_resident.argtypes = [vp, vp, P(Params), vp, P(P(Record)), P(i64), P(vp), vp, P(BatchStats)]
        L.vm_bam_writer_create.argtypes = [vp, cp, i64, P(vp)]
        L.vm_bam_writer_free.argtypes = [vp]; L.vm_bam_writer_free.restype = None
        L.vm_bam_header.argtypes = [vp, P(vp), P(i64)]
        L.vm_bam_encode.argtypes = [vp, cp, i64, P(vp), P(i64)]
        L.vm_bam_compress_parts.argtypes = [vp, vp, vp, vp, vp, i64, P(vp), P(i64)]
        L.vm_bam_sorter_create.argtypes = [vp, i64, P(vp)]
        L.vm_bam_sorter_free.argtypes = [vp]; L.vm_bam_sorter_free.restype = None
        L.vm_bam_sorter_add_parts.argtypes = [vp, vp, vp, vp, vp, i64, P(vp), P(i64)]
        L.vm_bam_sorter_plan.argtypes = [vp, vp, i64, i64, P(i64)]
        L.vm_bam_sorter_chunk.argtypes = [vp, i64, P(vp), P(i64)]
        L.vm_bam_sorter_index.argtypes = [vp, P(vp), P(i64)]
        L.vm_bgzf_compress.argtypes = [vp, vp, i64, P(vp), P(i64)]
        L.vm_bgzf_decompress.argtypes = [vp, vp, i64, P(vp), P(i64)]
        L.vm_gzip_decompress.argtypes = [vp, vp, i64, P(vp), P(i64)]
        L.vm_gzip_decompress_stats.argtypes = [vp, vp, i64, P(vp), P(i64), P(C.c_double), C.c_int]
        L.vm_fastq_reader_open_opts.argtypes = [vp, cp, C.c_int, P(vp)]
        L.vm_bam_reader_open.argtypes = [vp, cp, P(vp)]; L.vm_bam_reader_open_tags.argtypes = [vp, cp, cp, P(vp)]; L.vm_bam_reader_close.argtypes = [vp]; L.vm_bam_reader_close.restype = None
        L.vm_bam_reader_read.argtypes = [vp, i64, i64] + [P(vp), P(P(i64))] * 4; L.vm_bam_reader_read.restype = i64
        L.vm_bam_reader_stats.argtypes = [vp, P(C.c_double), C.c_int]
        L.vm_fastq_reader_open.argtypes = [vp, cp, P(vp)]; L.vm_fastq_reader_close.argtypes = [vp]; L.vm_fastq_reader_close.restype = None
        L.vm_fastq_reader_read.argtypes = [vp, i64, i64] + [P(vp), P(P(i64))] * 4; L.vm_fastq_reader_read.restype = i64
        L.vm_fastq_reader_stats.argtypes = [vp, P(C.c_double), C.c_int]

    def err(self):
        return self.L.vm_last_error().decode()

    def check(self, rc):
        if rc < 0:
            raise VmxError(rc, self.err())
        return rc

    def params(self, mode='H', **kw):
        p = Params()
        self.L.vm_params_default(C.byref(p), MODES[mode])
        for k, v in kw.items():
            setattr(p, k, v)
        return p


_default = None


def chain_counters(lib, enable=0):
    """vm_debug_chain_counters: dict of the row chain kernels' counters (enable: 1 on, 0 read, -1 read and reset)"""
    out = (C.c_ulonglong * 8)()
    lib.check(lib.L.vm_debug_chain_counters(int(enable), out))
    keys = ('global_anchors', 'global_scans_past_window', 'global_insertions_through_hbm', 'global_opcount',
            'local_anchors', 'local_scans_past_window', 'local_insertions_through_hbm', 'local_opcount')
    return dict(zip(keys, [int(x) for x in out]))


def load():
    global _default
    if _default is None:
        _default = VmxLib()
    return _default


class Context:
    """one GPU + stream + work buffers (vm_ctx). Fails loudly without a device."""

    def __init__(self, device=0, lib=None):
        self.lib = lib or load()
        h = C.c_void_p()
        self.lib.check(self.lib.L.vm_ctx_create(device, C.byref(h)))
        self.h = h; self.device = int(device)

    def set_inflight(self, n_contexts):
        """tell the context how many contexts share its GPU (vm_ctx_set_inflight)"""
        self.lib.check(self.lib.L.vm_ctx_set_inflight(self.h, int(n_contexts)))

    def set_blocking_sync(self, on=True):
        """sleep instead of spinning while waiting for the GPU (vm_ctx_set_blocking_sync)"""
        self.lib.check(self.lib.L.vm_ctx_set_blocking_sync(self.h, int(bool(on))))

    def mem_info(self):
        """(free, total) bytes of the device's memory"""
        f = C.c_int64(); t = C.c_int64()
        self.lib.check(self.lib.L.vm_ctx_mem_info(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def attach_depth(self, depth):
        """vm_ctx_attach_depth: while `depth` (a Depth made on this context; None detaches) is attached, every sam_emit_device and paf_emit_device
        call on this context also adds its records to it, with no further wait or upload and the same returned bytes"""
        self.lib.check(self.lib.L.vm_ctx_attach_depth(self.h, depth.h if depth is not None else None))

    def close(self):
        if self.h:
            for ref in getattr(self, '_depths', []):      # (their counts live in this context's memory)
                d = ref()
                if d is not None:
                    d.close()
            self.lib.L.vm_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers
    def _take(self, ptr, n, dtype):
        a = np.ctypeslib.as_array(ptr, shape=(max(int(n), 1),))[:int(n)].astype(dtype, copy=True)
        self.lib.L.vm_free(ptr)
        return a

    def table(self, which):
        p = C.c_void_p()
        n = self.lib.check(self.lib.L.vm_table(self.h, which, C.byref(p)))
        ty = C.c_float if which < 4 else C.c_double
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ty)), shape=(n,)).copy()
        self.lib.L.vm_free(p)
        return a

    # ---- DP primitives
    def edit_distance_batch(self, queries, targets):
        q, qo = _cat(queries); t, to = _cat(targets)
        out = C.POINTER(C.c_int64)()
        self.lib.check(self.lib.L.vm_edit_distance_batch(self.h, len(queries), q, qo.ctypes.data, t, to.ctypes.data, C.byref(out)))
        return self._take(out, len(queries), np.int64)

    def edit_distance_bound_batch(self, queries, targets, tier=2):
        q, qo = _cat(queries); t, to = _cat(targets)
        out = C.POINTER(C.c_int64)()
        self.lib.check(self.lib.L.vm_edit_distance_bound_batch(self.h, tier, len(queries), q, qo.ctypes.data, t, to.ctypes.data, C.byref(out)))
        return self._take(out, len(queries), np.int64)

    def edit_distance(self, q, t):
        q, t = _b(q), _b(t)
        return self.lib.check(self.lib.L.vm_edit_distance(self.h, q, len(q), t, len(t)))

    def k_extend_batch(self, targets, queries, match=2, mismatch=-4, o=4, e=4, bw=100, zdrop=50):
        t, to = _cat(targets); q, qo = _cat(queries)
        te = C.POINTER(C.c_int32)(); qe = C.POINTER(C.c_int32)(); sc = C.POINTER(C.c_int32)()
        n = len(targets)
        self.lib.check(self.lib.L.vm_k_extend_batch(self.h, match, mismatch, o, e, bw, zdrop, n, t, to.ctypes.data, q, qo.ctypes.data,
                                                    C.byref(te), C.byref(qe), C.byref(sc)))
        return self._take(sc, n, np.int32), self._take(te, n, np.int32), self._take(qe, n, np.int32)

    def k_cigar_batch(self, targets, queries, match=2, mismatch=-4, o1=4, e1=2, o2=24, e2=1, eqx=False):
        t, to = _cat(targets); q, qo = _cat(queries)
        n = len(targets)
        sc = Score(match, mismatch, o1, e1, o2, e2)
        cg = C.c_void_p(); co = C.POINTER(C.c_int64)(); ss = C.POINTER(C.c_int32)()
        self.lib.check(self.lib.L.vm_k_cigar_batch(self.h, C.byref(sc), int(eqx), n, t, to.ctypes.data, q, qo.ctypes.data,
                                                   C.byref(cg), C.byref(co), C.byref(ss)))
        off = self._take(co, n + 1, np.int64)
        blob = C.string_at(cg.value, int(off[-1])) if off[-1] else b''
        self.lib.L.vm_free(cg)
        cigars = [blob[off[i]:off[i + 1] - 1].decode() for i in range(n)]
        return cigars, self._take(ss, n, np.int32)

    def k_cigar_batch_banded(self, targets, queries, match=2, mismatch=-4, o1=4, e1=2, o2=24, e2=1, eqx=False):
        """the gap-fill schedule of vm_align_batch (banded first, unproven problems redone in full): (cigars, band_flag, stats dict)"""
        t, to = _cat(targets); q, qo = _cat(queries)
        n = len(targets)
        sc = Score(match, mismatch, o1, e1, o2, e2)
        cg = C.c_void_p(); co = C.POINTER(C.c_int64)(); fl = C.POINTER(C.c_int32)(); st = (C.c_int64 * 6)()
        self.lib.check(self.lib.L.vm_k_cigar_batch_banded(self.h, C.byref(sc), int(eqx), n, t, to.ctypes.data, q, qo.ctypes.data,
                                                          C.byref(cg), C.byref(co), C.byref(fl), st))
        off = self._take(co, n + 1, np.int64)
        blob = C.string_at(cg.value, int(off[-1])) if off[-1] else b''
        self.lib.L.vm_free(cg)
        cigars = [blob[off[i]:off[i + 1] - 1].decode() for i in range(n)]
        return cigars, self._take(fl, n, np.int32), {'eligible': st[0], 'proven': st[1], 'redo': st[2], 'not_eligible': st[3],
                                                          'redo_wide': st[4], 'redo_full': st[5]}

    def k_cigar(self, target, query, match=2, mismatch=-4, gap_open_1=4, gap_extend_1=2, gap_open_2=24, gap_extend_2=1,
                bw=-1, zdropvalue=-1, eqx=False):
        """mp.k_cigar's argument list and return tuple (cigar, zdropcode, q_e, t_e, del, ins) (mammap_clrnano.py:21554, :2381)"""
        t, q = _b(target), _b(query)
        sc = Score(match, mismatch, gap_open_1, gap_extend_1, gap_open_2, gap_extend_2)
        out = CigarOut()
        self.lib.check(self.lib.L.vm_k_cigar(self.h, t, len(t), q, len(q), C.byref(sc), bw, zdropvalue, int(eqx), C.byref(out)))
        cg = C.string_at(out.cigar).decode() if out.cigar else ''
        self.lib.L.vm_free(out.cigar)
        return cg, 0, out.q_e, out.t_e, 0, 0

    # ---- global chain stage
    def chain_global_batch(self, prm, kmersize, anchors_list, readlens, want_raw=False):
        n = len(anchors_list)
        aoff = np.zeros(n + 1, np.int64)
        for i, a in enumerate(anchors_list):
            aoff[i + 1] = aoff[i] + len(a)
        rows = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1, 4) for a in anchors_list]) if n else np.zeros((0, 4), np.int64))
        rl = np.ascontiguousarray(readlens, dtype=np.int64)
        out = ChainsOut()
        self.lib.check(self.lib.L.vm_chain_global_batch(self.h, C.byref(prm), kmersize, n, rows.ctypes.data, aoff.ctypes.data, rl.ctypes.data,
                                                        int(want_raw), C.byref(out)))
        res = []
        rpo = np.ctypeslib.as_array(out.read_path_off, shape=(n + 1,)).copy()
        npaths = int(rpo[-1])
        po = np.ctypeslib.as_array(out.path_off, shape=(npaths + 1,)).copy()
        nrows = int(po[-1])
        pa = np.ctypeslib.as_array(out.path_anchors, shape=(max(nrows, 1), 4))[:nrows].copy()
        tot = int(aoff[-1])
        for r in range(n):
            d = {'need_reverse': bool(out.need_reverse[r]), 'mapq': int(out.mapq[r]), 'score': float(out.score[r]),
                 'fast_used': bool(out.fast_used[r]), 'gmax': int(out.gmax[r]), 'opcount': int(out.opcount[r]),
                 'paths': [pa[po[p]:po[p + 1]] for p in range(rpo[r], rpo[r + 1])]}
            if want_raw:
                a, b = int(aoff[r]), int(aoff[r + 1])
                d['S'] = np.ctypeslib.as_array(out.S, shape=(max(tot, 1),))[a:b].copy()
                d['P'] = np.ctypeslib.as_array(out.P, shape=(max(tot, 1),))[a:b].copy()
                d['S_arg'] = np.ctypeslib.as_array(out.S_arg, shape=(max(tot, 1),))[a:b].copy()
            res.append(d)
        self.lib.L.vm_chains_out_free(C.byref(out))
        return res

    # ---- seed stage
    def sketch_batch(self, k, w, seqs):
        s, off = _cat(seqs)
        n = len(seqs)
        h = C.POINTER(C.c_uint64)(); p = C.POINTER(C.c_int32)(); z = C.POINTER(C.c_int8)(); oo = C.POINTER(C.c_int64)()
        self.lib.check(self.lib.L.vm_sketch_batch(self.h, k, w, n, s, off.ctypes.data, C.byref(h), C.byref(p), C.byref(z), C.byref(oo)))
        o = self._take(oo, n + 1, np.int64)
        m = int(o[-1])
        H = self._take(h, m, np.uint64); Pp = self._take(p, m, np.int32); Z = self._take(z, m, np.int8)
        return [(H[o[i]:o[i + 1]], Pp[o[i]:o[i + 1]], Z[o[i]:o[i + 1]]) for i in range(n)]

    def map(self, index, seq, check_num=100, mid_occ=-1):
        """vm_map: the reference's per-read call `index_object.map(seq, check_num=, mid_occ=)` (mammap_clrnano.py:23985) -> (n, 4) int64 rows"""
        sq = _b(seq)
        a = C.POINTER(C.c_int64)(); n = C.c_int64(0)
        self.lib.check(self.lib.L.vm_map(self.h, index.h, sq, len(sq), int(check_num), int(mid_occ), C.byref(a), C.byref(n)))
        rows = np.ctypeslib.as_array(a, shape=(max(n.value, 1), 4))[:n.value].copy()
        self.lib.L.vm_free(a)
        return rows

    def chain_linked(self, rows, which, kmersize, skipcost, maxdiff, maxgap, g_max_scores=0., g_max_index=0, pre_S=None, pre_P=None, prereadloc=0):
        """one batch of -mode asm's linked chain DPs (vm_chain_linked): dict(gmax, S, P, S_arg_hot, n_cold, cold_max, opcount, carry...)"""
        a = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 4)
        ps = np.ascontiguousarray(pre_S if pre_S is not None else [], dtype=np.float64)
        pp = np.ascontiguousarray(pre_P if pre_P is not None else [], dtype=np.int64)
        out = LinkedOut()
        self.lib.check(self.lib.L.vm_chain_linked(self.h, which, kmersize, float(skipcost), int(maxdiff), int(maxgap), len(a), a.ctypes.data, len(ps), ps.ctypes.data,
                                                  pp.ctypes.data, float(g_max_scores), int(g_max_index), int(prereadloc), C.byref(out)))
        n = len(a)
        r = {'gmax': out.gmax, 'n_hot': out.n_hot, 'n_cold': out.n_cold, 'cold_max': out.cold_max, 'opcount': out.opcount,
             'S': np.ctypeslib.as_array(out.S, shape=(n,)).copy(), 'P': np.ctypeslib.as_array(out.P, shape=(n,)).copy(),
             'S_arg_hot': np.ctypeslib.as_array(out.S_arg_hot, shape=(max(out.n_hot, 1),))[:out.n_hot].copy(),
             'carry_status': out.carry_status, 'saved': out.saved, 'n_carry': out.n_carry}
        if out.carry_status == 0 and out.saved:
            m = out.n_carry
            r.update(carry_S=np.ctypeslib.as_array(out.carry_S, shape=(m,)).copy(), carry_P=np.ctypeslib.as_array(out.carry_P, shape=(m,)).copy(),
                     carry_rows=np.ctypeslib.as_array(out.carry_rows, shape=(m, 4)).copy(), carry_g_max_scores=out.carry_g_max_scores,
                     carry_prereadloc=out.carry_prereadloc)
        self.lib.L.vm_linked_out_free(C.byref(out))
        return r

    def map_batch(self, index, seqs, check_num=100, mid_occ=-1):
        s, off = _cat(seqs)
        n = len(seqs)
        a = C.POINTER(C.c_int64)(); ao = C.POINTER(C.c_int64)()
        self.lib.check(self.lib.L.vm_map_batch(self.h, index.h, check_num, mid_occ, n, s, off.ctypes.data, C.byref(a), C.byref(ao)))
        o = self._take(ao, n + 1, np.int64)
        tot = int(o[-1])
        rows = np.ctypeslib.as_array(a, shape=(max(tot, 1), 4))[:tot].copy()
        self.lib.L.vm_free(a)
        return [rows[o[i]:o[i + 1]] for i in range(n)]


def _collect_records(ctx, recs, n, blob, stats):
    out = []
    base = blob.value
    for i in range(n):
        r = recs[i]
        cg = C.string_at(base + r.cigar_off, r.cigar_len).decode()
        out.append((r.read_idx, r.contig, '+' if r.strand == 1 else '-', r.q_st, r.q_en, r.r_st, r.r_en, r.mapq, cg))
    ctx.lib.L.vm_free(recs); ctx.lib.L.vm_free(blob)
    sd = {k: getattr(stats, k) for k, _ in BatchStats._fields_ if k != 'ms_stage'}
    sd['ms_stage'] = list(stats.ms_stage)
    return out, sd


def align_batch(ctx, index, prm, seqs):
    """the batched path: reads -> (status per read, records as 9-tuples with read index / contig index, stats)"""
    s, off = _cat(seqs)
    n = len(seqs)
    status = np.zeros(max(n, 1), np.int32)
    recs = C.POINTER(Record)(); nrec = C.c_int64(); blob = C.c_void_p(); stats = BatchStats()
    ctx.lib.check(ctx.lib.L.vm_align_batch(ctx.h, index.h, C.byref(prm), n, s, off.ctypes.data, C.byref(recs), C.byref(nrec), C.byref(blob),
                                           status.ctypes.data, C.byref(stats)))
    out, sd = _collect_records(ctx, recs, nrec.value, blob, stats)
    return status[:n], out, sd


def align_asm(ctx, index, prm, contig, split_len=0, batch_anchors=0, window=0):
    """-mode asm on one assembly contig (vm_align_asm): (status, records as 9-tuples)"""
    s = contig if isinstance(contig, bytes) else contig.encode()
    recs = C.POINTER(Record)(); nrec = C.c_int64(); blob = C.c_void_p(); st = C.c_int32()
    ctx.lib.check(ctx.lib.L.vm_align_asm(ctx.h, index.h, C.byref(prm), s, len(s), split_len, batch_anchors, window, C.byref(recs), C.byref(nrec), C.byref(blob), C.byref(st)))
    out, _ = _collect_records(ctx, recs, nrec.value, blob, BatchStats())
    return st.value, out


def align_trace(ctx, index, prm, seqs, stage):
    """segment lists of every read after stage 0 / 3 / 5 of the extend phase (vm_align_trace): list of (n_i, 5) int64 arrays"""
    s, off = _cat(seqs)
    n = len(seqs)
    rows = C.POINTER(C.c_int64)(); ro = C.POINTER(C.c_int64)()
    ctx.lib.check(ctx.lib.L.vm_align_trace(ctx.h, index.h, C.byref(prm), n, s, off.ctypes.data, int(stage), C.byref(rows), C.byref(ro)))
    o = ctx._take(ro, n + 1, np.int64)
    tot = int(o[-1])
    a = np.ctypeslib.as_array(rows, shape=(max(tot, 1), 5))[:tot].copy()
    ctx.lib.L.vm_free(rows)
    return [a[o[i]:o[i + 1]] for i in range(n)]


class RawBatch:
    """result of vm_align_batch kept in library memory (no per-record Python objects): what the native SAM emitter consumes"""

    def __init__(self, ctx, status, recs, nrec, blob, stats):
        self.ctx, self.status, self.recs, self.nrec, self.blob = ctx, status, recs, nrec, blob
        self.stats = {k: getattr(stats, k) for k, _ in BatchStats._fields_ if k != 'ms_stage'}
        self.stats['ms_stage'] = list(stats.ms_stage)

    def close(self):
        if self.recs is not None:
            self.ctx.lib.L.vm_free(self.recs); self.ctx.lib.L.vm_free(self.blob)
            self.recs = self.blob = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def align_batch_raw(ctx, index, prm, seq_blob, seq_off):
    """vm_align_batch on a read blob (uint8 array + int64 offsets[n + 1]); the records stay in library memory (RawBatch)"""
    seq_blob = _u8(seq_blob); seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    n = len(seq_off) - 1
    status = np.zeros(max(n, 1), np.int32)
    recs = C.POINTER(Record)(); nrec = C.c_int64(); blob = C.c_void_p(); stats = BatchStats()
    ctx.lib.check(ctx.lib.L.vm_align_batch(ctx.h, index.h, C.byref(prm), n, seq_blob.ctypes.data_as(C.c_char_p), seq_off.ctypes.data, C.byref(recs), C.byref(nrec),
                                           C.byref(blob), status.ctypes.data, C.byref(stats)))
    return RawBatch(ctx, status[:n], recs, nrec.value, blob, stats)


def sam_emit(lib, index, opts, names, name_off, seqs, seq_off, raw, quals=None, qual_off=None, comments=None, com_off=None, nthreads=8):
    """SAM lines of a batch (vm_sam_emit): returns (text as a uint8 array, text_off[n + 1], n_lines, n_skipped). Blobs are uint8 arrays,
    offsets int64; quals / comments may be None."""
    names = _u8(names); seqs = _u8(seqs)
    name_off = np.ascontiguousarray(name_off, dtype=np.int64); seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    n = len(seq_off) - 1
    q = _u8(quals) if quals is not None else None; qo = np.ascontiguousarray(qual_off, dtype=np.int64) if quals is not None else None
    cm = _u8(comments) if comments is not None else None; co = np.ascontiguousarray(com_off, dtype=np.int64) if comments is not None else None
    text = C.c_void_p(); toff = C.POINTER(C.c_int64)(); nl = C.c_int64(); ns = C.c_int64()
    lib.check(lib.L.vm_sam_emit(index.h, C.byref(opts), n, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
                                q.ctypes.data if q is not None else None, qo.ctypes.data if qo is not None else None,
                                cm.ctypes.data if cm is not None else None, co.ctypes.data if co is not None else None,
                                C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob, raw.status.ctypes.data if len(raw.status) else None, int(nthreads),
                                C.byref(text), C.byref(toff), C.byref(nl), C.byref(ns)))
    off = np.ctypeslib.as_array(toff, shape=(n + 1,)).copy()
    lib.L.vm_free(toff)
    tot = int(off[-1])
    buf = _OwnedText(lib, text, tot)          # a view of the library's buffer (no copy of ~150 MB per batch); freed with the object
    return buf.array, off, nl.value, ns.value


def sam_emit_device(ctx, index, opts, names, name_off, seqs, seq_off, raw, quals=None, qual_off=None, *, comments=None, com_off=None):
    """SAM lines of a batch made on the GPU (vm_sam_emit_device, on the context's stream): sam_emit's return tuple, byte for byte. With
    comments / com_off (keywords only) the reads' comments are copied as sam_emit copies them (vm_sam_emit_device_comments); a reference with
    letters other than ACGTN raises VmxError(VM_ERR_UNSUPPORTED)."""
    lib = ctx.lib
    names = _u8(names); seqs = _u8(seqs)
    name_off = np.ascontiguousarray(name_off, dtype=np.int64); seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    n = len(seq_off) - 1
    q = _u8(quals) if quals is not None else None; qo = np.ascontiguousarray(qual_off, dtype=np.int64) if quals is not None else None
    text = C.c_void_p(); toff = C.POINTER(C.c_int64)(); nl = C.c_int64(); ns = C.c_int64()
    tail = (C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob, raw.status.ctypes.data if len(raw.status) else None, C.byref(text), C.byref(toff), C.byref(nl), C.byref(ns))
    head = (ctx.h, index.h, C.byref(opts), n, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
            q.ctypes.data if q is not None else None, qo.ctypes.data if qo is not None else None)
    if comments is None and com_off is None:
        lib.check(lib.L.vm_sam_emit_device(*head, *tail))
    else:
        cm = _u8(comments) if comments is not None else None; co = np.ascontiguousarray(com_off, dtype=np.int64) if com_off is not None else None
        lib.check(lib.L.vm_sam_emit_device_comments(*head, cm.ctypes.data if cm is not None and len(cm) else None, co.ctypes.data if co is not None else None, *tail))
    off = np.ctypeslib.as_array(toff, shape=(n + 1,)).copy()
    lib.L.vm_free(toff)
    buf = _OwnedText(lib, text, int(off[-1]))
    return buf.array, off, nl.value, ns.value


def paf_emit(lib, index, opts, names, name_off, seqs, seq_off, raw, nthreads=8):
    """PAF lines of a batch (vm_paf_emit; the rule: include/vacmapx.h): sam_emit's return tuple. One line where sam_emit writes a record line."""
    names = _u8(names); seqs = _u8(seqs)
    name_off = np.ascontiguousarray(name_off, dtype=np.int64); seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    n = len(seq_off) - 1
    text = C.c_void_p(); toff = C.POINTER(C.c_int64)(); nl = C.c_int64(); ns = C.c_int64()
    lib.check(lib.L.vm_paf_emit(index.h, C.byref(opts), n, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
                                C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob, raw.status.ctypes.data if len(raw.status) else None, int(nthreads),
                                C.byref(text), C.byref(toff), C.byref(nl), C.byref(ns)))
    off = np.ctypeslib.as_array(toff, shape=(n + 1,)).copy()
    lib.L.vm_free(toff)
    buf = _OwnedText(lib, text, int(off[-1]))
    return buf.array, off, nl.value, ns.value


def paf_emit_device(ctx, index, opts, names, name_off, seqs, seq_off, raw):
    """PAF lines of a batch made on the GPU (vm_paf_emit_device, on the context's stream): paf_emit's return tuple, byte for byte; a reference
    with letters other than ACGTN raises VmxError(VM_ERR_UNSUPPORTED)."""
    lib = ctx.lib
    names = _u8(names); seqs = _u8(seqs)
    name_off = np.ascontiguousarray(name_off, dtype=np.int64); seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
    n = len(seq_off) - 1
    text = C.c_void_p(); toff = C.POINTER(C.c_int64)(); nl = C.c_int64(); ns = C.c_int64()
    lib.check(lib.L.vm_paf_emit_device(ctx.h, index.h, C.byref(opts), n, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
                                       C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob, raw.status.ctypes.data if len(raw.status) else None,
                                       C.byref(text), C.byref(toff), C.byref(nl), C.byref(ns)))
    off = np.ctypeslib.as_array(toff, shape=(n + 1,)).copy()
    lib.L.vm_free(toff)
    buf = _OwnedText(lib, text, int(off[-1]))
    return buf.array, off, nl.value, ns.value


class Depth:
    """Per-window depth of coverage (vm_depth; the rule: include/vacmapx.h at vm_depth_add, in Python: vacmap_amd/depth.py). Made for one index, a
    window size and a MAPQ threshold; with a context the counts live on its GPU (add_device, Context.attach_depth), without one in host memory (add)."""

    REGIONS, SUMMARY = 0, 1

    def __init__(self, lib, h, ctx, nseq):
        self.lib, self.h, self.ctx, self.nseq = lib, h, ctx, nseq

    @classmethod
    def create(cls, index, window=500, min_mapq=0, ctx=None, lib=None):
        lib = ctx.lib if ctx is not None else (lib or load())
        h = C.c_void_p()
        lib.check(lib.L.vm_depth_create(ctx.h if ctx is not None else None, index.h, int(window), int(min_mapq), C.byref(h)))
        d = cls(lib, h, ctx, index.nseq)
        if ctx is not None:
            if not hasattr(ctx, '_depths'):
                ctx._depths = []
            ctx._depths.append(weakref.ref(d))
        return d

    @staticmethod
    def _blobs(names, name_off, seqs, seq_off):
        return _u8(names), np.ascontiguousarray(name_off, dtype=np.int64), _u8(seqs), np.ascontiguousarray(seq_off, dtype=np.int64)

    def add(self, index, opts, names, name_off, seqs, seq_off, raw, nthreads=8):
        """vm_depth_add (host accumulator): paf_emit's arguments; returns (n_lines, n_skipped) as sam_emit counts them"""
        names, name_off, seqs, seq_off = self._blobs(names, name_off, seqs, seq_off)
        nl = C.c_int64(); ns = C.c_int64()
        self.lib.check(self.lib.L.vm_depth_add(self.h, index.h, C.byref(opts), len(seq_off) - 1, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data, seq_off.ctypes.data,
                                               C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob, raw.status.ctypes.data if len(raw.status) else None, int(nthreads),
                                               C.byref(nl), C.byref(ns)))
        return nl.value, ns.value

    def add_device(self, ctx, index, opts, names, name_off, seqs, seq_off, raw):
        """vm_depth_add_device (an accumulator made on ctx): paf_emit_device's arguments; no text is made; returns (n_lines, n_skipped)"""
        names, name_off, seqs, seq_off = self._blobs(names, name_off, seqs, seq_off)
        nl = C.c_int64(); ns = C.c_int64()
        self.lib.check(self.lib.L.vm_depth_add_device(self.h, ctx.h, index.h, C.byref(opts), len(seq_off) - 1, names.ctypes.data, name_off.ctypes.data, seqs.ctypes.data,
                                                      seq_off.ctypes.data, C.cast(raw.recs, C.c_void_p), raw.nrec, raw.blob,
                                                      raw.status.ctypes.data if len(raw.status) else None, C.byref(nl), C.byref(ns)))
        return nl.value, ns.value

    def merge(self, other):
        """vm_depth_merge: self += other (any mix of host and device accumulators of one layout)"""
        self.lib.check(self.lib.L.vm_depth_merge(self.h, other.h))

    def add_counts(self, counts):
        """vm_depth_add_counts: self += a table that counts() returned for an accumulator of the same layout (another rank's)"""
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.lib.check(self.lib.L.vm_depth_add_counts(self.h, counts.ctypes.data, len(counts)))

    def counts(self):
        """(counts[n_windows], win_off[nseq + 1]) as int64 arrays"""
        cp = C.POINTER(C.c_int64)(); wp = C.POINTER(C.c_int64)(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_depth_counts(self.h, C.byref(cp), C.byref(wp), C.byref(n)))
        counts = np.ctypeslib.as_array(cp, shape=(max(n.value, 1),))[:n.value].copy()
        win_off = np.ctypeslib.as_array(wp, shape=(self.nseq + 1,)).copy()
        self.lib.L.vm_free(cp); self.lib.L.vm_free(wp)
        return counts, win_off

    def _text(self, which):
        t = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_depth_text(self.h, which, C.byref(t), C.byref(n)))
        out = C.string_at(t, n.value)
        self.lib.L.vm_free(t)
        return out

    def regions(self):
        """the regions text (bytes): one line per window, TNAME start end mean"""
        return self._text(self.REGIONS)

    def summary(self):
        """the summary text (bytes): one line per contig, TNAME length bases mean, and `total`"""
        return self._text(self.SUMMARY)

    def close(self):
        if self.h:
            self.lib.L.vm_depth_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sam_emit_device_times(ctx):
    """(upload, passes, download) wall seconds of the context's latest sam_emit_device call"""
    t = (C.c_double * 3)()
    ctx.lib.check(ctx.lib.L.vm_sam_emit_device_times(ctx.h, t))
    return tuple(t)


class _OwnedText:
    """uint8 view of a library-allocated buffer; the memory lives as long as any array derived from `.array` does"""

    def __init__(self, lib, ptr, n):
        self.lib, self.ptr = lib, ptr
        self.array = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(max(n, 1),))[:n]
        import weakref
        base = self.array
        while isinstance(getattr(base, 'base', None), np.ndarray):
            base = base.base
        weakref.finalize(base, lib.L.vm_free, ptr)


class PinnedPool:
    """page-locked host buffers (vm_pinned_alloc) handed out as uint8 arrays and taken back for reuse: the driver gathers a batch's reads into
    one, so that vm_align_batch's upload is a DMA instead of a staged copy on the aligner thread. get() falls back to pageable memory when the
    runtime refuses (returns a plain array; release() ignores those)."""

    def __init__(self, lib, device=-1):
        import threading
        self.lib, self.device, self.free, self.lock, self.owned = lib, int(device), [], threading.Lock(), {}

    def get(self, nbytes):
        nbytes = max(int(nbytes), 1)
        with self.lock:
            for i, (cap, ptr) in enumerate(self.free):
                if cap >= nbytes:
                    self.free.pop(i)
                    break
            else:
                cap, ptr = 0, None
        if ptr is None:
            cap = max(nbytes + nbytes // 4, 1 << 20)
            ptr = self.lib.L.vm_pinned_alloc(cap, self.device)
            if not ptr:
                return np.empty(nbytes, np.uint8)
        arr = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(cap,))
        with self.lock:
            self.owned[arr.ctypes.data] = (cap, ptr)
        return arr

    def release(self, arr):
        base = arr
        while isinstance(getattr(base, 'base', None), np.ndarray):
            base = base.base
        with self.lock:
            ent = self.owned.pop(base.ctypes.data, None)
            if ent is not None:
                self.free.append(ent)

    def close(self):
        """frees every buffer, those still handed out too: nothing may use one after this"""
        with self.lock:
            for cap, ptr in self.free + list(self.owned.values()):
                self.lib.L.vm_pinned_free(ptr)
            self.free, self.owned = [], {}


def blob_gather(lib, blob, off, idx, alloc=None):
    """entries idx of (blob, off) back to back: (uint8 array, int64 offsets) — one memcpy loop in the library (vm_blob_gather).
    alloc(nbytes) -> uint8 array of at least that many bytes to gather into (e.g. PinnedPool.get)"""
    blob = _u8(blob); off = np.ascontiguousarray(off, dtype=np.int64); idx = np.ascontiguousarray(idx, dtype=np.int64)
    n = len(idx)
    oo = np.empty(n + 1, np.int64)
    tot = int((off[idx + 1] - off[idx]).sum()) if n else 0
    out = alloc(max(tot, 1)) if alloc is not None else np.empty(max(tot, 1), np.uint8)
    lib.L.vm_blob_gather(blob.ctypes.data, off.ctypes.data, idx.ctypes.data, n, out.ctypes.data, oo.ctypes.data)
    return out[:tot], oo


def blob_gather_parts(lib, blobs, offs, order_keys):
    """several (blob, off) pairs merged into one blob whose entries follow ascending order_keys (one int64 key array per pair, e.g. the
    reads' indices in the input window): one memcpy loop in the library, no concatenation of the parts first"""
    blobs = [_u8(b) for b in blobs]; offs = [np.ascontiguousarray(o, dtype=np.int64) for o in offs]
    keys = np.concatenate([np.asarray(k, dtype=np.int64) for k in order_keys]) if blobs else np.zeros(0, np.int64)
    part = np.concatenate([np.full(len(k), i, np.int32) for i, k in enumerate(order_keys)]) if blobs else np.zeros(0, np.int32)
    local = np.concatenate([np.arange(len(k), dtype=np.int64) for k in order_keys]) if blobs else np.zeros(0, np.int64)
    order = np.argsort(keys, kind='stable')
    part = np.ascontiguousarray(part[order]); local = np.ascontiguousarray(local[order])
    tot = int(sum(int(o[-1]) for o in offs))
    out = np.empty(max(tot, 1), np.uint8)
    bp = (C.c_void_p * len(blobs))(*[b.ctypes.data for b in blobs]); op = (C.c_void_p * len(offs))(*[o.ctypes.data for o in offs])
    w = lib.L.vm_blob_gather_parts(bp, op, part.ctypes.data, local.ctypes.data, len(local), out.ctypes.data)
    return out[:w]


def _parts_order(blobs, offs, order_keys):
    keys = np.concatenate([np.asarray(k, dtype=np.int64) for k in order_keys]) if blobs else np.zeros(0, np.int64)
    part = np.concatenate([np.full(len(k), i, np.int32) for i, k in enumerate(order_keys)]) if blobs else np.zeros(0, np.int32)
    local = np.concatenate([np.arange(len(k), dtype=np.int64) for k in order_keys]) if blobs else np.zeros(0, np.int64)
    order = np.argsort(keys, kind='stable')
    return np.ascontiguousarray(part[order]), np.ascontiguousarray(local[order])


def blob_write_parts(lib, fd, blobs, offs, order_keys, file_off=None, nthreads=4):
    """blob_gather_parts written to the file descriptor `fd`: returns the bytes written. file_off = the current end of a regular file: the lines are
    copied by `nthreads` threads straight into the file's pages (vm_blob_write_parts_mmap; the descriptor's own position is moved past them); a
    descriptor that cannot be mapped, or file_off None: one writev stream, no assembled copy"""
    blobs = [_u8(b) for b in blobs]; offs = [np.ascontiguousarray(o, dtype=np.int64) for o in offs]
    part, local = _parts_order(blobs, offs, order_keys)
    bp = (C.c_void_p * len(blobs))(*[b.ctypes.data for b in blobs]); op = (C.c_void_p * len(offs))(*[o.ctypes.data for o in offs])
    if file_off is not None:
        w = lib.L.vm_blob_write_parts_mmap(int(fd), int(file_off), bp, op, part.ctypes.data, local.ctypes.data, len(local), int(nthreads))
        if w >= 0:
            os.lseek(int(fd), int(file_off) + int(w), os.SEEK_SET)
            return int(w)
        if w == -1:
            raise VmxError(-1, lib.err())
    w = lib.L.vm_blob_write_parts(int(fd), bp, op, part.ctypes.data, local.ctypes.data, len(local))
    if w < 0:
        raise VmxError(-1, lib.err())
    return int(w)


def _take_bytes(lib, p, n):
    b = C.string_at(p, n.value) if n.value else b''
    lib.L.vm_free(p)
    return b


def bgzf_compress(ctx, data):
    """bytes -> BGZF members (no EOF marker), deflated on the device (vm_bgzf_compress)"""
    data = bytes(data)
    p = C.c_void_p(); n = C.c_int64()
    ctx.lib.check(ctx.lib.L.vm_bgzf_compress(ctx.h, data, len(data), C.byref(p), C.byref(n)))
    return _take_bytes(ctx.lib, p, n)


def bgzf_decompress(ctx, data):
    """BGZF members (any writer's, with or without the EOF block) -> their bytes, inflated on the device (vm_bgzf_decompress)"""
    data = bytes(data)
    p = C.c_void_p(); n = C.c_int64()
    ctx.lib.check(ctx.lib.L.vm_bgzf_decompress(ctx.h, data, len(data), C.byref(p), C.byref(n)))
    return _take_bytes(ctx.lib, p, n)


GZIP_STATS = ('chunks_started', 'candidates_rejected', 'chunks_redone', 'first_chain_bytes', 'find_s', 'decode_s', 'window_s', 'resolve_s')


def gzip_decompress(ctx, data, stats=None):
    """gzip members (plain gzip: any writer's, one member or many) -> their bytes, inflated on the device in parallel chunks
    (vm_gzip_decompress_stats). stats: a dict that receives the call's GZIP_STATS, also when the call raises"""
    data = bytes(data)
    p = C.c_void_p(); n = C.c_int64()
    v = (C.c_double * len(GZIP_STATS))()
    rc = ctx.lib.L.vm_gzip_decompress_stats(ctx.h, data, len(data), C.byref(p), C.byref(n), v, len(GZIP_STATS))
    if stats is not None:
        stats.update(zip(GZIP_STATS, v))
    ctx.lib.check(rc)
    return _take_bytes(ctx.lib, p, n)


class _BlobReader:
    """what the device readers share: read() as Fastx.read(), stats() as a dict of the STATS names, close(). A subclass names its three
    C-ABI entries (_READ, _STATS_FN, _CLOSE), whose signatures are the same, and sets self.ctx, self.lib and self.h"""
    STATS = ()
    _READ = _STATS_FN = _CLOSE = None

    def read(self, max_reads, max_bases=1 << 62):
        """next chunk: dict of uint8 blobs and int64 offsets (names, seqs, quals, comments), or None at the end of the input"""
        ptrs = [C.c_void_p() for _ in range(4)]; offs = [C.POINTER(C.c_int64)() for _ in range(4)]
        args = []
        for p, o in zip(ptrs, offs):
            args += [C.byref(p), C.byref(o)]
        n = getattr(self.lib.L, self._READ)(self.h, int(max_reads), int(max_bases), *args)
        if n < 0:
            raise VmxError(int(n), self.lib.err())
        out = {}
        for key, p, o in zip(('names', 'seqs', 'quals', 'comments'), ptrs, offs):
            oo = np.ctypeslib.as_array(o, shape=(n + 1,)).copy(); self.lib.L.vm_free(o)
            tot = int(oo[-1])
            out[key] = _OwnedText(self.lib, p, tot).array
            out[key + '_off'] = oo
        return out if n > 0 else None

    def stats(self):
        v = (C.c_double * len(self.STATS))()
        self.lib.check(getattr(self.lib.L, self._STATS_FN)(self.h, v, len(self.STATS)))
        return dict(zip(self.STATS, list(v)))

    def close(self):
        if getattr(self, 'h', None):
            if self.ctx.h:                                   # (a reader outlives its context only by mistake: then its memory is left to the process)
                getattr(self.lib.L, self._CLOSE)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamReader(_BlobReader):
    """BAM reader into blobs (vm_bam_reader_*): BGZF inflate and record decoding on the device; read() as Fastx.read().
    tags: None (comments stay empty), '*' or 'all' (every auxiliary field), or a list / comma-separated string of two-character tags: the
    selected fields become each read's comment, `XX:T:value` joined by tabs, made on the device (vm_bam_reader_open_tags)"""
    STATS = ('io_busy_s', 'io_wait_s', 'inflate_s', 'walk_s', 'decode_s', 'download_s', 'handout_s', 'windows', 'file_bytes', 'inflated_bytes', 'records', 'dropped',
             'fields_dropped')
    _READ, _STATS_FN, _CLOSE = 'vm_bam_reader_read', 'vm_bam_reader_stats', 'vm_bam_reader_close'

    def __init__(self, ctx, path, tags=None):
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        if tags is None:
            self.lib.check(self.lib.L.vm_bam_reader_open(ctx.h, _b(path), C.byref(h)))
        else:
            spec = '*' if tags in ('*', 'all') else tags if isinstance(tags, str) else ','.join(tags)
            self.lib.check(self.lib.L.vm_bam_reader_open_tags(ctx.h, _b(path), _b(spec), C.byref(h)))
        self.h = h


class FastqReader(_BlobReader):
    """Reader of bgzipped FASTQ into blobs (vm_fastq_reader_*): BGZF inflate and the four-line parse on the device, by Fastx's own rule
    (include/vacmapx.h); read() as Fastx.read(). VmxError -7 at open: not gzip; plain gzip unless gzip='device'; FASTA unless fasta=True
    (Fastx reads those)"""
    STATS = ('io_busy_s', 'io_wait_s', 'inflate_s', 'parse_s', 'copy_s', 'download_s', 'handout_s', 'windows', 'file_bytes', 'inflated_bytes', 'records')
    _READ, _STATS_FN, _CLOSE = 'vm_fastq_reader_read', 'vm_fastq_reader_stats', 'vm_fastq_reader_close'

    def __init__(self, ctx, path, gzip='host', fasta=False):
        """gzip='device': a plain-gzip file is inflated on the device in parallel chunks (vm_fastq_reader_open_opts, VM_READER_GZIP_DEVICE)
        instead of being refused; stats() then has GZIP_STATS too. fasta=True (VM_READER_FASTA): the device parses by Fastx's whole rule,
        multi-line FASTA records and files that mix both kinds included, instead of refusing a record that begins with '>'"""
        if gzip not in ('host', 'device'):
            raise ValueError("gzip must be 'host' or 'device'")
        self.ctx, self.lib = ctx, ctx.lib
        h = C.c_void_p()
        flags = (1 if gzip == 'device' else 0) | (2 if fasta else 0)
        if gzip == 'device':
            self.STATS = FastqReader.STATS + GZIP_STATS
        if flags:
            self.lib.check(self.lib.L.vm_fastq_reader_open_opts(ctx.h, _b(path), flags, C.byref(h)))
        else:
            self.lib.check(self.lib.L.vm_fastq_reader_open(ctx.h, _b(path), C.byref(h)))
        self.h = h


class BamCodec:
    """vm_bam_writer: SAM header text -> reference table on the device; SAM lines -> BAM records -> BGZF members"""

    def __init__(self, ctx, header_text):
        self.ctx, self.lib = ctx, ctx.lib
        t = _b(header_text)
        h = C.c_void_p()
        self.lib.check(self.lib.L.vm_bam_writer_create(ctx.h, t, len(t), C.byref(h)))
        self.h = h

    def header(self):
        """BAM magic, header text and references as BGZF members"""
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_header(self.h, C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def encode(self, sam_text):
        """uncompressed BAM records of SAM lines"""
        t = _b(sam_text)
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_encode(self.h, t, len(t), C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def compress_parts(self, blobs, offs, order_keys):
        """the entries of several (blob, off) pairs in ascending order_keys (as blob_gather_parts), as BGZF members of their BAM records"""
        blobs = [_u8(b) for b in blobs]; offs = [np.ascontiguousarray(o, dtype=np.int64) for o in offs]
        part, local = _parts_order(blobs, offs, order_keys)
        bp = (C.c_void_p * max(len(blobs), 1))(*[b.ctypes.data for b in blobs]); op = (C.c_void_p * max(len(offs), 1))(*[o.ctypes.data for o in offs])
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_compress_parts(self.h, bp, op, part.ctypes.data, local.ctypes.data, len(local), C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.L.vm_bam_writer_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BamSorter:
    """vm_bam_sorter on a BamCodec: sorted runs per call, then the merge in chunks and the CSI index (include/vacmapx.h)"""

    def __init__(self, codec, chunk_bytes):
        self.codec, self.lib = codec, codec.lib
        h = C.c_void_p()
        self.lib.check(self.lib.L.vm_bam_sorter_create(codec.h, int(chunk_bytes), C.byref(h)))
        self.h = h

    def add_parts(self, blobs, offs, order_keys):
        """the lines (as BamCodec.compress_parts takes them) -> their BAM records in coordinate order, uncompressed: one run (b'' when there is no line)"""
        blobs = [_u8(b) for b in blobs]; offs = [np.ascontiguousarray(o, dtype=np.int64) for o in offs]
        part, local = _parts_order(blobs, offs, order_keys)
        bp = (C.c_void_p * max(len(blobs), 1))(*[b.ctypes.data for b in blobs]); op = (C.c_void_p * max(len(offs), 1))(*[o.ctypes.data for o in offs])
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_sorter_add_parts(self.h, bp, op, part.ctypes.data, local.ctypes.data, len(local), C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def plan(self, run_paths, file_base):
        """run_paths: the files of the non-empty runs in call order; file_base: bytes already in the output file. Returns the number of chunks"""
        raw = [os.fsencode(x) for x in run_paths]
        arr = (C.c_char_p * max(len(raw), 1))(*raw)
        n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_sorter_plan(self.h, arr, len(raw), int(file_base), C.byref(n)))
        return n.value

    def chunk(self, k):
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_sorter_chunk(self.h, int(k), C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def index(self):
        p = C.c_void_p(); n = C.c_int64()
        self.lib.check(self.lib.L.vm_bam_sorter_index(self.h, C.byref(p), C.byref(n)))
        return _take_bytes(self.lib, p, n)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.L.vm_bam_sorter_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Fastx:
    """FASTA / FASTQ(.gz) reader into blobs (vm_fastx_*): the native counterpart of mp.fastx_read (vacmap:445)"""

    def __init__(self, path, lib=None, byte_range=None):
        """byte_range = (begin, end): only the records whose first byte lies in [begin, end) of a plain file (vm_fastx_open_range)"""
        self.lib = lib or load()
        h = C.c_void_p()
        if byte_range is None:
            self.lib.check(self.lib.L.vm_fastx_open(_b(path), C.byref(h)))
        else:
            self.lib.check(self.lib.L.vm_fastx_open_range(_b(path), int(byte_range[0]), int(byte_range[1]), C.byref(h)))
        self.h = h

    def read(self, max_reads, max_bases=1 << 62):
        """next chunk: dict of uint8 blobs and int64 offsets (names, seqs, quals, comments), or None at the end of the input"""
        ptrs = [C.c_void_p() for _ in range(4)]; offs = [C.POINTER(C.c_int64)() for _ in range(4)]
        args = []
        for p, o in zip(ptrs, offs):
            args += [C.byref(p), C.byref(o)]
        n = self.lib.L.vm_fastx_read(self.h, int(max_reads), int(max_bases), *args)
        if n < 0:
            raise VmxError(int(n), self.lib.err())
        out = {}
        for key, p, o in zip(('names', 'seqs', 'quals', 'comments'), ptrs, offs):
            oo = np.ctypeslib.as_array(o, shape=(n + 1,)).copy(); self.lib.L.vm_free(o)
            tot = int(oo[-1])
            out[key] = _OwnedText(self.lib, p, tot).array          # a view of the library's buffer (a window is ~1 GB: no copy)
            out[key + '_off'] = oo
        return out if n > 0 else None

    def close(self):
        if self.h:
            self.lib.L.vm_fastx_close(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ResidentReads:
    """reads uploaded once into HBM (bench: inputs resident when the timed region starts)"""

    def __init__(self, ctx, seqs=None, concat=None, offsets=None):
        if seqs is not None:
            s, off = _cat(seqs)
        else:
            s = concat if isinstance(concat, (bytes, bytearray)) else np.ascontiguousarray(concat, dtype=np.uint8).tobytes()
            off = np.ascontiguousarray(offsets, dtype=np.int64)
        self.ctx = ctx; self.n = len(off) - 1; self.bases = int(off[-1])
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.L.vm_reads_upload(ctx.h, self.n, s, off.ctypes.data, C.byref(h)))
        self.h = h

    def reupload(self, concat, offsets, ctx=None):
        """another batch into this object's device buffers (vm_reads_reupload): `concat` a uint8 array (page-locked memory makes the copy a DMA), no
        alignment of this object in flight"""
        arr = _u8(concat); off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(off) - 1
        self.ctx.lib.check(self.ctx.lib.L.vm_reads_reupload((ctx or self.ctx).h, self.h, n, arr.ctypes.data, off.ctypes.data))
        self.n = n; self.bases = int(off[-1])

    def align_raw(self, index, prm, ctx=None):
        """vm_align_resident with the records left in library memory (RawBatch: what the native SAM emitter consumes)"""
        status = np.zeros(max(self.n, 1), np.int32)
        recs = C.POINTER(Record)(); nrec = C.c_int64(); blob = C.c_void_p(); stats = BatchStats()
        self.ctx.lib.check(self.ctx.lib.L.vm_align_resident((ctx or self.ctx).h, index.h, C.byref(prm), self.h, C.byref(recs), C.byref(nrec), C.byref(blob),
                                                            status.ctypes.data, C.byref(stats)))
        return RawBatch(self.ctx, status[:self.n], recs, nrec.value, blob, stats)

    def align(self, index, prm, want_records=True, ctx=None):
        """ctx: the context (streams + work pools) to run on; default = the one that uploaded the reads"""
        status = np.zeros(max(self.n, 1), np.int32)
        recs = C.POINTER(Record)(); nrec = C.c_int64(); blob = C.c_void_p(); stats = BatchStats()
        self.ctx.lib.check(self.ctx.lib.L.vm_align_resident((ctx or self.ctx).h, index.h, C.byref(prm), self.h, C.byref(recs), C.byref(nrec), C.byref(blob),
                                                            status.ctypes.data, C.byref(stats)))
        if want_records:
            out, sd = _collect_records(self.ctx, recs, nrec.value, blob, stats)
        else:
            self.ctx.lib.L.vm_free(recs); self.ctx.lib.L.vm_free(blob)
            out = None
            sd = {k: getattr(stats, k) for k, _ in BatchStats._fields_ if k != 'ms_stage'}
            sd['ms_stage'] = list(stats.ms_stage)
        return status[:self.n], out, sd

    def close(self):
        if self.h:
            self.ctx.lib.L.vm_reads_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def local_chain_batch(ctx, index, prm, seqs, paths_per_read):
    """seqs in chain orientation; paths_per_read: list (per read) of lists of (m,4) arrays (descending read order)"""
    s, off = _cat(seqs)
    n = len(seqs)
    rpo = np.zeros(n + 1, np.int64); po = [0]; rows = []
    for r, paths in enumerate(paths_per_read):
        rpo[r + 1] = rpo[r] + len(paths)
        for p in paths:
            p = np.asarray(p, dtype=np.int64).reshape(-1, 4)
            rows.append(p); po.append(po[-1] + len(p))
    po = np.asarray(po, dtype=np.int64)
    pa = np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4), np.int64))
    out = LocalOut()
    ctx.lib.check(ctx.lib.L.vm_local_chain_batch(ctx.h, index.h, C.byref(prm), n, s, off.ctypes.data, rpo.ctypes.data, po.ctypes.data,
                                                 pa.ctypes.data, C.byref(out)))
    co = np.ctypeslib.as_array(out.chain_off, shape=(n + 1,)).copy(); ro = np.ctypeslib.as_array(out.raw_off, shape=(n + 1,)).copy()
    ch = np.ctypeslib.as_array(out.chain, shape=(max(int(co[-1]), 1), 4))[:int(co[-1])].copy()
    rw = np.ctypeslib.as_array(out.raw, shape=(max(int(ro[-1]), 1), 4))[:int(ro[-1])].copy()
    res = [{'status': int(out.status[r]), 'variant': int(out.variant[r]), 'score': float(out.score[r]), 'chain': ch[co[r]:co[r + 1]],
            'raw': rw[ro[r]:ro[r + 1]]} for r in range(n)]
    ctx.lib.L.vm_local_out_free(C.byref(out))
    return res


def local_dp_batch(ctx, prm, rows_list, n_guides_total, readlens, want_sp=False, device_list=False):
    """vm_local_dp_batch: the local chain DPs on given rows. rows_list: per read an (m, 4) array (q, r, s, l) in the DP's input order (stable by q + l;
    mode R: by q); n_guides_total, readlens: per read. Returns per read dict(status, variant, fast_used, score, chain, S, P) — S / P are None where
    the entry does not define them (not asked for, the read not chained, S kept in LDS by the one-wavefront form)."""
    n = len(rows_list)
    off = np.zeros(n + 1, np.int64)
    for i, a in enumerate(rows_list):
        off[i + 1] = off[i] + len(a)
    rows = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.int64).reshape(-1, 4) for a in rows_list]) if n else np.zeros((0, 4), np.int64))
    ng = np.ascontiguousarray(n_guides_total, dtype=np.int32); rl = np.ascontiguousarray(readlens, dtype=np.int64)
    assert len(ng) == n and len(rl) == n
    out = LocalDpOut()
    flags = (LOCAL_DP_WANT_SP if want_sp else 0) | (LOCAL_DP_DEVICE_LIST if device_list else 0)
    try:
        ctx.lib.check(ctx.lib.L.vm_local_dp_batch(ctx.h, C.byref(prm), n, rows.ctypes.data, off.ctypes.data, ng.ctypes.data, rl.ctypes.data, flags, C.byref(out)))
        co = np.ctypeslib.as_array(out.chain_off, shape=(n + 1,)).copy()
        ch = np.ctypeslib.as_array(out.chain, shape=(max(int(co[-1]), 1), 4))[:int(co[-1])].copy()
        tot = int(off[-1])
        S = np.ctypeslib.as_array(out.S, shape=(max(tot, 1),))[:tot].copy() if want_sp and n else None
        Pp = np.ctypeslib.as_array(out.P, shape=(max(tot, 1),))[:tot].copy() if want_sp and n else None
        res = []
        for r in range(n):
            v = int(out.sp_valid[r])
            res.append({'status': int(out.status[r]), 'variant': int(out.variant[r]), 'fast_used': bool(out.fast_used[r]), 'score': float(out.score[r]),
                        'chain': ch[co[r]:co[r + 1]], 'S': S[off[r]:off[r + 1]] if v & 1 else None, 'P': Pp[off[r]:off[r + 1]] if v & 2 else None})
    finally:
        ctx.lib.L.vm_local_dp_out_free(C.byref(out))
    return res


REF_BUILD_STATS = ('read_s', 'inflate_s', 'parse_s', 'download_s', 'index_s', 'text_bytes', 'windows', 'contigs')     # vm_index_build_fasta_device's stats


class Index:
    """HBM-resident minimizer index (vm_index); mirrors what the reference reads from `mp.Aligner` (vacmap:344-367)."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.h = handle
        L = ctx.lib.L
        self.k = L.vm_index_k(handle); self.w = L.vm_index_w(handle); self.nseq = L.vm_index_nseq(handle)
        self.mid_occ = L.vm_index_mid_occ(handle)
        self.names, self.lens, self.offsets = [], [], []
        for i in range(self.nseq):
            nm = C.c_char_p(); ln = C.c_int64(); of = C.c_int64()
            L.vm_index_seq_info(handle, i, C.byref(nm), C.byref(ln), C.byref(of))
            self.names.append(nm.value.decode()); self.lens.append(ln.value); self.offsets.append(of.value)

    @classmethod
    def from_fasta(cls, ctx, path, k=15, w=10, reader='host', gzip='host'):
        """the index of a FASTA file, plain, gzip or bgzipped. reader='host': vm_index_build_fasta parses the text on one host thread;
        reader='native': vm_index_build_fasta_device parses it on the GPU (the same index, byte for byte) and leaves its statistics in
        idx.build_stats; a header line longer than a window raises VmxError(VM_ERR_UNSUPPORTED). gzip='device' (with reader='native'): a
        plain-gzip file is inflated on the GPU in parallel chunks instead of by zlib on a host thread (vm_index_build_fasta_device_opts)"""
        if reader not in ('host', 'native'):
            raise ValueError("reader must be 'host' or 'native'")
        if gzip not in ('host', 'device'):
            raise ValueError("gzip must be 'host' or 'device'")
        h = C.c_void_p()
        if reader == 'host':
            ctx.lib.check(ctx.lib.L.vm_index_build_fasta(ctx.h, _b(path), k, w, C.byref(h)))
            return cls(ctx, h)
        st = (C.c_double * 8)()
        if gzip == 'device':
            ctx.lib.check(ctx.lib.L.vm_index_build_fasta_device_opts(ctx.h, _b(path), k, w, 1, C.byref(h), st, 8))       # VM_READER_GZIP_DEVICE
        else:
            ctx.lib.check(ctx.lib.L.vm_index_build_fasta_device(ctx.h, _b(path), k, w, C.byref(h), st, 8))
        idx = cls(ctx, h)
        idx.build_stats = dict(zip(REF_BUILD_STATS, (float(x) for x in st)))
        for key in ('text_bytes', 'windows', 'contigs'):
            idx.build_stats[key] = int(idx.build_stats[key])
        return idx

    @classmethod
    def from_seqs(cls, ctx, names, seqs, k=15, w=10):
        n = len(names)
        keep, sa, la = _seq_ptrs(seqs)
        na = (C.c_char_p * max(n, 1))(*[_b(x) for x in names])
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.L.vm_index_build_mem(ctx.h, n, na, sa, la, k, w, C.byref(h)))
        del keep
        return cls(ctx, h)

    @classmethod
    def load(cls, ctx, path):
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.L.vm_index_load(ctx.h, _b(path), C.byref(h)))
        return cls(ctx, h)

    def save(self, path):
        self.ctx.lib.check(self.ctx.lib.L.vm_index_save(self.h, _b(path)))

    @classmethod
    def load_mmi(cls, ctx, path):
        """a minimap2 index file (`minimap2 -d`, format v3; src/vacmap/vacmap:324-344)"""
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.L.vm_index_load_mmi(ctx.h, _b(path), C.byref(h)))
        return cls(ctx, h)

    def save_mmi(self, path, bucket_bits=14):
        self.ctx.lib.check(self.ctx.lib.L.vm_index_save_mmi(self.h, _b(path), bucket_bits))

    # ---- multi-GPU replication (vacmap_amd/dist.py): metadata + the raw HBM pieces
    def meta(self):
        """bytes from which another process allocates an empty replica (vm_index_meta_get)"""
        n = C.c_int64()
        self.ctx.lib.check(self.ctx.lib.L.vm_index_meta_size(self.h, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        self.ctx.lib.check(self.ctx.lib.L.vm_index_meta_get(self.h, buf, n.value))
        return buf.raw

    @classmethod
    def from_meta(cls, ctx, meta):
        """empty replica on ctx's GPU with the geometry of `meta`; its blobs() are then filled by the broadcast"""
        h = C.c_void_p()
        ctx.lib.check(ctx.lib.L.vm_index_from_meta(ctx.h, meta, len(meta), C.byref(h)))
        return cls(ctx, h)

    def blobs(self):
        """[(device pointer, bytes)] of codes, positions, hash table, contig offsets (vm_index_blob)"""
        out = []
        for i in range(self.ctx.lib.L.vm_index_blob_count(self.h)):
            p = C.c_void_p(); n = C.c_int64()
            self.ctx.lib.check(self.ctx.lib.L.vm_index_blob(self.h, i, C.byref(p), C.byref(n)))
            out.append((p.value or 0, n.value))
        return out

    def seq(self, i, st=0, en=None):
        en = self.lens[i] if en is None else en
        buf = C.create_string_buffer(max(en - st, 1))
        n = self.ctx.lib.L.vm_index_seq(self.h, i, st, en, buf)
        return buf.raw[:max(n, 0)].decode()

    def n_minimizers(self):
        return self.ctx.lib.L.vm_index_n_minimizers(self.h)

    def n_distinct(self):
        return self.ctx.lib.L.vm_index_n_distinct(self.h)

    def minimizers(self):
        hh = C.POINTER(C.c_uint64)(); pp = C.POINTER(C.c_uint64)(); n = C.c_int64()
        self.ctx.lib.check(self.ctx.lib.L.vm_index_minimizers(self.h, C.byref(hh), C.byref(pp), C.byref(n)))
        return self.ctx._take(hh, n.value, np.uint64), self.ctx._take(pp, n.value, np.uint64)

    def close(self):
        if self.h:
            self.ctx.lib.L.vm_index_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
