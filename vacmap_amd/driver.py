"""Command-line driver: reads in, SAM out — the counterpart of the reference's `vacmap` script (src/vacmap/vacmap:75-152 options,
:186-218 read group, :324-370 index + header, :430-517 read loop with name de-duplication and BAM input; writer
src/vacmap/output_functions.py:172-235) around the MI355X library.

    python -m vacmap_amd.driver -ref ref.fa -read reads.fq -mode H -o out.sam [-t 8] [--eqx] [--MD] [--cs[=long]] [--H] ...
    python -m torch.distributed.run --nproc-per-node N -m vacmap_amd.driver ...        (one rank per GPU)

One process drives one GPU. The index is built on the GPU (or loaded from `<ref>.w<w>_k<k>.vmx`, the reference's `.mmi` naming rule,
vacmap:326; a minimap2 `.mmi` of that name is read too) and kept in HBM. Reads never become Python objects: the library's FASTX
reader (vm_fastx_read) fills blobs, `vacmap_amd.pipeline` cuts windows of `--window-batches` x `--batch-reads` reads into length-binned
batches, several batches are in flight, each worker thread aligns its batch on the GPU (vm_align_batch) and turns the records into SAM
text with `-t` host threads (vm_sam_emit, the C++ twin of vacmap_amd/sam.py) while the other batches align; every window is written
in input order. Like the reference's worker (:24116-24134) a read whose path or whose emission raises is skipped, and a read without
records produces no line. `-o out.paf` writes PAF lines instead (vm_paf_emit / vm_paf_emit_device, vacmap_amd/paf.py: one line where a .sam run
writes a record line, no header) on every text path a .sam takes.
With N ranks, rank 0 builds the index and broadcasts it over RCCL (vacmap_amd/dist.py), batch i of a window goes to rank i mod N, and
rank 0 gathers and writes the lines. `-mode asm` (assembly contigs; contig c -> rank c mod N): the contigs go through vm_align_batch with VM_MODE_ASM in
groups, in input order, and their lines come from the native emitter in its asm form (vm_sam_opts.asm_mode = iterator_get_bam_dict_str,
mammap_asm.py:22757; vacmap_amd/sam.py holds the same emitter in Python); `-workdir` is accepted and created like the reference's; only `--bam-writer native-sort` spills into it (its run files, removed at the end).
main() lists the stages of a run; the stage that opens something (process groups, context and index, output, the read stream's contexts and
page-locked buffers) releases it however the run ends. The environment variables the driver reads are the table SWITCHES.
"""
import argparse, concurrent.futures, contextlib, gzip, os, queue, shutil, struct, subprocess, sys, threading, time, types

from . import sam
# numpy is imported inside the functions that use it: a command-line run sets the allocator up (_keep_heap_pages) before numpy's first import


# Every environment variable the driver reads: (name, default, how its text is read, what it does). main() reads them once, when it starts
# (_switches); nothing below this table looks at the environment. INTEGRATION.md shows the same table to users.
_is1, _not0 = (lambda v: v == '1'), (lambda v: v != '0')
SWITCHES = (
    ('WORLD_SIZE', '1', int, 'torchrun: number of ranks; above 1 the process groups are created (nccl = RCCL for the index, gloo for SAM text)'),
    ('RANK', '0', int, 'torchrun: this process\'s rank'),
    ('LOCAL_RANK', '0', int, 'torchrun: this process\'s GPU unless --device names one'),
    ('VMX_FORCE_DIST', '0', _is1, '1: the N-rank start-up at world 1 too (process groups, index through a replica built from the broadcast metadata): '
                            'what an 8-GPU run executes, testable on one GPU'),
    ('VMX_GATHER_TIMEOUT', '1800', int, 'seconds after which the gloo group gives up on a rank that died (an error instead of a hang)'),
    ('VMX_DRIVER_MALLOPT', '1', _not0, '0: leave glibc\'s allocator alone (default: one arena, no mmap, no trimming, so that freed windows are reused)'),
    ('VMX_DRIVER_RAMP', '0', _is1, '1: the stream starts on one sized context and the others are sized in the background and join one by one '
                             '(measured: the first batch starts 1.6 s instead of 5.9 s after the loop begins, the loop takes the same 12.8 s '
                             'because hipMalloc under load slows the running batches, profiles/r05_zz_driver_long_ramped_start.json)'),
    ('VMX_NO_WARM', '0', _is1, '1: no sizing run before the stream (every context then grows its pools when it meets its first long batch); also turns the ramp and the feeders off'),
    ('VMX_MIN_FREE_GB', '10', float, 'HBM head-room after the sizing run: contexts are given up until this much is free'),
    ('VMX_SPIN_SYNC', '0', _is1, '1: threads that wait for the GPU spin instead of sleeping (default: sleep, the emitters need the cores)'),
    ('VMX_EMIT_THREADS', '0', int, 'host threads that produce SAM text, in all (0: -t)'),
    ('VMX_PARSE_THREADS', '0', int, 'parser threads when --parse-threads is 0 (0: max(1, min(4, t / 4)))'),
    ('VMX_SLICE_MB', '1024', float, 'size of the record-aligned slices a plain FASTA / FASTQ input is parsed in'),
    ('VMX_DRIVER_WINDOWS', '10', int, 'windows in memory at a time, input blobs and SAM text (at least 2)'),
    ('VMX_DRIVER_PINNED', '1', _not0, '0: gather a batch\'s reads into pageable instead of page-locked memory (the upload is then staged on the aligner thread); also turns the feeders off'),
    ('VMX_DRIVER_FEEDERS', '2', int, 'threads with a context of their own that gather and upload batches ahead of the aligners (0: the aligner thread does both)'),
    ('VMX_DRIVER_WRITEV', '1', _not0, '0: assemble a window\'s text and write() it instead of writing the batches\' texts straight to the descriptor'),
    ('VMX_EMIT_CONTEXTS', '2', int, '--sam-emitter device: threads that make SAM text on the GPU, each with a context of its own (at least 1)'),
    ('VMX_SKIP_EMIT', '0', _is1, '1: diagnostic, no SAM text is produced: the aligners alone'),
    ('VMX_DRIVER_TIMING', '', str, 'set: one stderr line of seconds by phase at the end; 2: also one line per batch'),
)


def _switches():
    """{name: value} of SWITCHES as the environment has them now"""
    return {name: read(os.environ.get(name, default)) for name, default, read, _ in SWITCHES}


def read_fastx(path, want_comment=False):
    """yields (name, seq, qual or None, comment or None) from FASTA / FASTQ, plain or .gz (mp.fastx_read shape, vacmap:445)"""
    op = gzip.open if path.endswith('.gz') else open
    with op(path, 'rt') as f:
        line = f.readline()
        while line:
            line = line.rstrip('\n')
            if not line:
                line = f.readline(); continue
            if line[0] == '>':
                head = line[1:]; seqs = []
                line = f.readline()
                while line and line[0] != '>':
                    seqs.append(line.strip()); line = f.readline()
                name, com = _split_header(head)
                yield name, ''.join(seqs), None, (com if want_comment and com else None)
            elif line[0] == '@':
                head = line[1:]
                seq = f.readline().strip(); f.readline(); qual = f.readline().strip()
                name, com = _split_header(head)
                yield name, seq, qual, (com if want_comment and com else None)
                line = f.readline()
            else:
                raise ValueError('not FASTA/FASTQ: %r' % line[:40])


def _split_header(head):
    """name | comment at the first blank or tab (kseq's rule)"""
    for i, ch in enumerate(head):
        if ch == ' ' or ch == '\t':
            return head[:i], head[i + 1:]
    return head, ''


_BAM_NT16 = '=ACMGRSVTWYHKDBN'


def _bam_tag_select(tags):
    """--bam-tags / tags=: None (no tags), '*' (every field: 'all' or '*'), or the frozenset of two-character tags of a list or comma-separated string"""
    if tags is None or tags == '' or tags == []:
        return None
    if isinstance(tags, str):
        if tags in ('all', '*'):
            return '*'
        tags = tags.split(',')
    tags = [t.decode('latin-1') if isinstance(t, bytes) else t for t in tags]
    for t in tags:
        if len(t) != 2 or not (t[0].isascii() and t[0].isalpha() and t[1].isascii() and t[1].isalnum()):
            raise ValueError('--bam-tags: %r is not a two-character tag (give a comma-separated list such as MM,ML,MN, or all)' % t)
    return frozenset(tags)


_AUX_INT = {'c': 'b', 'C': 'B', 's': 'h', 'S': 'H', 'i': 'i', 'I': 'I'}


def _f32_text(raw):
    """4 bytes of a float32 -> the shortest %.{p}g (p = 1 ... 9) that strtod and a cast read back as the same bits; None when not finite"""
    x, = struct.unpack('<f', raw)
    if x != x or x in (float('inf'), float('-inf')):
        return None
    for p in range(1, 10):
        s = '%.*g' % (p, x)
        try:
            if struct.pack('<f', float(s)) == raw:
                return s
        except OverflowError:                              # (rounds beyond FLT_MAX)
            pass
    return '%.9g' % x


def _bam_aux_text(aux, sel):
    """the aux bytes of a BAM record (SAMv1 4.2.4) as the tab-separated XX:T:value text of the selected fields (sel: '*' or a set of tags), in
    record order: the rule of vm_bam_reader_open_tags (include/vacmapx.h). A field SAM text cannot hold is left out; malformed bytes raise ValueError."""
    out, p, n = [], 0, len(aux)
    while p < n:
        if n - p < 3:
            raise ValueError('malformed BAM auxiliary data: fewer than 3 bytes are left for a field')
        tag, ty = aux[p:p + 2].decode('latin-1'), chr(aux[p + 2])
        p += 3
        val = None
        if ty in 'AcCsSiIf':
            size = 1 if ty in 'AcC' else 2 if ty in 'sS' else 4
            if p + size > n:
                raise ValueError('malformed BAM auxiliary data: a fixed-size value runs past the record')
            raw = aux[p:p + size]; p += size
            if ty == 'A':
                val = 'A:' + chr(raw[0]) if 0x20 <= raw[0] <= 0x7e else None
            elif ty == 'f':
                t = _f32_text(raw); val = None if t is None else 'f:' + t
            else:
                val = 'i:%d' % struct.unpack('<' + _AUX_INT[ty], raw)[0]
        elif ty in 'ZH':
            e = aux.find(b'\0', p)
            if e < 0:
                raise ValueError('malformed BAM auxiliary data: a Z or H value has no NUL inside the record')
            raw = aux[p:e]; p = e + 1
            ok = all(0x20 <= b <= 0x7e for b in raw) if ty == 'Z' else (len(raw) % 2 == 0 and all(b in b'0123456789abcdefABCDEF' for b in raw))
            val = ty + ':' + raw.decode('latin-1') if ok else None
        elif ty == 'B':
            if p + 5 > n:
                raise ValueError('malformed BAM auxiliary data: a B array runs past the record')
            sub, cnt = chr(aux[p]), struct.unpack_from('<I', aux, p + 1)[0]
            if sub not in 'cCsSiIf':
                raise ValueError('malformed BAM auxiliary data: unknown B array sub-type')
            size = 1 if sub in 'cC' else 2 if sub in 'sS' else 4
            if p + 5 + cnt * size > n:
                raise ValueError('malformed BAM auxiliary data: a B array runs past the record')
            p += 5
            if sel == '*' or tag in sel:                   # (an array nobody asked for is not turned into text)
                if sub == 'f':
                    ts = [_f32_text(aux[p + 4 * j:p + 4 * j + 4]) for j in range(cnt)]
                    val = None if any(t is None for t in ts) else 'B:f' + ''.join(',' + t for t in ts)
                else:
                    val = 'B:' + sub + ''.join(',%d' % v for v in struct.unpack_from('<%d%s' % (cnt, _AUX_INT[sub]), aux, p))
            p += cnt * size
        else:
            raise ValueError('malformed BAM auxiliary data: unknown field type')
        if val is not None and (sel == '*' or tag in sel):
            out.append(tag + ':' + val)
    return '\t'.join(out)


def read_bam(path, tags=None):
    """unaligned or aligned BAM -> (name, seq, qual or None, comment), the fields the reference takes from pysam (vacmap:455-471): a
    reverse-strand record is turned back to the read's own orientation, qualities 0xff mean absent. BGZF is a series of gzip members.
    comment: None, or with tags (None, 'all' / '*', a list or comma-separated string of two-character tags) the selected auxiliary fields as
    SAM text (_bam_aux_text), which the reference drops; they are not re-oriented (MM / ML are defined on the read as sequenced)."""
    sel = _bam_tag_select(tags)
    with gzip.open(path, 'rb') as f:
        if f.read(4) != b'BAM\x01':
            raise ValueError('not a BAM file: %s' % path)
        l_text, = struct.unpack('<i', f.read(4)); f.read(l_text)
        n_ref, = struct.unpack('<i', f.read(4))
        for _ in range(n_ref):
            l_name, = struct.unpack('<i', f.read(4)); f.read(l_name + 4)
        while True:
            h = f.read(4)
            if len(h) < 4:
                return
            bs, = struct.unpack('<i', h)
            rec = f.read(bs)
            if len(rec) < bs:
                raise ValueError('truncated BAM record')
            l_rn, n_cig, flag, l_seq = rec[8], struct.unpack_from('<H', rec, 12)[0], struct.unpack_from('<H', rec, 14)[0], struct.unpack_from('<i', rec, 16)[0]
            p = 32
            name = rec[p:p + l_rn - 1].decode(); p += l_rn + 4 * n_cig
            packed = rec[p:p + (l_seq + 1) // 2]; p += (l_seq + 1) // 2
            seq = ''.join(_BAM_NT16[b >> 4] + _BAM_NT16[b & 15] for b in packed)[:l_seq]
            q = rec[p:p + l_seq]
            qual = None if (l_seq == 0 or q[0] == 0xff) else bytes(x + 33 for x in q).decode('ascii')
            if l_seq == 0:
                continue                                   # "no sequence in BAM record" (vacmap:462)
            if flag & 16:
                seq = sam.revcomp(seq.upper()); qual = qual[::-1] if qual is not None else None
            yield name, seq, qual, (None if sel is None else _bam_aux_text(rec[p + l_seq:], sel))


def _bam_chunks(path, n_max, tags=None):
    """BAM records as the blob chunks the FASTX reader yields (names, upper-cased sequences, qualities; comments: the auxiliary fields that `tags`
    selects, as read_bam gives them, none without it)"""
    import numpy as np
    cur = []

    def pack(rows):
        out = {}
        for key, col in (('names', 0), ('seqs', 1), ('quals', 2), ('comments', 3)):
            bs = [(r[col] or '').encode('latin-1' if col == 3 else 'utf-8') for r in rows]
            out[key] = np.frombuffer(b''.join(bs), dtype=np.uint8)
            out[key + '_off'] = np.concatenate([[0], np.cumsum([len(b) for b in bs])]).astype(np.int64)
        return out
    for name, seq, qual, com in read_bam(path, tags):
        cur.append((name, seq.upper(), qual, com))
        if len(cur) >= n_max:
            yield pack(cur); cur = []
    if cur:
        yield pack(cur)


def _native_bam_chunks(path, n_max, lib, device, tags=None):
    """--bam-reader native: the chunks of _bam_chunks from lib.BamReader (BGZF inflate, record and auxiliary-field decoding on the GPU) on a context of its own.
    A .bam that is gzip but not BGZF (no member boundaries to inflate side by side) goes to the Python reader, with one line on stderr."""
    from .lib import BamReader, Context, VmxError
    ctx = Context(device, lib=lib)
    try:
        try:
            sel = _bam_tag_select(tags)
            rd = BamReader(ctx, path, None if sel is None else '*' if sel == '*' else sorted(sel))
        except VmxError as e:
            if e.code != -7:                               # VM_ERR_UNSUPPORTED
                raise
            sys.stderr.write('[vacmap_amd] --bam-reader native: %s is gzip but not BGZF, reading it with the Python BAM reader\n' % path)
            yield from _bam_chunks(path, n_max, tags)
            return
        try:
            yield from iter(lambda: rd.read(n_max), None)
        finally:
            rd.close()
    finally:
        ctx.close()


def _gzip_is_bgzf(path):
    """the first gzip member carries the BGZF extra subfield BC (SAMv1 4.1): what the device inflate needs to find the member boundaries"""
    with open(path, 'rb') as f:
        h = f.read(12)
        if len(h) < 12 or h[:3] != b'\x1f\x8b\x08' or not h[3] & 4:
            return False
        extra = f.read(h[10] | h[11] << 8)
    q = 0
    while q + 4 <= len(extra):
        if extra[q:q + 2] == b'BC':
            return True
        q += 4 + (extra[q + 2] | extra[q + 3] << 8)
    return False


def _native_fastq_chunks(path, n_max, lib, device, gzip_inflate='host', fasta_reads='host'):
    """--fastx-reader native: the chunks of lib.Fastx from lib.FastqReader (BGZF inflate and the FASTQ parse on the GPU) on a context of its own.
    What the device reader does not take (plain gzip: no member boundaries to inflate side by side; FASTA) goes to the host reader, with one
    line on stderr; the context is released before the host reader starts. gzip_inflate='device' (--gzip-inflate device): a plain-gzip file is
    inflated on the GPU in parallel chunks (FastqReader(gzip='device')) instead of falling back; what that reader refuses at open (FASTA, a
    block larger than the reader's chunk) still falls back, the line naming the reason. fasta_reads='device' (--fasta-reads device): the reader
    is opened with fasta=True and parses FASTA records (and files that mix both kinds) on the GPU instead of falling back on them."""
    from .lib import FastqReader, Fastx, Context, VmxError
    ctx = Context(device, lib=lib)
    rd = None
    try:
        try:
            if fasta_reads == 'device':
                rd = FastqReader(ctx, path, gzip=gzip_inflate, fasta=True)
            else:
                rd = FastqReader(ctx, path, gzip='device') if gzip_inflate == 'device' else FastqReader(ctx, path)
        except VmxError as e:
            if e.code != -7:                               # VM_ERR_UNSUPPORTED
                raise
            refused = str(e)
        if rd is not None:
            try:
                yield from iter(lambda: rd.read(n_max), None)
            finally:
                rd.close()
            return
    finally:
        ctx.close()
    why = 'is FASTA' if _gzip_is_bgzf(path) else 'is gzip but not BGZF'       # (the two things vm_fastq_reader_open refuses in a gzip file)
    if fasta_reads == 'device' and why == 'is FASTA':
        why = 'was refused by the device reader (%s)' % refused
    if gzip_inflate == 'device' and why != 'is FASTA':
        why = 'was refused by the device inflate (%s)' % refused
    sys.stderr.write('[vacmap_amd] --fastx-reader native: %s %s, reading it with the host reader\n' % (path, why))
    rd = Fastx(path, lib=lib)
    try:
        yield from iter(lambda: rd.read(n_max), None)
    finally:
        rd.close()


def _is_gzip(path):
    if not os.path.isfile(path):
        return False
    with open(path, 'rb') as f:
        return f.read(2) == b'\x1f\x8b'


def _is_plain_fastx(path):
    """an uncompressed FASTA / FASTQ file (byte ranges of it can be parsed independently)"""
    if path.endswith('.bam') or not os.path.isfile(path):
        return False
    with open(path, 'rb') as f:
        return f.read(2) != b'\x1f\x8b'


def _parse_slice(path, lib, a, b, n_max):
    from .lib import Fastx
    rd = Fastx(path, lib=lib, byte_range=(a, b))
    try:
        return list(iter(lambda: rd.read(n_max), None))
    finally:
        rd.close()


def _input_chunks(path, n_max, lib, device=0, bam_reader='python', parse_threads=0, share=(0, 1), slice_bytes=1 << 30, bam_tags=None, fastx_reader='host', gzip_inflate='host', fasta_reads='host'):
    """blob chunks (names, upper-cased sequences, qualities, comments; at most n_max records each) of one input in file order: a .bam through
    the native or the Python reader, a compressed FASTA / FASTQ file through one library reader. parse_threads > 0: a plain file is cut into
    record-aligned slices of about slice_bytes (vm_fastx_open_range) which that many threads parse ahead of the consumer, and share = (i, n)
    takes the i-th of n equal byte ranges of it (range mode: the rank's own). parse_threads = 0: one reader over the whole file.
    Closing the generator early releases the reader, its threads and the native BAM reader's context."""
    from .lib import Fastx
    if path.endswith('.bam'):
        yield from (_native_bam_chunks(path, n_max, lib, device, bam_tags) if bam_reader == 'native' else _bam_chunks(path, n_max, bam_tags))
        return
    if fastx_reader == 'native' and _is_gzip(path):
        yield from _native_fastq_chunks(path, n_max, lib, device, gzip_inflate, fasta_reads)
        return
    if not parse_threads or not _is_plain_fastx(path):
        rd = Fastx(path, lib=lib)
        try:
            yield from iter(lambda: rd.read(n_max), None)
        finally:
            rd.close()
        return
    size = os.path.getsize(path)
    lo, hi = size * share[0] // share[1], size * (share[0] + 1) // share[1]
    ns = max(1, -(-(hi - lo) // slice_bytes))
    cuts = [lo + (hi - lo) * i // ns for i in range(ns + 1)]
    pool = concurrent.futures.ThreadPoolExecutor(max_workers=parse_threads)
    try:
        futs, nxt = [], 0
        while nxt < ns or futs:
            while nxt < ns and len(futs) < parse_threads + 1:
                futs.append(pool.submit(_parse_slice, path, lib, cuts[nxt], cuts[nxt + 1], n_max)); nxt += 1
            yield from futs.pop(0).result()
    finally:
        pool.shutdown(wait=True, cancel_futures=True)


def _first_of_each_name(chunks, seen, lib):
    """the chunks without the reads whose name came before (vacmap:457,475,487); `seen`: the set of names so far, added to as they pass"""
    import numpy as np
    from .lib import blob_gather
    for ch in chunks:
        n = len(ch['seqs_off']) - 1
        nb, no = ch['names'].tobytes(), ch['names_off']
        keep = []
        for i in range(n):
            nm = nb[no[i]:no[i + 1]]
            if nm not in seen:
                seen.add(nm); keep.append(i)
        if len(keep) < n:
            ix = np.asarray(keep, dtype=np.int64)
            for key in ('names', 'seqs', 'quals', 'comments'):
                ch[key], ch[key + '_off'] = blob_gather(lib, ch[key], ch[key + '_off'], ix)
        yield ch


_HASH_POW = None


def name_hashes(blob, off):
    """64-bit hashes of the names in a blob (uint8 array + offsets), the same in every process (Python's hash() of bytes is salted per
    process): a position-weighted polynomial modulo 2^64 with a splitmix64 finish, in NumPy over the whole blob. Range mode compares the
    ranks' sets at the end of the run to give the reference's GLOBAL de-duplication by name (vacmap:457-487)."""
    global _HASH_POW
    import numpy as np
    off = np.asarray(off, dtype=np.int64)
    n = len(off) - 1
    if n <= 0:
        return np.zeros(0, np.uint64)
    lens = np.diff(off)
    mx = int(lens.max()) if n else 0
    if _HASH_POW is None or len(_HASH_POW) < mx + 1:
        pw = np.empty(max(mx + 1, 256), np.uint64); pw[0] = 1
        with np.errstate(over='ignore'):
            for i in range(1, len(pw)):
                pw[i] = pw[i - 1] * np.uint64(0x9E3779B97F4A7C15)
        _HASH_POW = pw
    b = np.asarray(blob, dtype=np.uint8)[off[0]:off[-1]]
    pos = np.arange(len(b), dtype=np.int64) - np.repeat(off[:-1] - off[0], lens)
    with np.errstate(over='ignore'):
        contrib = (b.astype(np.uint64) + np.uint64(1)) * _HASH_POW[pos]
        h = np.zeros(n, np.uint64)
        nz = lens > 0
        if len(contrib):
            st = (off[:-1] - off[0])[nz]
            h[nz] = np.add.reduceat(contrib, st)
        h = h + lens.astype(np.uint64) * np.uint64(0xD6E8FEB86659FD93)
        h ^= h >> np.uint64(30); h *= np.uint64(0xBF58476D1CE4E5B9); h ^= h >> np.uint64(27); h *= np.uint64(0x94D049BB133111EB); h ^= h >> np.uint64(31)
    return h


def cross_rank_duplicates(hashes_per_rank, files_per_rank):
    """{rank: name hashes to leave out of that rank's part}: of the occurrences of a name over all ranks' ranges, every one but the FIRST IN INPUT ORDER
    (lowest input-file number, then lowest rank = lowest byte range of that file); a rank holds a name at most once (its own windows de-duplicate)."""
    import numpy as np
    hs = np.concatenate([np.asarray(h, dtype=np.uint64) for h in hashes_per_rank]) if hashes_per_rank else np.zeros(0, np.uint64)
    fl = np.concatenate([np.asarray(f, dtype=np.int32) for f in files_per_rank]) if files_per_rank else np.zeros(0, np.int32)
    rk = np.concatenate([np.full(len(h), r, np.int32) for r, h in enumerate(hashes_per_rank)]) if hashes_per_rank else np.zeros(0, np.int32)
    order = np.lexsort((rk, fl, hs)); hs, rk = hs[order], rk[order]
    dup = np.zeros(len(hs), bool)
    if len(hs) > 1:
        dup[1:] = hs[1:] == hs[:-1]
    return {int(r): hs[dup & (rk == r)] for r in np.unique(rk[dup])}


def _span_hashes(buf, starts, lens):
    """name_hashes for names that lie at arbitrary places of one buffer (uint8 array): the spans are gathered into one blob first"""
    import numpy as np
    starts = np.asarray(starts, dtype=np.int64); lens = np.asarray(lens, dtype=np.int64)
    off = np.zeros(len(lens) + 1, np.int64); np.cumsum(lens, out=off[1:])
    idx = np.repeat(starts - off[:-1], lens) + np.arange(int(off[-1]), dtype=np.int64)
    return name_hashes(buf[idx], off)


def _filter_part(f, o, bad, block=64 << 20):
    """copy SAM part `f` to `o` without the alignment lines whose read name hashes into `bad` (sorted uint64 array); the names of a block of
    lines are hashed together in NumPy (one name_hashes call per LINE took minutes on a large part). Returns (hashes left out, lines left out)."""
    import numpy as np
    gone, gone_lines, tail = set(), 0, b''
    while True:
        blk = f.read(block)
        data = tail + blk
        if not data:
            break
        if blk:
            cut = data.rfind(b'\n') + 1
            if cut == 0:                                 # no complete line yet
                tail = data
                continue
            data, tail = data[:cut], data[cut:]
        else:
            tail = b''
            if not data.endswith(b'\n'):
                data += b'\n'
        a = np.frombuffer(data, dtype=np.uint8)
        ends = np.flatnonzero(a == 10)
        starts = np.concatenate([[0], ends[:-1] + 1]).astype(np.int64)
        tabs = np.flatnonzero(a == 9)
        ti = np.searchsorted(tabs, starts)
        nm_end = np.where(ti < len(tabs), tabs[np.minimum(ti, max(len(tabs) - 1, 0))] if len(tabs) else ends, ends)
        nm_end = np.minimum(nm_end, ends)
        body = a[starts] != 64                           # '@': header line
        h = np.zeros(len(starts), np.uint64)
        if body.any():
            h[body] = _span_hashes(a, starts[body], (nm_end - starts)[body])
        out_ = body & np.isin(h, bad)
        if out_.any():
            gone.update(int(x) for x in np.unique(h[out_])); gone_lines += int(out_.sum())
            keep = np.flatnonzero(~out_)
            # runs of kept lines are written as slices
            if len(keep):
                brk = np.flatnonzero(np.diff(keep) != 1)
                rs = np.concatenate([[0], brk + 1]); re_ = np.concatenate([brk, [len(keep) - 1]])
                for x, y in zip(rs, re_):
                    o.write(data[int(starts[keep[x]]):int(ends[keep[y]]) + 1])
        else:
            o.write(data)
        if not blk:
            break
    return gone, gone_lines


def _concat_parts(dst, parts, drop=None):
    """the ranks' SAM parts, in rank order, into one file (in-kernel copies; the parts are removed). drop[r]: name hashes whose lines are
    left out of part r (a read name that occurs EARLIER IN THE INPUT — an earlier file, or a lower byte range of the same file — inside another
    rank's range: the reference keeps the first occurrence only, vacmap:457-487) — that part is then copied block by block through a filter;
    returns the (reads, lines) left out."""
    import numpy as np
    gone_reads, gone_lines = set(), 0
    with open(dst, 'wb', buffering=0) as o:             # unbuffered: sendfile on the descriptor and write() through the object must not interleave out of order
        for r, pth in enumerate(parts):
            with open(pth, 'rb') as f:
                if drop and r in drop and len(drop[r]):
                    g, gl = _filter_part(f, o, np.sort(np.asarray(drop[r], dtype=np.uint64)))
                    gone_reads |= set((r, x) for x in g); gone_lines += gl
                else:
                    size = os.fstat(f.fileno()).st_size; off = 0
                    while off < size:
                        try:
                            n = os.sendfile(o.fileno(), f.fileno(), off, min(size - off, 1 << 30))
                        except OSError:
                            n = 0
                        if n <= 0:                      # (a file system without sendfile between regular files: plain copy)
                            f.seek(off)
                            for blk in iter(lambda: f.read(16 << 20), b''):
                                o.write(blk)
                            break
                        off += n
            os.remove(pth)
    return len(gone_reads), gone_lines


RG_ARGS = (('rg-id', 'ID'), ('rg-sm', 'SM'), ('rg-lb', 'LB'), ('rg-pl', 'PL'), ('rg-ds', 'DS'), ('rg-dt', 'DT'), ('rg-pu', 'PU'), ('rg-pi', 'PI'),
           ('rg-pg', 'PG'), ('rg-cn', 'CN'), ('rg-fo', 'FO'), ('rg-ks', 'KS'), ('rg-pm', 'PM'), ('rg-bc', 'BC'))       # vacmap:45-60


def build_parser():
    p = argparse.ArgumentParser(prog='vacmapx', description='MI355X-native VACmap path: seed, non-linear chain, extend; SAM output')
    p.add_argument('-ref', required=True); p.add_argument('-read', required=True, nargs='+', action='append')
    p.add_argument('-mode', required=True, choices=['H', 'L', 'S', 'R', 'asm']); p.add_argument('-workdir')
    p.add_argument('-o', default='-'); p.add_argument('--force', action='store_true'); p.add_argument('--nowriteindex', action='store_true')
    p.add_argument('-t', type=int, default=8); p.add_argument('-k', type=str, default='15'); p.add_argument('-w', type=str, default='10')
    p.add_argument('-c', type=int, default=100); p.add_argument('-maxdivergence', type=float)
    p.add_argument('-globalpenalty', type=float); p.add_argument('-localpenalty', type=float)
    p.add_argument('-globalmaxdiff', type=int, default=50); p.add_argument('-localmaxdiff', type=int, default=30)
    p.add_argument('--eqx', action='store_true'); p.add_argument('--MD', action='store_true')
    p.add_argument('--cs', nargs='?', const='short', default=None); p.add_argument('--L', action='store_true')
    p.add_argument('--markunbalancetra', action='store_true'); p.add_argument('--nodiscard', action='store_true')
    p.add_argument('--copycomments', action='store_true'); p.add_argument('--H', action='store_true')
    p.add_argument('--fakecigar', action='store_true'); p.add_argument('--Q', action='store_true')
    for a, _ in RG_ARGS:
        p.add_argument('--' + a, dest=a.replace('-', '_'))
    p.add_argument('--device', type=int, default=None); p.add_argument('--batch-reads', type=int, default=4096)
    p.add_argument('--window-batches', type=int, default=4); p.add_argument('--inflight', type=int, default=0, help='batches in flight on the GPU; 0 (default): five, then as many more (up to eight) as the HBM has room for after the sizing run')
    # N ranks (torchrun): 'range' = every rank parses its own byte range of each plain FASTA / FASTQ input and writes its own part of the SAM file
    # (<out>.partNNN, concatenated by rank 0 at the end unless --parts); 'batch' = every rank parses everything and keeps every N-th batch, rank 0
    # gathers the text (compressed / BAM input, stdout or BAM output); 'auto' picks 'range' whenever input and output allow it
    p.add_argument('--shard', choices=['auto', 'range', 'batch'], default='auto'); p.add_argument('--parts', action='store_true')
    p.add_argument('--parse-threads', type=int, default=0, help='parser threads per rank over record-aligned slices of a plain input (0: max(1, min(4, t / 4)))')
    p.add_argument('--debug', action='store_true', help='log every read the aligner skipped with its status (vacmap:127; mammap_clrnano.py:24120-24123)')
    p.add_argument('--bam-writer', choices=['samtools', 'native', 'native-sort'], default='samtools',
                   help='how -o x.bam is written: a `samtools view -b` pipe (default) or the GPU encoder and BGZF compressor (vacmap_amd.bamout); '
                        'native does not sort: .sorted.bam needs samtools or native-sort, which sorts by coordinate on the GPU and writes x.sorted.bam.csi '
                        '(run files go to a fresh directory under -workdir, else next to the output, and are removed)')
    p.add_argument('--bam-reader', choices=['python', 'native'], default='python',
                   help='how -read x.bam is read: the Python reader on one host thread (default) or BGZF inflate and record decoding on the GPU '
                        '(lib.BamReader, on a context of its own); a .bam that is gzip but not BGZF falls back to the Python reader')
    p.add_argument('--gzip-inflate', choices=['host', 'device'], default='host',
                   help='device: where --fastx-reader native or --ref-reader native meets a plain-gzip file (gzip, pigz, concatenated .gz: no BGZF members), '
                        'inflate it on the GPU in parallel chunks (lib.FastqReader / Index.from_fasta with gzip=\'device\') instead of falling back to the host '
                        'reader (reads) or inflating with zlib on a host thread (reference); what the device inflate refuses at open falls back with one stderr line')
    p.add_argument('--fasta-reads', choices=['host', 'device'], default='host',
                   help='device: where --fastx-reader native meets FASTA reads or contigs (x.fa.gz, bgzipped, or plain gzip with --gzip-inflate device), parse '
                        'the multi-line records on the GPU (lib.FastqReader with fasta=True) instead of falling back to the host reader')
    p.add_argument('--fastx-reader', choices=['host', 'native'], default='host',
                   help='how a compressed -read x.fastq.gz is read: zlib and the parser on one host thread (default) or BGZF inflate and the FASTQ parse on '
                        'the GPU (lib.FastqReader, on a context of its own); plain gzip and FASTA fall back to the host reader, plain files keep the threaded parser')
    p.add_argument('--ref-reader', choices=['host', 'native'], default='host',
                   help='how the FASTA of -ref is parsed when no cached index is found: on one host thread (default) or on the GPU (plain, gzip and bgzipped '
                        'files; lib.Index.from_fasta(reader=\'native\')); a header line longer than a window falls back to the host parser')
    p.add_argument('--bam-tags', metavar='LIST|all', default=None,
                   help='carry auxiliary fields of -read x.bam records to the output as optional fields (the reference drops them): a comma-separated list '
                        'of two-character tags (MM,ML,MN) or `all`; with --bam-reader native they are turned into SAM text on the GPU. They travel as the '
                        "read's comment, with or without --copycomments, through the host SAM emitter (the device's with --sam-emitter device-comments)")
    p.add_argument('--sam-emitter', choices=['host', 'device', 'device-comments'], default='host',
                   help='who makes the SAM text of a batch: -t host threads (default) or the GPU (merged CIGAR, NM, MD / cs, SA and the lines themselves, on '
                        'VMX_EMIT_CONTEXTS contexts of their own); with --copycomments, --bam-tags, or a reference that holds letters other than ACGTN, the host '
                        'emitter is used. device-comments: the GPU also copies the comments (--copycomments, --bam-tags), so only such a reference falls back')
    p.add_argument('--keep-unmapped', action='store_true',
                   help='modes H, L, S and R: a read that aligns nowhere, that the aligner skipped or whose SAM emission fails stays in the output as one '
                        'unmapped record (FLAG 4, MAPQ 0, the read and its qualities as given, RG and its comment fields) at its input position, so that '
                        'every input read occurs once; the reference, and the default, drop such reads. Every emitter and writer takes it; with '
                        '--bam-writer native-sort the unmapped records come last')
    p.add_argument('--depth', metavar='PREFIX', default=None,
                   help='per-window depth of coverage of the records the run writes, taken while their lines are made (on the GPU under --sam-emitter device): '
                        'PREFIX.regions.bed (contig, start, end, mean depth per window, empty windows included) and PREFIX.summary.txt (contig, length, covered '
                        'bases, mean; a last line `total`). M, = and X columns count, D and N do not (samtools depth without -J); means have two decimals. Every '
                        'mode, emitter and -o kind takes it')
    p.add_argument('--depth-window', type=int, default=500, help='--depth: the window size in bases (default 500; at most 2^28 windows in all)')
    p.add_argument('--depth-mapq', type=int, default=0, help='--depth: only records whose MAPQ column is at least this count (default 0)')
    return p


last_timing = {}          # wall seconds of the last main() call by phase (tools/driver_bench.py reads it)


def _keep_heap_pages(sw=None):
    """A window of input is ~1 GB of blobs, a batch's SAM text ~125 MB, all short-lived: glibc serves blocks that large from fresh mmap()s and
    unmaps them on free, so every byte the host pipeline writes lands on a page that is faulted in and zeroed first — measured on the FASTQ
    parser alone: 1.25 -> 2.85 GB/s once the pages are reused. One arena, no mmap for malloc, no trimming: freed blocks stay in the heap and
    the next window / batch reuses them. (VMX_DRIVER_MALLOPT=0 leaves the allocator alone.)"""
    if not (sw or _switches())['VMX_DRIVER_MALLOPT']:
        return
    try:
        import ctypes
        libc = ctypes.CDLL(None)
        libc.mallopt(-8, 1)                     # M_ARENA_MAX: worker threads allocate from the main heap too
        libc.mallopt(-4, 0)                     # M_MMAP_MAX: no direct mmap for large requests
        libc.mallopt(-1, 2 ** 31 - 1)           # M_TRIM_THRESHOLD: do not hand freed memory back
        libc.mallopt(-2, 256 << 20)             # M_TOP_PAD: grow the heap in large steps
    except Exception:
        pass


# ---------------------------------------------------------------- the stages of main(), in the order it runs them

def _parse_args(argv, comm, sw):
    """stage 1: the options, checked as far as they can be before anything is opened"""
    args, _unknown = build_parser().parse_known_args(argv)          # unknown flags are ignored like the reference's parse_known_args (vacmap:152)
    if comm is None:                            # (a process of its own, not a test harness that shares the interpreter)
        _keep_heap_pages(sw)
    try:
        _bam_tag_select(args.bam_tags)
    except ValueError as e:
        sys.exit(str(e))
    if args.o != '-' and not (args.o.endswith('.sam') or args.o.endswith('.bam') or args.o.endswith('.paf')):
        sys.exit("Output path must end with .sam, .paf, .bam, .sorted.bam, or be '-' for stdout.")
    args.paf = args.o.endswith('.paf')                  # PAF lines (vm_paf_emit / vm_paf_emit_device) on every text path a .sam takes; no header
    if args.paf and (args.copycomments or args.bam_tags):
        sys.exit('%s cannot be written to %s: a PAF line carries no comment fields; write .sam or .bam, or drop the option' % ('--copycomments' if args.copycomments else '--bam-tags', args.o))
    if args.keep_unmapped and args.mode == 'asm':
        sys.exit('--keep-unmapped is for the read modes H, L, S and R: -mode asm takes whole contigs, which nobody wants as unmapped records')
    if args.depth is not None and (not args.depth or args.depth_window < 1 or not 0 <= args.depth_mapq <= 255):
        sys.exit('--depth needs a file prefix, --depth-window a size of at least 1 and --depth-mapq a threshold in 0 .. 255')
    args.native_bam = args.bam_writer in ('native', 'native-sort') and args.o.endswith('.bam')
    args.native_sort = args.bam_writer == 'native-sort' and args.o.endswith('sorted.bam')
    if args.native_bam and args.o.endswith('sorted.bam') and not args.native_sort:
        sys.exit('--bam-writer native writes unsorted BAM only: write %s with --bam-writer native-sort or samtools, or name the output .bam' % args.o)
    return args


@contextlib.contextmanager
def _process_groups(comm, sw):
    """stage 2: who this process is among the ranks (comm, world, rank, local_rank, text_group, force). Under torchrun, or with VMX_FORCE_DIST=1,
    the groups are created here and destroyed on the way out — after a barrier when the run succeeded: no rank leaves while rank 0 still
    gathers and writes."""
    net = types.SimpleNamespace(comm=comm, world=1, rank=0, local_rank=0, text_group=None, force=comm is None and sw['VMX_FORCE_DIST'])
    own = comm is None and (sw['WORLD_SIZE'] > 1 or net.force)
    if own:
        import torch, torch.distributed as dist
        net.comm, net.local_rank = dist, sw['LOCAL_RANK']
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29541')
        torch.cuda.set_device(net.local_rank)
        dist.init_process_group(backend='nccl', device_id=torch.device('cuda', net.local_rank), rank=sw['RANK'], world_size=sw['WORLD_SIZE'])
    try:
        if own:
            # SAM text is host data gathered from a writer THREAD: a gloo (CPU) group suits it — an object gather over the nccl group would
            # stage its byte tensors on the calling thread's current device (cuda:0 in a new thread), not the rank's — and its timeout turns
            # a peer that died into an error instead of a hang
            import datetime
            net.text_group = net.comm.new_group(backend='gloo', timeout=datetime.timedelta(seconds=sw['VMX_GATHER_TIMEOUT']))
        if net.comm is not None:
            net.world, net.rank = net.comm.get_world_size(), net.comm.get_rank()
        yield net
        if own:
            net.comm.barrier()
    finally:
        if own:
            net.comm.destroy_process_group()


@contextlib.contextmanager
def _context_and_index(args, net, device):
    """stage 3: the first context and the index in its HBM: found or built by rank 0 (indexfile.find_index), broadcast to the others"""
    from .lib import Context
    ctx, index = Context(device), None
    try:
        if net.rank == 0:
            from .indexfile import find_index
            index = find_index(ctx, args.ref, int(args.k), int(args.w), write=not args.nowriteindex, log=sys.stderr, reader=args.ref_reader, gzip=args.gzip_inflate)
        if net.world > 1 or net.force:
            import torch
            from .dist import broadcast_index
            dev = torch.device('cuda', device) if torch.cuda.is_available() else torch.device('cpu')
            built = index
            index, t_bc = broadcast_index(ctx, built, src=0, device=dev, self_replica=(net.world == 1))
            if built is not None and built is not index:
                built.close()
            if net.force and net.rank == 0:
                sys.stderr.write('vacmapx: VMX_FORCE_DIST: process group %s, world %d, index through broadcast_index in %.2f s\n' % (net.comm.get_backend(), net.world, t_bc))
        yield ctx, index
    finally:
        if index is not None:
            index.close()
        ctx.close()


def _alignment_options(args, lib):
    """stage 4: (aligner parameters, read group, emitter options), the same for the read modes and asm"""
    from .lib import SamOpts
    prm = lib.params(args.mode)                     # mode defaults (vacmap:257-296), then the explicit options
    prm.check_num = args.c; prm.global_maxdiff = args.globalmaxdiff; prm.local_maxdiff = args.localmaxdiff
    prm.eqx = 1 if args.eqx else 0; prm.hardclip = 1 if args.H else 0
    if args.nodiscard: prm.nodiscard = 1
    if args.maxdivergence is not None: prm.maxdivergence = args.maxdivergence
    if args.globalpenalty is not None: prm.global_skipcost = args.globalpenalty
    if args.localpenalty is not None: prm.local_skipcost = args.localpenalty
    # read group: always present, like the reference (vacmap:186-218) — {'ID': '1', 'SM': 'sample'} unless --rg-* options are given
    rg = {}
    for a, tag in RG_ARGS:
        v = getattr(args, a.replace('-', '_'))
        if v is not None:
            rg[tag] = str(v)
    if rg and 'ID' not in rg:
        sys.exit('The --rg-id option is required when any other --rg-* option is supplied.')
    if not rg:
        rg = {'ID': '1', 'SM': 'sample'}
    mark = args.markunbalancetra or args.mode in ('H', 'L')          # mode defaults of vacmap:286-296 (False for asm unless asked)
    opts = SamOpts(int(bool(args.MD)), int(args.cs != 'long'), int(bool(args.L)), int(bool(mark)), int(bool(args.H)), int(bool(args.fakecigar)), rg['ID'].encode(),
                   int(args.mode == 'asm'), int(bool(args.keep_unmapped)))
    return prm, rg, opts


def _sharding(args, net):
    """stage 5: True for range mode (every rank parses its own byte range of each input and writes its own part of the SAM file), False for
    the batch scheme (every rank parses everything and keeps every N-th batch, rank 0 gathers the text)"""
    plain = all(_is_plain_fastx(pth) for grp in args.read for pth in grp)
    range_mode = net.world > 1 and args.mode != 'asm' and args.shard != 'batch' and plain and (args.o.endswith('.sam') or args.paf)
    if net.world > 1 and args.shard == 'range' and not range_mode:
        sys.exit('--shard range needs uncompressed FASTA / FASTQ input and a .sam or .paf output path')
    if range_mode:
        # every rank writes <out>.partNNN and rank 0 joins them: they must land in one directory. Ranks on several hosts only see each other's
        # parts on a shared file system — nothing here can check that, so `auto` falls back to the batch scheme (text gathered over gloo) and an
        # explicit `--shard range` goes on with a warning
        import socket
        hosts = [None] * net.world
        net.comm.all_gather_object(hosts, socket.gethostname(), group=net.text_group)
        if len(set(hosts)) > 1:
            if args.shard == 'auto':
                range_mode = False
                if net.rank == 0:
                    sys.stderr.write('vacmapx: ranks on %d hosts: --shard auto uses the batch scheme (SAM text gathered by rank 0); --shard range needs %s.partNNN on a shared file system\n' % (len(set(hosts)), args.o))
            elif net.rank == 0:
                sys.stderr.write('vacmapx: ranks on %d hosts with --shard range: %s.partNNN of every rank must be visible to rank 0 (shared file system)\n' % (len(set(hosts)), args.o))
    return range_mode


class Output:
    """What -o names on this rank, behind one interface: stdout, a text file, a rank's part file, a samtools pipe, a BamWriter or a
    SortedBamWriter (`native`: it takes a window as parts, bamout.BamWriter.write_parts). `sink` stays None on a rank that writes nothing."""

    def __init__(self, stdout=False, native=False):
        self.sink, self.proc, self.stdout, self.native, self.closed = None, None, stdout, native, False

    def write(self, data):
        self.sink.write(data)

    def write_parts(self, blobs, offs, order_keys):
        self.sink.write_parts(blobs, offs, order_keys)

    def flush(self):
        self.sink.flush()

    def fd(self):
        """the descriptor the batches' texts can be written to directly, or None"""
        try:
            return self.sink.fileno()
        except Exception:
            return None

    def finish(self):
        """the end of a run that succeeded: the output is closed (stdout: flushed); returns samtools' exit code after a pipe, else None"""
        if self.sink is None or self.closed:
            return None
        if self.stdout:
            self.sink.flush()
        else:
            self.sink.close()
        self.closed = True                               # (a close that raised leaves the rest to abort())
        return self.proc.wait() if self.proc is not None else None

    def abort(self):
        """the end of a run that failed: nothing more is written, the file is closed as it is, samtools is waited for, a native writer gives
        up its device memory and its run files"""
        if self.sink is None or self.closed:
            return
        self.closed = True
        with contextlib.suppress(Exception):
            if self.native:
                self.sink._abort()
            elif not self.stdout:
                self.sink.close()
        if self.proc is not None:
            self.proc.wait()

    def note(self):
        """the tail of the final stderr line after --bam-writer native-sort: the index file and what the merge in close() cost"""
        s = self.sink
        if not hasattr(s, 'merge_seconds'):
            return ''
        return '; sorted by coordinate, index %s.csi (merge of %d runs, %.1f MB of records: %.2f s)' % (s.path, len(s.runs), s.run_bytes / 1e6, s.merge_seconds)


def _text_sink(path):
    """'-' / .sam: text; .bam / .sorted.bam: a `samtools view -b` / `samtools sort --write-index` pipe (output_functions.py:200-208)"""
    if path == '-':
        return sys.stdout.buffer, None
    if path.endswith('.sam') or path.endswith('.paf'):
        return open(path, 'w+b'), None
    if not shutil.which('samtools'):
        sys.exit('writing %s needs the samtools binary on PATH (the reference pipes SAM text into it too); write .sam instead' % path)
    cmd = ['samtools', 'sort', '-@', '8', '--write-index', '-o', path, '-'] if path.endswith('sorted.bam') else ['samtools', 'view', '-b', '-@', '8', '-o', path, '-']
    proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, bufsize=1 << 20)
    return proc.stdin, proc


@contextlib.contextmanager
def _open_output(args, net, range_mode, index, rg, argv, device):
    """stage 6: the Output of this rank with the header in it (rank 0 writes it; in range mode into its part). A run that fails from here on
    aborts the output on its way out; a run that succeeds ends it in _finish."""
    out = Output(stdout=args.o == '-', native=args.native_bam)
    try:
        if range_mode:
            out.sink = open('%s.part%03d' % (args.o, net.rank), 'w+b')
        if net.rank == 0:
            head = sam.header_lines(list(zip(index.names, index.lens)), ' '.join(sys.argv if argv is None else ['vacmapx'] + list(argv)), rg)
            if args.native_bam:                                 # the header goes in as the BAM header
                from .bamout import BamWriter, SortedBamWriter
                if args.native_sort and args.workdir:           # sorted runs now, merge + index in close()
                    os.makedirs(args.workdir, exist_ok=True)
                out.sink = SortedBamWriter(args.o, head, device=device, workdir=args.workdir) if args.native_sort else BamWriter(args.o, head, device=device)
            else:
                if not range_mode:
                    out.sink, out.proc = _text_sink(args.o)
                for ln in ([] if args.paf else head):            # (PAF has no header)
                    out.write(ln.encode() + b'\n')
        yield out
    except BaseException:
        out.abort()
        raise


def _finish(out, rank, report):
    """stage 8: the output is closed, samtools waited for, and rank 0 writes the final stderr lines: report(tail) gives their text"""
    rc = out.finish()
    if rank != 0:
        return
    if rc:
        sys.stderr.write('Error: samtools exited with code %d\n' % rc)
    sys.stderr.write(report(out.note()))


def _blob(parts):
    import numpy as np
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(x) for x in parts], out=off[1:])
    return np.frombuffer(b''.join(parts) or b'\0', np.uint8), off


VM_ERR_UNSUPPORTED = -7


class DepthSink:
    """--depth PREFIX: the run's depth-of-coverage accumulators (lib.Depth; the rule: include/vacmapx.h at vm_depth_add). Under the device emitter one
    accumulator per emit context, attached when the context makes its first text of the stream (so the sizing run's warm-up calls do not count): the
    emit calls themselves add, on the GPU. Under the host emitter one host accumulator that the emit threads add to (vm_depth_add: atomic adds). A
    context that is given up hands its counts to the host accumulator first. finish() merges everything, sums the ranks on rank 0 and writes
    PREFIX.regions.bed and PREFIX.summary.txt there. Without --depth nothing is made and every method returns at once."""

    def __init__(self, args, lib, index):
        self.on = args.depth is not None
        self.args, self.lib, self.index = args, lib, index
        self.host, self.dev, self.lock = None, {}, threading.Lock()

    def _create(self, ctx=None):
        from .lib import Depth
        return Depth.create(self.index, self.args.depth_window, self.args.depth_mapq, ctx=ctx, lib=self.lib)

    def attach(self, ctx):
        """before a device emit call of the stream on ctx"""
        if self.on and id(ctx) not in self.dev:
            d = self._create(ctx)
            ctx.attach_depth(d)
            with self.lock:
                self.dev[id(ctx)] = (ctx, d)

    def add_host(self, opts, nb, no, sb, so, raw, nthreads):
        """beside a host emit call"""
        if not self.on:
            return
        with self.lock:
            if self.host is None:
                self.host = self._create()
        self.host.add(self.index, opts, nb, no, sb, so, raw, nthreads=nthreads)

    def release(self, ctx):
        """before ctx is closed: its accumulator's counts move to the host accumulator"""
        with self.lock:
            e = self.dev.pop(id(ctx), None)
            if e is not None and self.host is None:
                self.host = self._create()
        if e is not None:
            ctx.attach_depth(None)
            with self.lock:
                self.host.merge(e[1])
            e[1].close()

    def close(self):
        for ctx, d in self.dev.values():
            if ctx.h:
                ctx.attach_depth(None)
            d.close()
        self.dev = {}
        if self.host is not None:
            self.host.close(); self.host = None

    def finish(self, net):
        """after the last emit call: one accumulator (a device one when there is any), the other ranks' tables added on rank 0, the two files"""
        if not self.on:
            return
        try:
            accs = [d for _, d in self.dev.values()] + ([self.host] if self.host is not None else [])
            if not accs:
                accs = [self._create()]; self.host = accs[0]
            dst = accs[0]
            for d in accs[1:]:
                dst.merge(d)
            if net.world > 1:
                from .dist import gather_lines
                tables = gather_lines(dst.counts()[0], dst=0, group=net.text_group)
                if net.rank == 0:
                    for t in tables[1:]:
                        dst.add_counts(t)
            if net.rank == 0:
                with open(self.args.depth + '.regions.bed', 'wb') as f:
                    f.write(dst.regions())
                with open(self.args.depth + '.summary.txt', 'wb') as f:
                    f.write(dst.summary())
        finally:
            self.close()


def _carries_comments(args, path):
    """a .bam input's comments are the tags --bam-tags selected and go to the emitter with or without --copycomments; FASTA / FASTQ comments need --copycomments"""
    return bool(args.bam_tags) if path.endswith('.bam') else args.copycomments


def _device_emitter_wanted(args, rank):
    """--sam-emitter device, unless the run copies comments (with `device` the filter of :20686 stays on the host emitter): one stderr line says
    so. --sam-emitter device-comments hands the comments to the device emitter instead."""
    if args.sam_emitter == 'device-comments':               # the comment stage of k_sam_lines: neither fallback below is taken
        return True
    if args.sam_emitter != 'device':
        return False
    if args.copycomments:
        if rank == 0:
            sys.stderr.write('vacmapx: --copycomments needs the host SAM emitter: --sam-emitter device is not used\n')
        return False
    if args.bam_tags:                                       # the tags travel as comments, which only the host emitter copies
        _device_emitter_given_up('--bam-tags carries the tags as comments, which --sam-emitter device does not copy', rank)
        return False
    return True


def _device_emitter_given_up(why, rank):
    if rank == 0:
        sys.stderr.write('vacmapx: the host SAM emitter is used for the whole run (%s)\n' % why)


def _run_asm(args, net, lib, ctx, index, prm, opts, out, device, t_start, depth):
    """-mode asm (src/vacmap/vacmap:245-255, :394-411; worker mammap_asm.py:23462-23511): every input sequence is an assembly contig. --eqx is
    forced and maxdivergence set to 1 by vm_params_default(VM_MODE_ASM); contigs are aligned in groups (the long ones of a group side by side on
    the GPU) and their SAM lines written in input order. A contig the reference would skip (raised) is logged and skipped.
    With N ranks every rank parses the input, contig c of it goes to rank c mod N (contigs are independent: no data-path collective), and
    rank 0 gathers each group's lines and writes them in input order. Returns the final stderr line as _finish takes it."""
    from .lib import align_batch_raw, sam_emit, sam_emit_device, paf_emit, paf_emit_device, VmxError
    world, rank = net.world, net.rank
    on_device = [_device_emitter_wanted(args, rank)]
    with_c = args.copycomments or bool(args.bam_tags)
    if not args.workdir:
        sys.exit('workdir not provided! -workdir /path/to/workdir')                      # vacmap:247-249
    os.makedirs(args.workdir, exist_ok=True)
    # the fork hard-codes these, whatever -c / -maxdivergence say: check_num = -1 (mammap_asm.py:23206), maxdivergence = 1.0 (:23483), --eqx
    prm.eqx = 1; prm.check_num = -1; prm.maxdivergence = 1.0
    seen = set(); n_contigs = n_lines = n_skipped = 0

    def flush(group):
        """group: (input index, name, sequence, quality, comment — bytes) of consecutive input contigs, the same list on every rank"""
        nonlocal n_lines, n_skipped
        share = [g for g in group if g[0] % world == rank]
        done = {}                                                                           # input index -> text of its lines, None = skipped
        if share:
            nb, no = _blob([g[1] for g in share]); sb, so = _blob([g[2] for g in share])
            qb, qo = _blob([g[3] for g in share]); cb, co = _blob([g[4] for g in share])
            raw = align_batch_raw(ctx, index, prm, sb, so)
            # the asm emitter (iterator_get_bam_dict_str, mammap_asm.py:22757) in the native emitter: vm_sam_opts.asm_mode
            text = None
            if on_device[0]:                                                                # --sam-emitter device: on the run's own context
                try:
                    dev_c = with_c and args.sam_emitter == 'device-comments'
                    depth.attach(ctx)
                    if args.paf:
                        text, toff, _, ns = paf_emit_device(ctx, index, opts, nb, no, sb, so, raw)
                    else:
                        text, toff, _, ns = sam_emit_device(ctx, index, opts, nb, no, sb, so, raw, quals=qb, qual_off=qo, comments=cb if dev_c else None,
                                                            com_off=co if dev_c else None)
                except VmxError as e:
                    if e.code != VM_ERR_UNSUPPORTED:
                        raise
                    on_device[0] = False
                    _device_emitter_given_up(str(e), rank)
                    depth.release(ctx)
            if text is None:
                depth.add_host(opts, nb, no, sb, so, raw, max(1, args.t))
            if text is None and args.paf:
                text, toff, _, ns = paf_emit(lib, index, opts, nb, no, sb, so, raw, nthreads=max(1, args.t))
            elif text is None:
                text, toff, _, ns = sam_emit(lib, index, opts, nb, no, sb, so, raw, quals=qb, qual_off=qo, comments=cb if with_c else None,
                                             com_off=co if with_c else None, nthreads=max(1, args.t))
            for x, g in enumerate(share):
                if raw.status[x] != 0:                                                      # the worker's except (:23493-23498)
                    sys.stderr.write('%s is not aligned.\n' % g[1].decode()); done[g[0]] = None
                else:
                    done[g[0]] = text[int(toff[x]):int(toff[x + 1])].tobytes()
            raw.close()
        if world > 1:
            from .dist import gather_lines
            parts = gather_lines(done, dst=0, group=net.text_group)
            if rank != 0:
                return
            done = {}
            for d in parts:
                done.update(d)
        text = [done[gi] for gi in sorted(done) if done[gi] is not None]
        n_skipped += len(done) - len(text)
        n_lines += sum(t.count(b'\n') for t in text)
        if args.native_bam and text:                                                        # --bam-writer native: the group's lines in one BAM call
            text = [b''.join(text)]
        for t in text:
            out.write(t)

    group, gbases = [], 0
    for path in (p for grp in args.read for p in grp):
        # (.bam input like every other mode: vacmap:452-470)
        with contextlib.closing(_input_chunks(path, 64, lib, device, args.bam_reader, bam_tags=args.bam_tags, fastx_reader=args.fastx_reader, gzip_inflate=args.gzip_inflate, fasta_reads=args.fasta_reads)) as chunks:
            for ch in _first_of_each_name(chunks, seen, lib):
                if not _carries_comments(args, path):
                    import numpy as np
                    ch['comments_off'] = np.zeros(len(ch['seqs_off']), np.int64)
                nb, no, sb, so = ch['names'].tobytes(), ch['names_off'], ch['seqs'].tobytes(), ch['seqs_off']
                qb, qo, cb, co = ch['quals'].tobytes(), ch['quals_off'], ch['comments'].tobytes(), ch['comments_off']
                for i in range(len(so) - 1):
                    keep = n_contigs % world == rank                                       # the other ranks' contigs only hold their place
                    group.append((n_contigs, nb[no[i]:no[i + 1]], sb[so[i]:so[i + 1]] if keep else b'', (b'' if args.Q or not keep else qb[qo[i]:qo[i + 1]]),
                                  cb[co[i]:co[i + 1]] if keep else b''))
                    n_contigs += 1
                    gbases += so[i + 1] - so[i]
                    if len(group) >= 64 * world or gbases >= 400_000_000 * world:
                        flush(group); group, gbases = [], 0
    if group:
        flush(group)
    return lambda tail: 'vacmapx: %d contigs, %d %s lines, %d contigs skipped, %.1f s%s\n' % (n_contigs, n_lines, 'PAF' if args.paf else 'SAM', n_skipped, max(time.time() - t_start, 0.001), tail)


class Window:
    """a window of input (blobs) with the rank's plan of it; futs[i]: the SAM text of batch i, on its way through the emit pool"""

    def __init__(self, wnd, plan):
        self.wnd, self.plan = wnd, plan
        self.has_q = bool(wnd['quals_off'][-1]); self.has_c = bool(wnd['comments_off'][-1])
        self.futs = [None] * len(plan)
        self.left = len(plan)
        self.ready = threading.Event()              # every batch of the window has been aligned and handed to the emit pool
        if not plan:
            self.ready.set()


class Batch:
    """what an aligner thread is handed: batch i of window w, and what a feeder prepared of it — (read blob, offsets, the upload slot that
    holds them in HBM) — or None when the aligner gathers and uploads the reads itself"""

    def __init__(self, w, i, fed=None):
        self.w, self.i, self.fed = w, i, fed


class ReadStream:
    """Stage 7 for the read modes. A reader thread parses windows of --window-batches x --batch-reads reads (wq), the aligner threads of
    pipeline.Pipeline.run_stream take the batches of each window in schedule order (job_source; through the feeders, which gather and upload
    ahead of them), hand the records to the emit pool, and the writer thread writes every window's lines in input order (oq). The first
    error of any thread (errs) ends all of them. run() starts and joins the threads; leaving the `with` block releases the pinned pool and the
    pipeline's contexts."""

    def __init__(self, args, sw, net, lib, ctx, index, prm, opts, out, range_mode, device, t_start, depth):
        from . import lib as V, pipeline
        self.V = V                                          # (the module, imported late: see the note at the imports)
        self.depth = depth                                  # --depth (DepthSink)
        self.args, self.sw, self.net, self.lib, self.index, self.prm, self.opts, self.out = args, sw, net, lib, index, prm, opts, out
        self.range_mode, self.device, self.rank, self.world = range_mode, device, net.rank, net.world
        self.ramp_on = sw['VMX_DRIVER_RAMP'] and not sw['VMX_NO_WARM']
        # host threads (-t in all): `inflight` of them feed the GPU (gather a batch's reads, vm_align_batch) and mostly wait for it; the SAM
        # text of finished batches is produced by a pool of emit_jobs concurrent vm_sam_emit calls of emit_threads threads each, so that the
        # GPU never waits for text and the text never waits for the GPU
        emit_total = sw['VMX_EMIT_THREADS'] or args.t
        self.emit_jobs = max(1, min(4, emit_total // 4))
        self.emit_threads = max(1, emit_total // self.emit_jobs)
        self.emit_pool = None
        # --sam-emitter device: the emit jobs run on VMX_EMIT_CONTEXTS threads, each with a context of its own (as the feeders have); the aligner
        # threads and their contexts are what they are without it
        self.emit_device = _device_emitter_wanted(args, net.rank)
        self.emit_comments = args.sam_emitter == 'device-comments'
        self.emit_ctxs, self.emit_free, self.emit_local = [], queue.Queue(), threading.local()
        self.emit_total = emit_total
        if self.emit_device:
            self.emit_jobs = max(1, sw['VMX_EMIT_CONTEXTS'])
        self.counts = {'reads': 0, 'lines': 0, 'skipped': 0}
        self.rank_hashes, self.rank_hash_file = [], []      # range mode: the names this rank has seen, compared across the ranks at the end
        self.errs = []
        self.n_slots = max(2, sw['VMX_DRIVER_WINDOWS'])      # (1.6 M-read run, profiles/r05_driver_long_*: 3 windows of 8 batches 145 k reads/s, 6 x 8: 180 k, 4 x 16: 195 k, 10 x 4: 205 k)
        self.slots = threading.Semaphore(self.n_slots)      # windows in memory at a time (input blobs + SAM text)
        self.wq = queue.Queue(maxsize=2)                    # reader -> job source
        self.oq = queue.Queue()                             # windows in input order -> writer
        self.pending = []                                   # windows taken from the reader ahead of the workers (the sizing run)
        self.sizing = None                                  # the sizing batch (blob, offsets): also sizes the feeders' upload slots
        self.feed_free, self.feed_ready, self.feed_lock = queue.Queue(), queue.Queue(), threading.Lock()
        self.feed_ctxs, self.feed_slots, self.feed_threads = [], [], []
        self.out_fd = out.fd() if (self.rank == 0 or range_mode) and sw['VMX_DRIVER_WRITEV'] else None
        self.pinned = self.pipe = None
        try:
            self.pipe = pipeline.Pipeline(index, prm, device=device, inflight=1 if self.ramp_on else (args.inflight or 5), first_ctx=ctx)
            self.blocking_sync(self.pipe.ctxs)
            # the batch's reads are gathered into page-locked memory: vm_align_batch's upload becomes a DMA the aligner thread does not wait for
            if sw['VMX_DRIVER_PINNED']:
                self.pinned = V.PinnedPool(lib, device)
            for _ in range(self.emit_jobs if self.emit_device else 0):       # before the sizing run: trim_to_memory then sees their HBM (size_emitters)
                ecx = V.Context(device, lib=lib)
                self.emit_ctxs.append(ecx); self.emit_free.put(ecx)
            self.blocking_sync(self.emit_ctxs)
        except BaseException:
            self.close()
            raise
        # Feeders: threads with a context of their own take the next batch of the schedule, gather its reads into page-locked memory and stream
        # them into HBM (vm_reads_reupload into a few reusable slots) AHEAD of the aligning contexts, which then run vm_align_resident — the
        # aligner thread's context no longer idles through the gather, and the copy of batch i + 1 runs under the kernels of batch i
        self.n_feed = sw['VMX_DRIVER_FEEDERS'] if self.pinned is not None else 0
        now = time.time()
        self.t0 = self.t_prog = now; self.n_prog = 0; self.next_prog = 100000
        self.tm = {'setup': now - t_start, 'wait_input': 0.0, 'assemble_write': 0.0, 'job_gather': 0.0, 'job_align': 0.0, 'job_emit': 0.0}
        self.tml = threading.Lock()

    def close(self):
        for ecx in self.emit_ctxs:
            ecx.close()
        self.emit_ctxs = []
        if self.pinned is not None:
            self.pinned.close(); self.pinned = None
        if self.pipe is not None:
            self.pipe.close(drop_first=True); self.pipe = None       # (the first context is the caller's)

    def blocking_sync(self, ctxs):
        if not self.sw['VMX_SPIN_SYNC']:
            for cx in ctxs:
                cx.set_blocking_sync(True)                # the emitters need the cores the waiting aligner threads would spin on

    def add_time(self, key, dt):
        with self.tml:
            self.tm[key] += dt

    def progress(self, count):
        """the reference's progress line, every 100 000 sequences (vacmap:498-514)"""
        if self.rank != 0 or count < self.next_prog:
            return
        now = time.time()
        dt, tt = max(now - self.t_prog, 0.001), max(now - self.t0, 0.001)
        sys.stderr.write('%d / sec in the last %d minutes, %d / sec AVG. %d sequences processed.\n'
                         % (round((count - self.n_prog) / dt), max(round(dt / 60), 1), round(count / tt), count))
        self.t_prog, self.n_prog = now, count
        self.next_prog = (count // 100000 + 1) * 100000

    def windows(self):
        """input records in arrival order as blobs (names, upper-cased sequences, qualities, comments), de-duplicated by name
        (vacmap:457,475,487; in range mode inside the rank's own part of the input), one window of at most win_reads reads at a time. A plain
        file is parsed in slices by `parse_threads` threads ahead of the consumer (one thread parses ~3 GB/s: a third of what one GPU aligns)."""
        import numpy as np
        args, sw, seen = self.args, self.sw, set()
        parse_threads = args.parse_threads or sw['VMX_PARSE_THREADS'] or max(1, min(4, args.t // 4))
        win_reads = max(1, args.batch_reads * args.window_batches)
        share = (self.rank, self.world) if self.range_mode else (0, 1)
        slice_bytes = max(1 << 20, int(sw['VMX_SLICE_MB'] * (1 << 20)))
        for file_no, path in enumerate(p for grp in args.read for p in grp):
            with contextlib.closing(_input_chunks(path, win_reads, self.lib, self.device, args.bam_reader, parse_threads, share, slice_bytes, args.bam_tags, args.fastx_reader, args.gzip_inflate, args.fasta_reads)) as chunks:
                for ch in _first_of_each_name(chunks, seen, self.lib):
                    n = len(ch['seqs_off']) - 1
                    if self.range_mode and n:
                        self.rank_hashes.append(name_hashes(ch['names'], ch['names_off']))
                        self.rank_hash_file.append(np.full(n, file_no, np.int32))          # ... in INPUT order: (file, byte range = rank)
                    if args.Q:
                        ch['quals_off'] = np.zeros(n + 1, np.int64)
                    if not _carries_comments(args, path):
                        ch['comments_off'] = np.zeros(n + 1, np.int64)
                    if n:
                        yield ch

    def to_workers(self, item):
        """a window (None: the end, an exception: the reader's failure) into wq; False when the run failed meanwhile"""
        while not self.errs:
            try:
                self.wq.put(item, timeout=0.2)
                return True
            except queue.Full:
                pass
        return False

    def reader(self):
        """input parsing runs ahead of the aligners (the FASTX reader releases the GIL)"""
        try:
            with contextlib.closing(self.windows()) as wins:
                for wnd in wins:
                    if not self.to_workers(wnd):
                        return
            self.to_workers(None)
        except BaseException as e:
            self.to_workers(e)

    def from_reader(self):
        """the next item of wq; None (the end) once the run has failed and the reader may have given up"""
        while True:
            try:
                return self.wq.get(timeout=0.2)
            except queue.Empty:
                if self.errs:
                    return None

    def size_run(self, cx):
        self.V.align_batch_raw(cx, self.index, self.prm, self.sizing[0], self.sizing[1]).close()

    def size_emitters(self, has_q):
        """--sam-emitter device: every emit context makes the sizing batch's text once (dropped), so that its buffers are in HBM when
        trim_to_memory looks; a reference the device emitter cannot serve shows here, before any batch"""
        import numpy as np
        if not self.emit_device or self.sizing is None:
            return
        sb, so = self.sizing
        n = len(so) - 1
        nb, no = np.full(n, ord('r'), np.uint8), np.arange(n + 1, dtype=np.int64)
        raw = self.V.align_batch_raw(self.pipe.ctxs[0], self.index, self.prm, sb, so)
        try:
            for ecx in self.emit_ctxs:
                if self.args.paf:
                    self.V.paf_emit_device(ecx, self.index, self.opts, nb, no, sb, so, raw)
                    continue
                self.V.sam_emit_device(ecx, self.index, self.opts, nb, no, sb, so, raw, quals=np.full(int(so[-1]), ord('I'), np.uint8) if has_q else None, qual_off=so if has_q else None)
        except self.V.VmxError as e:
            if e.code != VM_ERR_UNSUPPORTED:
                raise
            self.give_up_device(str(e))
        finally:
            raw.close()

    def give_up_device(self, why):
        """the host emitter from here on: the emit jobs share the host threads a host run has, and the emit contexts no thread owns are closed
        (a thread that owns one closes it when it next emits: drop_emit_context)"""
        with self.tml:
            if not self.emit_device:
                return
            self.emit_device = False
            self.emit_threads = max(1, self.emit_total // self.emit_jobs)
        _device_emitter_given_up(why, self.rank)
        while True:
            try:
                cx = self.emit_free.get_nowait()
            except queue.Empty:
                break
            self.depth.release(cx); cx.close()
        self.drop_emit_context()

    def drop_emit_context(self):
        cx = getattr(self.emit_local, 'cx', None)
        if cx is not None:
            self.depth.release(cx)
            cx.close(); self.emit_local.cx = None

    def plan(self, wnd):
        """the rank's batches of a window: lists of read indices in schedule order"""
        import numpy as np
        from . import pipeline
        plan = pipeline.plan_batches(np.diff(wnd['seqs_off']), self.args.batch_reads, self.args.window_batches)
        if not self.range_mode:
            plan = [plan[i] for i in range(self.rank, len(plan), self.world)]       # static sharding: batch i -> rank i mod N (range mode: the rank's own reads)
        return plan

    def size_contexts(self):
        """Size every context's grow-only work pools ONCE, before the stream starts: each context aligns the longest batch of the first window
        (its result is dropped). Without this a context meets its first long-read batch windows later, outgrows the pools its earlier,
        shorter batches sized, and pays for ~50 GB of re-allocation next to two other contexts' pools — seconds with the GPU idle
        (rocprofv3 trace of a 131 k-read run: no kernel resident 73 % of the time, 2 s batches; `profiles/r03_l_*`).
        Then contexts are given up or added by what the HBM holds. Returns Pipeline.run_stream's `ramp` (VMX_DRIVER_RAMP=1), else None."""
        import numpy as np
        pipe, args, size = self.pipe, self.args, self.size_run
        if not self.sw['VMX_NO_WARM']:
            first = self.from_reader()
            self.tm['first_window'] = time.time() - self.t_loop
            self.pending.append(first)
            plan0 = self.plan(first) if first is not None and not isinstance(first, BaseException) else None
            if plan0:
                ix0 = max(plan0, key=lambda ix: int(np.diff(first['seqs_off'])[ix].sum()))
                self.sizing = self.V.blob_gather(self.lib, first['seqs'], first['seqs_off'], ix0)
                # (one context after the other: hipMalloc serialises anyway, and a context that finds no memory left for its pools — a first window of
                # very long reads — is given up with the ones after it instead of failing the run: Pipeline.warm)
                try:
                    n_oom = pipe.warm(run=size, keep=2)
                    if n_oom and self.rank == 0:
                        sys.stderr.write('vacmapx: %d of %d batches in flight given up: no HBM left for their work pools\n' % (n_oom, n_oom + pipe.inflight))
                    self.size_emitters(bool(first['quals_off'][-1]))
                except BaseException as e:
                    self.errs.append(e)
            dropped = pipe.trim_to_memory(self.sw['VMX_MIN_FREE_GB'])
            if dropped and self.rank == 0:
                sys.stderr.write('vacmapx: %d of %d batches in flight given up to keep HBM head-room\n' % (dropped, dropped + pipe.inflight))
            if args.inflight == 0 and not self.ramp_on and not dropped and self.sizing is not None and not self.errs:
                # the scheduler's rule (bench.py runs the same): more batches in flight while another context's pools + head-room fit the HBM
                try:
                    if pipe.grow_to_memory(run=size, max_inflight=8):
                        self.blocking_sync(pipe.ctxs)
                except BaseException as e:
                    self.errs.append(e)
            self.tm['warm'] = time.time() - self.t_loop
        if self.ramp_on and self.sizing is not None and not self.errs:
            return dict(run=size, target=args.inflight, max_inflight=8, on_ctx=None if self.sw['VMX_SPIN_SYNC'] else (lambda cx: cx.set_blocking_sync(True)))
        return None

    def job_source(self):
        """the batches in schedule order; a window is planned when the first worker reaches it"""
        errs, oq = self.errs, self.oq
        while not errs:
            while not self.slots.acquire(timeout=0.2):       # (never parked for good: a failure elsewhere must end the run, not hang it)
                if errs:
                    oq.put(None)
                    return
            t0 = time.time()
            wnd = self.pending.pop(0) if self.pending else self.from_reader()
            self.add_time('wait_input', time.time() - t0)
            if isinstance(wnd, BaseException):
                errs.append(wnd); wnd = None
            if wnd is None:
                self.slots.release()
                break
            self.counts['reads'] += len(wnd['seqs_off']) - 1
            self.progress(self.counts['reads'])
            w = Window(wnd, self.plan(wnd))
            oq.put(w)
            for i in range(len(w.plan)):
                yield Batch(w, i)
        oq.put(None)

    def start_feeders(self):
        src = self.job_source()
        for _ in range(self.n_feed):
            fcx = self.V.Context(self.device, lib=self.lib)
            self.feed_ctxs.append(fcx)
            self.blocking_sync([fcx])
        n_up = (max(self.args.inflight or 8, self.pipe.inflight) if self.ramp_on else self.pipe.inflight) + self.n_feed + 1
        for _ in range(n_up):
            sl = self.V.ResidentReads(self.feed_ctxs[0], concat=self.sizing[0], offsets=self.sizing[1])
            self.feed_slots.append(sl); self.feed_free.put(sl)
        self.feed_threads = [threading.Thread(target=self.feeder, args=(fcx, src)) for fcx in self.feed_ctxs]
        for t in self.feed_threads:
            t.start()

    def stop_feeders(self):
        for _ in self.feed_threads if self.errs else ():
            self.feed_free.put(None)                      # (wakes a feeder that waits for a slot)
        for t in self.feed_threads:
            t.join()
        for sl in self.feed_slots:
            sl.close()
        for fcx in self.feed_ctxs:
            fcx.close()
        self.feed_threads, self.feed_slots, self.feed_ctxs = [], [], []

    def feeder(self, fcx, src):
        try:
            while not self.errs:
                with self.feed_lock:
                    job = next(src, None)
                if job is None:
                    break
                t0 = time.time()
                sb, so = self.V.blob_gather(self.lib, job.w.wnd['seqs'], job.w.wnd['seqs_off'], job.w.plan[job.i], alloc=self.pinned.get)
                sl = self.feed_free.get()
                while sl is None:                        # (a None is only queued to wake a feeder up on an error)
                    if self.errs:
                        return
                    sl = self.feed_free.get()
                sl.reupload(sb, so, ctx=fcx)
                self.add_time('job_gather', time.time() - t0)
                job.fed = (sb, so, sl)
                self.feed_ready.put(job)
        except BaseException as e:
            self.errs.append(e)
        finally:
            self.feed_ready.put(None)

    def fed_jobs(self):
        """what the feeders prepared, in completion order, until all of them are done"""
        done = 0
        while done < self.n_feed:
            job = self.feed_ready.get()
            if job is None:
                done += 1
                continue
            yield job

    def align(self, job, cx):
        """one batch: gather its reads from the window, align (GPU), hand the records to the emit pool; the library calls release the GIL"""
        w, i = job.w, job.i
        ix = w.plan[i]
        if job.fed is not None:                          # reads already in HBM
            sb, so, sl = job.fed
            t0 = t1 = time.time()
            raw = sl.align_raw(self.index, self.prm, ctx=cx)
            self.feed_free.put(sl)
        else:
            t0 = time.time()
            sb, so = self.V.blob_gather(self.lib, w.wnd['seqs'], w.wnd['seqs_off'], ix, alloc=self.pinned.get if self.pinned is not None else None)
            t1 = time.time()
            raw = self.V.align_batch_raw(cx, self.index, self.prm, sb, so)
        t2 = time.time()
        w.futs[i] = self.emit_pool.submit(self.emit, w, ix, sb, so, raw)
        with self.tml:
            tm = self.tm
            tm['job_gather'] += t1 - t0; tm['job_align'] += t2 - t1; tm['device_s'] = tm.get('device_s', 0.0) + raw.stats['ms_total'] * 1e-3
            if self.sw['VMX_DRIVER_TIMING'] == '2':
                sys.stderr.write('batch t=%.3f reads %d bases %d align %.3f device %.3f\n' % (t1 - self.t_loop, len(ix), int(so[-1]), t2 - t1, raw.stats['ms_total'] * 1e-3))
            w.left -= 1
            if w.left == 0:
                w.ready.set()

    def emit_context(self):
        """the calling emit thread's own context (taken when the thread makes its first text)"""
        cx = getattr(self.emit_local, 'cx', None)
        if cx is None:
            cx = self.emit_local.cx = self.emit_free.get_nowait()
        return cx

    def emit(self, w, ix, sb, so, raw):
        """the SAM text of one batch (emit pool): (read indices, text, line offsets, lines, reads skipped)"""
        import numpy as np
        t0 = time.time()
        try:
            if self.sw['VMX_SKIP_EMIT']:                 # diagnostic: aligners alone
                raw.close()
                return ix, np.zeros(0, np.uint8), np.zeros(len(ix) + 1, np.int64), 0, 0
            wnd, gather = w.wnd, self.V.blob_gather
            nb, no = gather(self.lib, wnd['names'], wnd['names_off'], ix)
            qb, qo = gather(self.lib, wnd['quals'], wnd['quals_off'], ix) if w.has_q else (None, None)
            cb, co = gather(self.lib, wnd['comments'], wnd['comments_off'], ix) if w.has_c else (None, None)
            text = None
            if self.emit_device:
                try:
                    dev_c = self.emit_comments and cb is not None
                    self.depth.attach(self.emit_context())
                    if self.args.paf:
                        text, toff, nl, ns = self.V.paf_emit_device(self.emit_context(), self.index, self.opts, nb, no, sb, so, raw)
                    else:
                        text, toff, nl, ns = self.V.sam_emit_device(self.emit_context(), self.index, self.opts, nb, no, sb, so, raw, quals=qb, qual_off=qo,
                                                                    comments=cb if dev_c else None, com_off=co if dev_c else None)
                except self.V.VmxError as e:
                    if e.code != VM_ERR_UNSUPPORTED:
                        raise
                    self.give_up_device(str(e))
            if text is None:
                self.drop_emit_context()
                self.depth.add_host(self.opts, nb, no, sb, so, raw, self.emit_threads)
            if text is None and self.args.paf:
                text, toff, nl, ns = self.V.paf_emit(self.lib, self.index, self.opts, nb, no, sb, so, raw, nthreads=self.emit_threads)
            elif text is None:
                text, toff, nl, ns = self.V.sam_emit(self.lib, self.index, self.opts, nb, no, sb, so, raw, quals=qb, qual_off=qo, comments=cb, com_off=co, nthreads=self.emit_threads)
            if self.args.debug and ns:                  # the reference's per-read failure log (--debug, mammap_clrnano.py:24120-24123)
                nbb = nb.tobytes() if hasattr(nb, 'tobytes') else bytes(nb)
                for x in np.nonzero(np.asarray(raw.status) != 0)[0]:
                    sys.stderr.write('vacmapx --debug: read %s skipped, status %d\n' % (nbb[int(no[x]):int(no[x + 1])].decode(errors='replace'), int(raw.status[x])))
            raw.close()
            self.add_time('job_emit', time.time() - t0)
            return ix, text, toff, nl, ns
        finally:
            if self.pinned is not None:
                self.pinned.release(sb)

    def writer(self):
        """a window's lines in input order (one more gather over the concatenated batch texts) while later windows align and emit"""
        t_cpu0 = time.thread_time()
        try:
            while True:
                w = self.oq.get()
                if w is None:
                    return
                while not w.ready.wait(0.2):
                    if self.errs:
                        return
                done = [f.result() for f in w.futs]
                t0 = time.time()
                self.write_window([r[1] for r in done], [r[2] for r in done], [r[0] for r in done], sum(r[3] for r in done), sum(r[4] for r in done))
                w.wnd = None; w.futs = None
                self.slots.release()
                self.add_time('assemble_write', time.time() - t0)
        except BaseException as e:
            self.errs.append(e)
        finally:
            with self.tml:
                self.tm['writer_cpu'] = time.thread_time() - t_cpu0
            for _ in range(self.n_slots):                # whatever ended the writer, nobody stays parked on a window slot
                self.slots.release()

    def write_window(self, texts, toffs, keys, nl, ns):
        """the batches' texts of one window (texts[b], toffs[b]: the lines of the reads keys[b]) to the output, in the order of the keys; with
        N ranks in the batch scheme rank 0 gathers the other ranks' batches first"""
        if self.world > 1 and not self.range_mode:
            from .dist import gather_lines
            allp = gather_lines((texts, toffs, keys, nl, ns), dst=0, group=self.net.text_group)
            if self.rank == 0:
                texts, toffs, keys = ([x for rp in allp for x in rp[j]] for j in range(3))
                nl = sum(rp[3] for rp in allp); ns = sum(rp[4] for rp in allp)
            else:
                texts = []
        self.counts['lines'] += nl; self.counts['skipped'] += ns
        if not texts:
            return
        if self.args.native_bam:                         # BAM records and BGZF members on the GPU, straight from the batches' texts
            self.out.write_parts(texts, toffs, keys)
        elif self.out_fd is not None:                    # straight from the batches' texts to the descriptor, no assembled copy of the window
            self.out.flush()
            self.V.blob_write_parts(self.lib, self.out_fd, texts, toffs, keys)
        else:
            self.out.write(memoryview(self.V.blob_gather_parts(self.lib, texts, toffs, keys)))

    def run(self):
        """the stream from the first window to the last line; raises the first error of any thread once every thread has ended"""
        errs, tm = self.errs, self.tm
        self.emit_pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.emit_jobs)
        rt, wt = threading.Thread(target=self.reader, daemon=True), threading.Thread(target=self.writer)
        rt.start(); wt.start()
        self.t_loop = time.time()
        try:
            ramp = self.size_contexts()
            if self.n_feed > 0 and self.sizing is not None:
                self.start_feeders()
                self.pipe.run_stream(self.fed_jobs(), self.align, errs, ramp=ramp)
            else:
                self.pipe.run_stream(self.job_source(), self.align, errs, ramp=ramp)
            tm['aligners_done'] = time.time() - self.t_loop; tm['contexts'] = float(self.pipe.inflight)
        except BaseException as e:
            if not any(e is x for x in errs):            # (run_stream raises the first of errs itself)
                errs.append(e)
        finally:
            if errs:
                self.oq.put(None)
            self.stop_feeders()
            wt.join()
            self.emit_pool.shutdown(wait=True)
            rt.join()                                    # (after a failure it has seen errs and let go of its input: to_workers)
        if errs:
            raise errs[0]
        tm['loop'] = time.time() - self.t_loop
        last_timing.clear(); last_timing.update(tm); last_timing['reads'] = self.counts['reads']
        if self.sw['VMX_DRIVER_TIMING']:
            sys.stderr.write('vacmapx timing (s): %s\n' % ' '.join('%s=%.2f' % kv for kv in tm.items()))

    def collect_parts(self):
        """Range mode, after the stream: every rank wrote its own part; the counts travel to rank 0, which joins the parts in rank order (the
        reference's output order is not the input's either: mammap_clrnano.py:24147-24150).
        The reference drops a read name it has seen before, anywhere in the input (vacmap:457-487); a rank only sees its own byte ranges, so the
        ranks' name hashes (8 bytes per read) travel with the counts and rank 0 leaves the later occurrences out while it joins the parts.
        "Earlier" is the INPUT's order, not the rank's — every hash travels with the number of the input file it came from; inside a file the
        ranks' byte ranges ascend with the rank. With two files, a name in file 1 inside rank 3's range and again in file 2 inside rank 0's
        keeps the file-1 record (sorted by hash, then file, then rank: every occurrence but the first goes), as the reference's single pass over
        the files does. No cross-rank duplicate — the rule — costs one sort."""
        import numpy as np
        from .dist import gather_lines
        args, counts = self.args, self.counts
        self.out.finish()
        myh = np.concatenate(self.rank_hashes) if self.rank_hashes else np.zeros(0, np.uint64)
        myf = np.concatenate(self.rank_hash_file) if self.rank_hash_file else np.zeros(0, np.int32)
        allc = gather_lines((counts['reads'], counts['lines'], counts['skipped'], myh, myf), dst=0, group=self.net.text_group)
        if self.rank != 0:
            return
        counts['reads'], counts['lines'], counts['skipped'] = (sum(c[i] for c in allc) for i in range(3))
        drop = cross_rank_duplicates([c[3] for c in allc], [c[4] for c in allc])
        if drop and args.parts:
            sys.stderr.write('vacmapx: %d read names occur in more than one rank\'s part (--parts keeps the parts as written: later occurrences are NOT removed)\n' % sum(len(v) for v in drop.values()))
        if not args.parts:
            tj = time.time()
            gr, gl = _concat_parts(args.o, ['%s.part%03d' % (args.o, r) for r in range(self.world)], drop)
            counts['reads'] -= gr; counts['lines'] -= gl
            if gr:
                sys.stderr.write('vacmapx: %d reads whose name occurred earlier in the input (another rank\'s range) were left out, %d SAM lines\n' % (gr, gl))
            last_timing['concat_parts'] = time.time() - tj

    def report(self, tail):
        """the final stderr lines (vacmap:535-541)"""
        tt, c = max(time.time() - self.t0, 0.001), self.counts
        return ('User time (h:m:s): %d:%d:%d %d / sec AVG. %d sequences processed.\n' % (tt // 3600, (tt % 3600) // 60, tt % 60, round(c['reads'] / tt), c['reads'])
                + 'vacmapx: %d reads, %d %s lines, %d reads skipped%s\n' % (c['reads'], c['lines'], 'PAF' if self.args.paf else 'SAM', c['skipped'], tail))


def main(argv=None, comm=None):
    """comm: an initialised torch.distributed module (tests); under torchrun (WORLD_SIZE > 1) the process group is created here.
    The stages in order; a stage that opens something is a context manager and releases it however the run ends."""
    t_start = time.time()
    sw = _switches()
    args = _parse_args(argv, comm, sw)
    with _process_groups(comm, sw) as net:
        if net.rank == 0 and args.o != '-' and os.path.exists(args.o) and not args.force:
            sys.exit('%s exists (use --force)' % args.o)
        if comm is None and net.world == 1 and __name__ == '__main__':
            os.environ.setdefault('VACMAPX_SKIP_TORCH', '1')        # one GPU from the command line: nothing here needs torch (its import is 1.5-2 s)
        from .lib import load
        lib = load()
        device = args.device if args.device is not None else net.local_rank
        with _context_and_index(args, net, device) as (ctx, index):
            prm, rg, opts = _alignment_options(args, lib)
            range_mode = _sharding(args, net)
            with _open_output(args, net, range_mode, index, rg, argv, device) as out, contextlib.closing(DepthSink(args, lib, index)) as depth:
                if args.mode == 'asm':
                    report = _run_asm(args, net, lib, ctx, index, prm, opts, out, device, t_start, depth)
                    depth.finish(net)
                else:
                    with contextlib.closing(ReadStream(args, sw, net, lib, ctx, index, prm, opts, out, range_mode, device, t_start, depth)) as stream:
                        stream.run()
                        depth.finish(net)                   # (before the emit contexts close: the device accumulators live in their memory)
                    if range_mode:
                        stream.collect_parts()
                    report = stream.report
                _finish(out, net.rank, report)
    return 0


if __name__ == '__main__':
    sys.exit(main())
