"""Native BAM output: SAM lines -> BAM records -> BGZF members on the GPU (vm_bam_*, csrc/k_bam.hip), written to a file.

The driver's `--bam-writer native` writes `.bam` through BamWriter instead of a `samtools view -b` pipe; `--bam-writer native-sort` writes
`.sorted.bam` and its `.csi` index through SortedBamWriter (vm_bam_sorter_*, csrc/k_bam_sort.hip) instead of a `samtools sort --write-index`
pipe. Compression runs on a Context of the writer's own, so it does not queue behind the aligner's batches on their streams.
"""
import os
import shutil
import tempfile
import time
import weakref
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .lib import BamCodec, BamSorter, Context

# the standard empty BGZF member that ends a BGZF file (SAMv1 §4.1.2)
BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


class BamWriter:
    """path: the .bam file (created); header_lines: the SAM header lines without newlines (sam.header_lines)"""

    def __init__(self, path, header_lines, device=0, lib=None):
        self.ctx = Context(device, lib=lib)
        self.codec = None
        self.f = None
        self._io = ThreadPoolExecutor(1)               # file writes of one window overlap the next window's encoding and compression
        self._pending = None
        try:
            self.codec = BamCodec(self.ctx, ''.join(ln + '\n' for ln in header_lines))
            self.f = open(path, 'wb')
            head = self.codec.header()
            self.header_bytes = len(head)
            self.f.write(head)
        except BaseException:
            self._io.shutdown()
            self._release()
            raise

    def _submit(self, fn, *args):
        if self._pending is not None:
            self._pending.result()                     # (in order, and a failed write surfaces here)
        self._pending = self._io.submit(fn, *args)

    def _drain(self):
        if self._pending is not None:
            p, self._pending = self._pending, None
            p.result()

    def _put(self, members):
        self._submit(self.f.write, members)

    def write(self, sam_text):
        """whole SAM lines (bytes)"""
        if sam_text:
            self.write_parts([np.frombuffer(sam_text, np.uint8)], [[0, len(sam_text)]], [[0]])

    def write_parts(self, blobs, offs, order_keys):
        """one window's lines: the entries of several (blob, offsets) pairs in ascending order_keys, as blob_write_parts takes them"""
        self._put(self.codec.compress_parts(blobs, offs, order_keys))

    def _release(self):
        if self.codec is not None:
            self.codec.close(); self.codec = None
        if self.ctx is not None:
            self.ctx.close(); self.ctx = None

    def _abort(self):
        """an error: nothing more is written; the device is released (and the run files of a sorting writer go)"""
        try:
            self._drain()
        except BaseException:
            pass
        if self.f is not None:
            self.f.close()
            self.f = None
        self._io.shutdown()
        self._release()

    def _finish(self):
        """what is still to be written before the EOF member"""

    def close(self):
        """the BGZF EOF member, then the file is closed"""
        try:
            self._drain()
            if self.f is not None:
                self._finish()
                self.f.write(BGZF_EOF)
        finally:
            if self.f is not None:
                self.f.close()
                self.f = None
            self._io.shutdown()
            self._release()


def coordinate_header(header_lines):
    """the header lines with SO:coordinate on the @HD line (an SO that is there is replaced, VN and other fields stay; no @HD line: one is put first)"""
    out, seen = [], False
    for ln in header_lines:
        if ln.startswith('@HD') and not seen:
            seen = True
            f = ln.split('\t')
            if any(x.startswith('SO:') for x in f[1:]):
                f = [f[0]] + ['SO:coordinate' if x.startswith('SO:') else x for x in f[1:]]
            else:
                f.append('SO:coordinate')
            ln = '\t'.join(f)
        out.append(ln)
    return out if seen else ['@HD\tVN:1.6\tSO:coordinate'] + out


def _write_file(path, data):
    with open(path, 'wb') as f:
        f.write(data)


class SortedBamWriter(BamWriter):
    """BamWriter's interface; close() leaves `path` sorted by coordinate and `path`.csi.

    Every write / write_parts call becomes a sorted run: the records, in order and uncompressed, in a file of a fresh directory under `workdir`
    (default: next to `path`), written on the I/O thread while the next window is encoded. close() merges the runs chunk by chunk (chunk_bytes
    of records each: gathered, compressed and indexed on the device) and writes the index. The run directory goes in close(), when a write
    raises, and when the writer is dropped."""

    def __init__(self, path, header_lines, device=0, lib=None, workdir=None, chunk_bytes=256 << 20):
        self.sorter = None
        self._dir = None
        super().__init__(path, coordinate_header(header_lines), device=device, lib=lib)
        self.path = path
        self.runs = []
        self.run_bytes = 0
        self.merge_seconds = 0.0
        try:
            self.sorter = BamSorter(self.codec, chunk_bytes)
            self._dir = tempfile.mkdtemp(prefix='.bamsort-', dir=workdir or os.path.dirname(os.path.abspath(path)))
            self._rm = weakref.finalize(self, shutil.rmtree, self._dir, True)
        except BaseException:
            self._abort()
            raise

    def write_parts(self, blobs, offs, order_keys):
        try:
            recs = self.sorter.add_parts(blobs, offs, order_keys)
            if recs:
                run = os.path.join(self._dir, 'run%06d' % len(self.runs))
                self.runs.append(run)
                self.run_bytes += len(recs)
                self._submit(_write_file, run, recs)
        except BaseException:
            self._abort()
            raise

    def _release(self):
        if self.sorter is not None:
            self.sorter.close(); self.sorter = None
        super()._release()
        if self._dir is not None:
            self._rm()
            self._dir = None

    def _finish(self):
        t0 = time.time()
        for k in range(self.sorter.plan(self.runs, self.header_bytes)):
            members = self.sorter.chunk(k)
            if members:
                self._put(members)                     # (written while the next chunk is read, gathered and compressed)
        self._drain()
        _write_file(self.path + '.csi', self.sorter.index())
        self.merge_seconds = time.time() - t0
