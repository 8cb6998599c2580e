"""Native BAM output: SAM lines -> BAM records -> BGZF members on the GPU (vm_bam_*, csrc/k_bam.hip), written to a file.

The driver's `--bam-writer native` writes `.bam` through BamWriter instead of a `samtools view -b` pipe. Compression runs on a Context of
the writer's own, so it does not queue behind the aligner's batches on their streams.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .lib import BamCodec, Context

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
            self.f.write(self.codec.header())
        except BaseException:
            self._io.shutdown()
            self._release()
            raise

    def _put(self, members):
        if self._pending is not None:
            self._pending.result()                     # (in order, and a failed write surfaces here)
        self._pending = self._io.submit(self.f.write, members)

    def write(self, sam_text):
        """whole SAM lines (bytes)"""
        if sam_text:
            self._put(self.codec.compress_parts([np.frombuffer(sam_text, np.uint8)], [[0, len(sam_text)]], [[0]]))

    def write_parts(self, blobs, offs, order_keys):
        """one window's lines: the entries of several (blob, offsets) pairs in ascending order_keys, as blob_write_parts takes them"""
        self._put(self.codec.compress_parts(blobs, offs, order_keys))

    def _release(self):
        if self.codec is not None:
            self.codec.close(); self.codec = None
        if self.ctx is not None:
            self.ctx.close(); self.ctx = None

    def close(self):
        """the BGZF EOF member, then the file is closed"""
        try:
            if self._pending is not None:
                self._pending.result()
                self._pending = None
            if self.f is not None:
                self.f.write(BGZF_EOF)
        finally:
            if self.f is not None:
                self.f.close()
                self.f = None
            self._io.shutdown()
            self._release()
