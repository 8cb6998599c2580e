"""TEST-ONLY: an independent pure-Python reader of CSI indices (CSIv1, the SAM/BAM format specification's companion document), written from
the specification. It shares no code with the product: the sorted-BAM tests parse the index the device wrote with it and fetch regions
through it, seeking to virtual offsets over the members that bam_codec.bgzf_members walks."""
import struct

import bam_codec as B

META_BIN = 37450                          # ((1 << 18) - 1) / 7 + 1 for depth 5: the pseudo-bin with the per-reference figures


def parse(data):
    """.csi file bytes -> {'min_shift', 'depth', 'aux', 'refs': [{'bins': {bin: (loffset, [(beg, end), ...])}, 'meta': (vbeg, vend, mapped, unmapped) | None}],
    'n_no_coor': int | None}. Checks that the file is BGZF with the EOF member and that nothing is left over."""
    raw = B.bgzf_decompress(data, require_eof=True)
    assert raw[:4] == b'CSI\1', 'bad CSI magic'
    min_shift, depth, l_aux = struct.unpack_from('<iii', raw, 4)
    p = 16
    aux = raw[p:p + l_aux]; p += l_aux
    n_ref = struct.unpack_from('<i', raw, p)[0]; p += 4
    refs = []
    for _ in range(n_ref):
        n_bin = struct.unpack_from('<i', raw, p)[0]; p += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            b, loff, n_chunk = struct.unpack_from('<IQi', raw, p); p += 16
            chunks = [struct.unpack_from('<QQ', raw, p + 16 * i) for i in range(n_chunk)]; p += 16 * n_chunk
            if b == bin_limit(depth) + 1:
                assert n_chunk == 2 and meta is None
                meta = (chunks[0][0], chunks[0][1], chunks[1][0], chunks[1][1])
            else:
                assert b < bin_limit(depth) and b not in bins and n_chunk > 0
                bins[b] = (loff, chunks)
        refs.append({'bins': bins, 'meta': meta})
    n_no_coor = None
    if p < len(raw):
        n_no_coor = struct.unpack_from('<Q', raw, p)[0]; p += 8
    assert p == len(raw), 'bytes left after the index'
    return {'min_shift': min_shift, 'depth': depth, 'aux': aux, 'refs': refs, 'n_no_coor': n_no_coor}


def bin_limit(depth):
    """number of bins of an index of that depth: ((1 << 3 * (depth + 1)) - 1) / 7"""
    return ((1 << (3 * (depth + 1))) - 1) // 7


def level_start(level):
    return ((1 << (3 * level)) - 1) // 7


def bin_level(b):
    lv = 0
    while b >= level_start(lv + 1):
        lv += 1
    return lv


def bin_span(b, min_shift=14, depth=5):
    """[beg, end) of the reference that a bin covers"""
    lv = bin_level(b)
    sh = min_shift + 3 * (depth - lv)
    return (b - level_start(lv)) << sh, (b - level_start(lv) + 1) << sh


def reg2bin(beg, end, min_shift=14, depth=5):
    """the smallest bin that holds [beg, end) (the specification's reg2bin)"""
    end -= 1
    s, t = min_shift, level_start(depth)
    for lv in range(depth, 0, -1):
        if beg >> s == end >> s:
            return t + (beg >> s)
        s += 3
        t -= 1 << (3 * (lv - 1))
    return 0


def reg2bins(beg, end, min_shift=14, depth=5):
    """every bin that may hold a record overlapping [beg, end) (the specification's reg2bins)"""
    out = []
    end -= 1
    s = min_shift + 3 * depth
    for lv in range(depth + 1):
        t = level_start(lv)
        out.extend(range(t + (beg >> s), t + (end >> s) + 1))
        s -= 3
    return out


def min_offset(idx, rid, beg):
    """no record that ends after `beg` starts before this virtual offset: the loffset of the smallest bin of the index that holds `beg`"""
    bins = idx['refs'][rid]['bins']
    s = idx['min_shift']
    for lv in range(idx['depth'], -1, -1):
        b = level_start(lv) + (beg >> s)
        if b in bins:
            return bins[b][0]
        s += 3
    return 0


def query_chunks(idx, rid, beg, end):
    """the merged, ascending list of (vbeg, vend) that has to be read for [beg, end) of reference rid"""
    bins = idx['refs'][rid]['bins']
    lo = min_offset(idx, rid, beg)
    ch = sorted(c for b in reg2bins(beg, end, idx['min_shift'], idx['depth']) if b in bins for c in bins[b][1] if c[1] > lo)
    out = []
    for c in ch:
        if out and c[0] <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], c[1]))
        else:
            out.append(c)
    return out


class Bam:
    """a BGZF BAM file in memory, addressable by virtual offset"""

    def __init__(self, data):
        mem = B.bgzf_members(data)
        self.cstart, self.ustart = {}, []
        c = u = 0
        for i, (m, pl) in enumerate(mem):
            self.cstart[c] = i
            self.ustart.append(u)
            c += len(m); u += len(pl)
        self.sizes = [len(pl) for _, pl in mem]
        self.raw = b''.join(pl for _, pl in mem)
        assert self.raw[:4] == b'BAM\1'
        lt = struct.unpack_from('<i', self.raw, 4)[0]
        self.text = self.raw[8:8 + lt].decode()
        p = 8 + lt
        nr = struct.unpack_from('<i', self.raw, p)[0]; p += 4
        self.refs = []
        for _ in range(nr):
            ln = struct.unpack_from('<i', self.raw, p)[0]
            self.refs.append((self.raw[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from('<i', self.raw, p + 4 + ln)[0])); p += 8 + ln
        self.body = p

    def u_of(self, voff):
        """virtual offset -> offset in the decompressed stream; the member must exist and the offset lie inside it (or at its end)"""
        i = self.cstart[voff >> 16]
        assert (voff & 0xffff) <= self.sizes[i]
        return self.ustart[i] + (voff & 0xffff)

    def record_at(self, u):
        """(next offset, refID, pos, end, flag, bin) of the record at decompressed offset u; end = pos + reference length of the stored CIGAR, or pos + 1"""
        bs, rid, pos, lrn, _mq, bn, ncig, flag = struct.unpack_from('<iiiBBHHH', self.raw, u)
        span = 0
        if ncig:
            for c in struct.unpack_from('<%dI' % ncig, self.raw, u + 36 + lrn):
                if c & 15 in (0, 2, 3, 7, 8):
                    span += c >> 4
        return u + 4 + bs, rid, pos, pos + (span or 1), flag, bn

    def scan(self):
        """every record of the file in order: list of (offset, refID, pos, end, flag, bin)"""
        out, u = [], self.body
        while u < len(self.raw):
            nxt, rid, pos, end, flag, bn = self.record_at(u)
            out.append((u, rid, pos, end, flag, bn))
            u = nxt
        assert u == len(self.raw)
        return out


def fetch(bam, idx, rid, beg, end):
    """decompressed offsets of the records of reference rid that overlap [beg, end), in file order, read through the index"""
    out = []
    for vb, ve in query_chunks(idx, rid, beg, end):
        u, stop = bam.u_of(vb), bam.u_of(ve)
        while u < stop:
            nxt, r, pos, e, _flag, _bn = bam.record_at(u)
            if r == rid and pos < end and e > beg:
                out.append(u)
            u = nxt
        assert u == stop, 'a chunk does not end at a record boundary'
    return out
