"""TEST-ONLY: an independent pure-Python BGZF / BAM reader (SAMv1 §4), written from the specification. It shares no code with the
product (vacmap_amd.driver.read_bam included): the BAM tests decode what the device wrote with it."""
import struct
import zlib

import numpy as np

BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')


def bgzf_members(data, require_eof=True):
    """walk the members by hand: gzip header with the BC subfield, BSIZE = member length - 1, <= 65 536 bytes, raw inflate, CRC32 and ISIZE.
    Returns the list of (member bytes, payload)."""
    out, p = [], 0
    if require_eof:
        assert data.endswith(BGZF_EOF), 'missing BGZF EOF block'
    while p < len(data):
        assert data[p:p + 4] == b'\x1f\x8b\x08\x04', 'bad gzip magic / flags at %d' % p
        xlen = struct.unpack_from('<H', data, p + 10)[0]
        extra = data[p + 12:p + 12 + xlen]
        q, bsize = 0, None
        while q < len(extra):
            si1, si2, slen = extra[q], extra[q + 1], struct.unpack_from('<H', extra, q + 2)[0]
            if si1 == 66 and si2 == 67:
                assert slen == 2
                bsize = struct.unpack_from('<H', extra, q + 4)[0]
            q += 4 + slen
        assert bsize is not None, 'no BC subfield'
        size = bsize + 1
        assert size <= 65536
        mem = data[p:p + size]
        assert len(mem) == size
        d = zlib.decompressobj(-15)
        payload = d.decompress(mem[12 + xlen:size - 8])
        assert d.eof and not d.unused_data, 'deflate stream does not end at the trailer'
        crc, isize = struct.unpack_from('<II', mem, size - 8)
        assert crc == zlib.crc32(payload), 'CRC32 mismatch'
        assert isize == len(payload), 'ISIZE mismatch'
        out.append((mem, payload))
        p += size
    return out


def bgzf_decompress(data, require_eof=True):
    return b''.join(pl for _, pl in bgzf_members(data, require_eof))


def reg2bin(beg, end):
    end -= 1
    for shift, off in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return off + (beg >> shift)
    return 0


_CIG = 'MIDNSHP=X'
_NT = '=ACMGRSVTWYHKDBN'
_BFMT = {'c': 'b', 'C': 'B', 's': 'h', 'S': 'H', 'i': 'i', 'I': 'I', 'f': 'f'}


def _f32(x):
    return struct.unpack('<f', struct.pack('<f', x))[0]


def _fmt_float(x):
    return repr(_f32(x))


def decode_record(rec, refs):
    """one BAM record (without block_size) -> SAM fields as text; integers print as i, floats as the float32 value's repr.
    Checks the stored bin against reg2bin."""
    refid, pos, lrn, mapq, binv, ncig, flag, lseq, nref, npos, tlen = struct.unpack_from('<iiBBHHHiiii', rec, 0)
    p = 32
    name = rec[p:p + lrn - 1].decode(); assert rec[p + lrn - 1] == 0; p += lrn
    cig = [struct.unpack_from('<I', rec, p + 4 * i)[0] for i in range(ncig)]; p += 4 * ncig
    seqb = rec[p:p + (lseq + 1) // 2]; p += (lseq + 1) // 2
    qual = rec[p:p + lseq]; p += lseq
    tags = []
    while p < len(rec):
        tg = rec[p:p + 2].decode(); ty = chr(rec[p + 2]); p += 3
        if ty == 'A':
            tags.append((tg, 'A', chr(rec[p]))); p += 1
        elif ty in 'cCsSiI':
            fmt = '<' + _BFMT[ty]; v = struct.unpack_from(fmt, rec, p)[0]; p += struct.calcsize(fmt)
            tags.append((tg, 'i', str(v)))
        elif ty == 'f':
            tags.append((tg, 'f', struct.unpack_from('<f', rec, p)[0])); p += 4
        elif ty in 'ZH':
            e = rec.index(b'\0', p); tags.append((tg, ty, rec[p:e].decode())); p = e + 1
        elif ty == 'B':
            sub = chr(rec[p]); cnt = struct.unpack_from('<I', rec, p + 1)[0]; p += 5
            fmt = '<%d%s' % (cnt, _BFMT[sub]); vals = struct.unpack_from(fmt, rec, p); p += struct.calcsize(fmt)
            tags.append((tg, 'B', (sub, list(vals))))
        else:
            raise AssertionError('unknown tag type %r' % ty)
    # a CIGAR of more than 65 535 operations: kSmN here, the real one in CG:B,I
    if ncig == 2 and (cig[0] & 15) == 4 and (cig[1] & 15) == 3 and any(t[0] == 'CG' and t[1] == 'B' for t in tags):
        cg = [t for t in tags if t[0] == 'CG' and t[1] == 'B'][0]
        assert cg[2][0] == 'I' and cig[0] >> 4 == lseq and cig[1] >> 4 == sum(c >> 4 for c in cg[2][1] if (c & 15) in (0, 2, 3, 7, 8))   # <l_seq>S<span>N
        cig = cg[2][1]
        tags = [t for t in tags if t is not cg]
    span = sum(c >> 4 for c in cig if (c & 15) in (0, 2, 3, 7, 8))
    assert binv == reg2bin(pos, pos + (span if span else 1)), 'bin %d != reg2bin' % binv
    cigs = ''.join('%d%s' % (c >> 4, _CIG[c & 15]) for c in cig) or '*'
    seq = ''.join(_NT[(seqb[i // 2] >> (4 * (1 - i % 2))) & 15] for i in range(lseq)) or '*'
    qs = '*' if lseq == 0 or all(q == 255 for q in qual) else ''.join(chr(q + 33) for q in qual)
    fields = [name, str(flag), refs[refid] if refid >= 0 else '*', str(pos + 1), str(mapq), cigs,
              ('=' if nref == refid and nref >= 0 else refs[nref]) if nref >= 0 else '*', str(npos + 1), str(tlen), seq, qs]
    return fields, tags


def read_bam(data):
    """BGZF BAM bytes -> (header text, reference names and lengths, list of (fields, tags))"""
    raw = bgzf_decompress(data)
    assert raw[:4] == b'BAM\1'
    lt = struct.unpack_from('<i', raw, 4)[0]
    text = raw[8:8 + lt].decode()
    p = 8 + lt
    nr = struct.unpack_from('<i', raw, p)[0]; p += 4
    refs = []
    for _ in range(nr):
        ln = struct.unpack_from('<i', raw, p)[0]
        refs.append((raw[p + 4:p + 4 + ln - 1].decode(), struct.unpack_from('<i', raw, p + 4 + ln)[0])); p += 8 + ln
    recs = records(raw[p:], [r[0] for r in refs])
    return text, refs, recs


def records(raw, names):
    out, p = [], 0
    while p < len(raw):
        bs = struct.unpack_from('<i', raw, p)[0]
        out.append(decode_record(raw[p + 4:p + 4 + bs], names)); p += 4 + bs
    return out


def sam_tags_of(line):
    """a SAM line's optional fields in the decoded form: ints as i, floats as float32 values, B arrays as (subtype, values)"""
    out = []
    for f in line.split('\t')[11:]:
        tg, ty, v = f[:2], f[3], f[5:]
        if ty == 'i':
            out.append((tg, 'i', str(int(v))))
        elif ty == 'f':
            out.append((tg, 'f', _f32(float(v))))
        elif ty == 'B':
            sub = v[0]
            vals = [x for x in v[2:].split(',')] if len(v) > 1 else []
            out.append((tg, 'B', (sub, [_f32(float(x)) if sub == 'f' else int(x) for x in vals])))
        else:
            out.append((tg, ty, v))
    return out


def same_as_sam(decoded, line):
    """decoded record equals a SAM line: the 11 fields as text (SEQ upper-cased, unknown letters as N), the tags by value"""
    fields, tags = decoded
    want = line.split('\t')
    exp = want[:11]
    if exp[9] != '*':
        exp[9] = ''.join(c if c in _NT else 'N' for c in exp[9].upper())
    if exp[6] == exp[2] and exp[2] != '*':
        exp[6] = '='
    got = list(fields)
    if got[6] == got[2] and got[2] != '*':
        got[6] = '='
    return got == exp and _tag_eq(tags, sam_tags_of(line))


def _tag_eq(a, b):
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if x[:2] != y[:2]:
            return False
        if x[1] == 'f':
            if not (x[2] == y[2] or (x[2] != x[2] and y[2] != y[2])):
                return False
        elif x[1] == 'B':
            if x[2][0] != y[2][0] or len(x[2][1]) != len(y[2][1]):
                return False
            for u, v in zip(x[2][1], y[2][1]):
                if not (u == v or (u != u and v != v)):
                    return False
        elif x[2] != y[2]:
            return False
    return True


def to_sam(decoded):
    """decoded record -> SAM line text (ints as i, floats as float32 reprs)"""
    fields, tags = decoded
    out = list(fields)
    for tg, ty, v in tags:
        if ty == 'f':
            out.append('%s:f:%s' % (tg, repr(v)))
        elif ty == 'B':
            out.append('%s:B:%s' % (tg, ','.join([v[0]] + [repr(x) if v[0] == 'f' else str(x) for x in v[1]])))
        else:
            out.append('%s:%s:%s' % (tg, ty, v))
    return '\t'.join(out)


def ont_quals(n, seed):
    """seeded ONT-like Phred strings: a Markov chain over quality values (runs of good and poor calls), not a constant"""
    rng = np.random.default_rng(seed)
    q = np.empty(n, np.int32)
    cur = 12
    steps = rng.integers(-3, 4, n)
    jumps = rng.random(n)
    for i in range(n):
        if jumps[i] < 0.02:
            cur = int(rng.integers(3, 30))
        else:
            cur = min(50, max(2, cur + int(steps[i]) // 2 + (1 if cur < 14 else -1 if cur > 20 else 0) * (i % 2)))
        q[i] = cur
    return ''.join(chr(33 + int(x)) for x in q)
