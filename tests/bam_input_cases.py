"""Shared builders of the BAM input tests (test_bam_input_emu.py, test_gpu_bam_input.py): BGZF files assembled here from raw deflate
streams (header with the BC subfield, CRC32, ISIZE), payloads, hand-assembled fixed-Huffman streams, BAM record streams. The references are
Python's zlib / gzip for the inflate and driver.read_bam / driver._bam_chunks for the records; nothing here shares code with the kernels."""
import gzip
import struct
import zlib

import numpy as np

BGZF_EOF = bytes.fromhex('1f8b08040000000000ff0600424302001b0003000000000000000000')
NT16 = '=ACMGRSVTWYHKDBN'


# ---------------------------------------------------------------- BGZF framing

def member(raw, payload, extra=b'', crc=None, isize=None):
    """one BGZF member around the raw deflate stream `raw` of `payload`; extra: other subfields before BC"""
    xlen = len(extra) + 6
    bsize = 12 + xlen + len(raw) + 8 - 1
    assert bsize < 65536
    return (b'\x1f\x8b\x08\x04\0\0\0\0\0\xff' + struct.pack('<H', xlen) + extra + b'BC\x02\0' + struct.pack('<H', bsize) + raw +
            struct.pack('<II', zlib.crc32(payload) if crc is None else crc, len(payload) if isize is None else isize))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flushes=0):
    """raw deflate (no zlib header); flushes: Z_FULL_FLUSH calls spread over the data (multi-block members with empty stored blocks)"""
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    out = b''
    cuts = [len(data) * i // (flushes + 1) for i in range(flushes + 2)]
    for i in range(flushes + 1):
        out += c.compress(data[cuts[i]:cuts[i + 1]])
        if i < flushes:
            out += c.flush(zlib.Z_FULL_FLUSH)
    return out + c.flush()


def bgzf(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, block=65280, flushes=0, eof=True, extra=b''):
    """data as BGZF members of `block` payload bytes (level 0 members hold at most 60 000: stored blocks add 5 bytes per 65 535)"""
    if level == 0:
        block = min(block, 60000)
    out = b''
    for i in range(0, len(data), block):
        pl = data[i:i + block]
        out += member(deflate(pl, level, strategy, flushes), pl, extra)
    return out + (BGZF_EOF if eof else b'')


def split_members(z):
    """[(offset, member bytes)] of the complete members of a BGZF file, by BSIZE"""
    out, at = [], 0
    while at + 18 <= len(z):
        xlen = struct.unpack_from('<H', z, at + 10)[0]
        q, bsize = at + 12, None
        while q < at + 12 + xlen:
            si, sl = z[q:q + 2], struct.unpack_from('<H', z, q + 2)[0]
            if si == b'BC':
                bsize = struct.unpack_from('<H', z, q + 4)[0]
            q += 4 + sl
        if at + bsize + 1 > len(z):
            break
        out.append((at, z[at:at + bsize + 1]))
        at += bsize + 1
    return out


def block_types(mem):
    """(BTYPE of the first deflate block, BFINAL of the first block) of one member, read from the header bits"""
    xlen = struct.unpack_from('<H', mem, 10)[0]
    b = mem[12 + xlen]
    return (b >> 1) & 3, b & 1


# ---------------------------------------------------------------- payloads

def periodic(period, n, seed=0):
    unit = np.random.default_rng(seed * 1000 + period).integers(0, 256, period).astype(np.uint8).tobytes()
    return (unit * (n // period + 1))[:n]


def far_text(seed=3):
    """text whose second half repeats pieces of the first at distance 32 768 exactly"""
    rng = np.random.default_rng(seed)
    a = rng.integers(97, 123, 32768).astype(np.uint8).tobytes()
    b = bytearray(rng.integers(97, 123, 32000).astype(np.uint8).tobytes())
    for s in range(0, 32000 - 300, 700):
        b[s:s + 260] = a[s:s + 260]
    return a + bytes(b)


class Bits:
    """LSB-first bit writer; Huffman codes go in MSB-first (RFC 1951 §3.1.1)"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, val, nbits):
        self.v |= val << self.n; self.n += nbits

    def code(self, val, nbits):
        self.put(int(format(val, '0%db' % nbits)[::-1], 2), nbits)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, 'little')


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def fixed_stream(tokens, final=True):
    """one fixed-Huffman block of tokens: an int is a literal, (length, distance) a match. Returns (raw deflate, the bytes it stands for)"""
    w = Bits()
    w.put(1 if final else 0, 1); w.put(1, 2)
    out = bytearray()

    def lit(sym):
        if sym < 144: w.code(0x30 + sym, 8)
        elif sym < 256: w.code(0x190 + sym - 144, 9)
        elif sym < 280: w.code(sym - 256, 7)
        else: w.code(0xc0 + sym - 280, 8)
    for t in tokens:
        if isinstance(t, int):
            lit(t); out.append(t)
            continue
        ln, d = t
        li = max(i for i in range(29) if _LBASE[i] <= ln and (i < 28 or ln == 258))
        if ln == 258: li = 28
        lit(257 + li); w.put(ln - _LBASE[li], _LEXT[li])
        di = max(i for i in range(30) if _DBASE[i] <= d)
        w.code(di, 5); w.put(d - _DBASE[di], _DEXT[di])
        for _ in range(ln):
            out.append(out[-d] if d <= len(out) else 0)             # (a distance before the start: the malformed-input tests)
    lit(256)
    return w.bytes(), bytes(out)


def overlap_member(seed):
    """a fixed-Huffman member that forces dist < len at every distance 1 ... 64, with literal runs of 1 ... 70 bytes in between"""
    rng = np.random.default_rng(seed)
    toks = []
    for d in range(1, 65):
        toks += [int(x) for x in rng.integers(0, 256, int(rng.integers(1, 71)) + d)]
        toks.append((int(rng.integers(d + 1, 259)), d))
    raw, data = fixed_stream(toks)
    return member(raw, data), data


# ---------------------------------------------------------------- BAM streams

def bam_header(text='', refs=()):
    b = b'BAM\x01' + struct.pack('<i', len(text)) + text.encode() + struct.pack('<i', len(refs))
    for name, ln in refs:
        b += struct.pack('<i', len(name) + 1) + name.encode() + b'\0' + struct.pack('<i', ln)
    return b


def bam_record(name, seq, qual, flag, n_cigar=0, tags=b''):
    """one unaligned-style record (with its block_size); qual None: 0xff; n_cigar: that many 1M operations (skipped by a reader)"""
    code = {c: i for i, c in enumerate(NT16)}
    nm = name.encode() + b'\0'
    packed = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i // 2] |= code[ch] << (4 if i % 2 == 0 else 0)
    q = bytes([0xff] * len(seq)) if qual is None else bytes(ord(c) - 33 for c in qual)
    rec = struct.pack('<iiBBHHHiiii', -1, -1, len(nm), 0, 4680, n_cigar, flag, len(seq), -1, -1, 0) + nm + struct.pack('<I', 1 << 4) * n_cigar + bytes(packed) + q + tags
    return struct.pack('<i', len(rec)) + rec


def random_reads(n, seed, min_len=1, max_len=3000, letters='ACGT'):
    """(name, seq, qual or None, flag) with both strands, some without qualities, some with IUPAC letters"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = int(rng.integers(min_len, max_len + 1))
        al = NT16 if i % 7 == 3 else letters
        seq = ''.join(al[j] for j in rng.integers(0, len(al), ln))
        qual = None if i % 5 == 4 else ''.join(chr(33 + int(x)) for x in rng.integers(0, 60, ln))
        out.append(('read%d/%d' % (seed, i), seq, qual, 16 if i % 3 == 1 else (4 if i % 3 == 2 else 0)))
    return out


def ref_records(stream):
    """byte-level records of an inflated BAM stream, after SAMv1 §4.2 and the rules of driver.read_bam: (name, seq, qual or None) as bytes,
    reverse-strand records turned back, records without bases dropped. Raises ValueError where a record does not fit its block_size."""
    p = 12 + struct.unpack_from('<i', stream, 4)[0]
    n_ref = struct.unpack_from('<i', stream, p - 4)[0]
    for _ in range(n_ref):
        p += 8 + struct.unpack_from('<i', stream, p)[0]
    comp = bytes.maketrans(b'ACGTN', b'TGCAN')
    out = []
    while p < len(stream):
        if p + 36 > len(stream):
            raise ValueError('truncated record')
        bs = struct.unpack_from('<i', stream, p)[0]
        l_rn, n_cig, flag, l_seq = stream[p + 12], struct.unpack_from('<H', stream, p + 16)[0], struct.unpack_from('<H', stream, p + 18)[0], struct.unpack_from('<i', stream, p + 20)[0]
        if bs < 32 or l_rn < 1 or l_seq < 0 or 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs or p + 4 + bs > len(stream):
            raise ValueError('record does not fit')
        q = p + 36
        name = stream[q:q + l_rn - 1]; q += l_rn + 4 * n_cig
        packed = stream[q:q + (l_seq + 1) // 2]; q += (l_seq + 1) // 2
        seq = ''.join(NT16[b >> 4] + NT16[b & 15] for b in packed)[:l_seq].encode()
        qual = None if l_seq == 0 or stream[q] == 0xff else bytes((x + 33) & 255 for x in stream[q:q + l_seq])
        p += 4 + bs
        if l_seq == 0:
            continue
        if flag & 16:
            seq = seq.translate(comp)[::-1]; qual = qual[::-1] if qual is not None else None
        out.append((name, seq, qual))
    return out


def chunks_of_records(recs, n_max):
    """the blob chunks of driver._bam_chunks for byte-level records"""
    out = []
    for i in range(0, len(recs), n_max):
        rows = recs[i:i + n_max]
        ch = {}
        for key, col in (('names', 0), ('seqs', 1), ('quals', 2)):
            bs = [r[col] or b'' for r in rows]
            ch[key] = np.frombuffer(b''.join(bs), dtype=np.uint8)
            ch[key + '_off'] = np.concatenate([[0], np.cumsum([len(b) for b in bs])]).astype(np.int64)
        ch['comments'] = np.zeros(0, np.uint8); ch['comments_off'] = np.zeros(len(rows) + 1, np.int64)
        out.append(ch)
    return out


def same_chunks(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        for key in ('names', 'seqs', 'quals', 'comments'):
            assert g[key + '_off'].tolist() == w[key + '_off'].tolist(), key
            assert bytes(g[key]) == bytes(w[key]), key


def read_all(reader, max_reads, max_bases=1 << 62):
    out = []
    while True:
        ch = reader.read(max_reads, max_bases)
        if ch is None:
            return out
        out.append(ch)


def inflate_cases(bam_bytes):
    """name -> BGZF file bytes: every block type, multi-block members, the framing edge cases, the payload classes"""
    rng = np.random.default_rng(11)
    rnd = rng.integers(0, 256, 70000).astype(np.uint8).tobytes()
    text = rng.integers(97, 101, 150000).astype(np.uint8).tobytes()
    C = {}
    C['stored'] = bgzf(text, 0)
    C['fixed'] = bgzf(text, 6, zlib.Z_FIXED)
    for lv in (1, 6, 9):
        C['dynamic%d' % lv] = bgzf(bam_bytes, lv)
    C['huffman_only'] = bgzf(bam_bytes[:100000], 6, zlib.Z_HUFFMAN_ONLY)
    C['rle'] = bgzf(bam_bytes[:100000], 6, zlib.Z_RLE)
    C['full_flush'] = bgzf(bam_bytes[:140000], 6, flushes=3)
    C['extra_subfield'] = bgzf(text[:70000], 6, extra=b'XY\x03\0abc')
    for n in (0, 1, 65279, 65280):
        C['size%d' % n] = member(deflate(rnd[:n] if n < 2 else periodic(97, n)), rnd[:n] if n < 2 else periodic(97, n)) + BGZF_EOF
    C['empty_mid'] = bgzf(text[:1000]) [:-28] + member(deflate(b''), b'') + member(b'\x01\0\0\xff\xff', b'') + bgzf(text[1000:3000])
    C['no_eof'] = bgzf(text[:80000], 6, eof=False)
    C['zeros'] = bgzf(b'\0' * 200000, 6)
    C['random'] = bgzf(rnd, 6)
    C['periods'] = b''.join(member(deflate(periodic(p, 3000 + 17 * p), 9), periodic(p, 3000 + 17 * p)) for p in range(1, 71))
    C['dist32768'] = bgzf(far_text(), 9)
    C['overlap_fixed'] = b''.join(overlap_member(s)[0] for s in range(4))
    return C


# ---------------------------------------------------------------- the scale file

def scale_records(n_bytes, seed=17, pool=64):
    """an unaligned BAM stream of at least n_bytes: 15 kb ONT-shape reads (lengths 2 ... 40 kb), qualities from bam_codec.ont_quals, a third of
    the records stored reverse-strand. Read i is a rotation of pool read i mod `pool` (a Markov-chain quality string costs 10 ms to make, 2 GB
    need 90 000). Returns (header, [record bytes], [(crc32 name, crc32 bases, crc32 qualities) of every read in its own orientation])"""
    import bam_codec as B
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(15000, 4000, pool), 2000, 40000).astype(np.int64)
    code = np.array([1, 2, 4, 8], np.uint8)
    seqs = [code[rng.integers(0, 4, int(n))] for n in lens]
    quals = [np.frombuffer(B.ont_quals(int(n), seed * 100 + k).encode(), np.uint8) - 33 for k, n in enumerate(lens)]
    letter = np.zeros(16, np.uint8); letter[[1, 2, 4, 8]] = np.frombuffer(b'ACGT', np.uint8)
    comp = np.zeros(16, np.uint8); comp[[1, 2, 4, 8]] = [8, 4, 2, 1]
    recs, want, tot, i = [], [], 0, 0
    while tot < n_bytes:
        k = i % pool
        n = int(lens[k])
        s = np.roll(seqs[k], (i * 131) % n); q = np.roll(quals[k], (i * 17) % n)
        name = b'read%09d' % i
        flag = 16 if i % 3 == 1 else 4
        want.append((zlib.crc32(name), zlib.crc32(letter[s].tobytes()), zlib.crc32((q + 33).astype(np.uint8).tobytes())))
        if flag & 16:
            s = comp[s][::-1]; q = q[::-1]
        c = np.concatenate([s, np.zeros(n & 1, np.uint8)])
        body = struct.pack('<iiBBHHHiiii', -1, -1, len(name) + 1, 0, 4680, 0, flag, n, -1, -1, 0) + name + b'\0' + ((c[0::2] << 4) | c[1::2]).tobytes() + q.astype(np.uint8).tobytes()
        recs.append(struct.pack('<i', len(body)) + body)
        tot += len(recs[-1]); i += 1
    return bam_header('@HD\tVN:1.6\tSO:unsorted\n'), recs, want


def write_bgzf_zlib(path, pieces, level=6, threads=16):
    """the concatenation of `pieces` as BGZF members of 65 280 bytes deflated by zlib on `threads` threads (zlib releases the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    with open(path, 'wb') as f, ThreadPoolExecutor(threads) as pool:
        buf = bytearray()

        def flush(final):
            n = len(buf) if final else len(buf) // 65280 * 65280
            blocks = [bytes(buf[i:i + 65280]) for i in range(0, n, 65280)]
            for m in pool.map(lambda pl: member(deflate(pl, level), pl), blocks):
                f.write(m)
            del buf[:n]
        for p in pieces:
            buf += p
            if len(buf) >= 64 << 20:
                flush(False)
        flush(True)
        f.write(BGZF_EOF)


def write_bgzf_device(path, pieces, ctx, piece_bytes=256 << 20):
    """the same stream through the product's own deflate kernel (lib.bgzf_compress), members of 65 280 bytes"""
    from vacmap_amd.lib import bgzf_compress
    with open(path, 'wb') as f:
        buf = bytearray()
        for p in pieces:
            buf += p
            if len(buf) >= piece_bytes:
                n = len(buf) // 65280 * 65280
                f.write(bgzf_compress(ctx, bytes(buf[:n]))); del buf[:n]
        if buf:
            f.write(bgzf_compress(ctx, bytes(buf)))
        f.write(BGZF_EOF)


def read_checksums(reader, max_reads=4096):
    """[(crc32 name, crc32 bases, crc32 qualities)] of everything a reader hands out"""
    out = []
    while True:
        ch = reader.read(max_reads)
        if ch is None:
            return out
        cols = []
        for key in ('names', 'seqs', 'quals'):
            blob, off = ch[key], ch[key + '_off']
            mv = memoryview(np.ascontiguousarray(blob))
            cols.append([zlib.crc32(mv[int(off[j]):int(off[j + 1])]) for j in range(len(off) - 1)])
        out += list(zip(*cols))
