"""Shared builders of the bgzipped-FASTQ input tests (test_fastq_input_emu.py, test_gpu_fastq_input.py): seeded FASTQ texts that hold every
shape the rule of vm_fastq_reader_read names (include/vacmapx.h), streams with a record or line boundary at a chosen byte, single edits of
a valid text, and a plain Python statement of the rule (parse). The reference of the tests is lib.Fastx on the same file; nothing here
shares code with the kernels."""
import re
import zlib

import numpy as np

import bam_input_cases as K

IUPAC = 'ACGTNRYKMSWBDHVacgtnrykm'
QUAL_NO_GT = ''.join(chr(c) for c in range(33, 127) if chr(c) != '>')


def _seq(rng, n, letters='ACGT'):
    return ''.join(letters[j] for j in rng.integers(0, len(letters), n))


def _qual(rng, n, alphabet=QUAL_NO_GT):
    return ''.join(alphabet[j] for j in rng.integers(0, len(alphabet), n))


def shape_records(seed=1, long_read=200000):
    """[(header line without '@', bases, plus line, qualities)]: every shape of the issue's list among random reads"""
    rng = np.random.default_rng(seed)
    out = []

    def rnd(k):
        for i in range(k):
            n = int(rng.integers(1, 700))
            out.append(('r%d_%d' % (seed, len(out)), _seq(rng, n), '+', _qual(rng, n)))
    rnd(5)
    for n in (0, 1, 63, 64, 65):
        out.append(('len%d' % n, _seq(rng, n), '+', _qual(rng, n)))
        rnd(1)
    out.append(('lower', _seq(rng, 300, 'acgtn'), '+', _qual(rng, 300)))
    out.append(('iupac', _seq(rng, 500, IUPAC), '+', _qual(rng, 500)))
    out.append(('other bytes', 'AC-.*zZ{`[@a', '+', _qual(rng, 12)))                       # bytes on both sides of a-z stay
    out.append(('nocomment', _seq(rng, 80), '+', _qual(rng, 80)))
    out.append(('sp a comment with  two blanks', _seq(rng, 80), '+', _qual(rng, 80)))
    out.append(('tab\ta comment\twith tabs', _seq(rng, 80), '+', _qual(rng, 80)))
    out.append((' x', _seq(rng, 10), '+', _qual(rng, 10)))                                  # "@ x": empty name, comment x
    out.append(('trailing ', _seq(rng, 10), '+', _qual(rng, 10)))                           # a separator and an empty comment
    out.append(('big MM:Z:' + _seq(rng, 5000, 'C+m,0123456789;'), _seq(rng, 900), '+', _qual(rng, 900)))
    out.append(('n' * 200 + '\t' + _qual(rng, 3000), _seq(rng, 90), '+', _qual(rng, 90)))   # the separator beyond the first 64 bytes
    for total in (64, 65):                                                                    # header lines of exactly 64 and 65 bytes
        out.append(('h' * (total - 1 - 4) + ' c' + 'dd'[:2], _seq(rng, 20), '+', _qual(rng, 20)))
        out.append(('H' * (total - 1), _seq(rng, 20), '+', _qual(rng, 20)))
    out.append(('q_at', _seq(rng, 40), '+', '@' + _qual(rng, 39)))
    out.append(('q_plus', _seq(rng, 40), '+', '+' + _qual(rng, 39)))
    out.append(('q_at_only', 'A', '+', '@'))
    out.append(('empty', '', '+', ''))
    out.append(('plusname', _seq(rng, 33), '+plusname some text', _qual(rng, 33)))
    out.append(('unequal', _seq(rng, 50), '+', _qual(rng, 7)))                              # the lengths are not compared
    rnd(3)
    if long_read:
        out.append(('long', _seq(rng, long_read), '+', _qual(rng, long_read)))
    rnd(6)
    return out


def text_of(recs, eol='lf', seed=5, start_blank=False, between_blank=True, end_blank=False, final_nl=True):
    """the FASTQ text: eol 'lf', 'crlf' or 'mixed' (seeded per line); blank and white-space-only lines at the start, between records, at the end"""
    rng = np.random.default_rng(seed)

    def e():
        return b'\r\n' if eol == 'crlf' or (eol == 'mixed' and rng.integers(0, 2)) else b'\n'
    blanks = [b'', b' ', b'\t', b' \t ', b'\r']
    out = bytearray()
    if start_blank:
        for b in blanks:
            out += b + e()
    for i, (h, s, p, q) in enumerate(recs):
        for ln in (b'@' + h.encode(), s.encode(), p.encode(), q.encode()):
            out += ln + e()
        if between_blank and i % 4 == 1:
            out += blanks[(i // 4) % len(blanks)] + e()
    if end_blank:
        for b in blanks[::-1]:
            out += b + e()
    if not final_nl:
        while out[-1:] in (b'\n', b'\r'):
            del out[-1:]
        if end_blank:
            out += b'\n \t'                                                                  # an unterminated white-space line ends the file
    return bytes(out)


def boundary_text(cut, crlf_split, seed=9):
    """a text whose byte `cut` is the first byte behind a quality line's newline (crlf_split False), or the '\\n' of a quality line's '\\r\\n'
    (crlf_split True: a window that ends at `cut` ends between the two)"""
    rng = np.random.default_rng(seed)
    out = bytearray()
    while len(out) < cut - 3000:
        n = int(rng.integers(50, 600))
        out += b'@b%d\n%s\n+\n%s\n' % (len(out), _seq(rng, n).encode(), _qual(rng, n).encode())
    name = b'f' if (cut - len(out) - 7) % 2 == 0 else b'ff'
    n = (cut - len(out) - 6 - len(name)) // 2
    out += b'@' + name + b'\n' + _seq(rng, n).encode() + b'\n+\n' + _qual(rng, n).encode() + (b'\r\n' if crlf_split else b'\n')
    assert (out[cut - 1:cut + 1] == b'\r\n' and len(out) == cut + 1) if crlf_split else (out[cut - 1:cut] == b'\n' and len(out) == cut)
    for k in range(30):
        n = int(rng.integers(50, 600))
        out += b'@a%d x\n%s\n+\n%s\n' % (k, _seq(rng, n).encode(), _qual(rng, n).encode())
    return bytes(out)


def parse(text):
    """the rule in plain Python: ([(name, comment, bases, qualities)], None | 'truncated' | 'header' | 'fasta')"""
    lines = text.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    lines = [ln[:-1] if ln.endswith(b'\r') else ln for ln in lines]
    recs, i = [], 0
    while i < len(lines):
        ln = lines[i]; i += 1
        if ln.strip(b' \t\r') == b'':
            continue
        if ln[:1] == b'>':
            return recs, 'fasta'
        if ln[:1] != b'@':
            return recs, 'header'
        if i + 3 > len(lines):
            return recs, 'truncated'
        m = re.search(rb'[ \t]', ln[1:])
        name, com = (ln[1:1 + m.start()], ln[2 + m.start():]) if m else (ln[1:], b'')
        up = bytes(c - 32 if 97 <= c <= 122 else c for c in lines[i])
        recs.append((name, com, up, lines[i + 2])); i += 3
    return recs, None


def chunk_records(chunks):
    out = []
    for ch in chunks:
        cols = []
        for key in ('names', 'comments', 'seqs', 'quals'):
            b, o = bytes(ch[key]), ch[key + '_off']
            cols.append([b[int(o[j]):int(o[j + 1])] for j in range(len(o) - 1)])
        out += list(zip(*cols))
    return out


def edits(text, n, seed):
    """n single edits of a valid text: delete a newline, insert a newline, insert '\\r', insert a blank line, cut at a random byte"""
    rng = np.random.default_rng(seed)
    nl = [i for i, c in enumerate(text) if c == 10]
    for k in range(n):
        kind = k % 5
        at = int(rng.integers(0, len(text) + 1))
        if kind == 0:
            p = nl[int(rng.integers(0, len(nl)))]
            yield 'delete_nl', text[:p] + text[p + 1:]
        elif kind == 1:
            yield 'insert_nl', text[:at] + b'\n' + text[at:]
        elif kind == 2:
            yield 'insert_cr', text[:at] + b'\r' + text[at:]
        elif kind == 3:
            p = nl[int(rng.integers(0, len(nl)))] + 1
            yield 'blank_line', text[:p] + [b'\n', b' \n', b'\t\r\n'][k % 3] + text[p:]
        else:
            yield 'cut', text[:at]


def scale_text(n_bytes, seed=17, pool=64):
    """FASTQ text of at least n_bytes as a list of record pieces: 15 kb ONT-shape reads (2 ... 40 kb) with bam_codec.ont_quals qualities; read i is a
    rotation of pool read i mod pool. Returns (pieces, [(crc32 name, crc32 bases, crc32 qualities)])"""
    import bam_codec as B
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(15000, 4000, pool), 2000, 40000).astype(np.int64)
    seqs = [np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, int(n))] for n in lens]
    quals = [np.frombuffer(B.ont_quals(int(n), seed * 100 + k).encode(), np.uint8) for k, n in enumerate(lens)]
    pieces, want, tot, i = [], [], 0, 0
    while tot < n_bytes:
        k = i % pool
        n = int(lens[k])
        s = np.roll(seqs[k], (i * 131) % n).tobytes(); q = np.roll(quals[k], (i * 17) % n).tobytes()
        name = b'read%09d' % i
        want.append((zlib.crc32(name), zlib.crc32(s), zlib.crc32(q)))
        pieces.append(b'@' + name + b' ch=%d\n' % (i % 512) + s + b'\n+\n' + q + b'\n')
        tot += len(pieces[-1]); i += 1
    return pieces, want
