"""Shared builders of the FASTA-reads tests (test_fasta_reads_emu.py, test_gpu_fasta_reads.py): seeded multi-line FASTA texts that hold every
shape the rule of VM_READER_FASTA names (include/vacmapx.h), texts with a chosen byte at a window's end, files that mix FASTQ and FASTA
records, and a plain Python statement of the rule (parse). The reference of the tests is lib.Fastx on the same file; nothing here shares
code with the kernels."""
import re
import zlib

import numpy as np

import fastq_input_cases as F

LINE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097)


def _seq(rng, n, letters='ACGT'):
    return F._seq(rng, n, letters).encode()


def wrap(s, width=60):
    return [s[i:i + width] for i in range(0, len(s), width)] or [b'']


def shape_records(seed=1, long_line=200000):
    """[(header line without '>', [body lines])]: every shape of the rule among random records"""
    rng = np.random.default_rng(seed)
    out = []

    def rnd(k):
        for _ in range(k):
            n, w = int(rng.integers(1, 3000)), int(rng.integers(20, 130))
            out.append((b'r%d_%d' % (seed, len(out)), wrap(_seq(rng, n), w)))
    rnd(4)
    out.append((b'nobody', []))                                                             # 0, 1, 2 and many body lines
    out.append((b'one', [_seq(rng, 70)]))
    out.append((b'two', [_seq(rng, 60), _seq(rng, 31)]))
    rnd(1)
    for n in LINE_LENGTHS:
        out.append((b'len%d' % n, [_seq(rng, 40), _seq(rng, n), _seq(rng, 33)]))
        out.append((b'only%d' % n, [_seq(rng, n)]))
    out.append((b'lower', wrap(_seq(rng, 300, 'acgtn'))))
    out.append((b'iupac', wrap(_seq(rng, 500, F.IUPAC))))
    out.append((b'other bytes', [b'AC-.*zZ{`[@a', b'`a{z']))                               # bytes on both sides of a-z stay
    out.append((b'interior', [b'AC GT', b'AC\tgt  NN', b'A \t C']))
    out.append((b'ends', [b'  ACGT', b'ACGT \t', b' \t ac gt\t ', b' ', b'\t', b' \t ', b'', b'  A  ']))
    out.append((b'cr', [b'NN\r', b'\r', b' \r ', b'AC\r\r', b'\r\rGT']))                     # a '\r' that is not the line's last stays
    out.append((b'gt_behind_blank', [b'ACGT', b' >x', b'\t>y z', b'AC']))
    out.append((b'fastq_looking', [b'@q1', b'ACGT', b'+', b'IIII', b'@', b'+x']))
    out.append((b'nocomment', [_seq(rng, 80)]))
    out.append((b'sp a comment with  two blanks', [_seq(rng, 80)]))
    out.append((b'tab\ta comment\twith tabs', [_seq(rng, 80)]))
    out.append((b' x', [_seq(rng, 10)]))                                                    # "> x": empty name, comment x
    out.append((b'', [_seq(rng, 10)]))                                                      # ">" alone
    out.append((b'', []))
    out.append((b'trailing ', [_seq(rng, 10)]))
    out.append((b'big ' + _seq(rng, 5000, 'C+m,0123456789;'), wrap(_seq(rng, 900))))
    out.append((b'n' * 200 + b'\t' + _seq(rng, 3000, F.QUAL_NO_GT), [_seq(rng, 90)]))        # the separator beyond the first 64 bytes
    for total in (64, 65):                                                                  # header lines of exactly 64 and 65 bytes
        out.append((b'h' * (total - 1 - 4) + b' cdd', [_seq(rng, 20)]))
        out.append((b'H' * (total - 1), [_seq(rng, 20)]))
    rnd(2)
    if long_line:
        s = _seq(rng, long_line)
        out.append((b'long_unwrapped', [s]))
        out.append((b'long_wrapped', wrap(s)))
    rnd(4)
    return out


def text_of(recs, eol='lf', seed=5, start_blank=False, between_blank=True, end_blank=False, final_nl=True):
    """the FASTA text: eol 'lf', 'crlf' or 'mixed' (seeded per line); blank and white-space-only lines at the start, between records (by the
    rule they are body lines of the record in front), inside records and at the end"""
    rng = np.random.default_rng(seed)

    def e():
        return b'\r\n' if eol == 'crlf' or (eol == 'mixed' and rng.integers(0, 2)) else b'\n'
    blanks = [b'', b' ', b'\t', b' \t ', b'\r']
    out = bytearray()
    if start_blank:
        for b in blanks:
            out += b + e()
    for i, (h, body) in enumerate(recs):
        out += b'>' + h + e()
        for j, ln in enumerate(body):
            out += ln + e()
            if between_blank and i % 5 == 2 and j == 0:
                out += blanks[(i // 5) % len(blanks)] + e()                                  # inside the record
        if between_blank and i % 4 == 1:
            out += blanks[(i // 4) % len(blanks)] + e()
    if end_blank:
        for b in blanks[::-1]:
            out += b + e()
    if not final_nl:
        while out[-1:] in (b'\n', b'\r'):
            del out[-1:]
        if end_blank:
            out += b'\n \t'
    return bytes(out)


def parse(text):
    """the rule in plain Python: ([(name, comment, bases, qualities)], None | 'truncated' | 'header', the bad header's first 40 bytes)"""
    lines = text.split(b'\n')
    if lines[-1] == b'':
        lines.pop()
    lines = [ln[:-1] if ln.endswith(b'\r') else ln for ln in lines]

    def head(ln):
        m = re.search(rb'[ \t]', ln[1:])
        return [ln[1:1 + m.start()], ln[2 + m.start():]] if m else [ln[1:], b'']
    recs, state, cur = [], 0, None
    for ln in lines:
        if state == 0:
            if ln.strip(b' \t\r') == b'':
                continue
            if ln[:1] == b'>':
                cur = head(ln) + [bytearray(), b'']; recs.append(cur); state = 4
            elif ln[:1] == b'@':
                cur = head(ln) + [bytearray(), b'']; state = 1
            else:
                return [tuple(bytes(x) for x in r) for r in recs], 'header', ln[:40]
        elif state == 1:
            cur[2] += ln.upper(); state = 2
        elif state == 2:
            state = 3
        elif state == 3:
            cur[3] = ln; recs.append(cur); state = 0
        elif ln[:1] == b'>':
            cur = head(ln) + [bytearray(), b'']; recs.append(cur)
        else:
            cur[2] += ln.strip(b' \t').upper()
    return [tuple(bytes(x) for x in r) for r in recs], 'truncated' if state in (1, 2, 3) else None, None


# the texts of the rule's "consequences", with what they must give
RULE_TEXTS = (
    (b'>f1\nAC\n\n@q\nAC\n+\nII\n', [(b'f1', b'', b'AC@QAC+II', b'')]),
    (b'@q1\nAC\n+\nII\n>f1\nAC\n@q2\nGG\n+\nII\n', [(b'q1', b'', b'AC', b'II'), (b'f1', b'', b'AC@Q2GG+II', b'')]),
    (b'>a\nAC\n >x\nGT\n', [(b'a', b'', b'AC>XGT', b'')]),
    (b'>a\nAC GT\nNN\r\r\n \r \r\n', [(b'a', b'', b'AC GTNN\r\r', b'')]),
    (b'>\n\n>c3', [(b'', b'', b'', b''), (b'c3', b'', b'', b'')]),
    (b'@q ab\n ac gt \n+\n II \n', [(b'q', b'ab', b' AC GT ', b' II ')]),
)

SHORT_FASTA = (b'>c1 d\nACGTACGT\n', b'>c1\nACGT\nACGT\n', b'>c1', b'>c1 d\n', b'\n \n>c1\nacgt', b'>c1\nAC\n>c2\nGT\n', b'\n>c1 d\nACGT\nACGT\n>c2\nAC\n')


def filler(rng, upto, width=60):
    """FASTA records of wrapped lines, ending on a newline, of exactly `upto` bytes"""
    out = bytearray()
    k = 0
    while len(out) < upto - 2000:
        out += b'>f%d c\n' % k + b'\n'.join(wrap(_seq(rng, int(rng.integers(100, 900))), width)) + b'\n'
        k += 1
    rest = upto - len(out)                                                                   # one record of exactly the bytes that are left
    assert rest > 8
    out += b'>z\n' + _seq(rng, rest - 4) + b'\n'
    assert len(out) == upto
    return out


def boundary_text(cut, kind, seed=9):
    """a text whose byte `cut` (the first byte of the second window when the first ends at `cut`) is: 'start' the '>' of a record; 'crlf' the
    '\\n' of a body line's '\\r\\n'; 'header' the first body byte behind a header's newline"""
    rng = np.random.default_rng(seed)
    if kind == 'start':
        out = filler(rng, cut)
    elif kind == 'crlf':
        out = filler(rng, cut - 70)
        out += b'>s x\n' + _seq(rng, 70 - 5 - 1) + b'\r'
    else:
        out = filler(rng, cut - 8)
        out += b'>hdr cc\n'
    assert len(out) == cut, (len(out), cut)
    if kind == 'crlf':
        out += b'\nGGCC\r\n'
    elif kind == 'header':
        out += b'ACGT\nAC\n'
    for k in range(20):
        out += b'>a%d x\n' % k + b'\n'.join(wrap(_seq(rng, int(rng.integers(50, 600))))) + b'\n'
    assert {'start': out[cut:cut + 1] == b'>', 'crlf': out[cut - 1:cut + 1] == b'\r\n', 'header': out[cut - 8:cut] == b'>hdr cc\n'}[kind]
    return bytes(out)


def long_record_text(n, wrapped, seed=3):
    """one record of n bases between two small ones; returns (text, bases)"""
    rng = np.random.default_rng(seed)
    s = _seq(rng, n, 'ACGTacgtN')
    body = b'\n'.join(wrap(s)) if wrapped else s
    return b'>first\nACGT\n>big one\n' + body + b'\n>last\nGG\n', s.upper()


def scale_text(n_bytes, seed=17, pool=64):
    """FASTA text of at least n_bytes as a list of record pieces: 15 kb reads (2 ... 40 kb), even records on one line, odd ones wrapped at 60;
    read i is a rotation of pool read i mod pool. Returns (pieces, [(crc32 name, crc32 bases, crc32 of nothing)])"""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(15000, 4000, pool), 2000, 40000).astype(np.int64)
    seqs = [np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, int(n))] for n in lens]
    pieces, want, tot, i = [], [], 0, 0
    while tot < n_bytes:
        k = i % pool
        n = int(lens[k])
        s = np.roll(seqs[k], (i * 131) % n).tobytes()
        name = b'read%09d' % i
        want.append((zlib.crc32(name), zlib.crc32(s), zlib.crc32(b'')))
        body = (b'\n'.join(wrap(s)) if i % 2 else s) + b'\n'
        pieces.append(b'>' + name + b' ch=%d\n' % (i % 512) + body)
        tot += len(pieces[-1]); i += 1
    return pieces, want


def alignment_records(seed=31):
    """64 x 17 records of one body line each, lengths 0 ... 63: the name length of each record walks the source start of its body line
    through every residue mod 16 while the destination start (the sum of the lengths before) walks through them at another pace.
    Returns (records for text_of, the set of (source, destination) residues)"""
    rng = np.random.default_rng(seed)
    recs, pairs, src, dst = [], set(), 0, 0
    for i in range(64 * 17):
        n = i % 64
        name = b'w' * (1 + (dst + i // 64 - (src + 3)) % 16)
        recs.append((name, [_seq(rng, n, 'ACGTacgtNn')]))
        src += 1 + len(name) + 1                                                             # '>', the name, '\n'
        pairs.add((src % 16, dst % 16))
        src += n + 1; dst += n
    return recs, pairs
