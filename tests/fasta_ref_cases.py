"""Reference FASTA texts for the device parser (vm_index_build_fasta_device, csrc/k_fasta_in.hip), shared by the emulator and the GPU tests, a
second statement of the line rule in Python, and the comparison: the index of the host parser and the index of the device parser, saved,
are the same file."""
import gzip
import os

import numpy as np

import bam_input_cases as K

KW = dict(k=7, w=3)                     # small: the index build of a 200 kb text stays in seconds on the emulator
UNSUPPORTED = -7


def parse(text):
    """the rule (include/vacmapx.h): [(name, upper-case letters)]"""
    out = []
    for ln in text.split(b'\n'):
        ln = ln.rstrip(b'\r')
        if not ln:
            continue
        if ln[:1] == b'>':
            name = ln[1:]
            for i, c in enumerate(name):
                if c in b' \t':
                    name = name[:i]
                    break
            out.append([name, []])
        elif out:
            out[-1][1].append(ln)
    return [(n, bytes(c - 32 if 97 <= c <= 122 else c for c in b''.join(p))) for n, p in out]


def n_other(text):
    return sum(1 for _, s in parse(text) for c in s if c not in b'ACGTN')


def seq(rng, n, letters='ACGT'):
    return np.frombuffer(letters.encode(), np.uint8)[rng.integers(0, len(letters), int(n))].tobytes()


def wrap(s, width, eol=b'\n'):
    return b''.join(s[i:i + width] + eol for i in range(0, len(s), width))


def fasta(contigs, width=60, eol=b'\n'):
    return b''.join(b'>' + n + eol + wrap(s, width, eol) for n, s in contigs)


def forms(text, block=65280, eof=True, level=6):
    """the three files of one text"""
    return {'plain': text, 'bgzf': K.bgzf(text, level, block=block, eof=eof), 'gzip': gzip.compress(text, 6)}


def vmx_bytes(idx, path):
    idx.save(path)
    with open(path, 'rb') as f:
        return f.read()


def vmx_of_rule(text, vmx):
    """(names, lengths, bases) of a .vmx file against the rule in Python"""
    want = parse(text)
    hdr = np.frombuffer(vmx[8:56], np.int64)
    at, names, lens = 56, [], []
    for _ in range(int(hdr[2])):
        nl = int(np.frombuffer(vmx[at:at + 8], np.int64)[0]); names.append(vmx[at + 8:at + 8 + nl]); lens.append(int(np.frombuffer(vmx[at + 8 + nl:at + 16 + nl], np.int64)[0])); at += 16 + nl
    assert names == [n for n, _ in want] and lens == [len(s) for _, s in want]
    assert vmx[at:at + int(hdr[4])] == b''.join(s for _, s in want)


def other_message(VL, ctx, idx):
    """n_other_letters through its visible effect: the device SAM emitter's refusal (None: it serves the index)"""
    import sam_device_cases as SD
    try:
        SD.run_device(VL, ctx, idx, SD.Case('none', []))
    except VL.VmxError as e:
        assert e.code == UNSUPPORTED
        return str(e)
    return None


def build(VL, ctx, path, reader):
    """(index, None) or (None, VmxError)"""
    try:
        return VL.Index.from_fasta(ctx, path, reader=reader, **KW), None
    except VL.VmxError as e:
        return None, e


def check_text(VL, ctx, tmp_path, text, block=65280, eof=True, level=6, which=('plain', 'bgzf', 'gzip')):
    """the host index of the plain text, saved twice, is one file; the native reader on all three forms and the host reader on the two
    compressed forms give that file and the same refusal of the device SAM emitter. Returns the native readers' statistics by form."""
    d = str(tmp_path)
    files = forms(text, block, eof, level)
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(d, 'ref_%s.fa%s' % (name, '' if name == 'plain' else '.gz'))
        with open(paths[name], 'wb') as f:
            f.write(data)
    host = VL.Index.from_fasta(ctx, paths['plain'], **KW)
    want = vmx_bytes(host, os.path.join(d, 'host.vmx'))
    assert vmx_bytes(host, os.path.join(d, 'host2.vmx')) == want
    vmx_of_rule(text, want)
    msg = other_message(VL, ctx, host)
    assert (msg is not None) == (n_other(text) > 0) and (msg is None or ' %d letters' % n_other(text) in msg)
    host.close()
    stats = {}
    for name in which:
        for reader in (('native',) if name == 'plain' else ('native', 'host')):
            idx = VL.Index.from_fasta(ctx, paths[name], reader=reader, **KW)
            try:
                assert vmx_bytes(idx, os.path.join(d, 'got.vmx')) == want, (name, reader)
                assert other_message(VL, ctx, idx) == msg, (name, reader)
                if reader == 'native':
                    stats[name] = idx.build_stats
                    assert idx.build_stats['text_bytes'] == len(text) and idx.build_stats['contigs'] == len(parse(text))
            finally:
                idx.close()
    return stats


# ---------------------------------------------------------------- texts

def eol_texts():
    rng = np.random.default_rng(5)
    a, b, c = seq(rng, 700, 'ACGTacgtNn'), seq(rng, 333), seq(rng, 61)
    out = {}
    out['lf'] = fasta([(b'c1 first', a), (b'c2', b), (b'c3\tx', c)])
    out['crlf'] = fasta([(b'c1 first', a), (b'c2', b), (b'c3\tx', c)], eol=b'\r\n')
    out['mixed'] = b'>c1 d\r\n' + wrap(a[:300], 60) + wrap(a[300:], 50, b'\r\n') + b'>c2\n' + wrap(b, 70, b'\r\r\n') + b'>c3\r\r\n' + c
    out['interior_cr'] = b'>c1\nACGT\rACGT\nAC\r\rGT\r\n\rACGT\n>c2\r\nGG\rCC'
    out['blanks'] = b'\n\r\n\r\r\n>c1\n' + wrap(a, 60) + b'\n\r\n>c2\n\n' + wrap(b, 60) + b'\r\n\n\r\n'
    # '\r' runs across a 1024-byte step and a 4096-byte chunk of the device parser, a line of 2100 '\r', an interior run longer than a step
    out['cr_runs'] = (b'>c1\n' + a[:600] + b[:333] + c + a[:6] + b'\r' * 40 + b'\n' + seq(rng, 3030) + b'\r' * 30 + b'\n' + b'\r' * 2100 + b'\nAC' + b'\r' * 1100 + b'GT\n' +
                      b'>c2\r\n' + b + b'\r' * 1500)
    out['no_final_nl'] = fasta([(b'c1', a), (b'c2', b)])[:-1]
    out['final_cr_no_nl'] = fasta([(b'c1', a), (b'c2', b)])[:-1] + b'\r\r'
    return out


def header_texts():
    rng = np.random.default_rng(6)
    a, b = seq(rng, 500), seq(rng, 130)
    out = {}
    out['gt_alone'] = b'>\n' + wrap(a, 60) + b'>c2\n' + wrap(b, 60)
    out['gt_blank_x'] = b'> x\n' + wrap(a, 60) + b'>a\tb c\n' + wrap(b, 60)
    out['header_last_nl'] = fasta([(b'c1', a)]) + b'>last\n'
    out['header_last_no_nl'] = fasta([(b'c1', a)]) + b'>last and more'
    out['two_headers'] = b'>c1\n>c2 empty before\n' + wrap(a, 60) + b'>c3\r\n>c4\n' + wrap(b, 60) + b'>c5\n'
    out['dropped_lines'] = wrap(b, 60) + b'\nACGT\n' + fasta([(b'c1', a)])
    out['no_header'] = wrap(a, 60)
    out['empty'] = b''
    out['only_blank'] = b'\n\r\n'
    out['gt_inside'] = b'>c1\nAC>GT\n' + wrap(a, 60) + b' >x\n\r>y\n'
    return out


def letter_texts():
    rng = np.random.default_rng(7)
    out = {}
    out['acgtn'] = fasta([(b'c1', seq(rng, 900, 'acgtn')), (b'c2', seq(rng, 100, 'ACGTN'))])
    out['iupac'] = fasta([(b'c1', seq(rng, 900, 'ACGTRYKMSWBDHVNacgtrykmswbdhvn'))])
    out['blank_inside'] = b'>c1\nACGT ACGT\n' + wrap(seq(rng, 300), 60) + b'   \n \t \r\n' + wrap(seq(rng, 100), 60)
    return out


def width_text(width, seed=8):
    rng = np.random.default_rng(seed)
    n = max(3 * width + width // 2, 700)
    return fasta([(b'w%d a' % width, seq(rng, n, 'ACGTacgtn')), (b'x', seq(rng, 2 * width + 1))], width=width)


def long_line_text():
    """one unwrapped 200 kb line, then a wrapped contig"""
    rng = np.random.default_rng(9)
    return b'>big one\n' + seq(rng, 200000, 'ACGTacgtN') + b'\r\n>small\n' + wrap(seq(rng, 5000), 60)


def boundary_text(at, seed=10):
    """the '>' of the second contig is byte `at` of the text"""
    rng = np.random.default_rng(seed)
    head = b'>c1\n'
    body = at - len(head)
    lines = wrap(seq(rng, body - (body + 60) // 61, 'ACGTacgt'), 60)
    text = head + lines
    text = text[:at - 1] + b'\n' if len(text) >= at else text + seq(rng, at - 1 - len(text)) + b'\n'
    assert len(text) == at
    return text + b'>c2 at the boundary\n' + wrap(seq(rng, 3000), 60)


def crlf_split_text(at, seed=11):
    """CRLF lines; byte at - 1 is a '\\r' and byte at its '\\n'"""
    rng = np.random.default_rng(seed)
    text = b'>c1\r\n'
    while len(text) + 62 < at - 1:
        text += seq(rng, 60) + b'\r\n'
    text += seq(rng, at - 1 - len(text)) + b'\r\n'
    assert text[at - 1:at + 1] == b'\r\n'
    return text + wrap(seq(rng, 2000), 60, b'\r\n') + b'>c2\r\n' + wrap(seq(rng, 1000), 60, b'\r\n')


def header_split_text(at, seed=12):
    """byte `at` lies inside a header line of 300 bytes"""
    rng = np.random.default_rng(seed)
    text = b'>c1\n'
    while len(text) + 61 < at - 100:
        text += seq(rng, 60) + b'\n'
    text += seq(rng, at - 100 - len(text) - 1) + b'\n'
    assert len(text) == at - 100
    return text + b'>c2 ' + b'd' * 295 + b'\n' + wrap(seq(rng, 4000), 60) + b'>c3\n' + wrap(seq(rng, 100), 60)


def long_header_text(n=70000, seed=13):
    rng = np.random.default_rng(seed)
    return b'>c1\n' + wrap(seq(rng, 1000), 60) + b'>c2 ' + b'x' * n + b'\n' + wrap(seq(rng, 1000), 60)


def alignment_text():
    """kept runs (sequence lines) at every (source mod 16, destination mod 16). A group is a header and 16 lines whose length is a multiple of
    16: the destination residue stays while the source residue, one newline further per line, takes all 16 values; one line of 16 m + 1
    letters ends the group and moves the destination residue on. The header lengths differ from group to group. Returns (text, the pairs)."""
    rng = np.random.default_rng(14)
    parts, pairs, src, dst = [], set(), 0, 0
    for g in range(16):
        name = b'>g%d %s\n' % (g, b'h' * (g * 5 % 23))
        parts.append(name); src += len(name)
        for j in range(17):
            n = (16, 48, 32, 64)[g % 4] + (j == 16)
            pairs.add((src % 16, dst % 16))
            parts.append(seq(rng, n, 'ACGTacgtNn') + b'\n'); src += n + 1; dst += n
    return b''.join(parts), pairs


def scale_text(n_bytes, seed=15):
    """about n_bytes of 60-column FASTA in 5 contigs, one of a few hundred bytes; as a list of pieces"""
    rng = np.random.default_rng(seed)
    unit = np.frombuffer(wrap(seq(rng, 60 * 4096), 60), np.uint8)
    pieces = []
    share = [0.37, 0.0, 0.31, 0.2, 0.12]
    for c, f in enumerate(share):
        pieces.append(b'>chr%d scale\n' % (c + 1))
        if f == 0.0:
            pieces.append(wrap(seq(rng, 333), 60))
            continue
        lines = int(n_bytes * f) // 61
        for a in range(0, lines, 4096):
            m = min(4096, lines - a)
            pieces.append(np.roll(unit[:m * 61].reshape(m, 61), (a // 4096 + c) % 57, axis=0).tobytes())
        pieces.append(seq(rng, 17 + c) + b'\n')
    return pieces


def edits(text, n, seed):
    import fastq_input_cases as F
    return F.edits(text, n, seed)
