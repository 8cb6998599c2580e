"""Shared by test_bam_tags_emu.py and test_gpu_bam_tags.py: the specification of a BAM record's auxiliary fields as SAM text (aux_text, written
from SAMv1 §4.2.4 and the rules of vm_bam_reader_open_tags' header comment; it shares no code with the driver or the kernels), builders of aux
bytes, the case sets, and the checks that both suites run against a context (the emulator build's or the device's)."""
import struct

import numpy as np

import bam_input_cases as K

_FIXED = {'A': 1, 'c': 1, 'C': 1, 's': 2, 'S': 2, 'i': 4, 'I': 4, 'f': 4}
_FMT = {'c': 'b', 'C': 'B', 's': 'h', 'S': 'H', 'i': 'i', 'I': 'I', 'f': 'f'}
VM_ERR_ARG, VM_ERR_IO = -1, -5


# ---------------------------------------------------------------- the specification

def float_text(bits):
    """a finite float32 (given by its bits): the shortest '%.{p}g', p = 1 ... 9, that strtod followed by a cast reads back as the same float32"""
    x = np.array([bits], np.uint32).view(np.float32)[0]
    with np.errstate(over='ignore'):
        for p in range(1, 10):
            s = '%.*g' % (p, float(x))
            if np.float32(float(s)) == x:
                return s
    raise AssertionError('no p <= 9 reads back: %08x' % bits)


def _finite(bits):
    return (bits >> 23) & 0xff != 0xff


def aux_text(aux, select):
    """(text, n_dropped) of a record's aux bytes; select: None (nothing: the bytes are not looked at), '*' (every field) or a collection of
    two-character tags. ValueError when the bytes are malformed."""
    if select is None:
        return '', 0
    want = None if isinstance(select, str) and select in ('*', 'all') else {t.encode() if isinstance(t, str) else bytes(t) for t in select}
    out, dropped, p, n = [], 0, 0, len(aux)
    while p < n:
        if n - p < 3:
            raise ValueError('fewer than 3 bytes left')
        tag, ty = aux[p:p + 2], chr(aux[p + 2])
        p += 3
        text = None                                      # None: dropped
        if ty in _FIXED:
            size = _FIXED[ty]
            if p + size > n:
                raise ValueError('fixed-size value past the end')
            raw = aux[p:p + size]
            p += size
            if ty == 'A':
                if 0x20 <= raw[0] <= 0x7e:
                    text = 'A:' + chr(raw[0])
            elif ty == 'f':
                bits = struct.unpack('<I', raw)[0]
                if _finite(bits):
                    text = 'f:' + float_text(bits)
            else:
                text = 'i:%d' % struct.unpack('<' + _FMT[ty], raw)[0]
        elif ty in 'ZH':
            e = aux.find(b'\0', p)
            if e < 0:
                raise ValueError('no NUL')
            val = aux[p:e]
            p = e + 1
            if ty == 'Z':
                ok = all(0x20 <= b <= 0x7e for b in val)
            else:
                ok = len(val) % 2 == 0 and all(chr(b) in '0123456789ABCDEFabcdef' for b in val)
            if ok:
                text = ty + ':' + val.decode('ascii')
        elif ty == 'B':
            if p + 5 > n:
                raise ValueError('B header past the end')
            sub, cnt = chr(aux[p]), struct.unpack_from('<I', aux, p + 1)[0]
            if sub not in 'cCsSiIf':
                raise ValueError('unknown B sub-type')
            size = _FIXED[sub]
            if p + 5 + cnt * size > n:
                raise ValueError('B array past the end')
            if sub == 'f':
                vals = np.frombuffer(aux, '<u4', cnt, p + 5) if (p + 5) % 4 == 0 else np.frombuffer(bytes(aux[p + 5:p + 5 + 4 * cnt]), '<u4')
                if all(_finite(int(b)) for b in vals):
                    text = 'B:f' + ''.join(',' + float_text(int(b)) for b in vals)
            else:
                vals = struct.unpack_from('<%d%s' % (cnt, _FMT[sub]), aux, p + 5)
                text = 'B:' + sub + ''.join(',%d' % v for v in vals)
            p += 5 + cnt * size
        else:
            raise ValueError('unknown type')
        if want is not None and tag not in want:
            continue
        if text is None:
            dropped += 1
        else:
            out.append(tag.decode('latin-1') + ':' + text)
    return '\t'.join(out), dropped


# ---------------------------------------------------------------- builders

def fld(tag, ty, val=None, sub=None):
    """one aux field. A: a character or a byte value; integers and f: a number (f also takes ('bits', u32)); Z / H: str or bytes; B: sub-type and a list"""
    t = tag.encode() + ty.encode()
    if ty == 'A':
        return t + (bytes([val]) if isinstance(val, int) else val.encode())
    if ty == 'f' and isinstance(val, tuple):
        return t + struct.pack('<I', val[1])
    if ty in _FMT:
        return t + struct.pack('<' + _FMT[ty], val)
    if ty in 'ZH':
        return t + (val if isinstance(val, bytes) else val.encode()) + b'\0'
    assert ty == 'B'
    body = np.asarray(val, np.uint32).astype('<u4').tobytes() if sub == 'F' else struct.pack('<%d%s' % (len(val), _FMT[sub]), *val)
    return t + (b'f' if sub == 'F' else sub.encode()) + struct.pack('<I', len(val)) + body          # sub 'F': a float array given as bit patterns


F_EDGES = [  # (float32 bits, the text, written by hand from the rule)
    (0x00000000, '0'), (0x80000000, '-0'),
    (0x00000001, '1e-45'),                   # the smallest denormal, 1.4013e-45: 1e-45 is above half of it
    (0x007fffff, '1.1754942e-38'),           # the largest denormal
    (0x00800000, '1.1754944e-38'),           # FLT_MIN
    (0x7f7fffff, '3.4028235e+38'),           # FLT_MAX
    (0x3dcccccd, '0.1'), (0x3f800000, '1'),
    (0x3f800001, '1.0000001'), (0x3f7fffff, '0.99999994'),      # 1 + 1 ulp, 1 - 1 ulp
    (0x4b800000, '16777216'), (0x4b7fffff, '16777215'),         # 2^24 (1.677722e+07 is 16 777 220, another float), 2^24 - 1
    (0x501502f9, '1e+10'),
    (0x38d1b716, '9.999999e-05'), (0x38d1b717, '0.0001'),      # the float below 1e-04f (exponent form), and 1e-04f = 9.9999998e-05: decimal exponent -4, fixed form
    (0xbf000000, '-0.5'), (0x42f6e979, '123.456'), (0x7e967699, '1e+38'), (0x0da24260, '1e-30'),
]


def every_type_record():
    """(aux bytes, the text for select='*', written by hand)"""
    aux = (fld('XA', 'A', 'q') + fld('Xc', 'c', -128) + fld('XC', 'C', 255) + fld('Xs', 's', -32768) + fld('XS', 'S', 65535) + fld('Xi', 'i', -2147483648) +
           fld('XI', 'I', 4294967295) + fld('Xf', 'f', 0.25) + fld('XZ', 'Z', 'a b:c') + fld('XH', 'H', '1AE301') + fld('Bc', 'B', [-1, 0, 127], 'c') +
           fld('BC', 'B', [0, 9, 10, 255], 'C') + fld('Bs', 'B', [-32768, 32767], 's') + fld('BS', 'B', [65535], 'S') + fld('Bi', 'B', [-2147483648, 7], 'i') +
           fld('BI', 'B', [4294967295], 'I') + fld('Bf', 'B', [1.5, -2.0, 1e10], 'f') + fld('B0', 'B', [], 'C'))
    text = ('XA:A:q\tXc:i:-128\tXC:i:255\tXs:i:-32768\tXS:i:65535\tXi:i:-2147483648\tXI:i:4294967295\tXf:f:0.25\tXZ:Z:a b:c\tXH:H:1AE301\tBc:B:c,-1,0,127\t'
            'BC:B:C,0,9,10,255\tBs:B:s,-32768,32767\tBS:B:S,65535\tBi:B:i,-2147483648,7\tBI:B:I,4294967295\tBf:B:f,1.5,-2,1e+10\tB0:B:C')
    return aux, text


def _boundary_values(sub, count, shift):
    """`count` values of an integer sub-type that step through every digit-count boundary of its range (9/10, 99/100, ..., -9/-10, ..., the
    minimum and the maximum), rotated by `shift` so that the boundaries fall on both sides of a 64-element step"""
    lo, hi = {'c': (-128, 127), 'C': (0, 255), 's': (-32768, 32767), 'S': (0, 65535), 'i': (-2 ** 31, 2 ** 31 - 1), 'I': (0, 2 ** 32 - 1)}[sub]
    edge = [lo, hi, 0]
    for k in range(1, 11):
        for v in (10 ** k - 1, 10 ** k, -(10 ** k - 1), -(10 ** k)):
            if lo <= v <= hi:
                edge.append(v)
    return [edge[(j + shift) % len(edge)] for j in range(count)]


COUNTS = (0, 1, 63, 64, 65, 129, 5000)


def random_float_bits(n, seed):
    bits = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    bad = (bits >> 23) & 0xff == 0xff
    bits[bad] &= np.uint32(0xbfffffff)                                   # non-finite ones replaced
    return bits


def edge_records():
    """[(name, aux)]: every type at its edges"""
    R = []
    ints = b''
    for ty, (lo, hi) in (('c', (-128, 127)), ('C', (0, 255)), ('s', (-32768, 32767)), ('S', (0, 65535)), ('i', (-2 ** 31, 2 ** 31 - 1)), ('I', (0, 2 ** 32 - 1))):
        ints += fld('l' + ty, ty, lo) + fld('h' + ty, ty, hi)
    R.append(('ints', ints))
    for n in (0, 1, 63, 64, 65, 200):
        z = ''.join(' :az~'[j % 5] if j % 7 else chr(33 + j % 90) for j in range(n))
        R.append(('z%d' % n, fld('aa', 'i', n) + fld('zz', 'Z', z) + fld('bb', 'C', 7)))
    R.append(('hex', fld('h0', 'H', '') + fld('h1', 'H', '1AE301') + fld('h2', 'H', 'deadBEEF')))
    for sub in 'cCsSiI':
        aux = b''
        for k, cnt in enumerate(COUNTS):
            aux += fld('%s%d' % (sub, k), 'B', _boundary_values(sub, cnt, 3 * k + cnt % 5), sub)
        R.append(('B' + sub, aux))
    fb = [b for b, _ in F_EDGES]
    aux = b''
    for k, cnt in enumerate(COUNTS):
        aux += fld('f%d' % k, 'B', (fb * (cnt // len(fb) + 1))[:cnt], 'F')
    R.append(('Bf', aux))
    R.append(('Bf_bulk', fld('fb', 'B', list(random_float_bits(20000, 5)) + fb, 'F') + fld('fe', 'f', ('bits', 0x3dcccccd))))
    R.append(('floats', b''.join(fld('e%c' % (65 + k), 'f', ('bits', b)) for k, (b, _) in enumerate(F_EDGES))))
    R.append(('every', every_type_record()[0]))
    R.append(('none', b''))
    R.append(('dup', fld('MM', 'Z', 'C+m,1;') + fld('ML', 'B', [1, 2], 'C') + fld('MM', 'Z', 'second') + fld('NM', 'i', 3)))
    return R


def dropped_records():
    """[(name, aux, n_dropped for select='*')]: the other fields of each record stay"""
    nan70 = [0x3f800000] * 70
    nan70[65] = 0x7fc00000
    return [('tab', fld('a1', 'i', 1) + fld('zt', 'Z', 'a\tb') + fld('a2', 'i', 2), 1),
            ('x1f', fld('zc', 'Z', b'ab\x1f') + fld('a2', 'Z', 'kept'), 1),
            ('x7f', fld('a1', 'C', 1) + fld('zd', 'Z', b'\x7f'), 1),
            ('A', fld('aa', 'A', 0x0a) + fld('ab', 'A', '!') + fld('ac', 'A', 0x7f), 2),
            ('H', fld('h1', 'H', 'ABC') + fld('h2', 'H', '12G4') + fld('h3', 'H', 'ab'), 2),
            ('inf', fld('f1', 'f', ('bits', 0x7f800000)) + fld('f2', 'f', 1.0) + fld('f3', 'f', ('bits', 0xff800000)) + fld('f4', 'f', ('bits', 0x7fc00001)), 3),
            ('nan65', fld('a1', 'i', 5) + fld('bf', 'B', nan70, 'F') + fld('b2', 'B', [0x3f800000] * 70, 'F'), 1)]


def malformed_aux():
    """name -> aux bytes that must fail the read"""
    return {'type': fld('a1', 'i', 1) + b'xxQ\x01\x02\x03\x04',
            'subtype': b'bbBd' + struct.pack('<I', 1) + b'\0' * 8,
            'short': fld('a1', 'i', 1) + b'xx',
            'fixed': fld('a1', 'Z', 'ok') + b'xxi\x01\x02',
            'nul': fld('a1', 'i', 1) + b'zzZ' + b'abc' * 30,
            'count': b'bbBS' + struct.pack('<I', 1000) + b'\0' * 100}


def aux_values(aux):
    """well-formed aux bytes in the decoded form of bam_codec.decode_record: (tag, 'i', decimal text), (tag, 'f', the 4 bytes), (tag, 'B', (sub-type, values)), text otherwise"""
    out, p = [], 0
    while p < len(aux):
        tg, ty = aux[p:p + 2].decode(), chr(aux[p + 2])
        p += 3
        if ty == 'A':
            out.append((tg, 'A', chr(aux[p]))); p += 1
        elif ty == 'f':
            out.append((tg, 'f', bytes(aux[p:p + 4]))); p += 4
        elif ty in _FMT:
            out.append((tg, 'i', str(struct.unpack_from('<' + _FMT[ty], aux, p)[0]))); p += _FIXED[ty]
        elif ty in 'ZH':
            e = aux.index(b'\0', p); out.append((tg, ty, aux[p:e].decode())); p = e + 1
        else:
            sub, cnt = chr(aux[p]), struct.unpack_from('<I', aux, p + 1)[0]
            out.append((tg, 'B', (sub, list(struct.unpack_from('<%d%s' % (cnt, _FMT[sub]), aux, p + 5))))); p += 5 + cnt * _FIXED[sub]
    return out


def reads_with(aux_list, seed=7, flags=(0, 16, 4)):
    """[(name, seq, qual, flag, aux)]: short reads around the given aux regions"""
    base = K.random_reads(len(aux_list), seed, 5, 300)
    return [(nm, seq, qual, flags[i % len(flags)], aux) for i, ((nm, seq, qual, _), aux) in enumerate(zip(base, aux_list))]


def ubam(reads, block=65280, level=6):
    return K.bgzf(K.bam_header('@HD\tVN:1.6\tSO:unsorted\n') + b''.join(K.bam_record(nm, seq, qual, flag, tags=aux) for nm, seq, qual, flag, aux in reads), level, block=block)


def spec_comments(reads, select):
    """([comment bytes of every kept read], fields dropped)"""
    out, nd = [], 0
    for nm, seq, qual, flag, aux in reads:
        if not seq:
            continue
        t, d = aux_text(aux, select)
        out.append(t.encode('latin-1')); nd += d
    return out, nd


# ---------------------------------------------------------------- checks run by both suites

def reader_comments(ctx, path, select, max_reads=4096, max_bases=1 << 62):
    """([comment bytes per read], stats, chunks) of lib.BamReader(tags=select); the comment offsets of every chunk are checked for consistency"""
    from vacmap_amd.lib import BamReader
    rd = BamReader(ctx, path, tags=select)
    try:
        chunks = K.read_all(rd, max_reads, max_bases)
        st = rd.stats()
    finally:
        rd.close()
    got = []
    for ch in chunks:
        co, cb = ch['comments_off'], bytes(ch['comments'])
        assert len(co) == len(ch['seqs_off']) == len(ch['names_off']) and co[0] == 0 and co[-1] == len(cb) and np.all(np.diff(co) >= 0)
        got += [cb[int(co[j]):int(co[j + 1])] for j in range(len(co) - 1)]
    return got, st, chunks


def check_against_spec(ctx, tmp_path, reads, select, sizes=(4096,), block=65280, drops=None, driver_too=True):
    """the reader's comments equal the specification's, byte for byte, at every chunk size; names, bases and qualities equal today's reader's;
    driver.read_bam(tags=) states the same rule"""
    from vacmap_amd import driver
    p = str(tmp_path / 'tags.bam')
    open(p, 'wb').write(ubam(reads, block))
    want, nd = spec_comments(reads, select)
    plain = list(driver._bam_chunks(p, sizes[0]))
    for n in sizes:
        got, st, chunks = reader_comments(ctx, p, select, n)
        assert len(got) == len(want)
        for j, (g, w) in enumerate(zip(got, want)):
            assert g == w, 'read %d: %r... != %r...' % (j, g[:80], w[:80])
        assert st['fields_dropped'] == (nd if drops is None else drops)
        if n == sizes[0]:
            for g, w in zip(chunks, plain):
                for key in ('names', 'seqs', 'quals'):
                    assert g[key + '_off'].tolist() == w[key + '_off'].tolist() and bytes(g[key]) == bytes(w[key]), key
    if driver_too:
        rows = list(driver.read_bam(p, tags=select))
        assert [(r[3] or '').encode('latin-1') for r in rows] == want
        ch = list(driver._bam_chunks(p, 7, tags=select))
        assert [bytes(c['comments'])[int(c['comments_off'][j]):int(c['comments_off'][j + 1])] for c in ch for j in range(len(c['comments_off']) - 1)] == want
    return p


def driver_inputs(tmp_path):
    """a small reference and about 20 reads as uBAM with MM, ML (hundreds of values), MN, rq:f, np:i and a colon-valued Z; some records stored
    reverse-strand. Returns (reference path, BAM path, reads as (name, seq, qual, flag, aux) in the read's own orientation of seq)"""
    import bam_codec as B
    from vacmap_amd import synth
    contigs = synth.make_reference([30000, 12000], seed=51)
    fa = tmp_path / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    n = 20
    cat, off, _ = synth.sample_reads_concat(contigs, n, mean_len=700, err=0.05, seed=52, min_len=500, max_len=1000)
    rng = np.random.default_rng(53)
    reads = []
    for i in range(n):
        seq = cat[off[i]:off[i + 1]].tobytes().decode()
        qual = B.ont_quals(len(seq), 200 + i)
        nml = 150 + 37 * i
        aux = (fld('MM', 'Z', 'C+m?,' + ','.join(str(int(x)) for x in rng.integers(0, 9, nml)) + ';') + fld('ML', 'B', [int(x) for x in rng.integers(0, 256, nml)], 'C') +
               fld('MN', 'i', len(seq)) + fld('rq', 'f', ('bits', int(random_float_bits(1, 300 + i)[0] & 0x3fffffff | 0x3f000000))) + fld('np', 'i', 3 + i) +
               fld('st', 'Z', '2026-01-02T03:04:%02d.000+00:00' % i))
        if i % 3 == 1:
            reads.append(('t%d' % i, synth.tostr(synth.revcomp(np.frombuffer(seq.encode(), np.uint8))), qual[::-1], 16, aux))
        else:
            reads.append(('t%d' % i, seq, qual, 0 if i % 3 == 0 else 4, aux))
    bam = tmp_path / 'tagged.bam'
    bam.write_bytes(ubam(reads, block=4000))
    return fa, bam, reads


def check_driver(ctx, tmp_path, monkeypatch, capsys):
    """test 7 of the suite: both readers, every line's tail, the BAM round trip, the device emitter's line, and no tags without the option"""
    import bam_codec as B
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, bam, reads = driver_inputs(tmp_path)
    common = ['-ref', str(fa), '-t', '2', '--nowriteindex', '--batch-reads', '4', '--window-batches', '2', '--inflight', '2', '-workdir', str(tmp_path / 'wd'), '-mode', 'H',
              '-read', str(bam)]

    def body(path):
        return [x for x in open(path).read().split('\n') if x and not x.startswith('@')]
    sel = ['MM', 'ML', 'MN']
    assert driver.main(common + ['-o', str(tmp_path / 'py.sam'), '--bam-tags', 'MM,ML,MN']) == 0
    assert driver.main(common + ['-o', str(tmp_path / 'nat.sam'), '--bam-tags', 'MM,ML,MN', '--bam-reader', 'native']) == 0
    a, b = body(tmp_path / 'py.sam'), body(tmp_path / 'nat.sam')
    assert a == b and len(a) >= len(reads) - 2
    want = {nm: aux_text(aux, sel)[0] for nm, _, _, _, aux in reads}
    for line in a:
        f = line.split('\t')
        assert line.endswith('\t' + want[f[0]]) and 'rq:f:' not in line and 'st:Z:' not in line, f[0]
    capsys.readouterr()
    assert driver.main(common + ['-o', str(tmp_path / 'dev.sam'), '--bam-tags', 'MM,ML,MN', '--bam-reader', 'native', '--sam-emitter', 'device']) == 0
    err = capsys.readouterr().err
    assert err.count('the host SAM emitter is used for the whole run (--bam-tags') == 1 and '--copycomments needs' not in err
    assert body(tmp_path / 'dev.sam') == a
    assert driver.main(common + ['-o', str(tmp_path / 'no.sam'), '--bam-reader', 'native']) == 0
    c = body(tmp_path / 'no.sam')
    assert len(c) == len(a) and not any('MM:Z:' in x or 'ML:B:' in x or 'MN:i:' in x for x in c)
    assert [x.split('\t')[:11] for x in c] == [x.split('\t')[:11] for x in a]
    # BAM round trip: every field but the colon-valued one, arrays with their sub-type, floats bit-equal
    assert driver.main(common + ['-o', str(tmp_path / 'rt.bam'), '--bam-tags', 'all', '--bam-reader', 'native', '--bam-writer', 'native']) == 0
    _, _, recs = B.read_bam(open(tmp_path / 'rt.bam', 'rb').read())
    by = {nm: aux for nm, _, _, _, aux in reads}
    assert len(recs) == len(a)
    for f, tags in recs:
        exp = [t for t in aux_values(by[f[0]]) if t[0] != 'st']
        got = [(tg, ty, struct.pack('<f', v) if ty == 'f' else v) for tg, ty, v in tags if tg in ('MM', 'ML', 'MN', 'rq', 'np', 'st')]
        assert got == exp, (f[0], got[:3], exp[:3])
