#!/usr/bin/env python
"""Plain gzip inflated on the device (vm_gzip_decompress, csrc/k_gzip_in.hip) against zlib on one host thread.

    python tools/gzip_input_bench.py --mb 256 --rounds 3 --out profiles/gzip_input_decompress.json

writes a FASTQ text of 15 kb reads, deflates it with zlib level 6 into one plain-gzip member per 64 MB (what `cat *.fastq.gz` gives), and
times, alternated for --rounds rounds, `host` (zlib.decompress of the whole file) and `device_<KB>` for VMX_GZ_CHUNK of 16, 32, 64 and
128 KB (lib.gzip_decompress: upload, the five kernels, the link check, download). Every round is a child process of its own under its own
time limit; it inflates a small file first (warm-up: library load, context, first allocations). A child that fails or runs out of time
ends the run: nothing more is started.

    python tools/gzip_input_bench.py --profile-file PATH      # one device inflate and nothing else: the program for rocprofv3 --kernel-trace --stats

    python tools/gzip_input_bench.py --readers --gb 2.1 --ref-gb 3.1 --rounds 3 --out profiles/gzip_input_reader.json

the readers: a FASTQ file of 15 kb reads as plain gzip (level 6, one member per 64 MB) and bgzipped, and an hg38-shape reference (tools/ref_load_bench.py's) as
plain gzip. Alternated for --rounds rounds, every measurement a process of its own after a warm-up on a small file of the same kind:
`reads_device_<KB>` FastqReader(gzip='device') at VMX_GZ_CHUNK 16 / 32 / 64 / 128 KB, `reads_host` lib.Fastx on the same plain-gzip file,
`reads_bgzf` FastqReader on the bgzipped file (the ceiling), in reads/s; `ref_device_<KB>` Index.from_fasta(reader='native', gzip='device')
and `ref_zlib` Index.from_fasta(reader='native') (zlib on a host thread) on the reference, in seconds.
"""
import argparse, json, os, subprocess, sys, time, zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np

CHUNKS_KB = (16, 32, 64, 128)


def fastq_text(n_bytes, L=15000, seed=9):
    rng = np.random.default_rng(seed)
    n = n_bytes // (2 * L + 17) + 1
    rows = np.empty((n, 2 * L + 17), np.uint8)                          # @r<10 digits> \n bases \n+\n qualities \n
    rows[:, :2] = np.frombuffer(b'@r', np.uint8)
    rows[:, 2:12] = (np.arange(n)[:, None] // 10 ** np.arange(9, -1, -1) % 10 + 48).astype(np.uint8)
    rows[:, 12] = 10; rows[:, 13 + L:16 + L] = np.frombuffer(b'\n+\n', np.uint8); rows[:, 16 + 2 * L] = 10
    for a in range(0, n, 256):
        m = min(256, n - a)
        rows[a:a + m, 13:13 + L] = np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, (m, L))]
        rows[a:a + m, 16 + L:16 + 2 * L] = (33 + np.clip(rng.normal(28, 7, (m, L)), 2, 40)).astype(np.uint8)
    return rows.tobytes()


def gzip_members(text, level=6, piece=64 << 20, threads=16):
    from concurrent.futures import ThreadPoolExecutor

    def one(p):
        co = zlib.compressobj(level, zlib.DEFLATED, 31)
        return co.compress(p) + co.flush()
    with ThreadPoolExecutor(threads) as pool:
        return b''.join(pool.map(one, [text[a:a + piece] for a in range(0, len(text), piece)]))


def child(args):
    from vacmap_amd.lib import Context, gzip_decompress
    z = open(args.profile_file, 'rb').read()
    ctx = Context(0)
    warm = gzip_members(fastq_text(4 << 20, seed=1), 1)
    gzip_decompress(ctx, warm)
    res = {}
    if args.host:
        t0 = time.perf_counter()
        d = zlib.decompressobj(31)
        n, rest = 0, z
        while rest:                                                     # member after member, as gzip.decompress does
            n += len(d.decompress(rest)); rest = d.unused_data
            d = zlib.decompressobj(31)
        res['host'] = {'wall_s': time.perf_counter() - t0, 'text_bytes': n}
    for kb in args.chunks_kb:
        os.environ['VMX_GZ_CHUNK'] = str(kb << 10)
        st = {}
        t0 = time.perf_counter()
        out = gzip_decompress(ctx, z, st)
        res['device_%d' % kb] = {'wall_s': time.perf_counter() - t0, 'text_bytes': len(out), 'stats': st}
    ctx.close()
    print('RESULT ' + json.dumps(res))


def child_reader(args):
    """one measurement of the readers: RESULT {wall_s, reads | contigs, stats}"""
    from vacmap_amd.lib import Context, FastqReader, Fastx, Index
    kind, path, warm = args.child_reader, args.path, args.warm
    if args.chunk_kb:
        os.environ['VMX_GZ_CHUNK'] = str(args.chunk_kb << 10)
    ctx = Context(0)

    def reads(p):
        rd = Fastx(p, lib=ctx.lib) if kind == 'reads_host' else FastqReader(ctx, p, gzip='device') if kind == 'reads_device' else FastqReader(ctx, p)
        n, bases = 0, 0
        t0 = time.perf_counter()
        while True:
            ch = rd.read(4096)
            if ch is None:
                break
            n += len(ch['seqs_off']) - 1; bases += int(ch['seqs_off'][-1])
        dt = time.perf_counter() - t0
        st = rd.stats() if hasattr(rd, 'stats') else None
        rd.close()
        return {'wall_s': dt, 'reads': n, 'bases': bases, 'reads_per_s': n / dt, 'stats': st}

    def ref(p):
        kw = dict(k=15, w=10, reader='native')
        if kind == 'ref_device':
            kw['gzip'] = 'device'
        t0 = time.perf_counter()
        idx = Index.from_fasta(ctx, p, **kw)
        dt = time.perf_counter() - t0
        res = {'wall_s': dt, 'contigs': idx.nseq, 'bases': int(sum(idx.lens)), 'stats': idx.build_stats}
        idx.close()
        return res
    fn = ref if kind.startswith('ref') else reads
    fn(warm)
    res = fn(path)
    ctx.close()
    print('RESULT ' + json.dumps(res))


def readers_main(args):
    sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bam_input_cases as K
    import ref_load_bench as RB
    from vacmap_amd import synth
    t0 = time.time()
    d = os.path.join(args.tmp, 'gzip_input_bench_%d' % os.getpid())
    os.makedirs(d, exist_ok=True)
    P = {k: os.path.join(d, n) for k, n in (('fq_gz', 'reads.fastq.gz'), ('fq_bgzf', 'reads.bgzf.fastq.gz'), ('fq_warm', 'warm.fastq.gz'), ('fq_warm_bgzf', 'warm.bgzf.fastq.gz'),
                                            ('fa', 'ref.fa'), ('fa_gz', 'ref.fa.gz'), ('fa_warm', 'warm.fa'), ('fa_warm_gz', 'warm.fa.gz'))}
    block = fastq_text(128 << 20)                                       # (reads repeat 128 MB apart: far outside deflate's 32 KB)
    reps = max(1, int(args.gb * 1e9) // len(block))
    n_reads = reps * (len(block) // (2 * 15000 + 17))
    open(P['fq_gz'], 'wb').write(gzip_members(block, args.level) * reps)
    K.write_bgzf_zlib(P['fq_bgzf'], (block for _ in range(reps)), level=args.level)
    warm = fastq_text(4 << 20, seed=1)
    open(P['fq_warm'], 'wb').write(gzip_members(warm, args.level)); K.write_bgzf_zlib(P['fq_warm_bgzf'], [warm], level=args.level)
    res = {'fastq_text_bytes': len(block) * reps, 'reads': n_reads, 'level': args.level, 'rounds': []}
    del block
    runs = [('reads_device_%d' % kb, 'reads_device', 'fq_gz', 'fq_warm', kb) for kb in args.chunks_kb] + [('reads_host', 'reads_host', 'fq_gz', 'fq_warm', 0), ('reads_bgzf', 'reads_bgzf', 'fq_bgzf', 'fq_warm_bgzf', 0)]
    if args.ref_gb > 0:
        lens = synth.hg38_like_lengths(int(args.ref_gb * 1e9))
        res['ref_text_bytes'] = RB.write_fasta(P['fa'], synth.make_reference_fast(lens, seed=5), [b'chr%d synthetic' % (i + 1) for i in range(len(lens))])
        RB.write_fasta(P['fa_warm'], synth.make_reference_fast([8_000_000, 2_000_000], seed=6), [b'w1', b'w2'])
        RB.write_gzip_members(P['fa_gz'], P['fa']); RB.write_gzip_members(P['fa_warm_gz'], P['fa_warm'])
        os.remove(P['fa']); os.remove(P['fa_warm'])
        runs += [('ref_device_%d' % kb, 'ref_device', 'fa_gz', 'fa_warm_gz', kb) for kb in args.chunks_kb] + [('ref_zlib', 'ref_zlib', 'fa_gz', 'fa_warm_gz', 0)]
    res['file_bytes'] = {k: os.path.getsize(p) for k, p in P.items() if os.path.exists(p)}
    res['generate_s'] = time.time() - t0
    print('generated in %.0f s: %s' % (res['generate_s'], json.dumps(res['file_bytes'])), flush=True)
    ok = True
    for r in range(args.rounds):
        rnd = {}
        for name, kind, f, w, kb in runs:
            cmd = [sys.executable, os.path.abspath(__file__), '--child-reader', kind, '--path', P[f], '--warm', P[w], '--chunk-kb', str(kb)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit)
            except subprocess.TimeoutExpired:
                print('%s: no result in %d s: stopping' % (name, args.limit), flush=True); ok = False
                break
            line = [x for x in p.stdout.decode().split('\n') if x.startswith('RESULT ')]
            if p.returncode != 0 or not line:
                print('%s: exit %d\n%s' % (name, p.returncode, p.stderr.decode()[-1500:]), flush=True); ok = False
                break
            rnd[name] = json.loads(line[0][7:])
            print('round %d %s: %.2f s%s' % (r, name, rnd[name]['wall_s'], ', %.0f reads/s' % rnd[name]['reads_per_s'] if 'reads_per_s' in rnd[name] else ''), flush=True)
        res['rounds'].append(rnd)
        if not ok:
            break
    names = [x[0] for x in runs]
    res['wall_s'] = {n: [rd[n]['wall_s'] for rd in res['rounds'] if n in rd] for n in names}
    res['reads_per_s'] = {n: [rd[n]['reads_per_s'] for rd in res['rounds'] if n in rd] for n in names if n.startswith('reads')}
    res['complete'] = ok
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ('wall_s', 'reads_per_s', 'complete')}))
    for p in P.values():
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(d)
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--readers', action='store_true'); ap.add_argument('--gb', type=float, default=2.1); ap.add_argument('--ref-gb', type=float, default=3.1)
    ap.add_argument('--child-reader', default=None); ap.add_argument('--path', default=None); ap.add_argument('--warm', default=None); ap.add_argument('--chunk-kb', type=int, default=0)
    ap.add_argument('--mb', type=int, default=256); ap.add_argument('--rounds', type=int, default=3); ap.add_argument('--tmp', default='/tmp')
    ap.add_argument('--out', default=None); ap.add_argument('--limit', type=int, default=240); ap.add_argument('--level', type=int, default=6)
    ap.add_argument('--profile-file', default=None); ap.add_argument('--host', action='store_true')
    ap.add_argument('--chunks-kb', type=lambda s: [int(x) for x in s.split(',')], default=list(CHUNKS_KB))
    args = ap.parse_args()
    if args.child_reader:
        return child_reader(args)
    if args.profile_file:
        return child(args)
    if args.readers:
        return readers_main(args)
    t0 = time.time()
    text = fastq_text(args.mb << 20)
    z = gzip_members(text, args.level)
    path = os.path.join(args.tmp, 'gzip_input_bench_%d.fastq.gz' % os.getpid())
    open(path, 'wb').write(z)
    res = {'text_bytes': len(text), 'file_bytes': len(z), 'level': args.level, 'generate_s': time.time() - t0, 'rounds': []}
    del text, z
    print('generated %.0f MB of text, %.0f MB of gzip in %.0f s' % (res['text_bytes'] / 1e6, res['file_bytes'] / 1e6, res['generate_s']), flush=True)
    ok = True
    for r in range(args.rounds):
        cmd = [sys.executable, os.path.abspath(__file__), '--profile-file', path, '--host', '--chunks-kb', ','.join(str(k) for k in args.chunks_kb)]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print('round %d: no result in %d s: stopping' % (r, args.limit), flush=True); ok = False
            break
        line = [x for x in p.stdout.decode().split('\n') if x.startswith('RESULT ')]
        if p.returncode != 0 or not line:
            print('round %d: exit %d\n%s' % (r, p.returncode, p.stderr.decode()[-1500:]), flush=True); ok = False
            break
        res['rounds'].append(json.loads(line[0][7:]))
        print('round %d: %s' % (r, json.dumps({k: round(v['wall_s'], 3) for k, v in res['rounds'][-1].items()})), flush=True)
    os.remove(path)
    names = sorted({k for rd in res['rounds'] for k in rd})
    res['wall_s'] = {n: [rd[n]['wall_s'] for rd in res['rounds'] if n in rd] for n in names}
    res['text_mb_per_s'] = {n: [res['text_bytes'] / 1e6 / w for w in v] for n, v in res['wall_s'].items()}
    res['spread_s'] = {n: (max(v) - min(v) if v else None) for n, v in res['wall_s'].items()}
    res['complete'] = ok
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ('wall_s', 'text_mb_per_s', 'spread_s', 'complete')}))
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
