#!/usr/bin/env python3
"""Native BAM output: throughput of the encoder and deflate kernels, and the driver end to end with --bam-writer native against SAM.

    python tools/bam_bench.py kernels [--gb 2] [--out profiles/bam_kernels.json]
        >= --gb GB of BAM records: SAM text of synthetic ONT-shape reads (seeded, non-constant qualities) encoded on the device, then the
        records BGZF-compressed on the device. Wall time per stage; run it under `rocprofv3 --kernel-trace --stats -- python ...` for the
        kernels' own time (k_bam_size + k_bam_encode, k_bgzf_deflate).
    python tools/bam_bench.py driver [--reads 40960] [--replicate 8] [--ref-mb 100] [--rounds 3] [--tmp DIR] [--out profiles/bam_driver.json]
        tools/driver_bench.py's input shape (one 100 Mb contig, ONT reads of mean 15 kb) with seeded qualities, the generated reads written
        --replicate times under new names; `-o out.sam` and `-o out.bam --bam-writer native` alternated in fresh processes on the full and a
        quarter-length input: marginal (steady-state) reads/s, output sizes, the writer thread's CPU seconds.
    python tools/bam_bench.py sorted [same options] [--out profiles/bam_sorted_driver.json]
        the same runs with `-o out.bam --bam-writer native` (the baseline: unsorted) and `-o out.sorted.bam --bam-writer native-sort` alternated:
        what sorting and indexing cost. Per sorted run also the wall time of the merge in close(), its GB/s of record bytes and the run files' bytes.
    python tools/bam_bench.py input [--gb 2] [--only reader] [--tmp DIR] [--out profiles/bam_input_reader.json]
        native BAM input (lib.BamReader): >= --gb GB of unaligned BAM (15 kb ONT-shape reads, tests/bam_input_cases.scale_records) written once
        as zlib level 6 members and once through the device deflate; the reader alone on both (reads/s, GB/s of file and of inflated bytes,
        the reader's own phase times), a bench.py line of the same session (what the reader must feed), driver._bam_chunks on the first
        2 000 records (the parent's reader) and one host thread of gzip.decompress on the same file. --only reader: the first part alone,
        for a run under `rocprofv3 --kernel-trace --stats`.
    python tools/bam_bench.py input --tags [--gb 2] [--tmp DIR] [--out profiles/bam_tags_reader.json]
        the same file shape with MM / ML / MN on every read (one ML value per 8 bases, zlib level 6 members), read with tags=None (the reader as
        it is without tags) and with tags='*' (the auxiliary fields turned into comment text on the device), two passes each: reads/s, the
        producer's per-step clocks and the comment bytes per read of the second passes. Run it under `rocprofv3 --kernel-trace --stats` with a
        smaller --gb for the aux kernels' own time next to k_bgzf_inflate's.
    python tools/bam_bench.py fasta-input [--gb 2] [--asm-gb 3.1] [--rounds 3] [--only hifi_line,hifi_wrapped,assembly,fastq] [--out profiles/fasta_reads_reader.json]
        FASTA reads on the device (lib.FastqReader(fasta=True)) against lib.Fastx on the same bgzipped files: 15 kb reads on one line and
        wrapped at 60, an hg38-shape assembly of 24 contigs, and the FASTQ file of fastq-input through fasta=True against fasta=False.
        Every step is a child process under --run-timeout. For the kernels' own time run it under `rocprofv3 --kernel-trace --stats` with
        --gb 0.5 --rounds 1.
    python tools/bam_bench.py input-driver [--reads 40960] [--replicate 8] [--rounds 3] [--out profiles/bam_input_driver.json]
        the driver on the same reads as plain FASTQ and as unaligned BAM with --bam-reader native, alternated in fresh processes: the
        driver's own wait_input seconds and loop time per run.
"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

HDR = '@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:100000000\n'


def quals(n, rng):
    """Phred strings with runs: smoothed noise around a drifting mean, a few dropouts (never a constant)"""
    noise = rng.normal(0, 1, n + 16)
    sm = np.convolve(noise, np.ones(16) / 4.0, mode='valid')[:n]
    q = 14 + 5 * sm + 6 * np.sin(np.arange(n) / 300.0 + rng.random() * 6)
    q[rng.random(n) < 0.01] = 3
    return (np.clip(q, 2, 50).astype(np.uint8) + 33)


def sam_unit(n_reads, seed):
    from vacmap_amd import synth
    ref = synth.make_reference([2_000_000], seed=seed)[0]
    cat, off, _ = synth.sample_reads_concat([ref], n_reads, mean_len=15000, err=0.10, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    out = []
    for i in range(n_reads):
        s = cat[off[i]:off[i + 1]]
        out.append(b'%08x-read%d\t%d\tchr1\t%d\t60\t%dM\t*\t0\t0\t%s\t%s\tNM:i:%d\tRG:Z:1\n'
                   % (int(rng.integers(0, 1 << 31)), i, 16 * (i & 1), int(rng.integers(1, 90_000_000)), len(s), s.tobytes(), quals(len(s), rng).tobytes(),
                      int(rng.integers(0, len(s) // 8))))
    return b''.join(out)


def kernels(args):
    from vacmap_amd.lib import Context, BamCodec, bgzf_compress
    ctx = Context(0)
    codec = BamCodec(ctx, HDR)
    unit = sam_unit(4000, 5)                                          # ~100 MB of SAM text
    per = max(1, (256 << 20) // len(unit))
    chunk = unit * per
    codec.encode(chunk[:1 << 20].rsplit(b'\n', 2)[0] + b'\n')       # warm-up (pools)
    t_enc = t_z = 0.0; sam_b = bam_b = z_b = 0
    while bam_b < args.gb * 1e9:
        t0 = time.time(); rec = codec.encode(chunk); t1 = time.time()
        z = bgzf_compress(ctx, rec); t2 = time.time()
        t_enc += t1 - t0; t_z += t2 - t1; sam_b += len(chunk); bam_b += len(rec); z_b += len(z)
    r = {'sam_bytes': sam_b, 'bam_bytes': bam_b, 'bgzf_bytes': z_b, 'ratio': z_b / bam_b,
         'encode_call_GBps_of_sam': sam_b / t_enc / 1e9, 'bgzf_call_GBps_of_bam': bam_b / t_z / 1e9,
         'note': 'wall time of the calls (host copies included); kernel time from rocprofv3 --kernel-trace --stats'}
    print(json.dumps(r))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(r, open(args.out, 'w'), indent=1)
    codec.close(); ctx.close()


def driver(args, kinds=('sam', 'bam')):
    """Steady-state reads/s, as tools/driver_bench.py measures it: a run's read loop includes the start-up of its contexts (several seconds
    of pool allocation whatever the input's length, and it varies from process to process), so the rate is the MARGINAL one between a full
    and a quarter-length input, (reads_full - reads_quarter) / (loop_full - loop_quarter). SAM and BAM runs alternate, each in a fresh
    process, and every output is deleted after its run."""
    import shutil
    from vacmap_amd import synth
    os.makedirs(args.tmp, exist_ok=True)
    ref = synth.make_reference([int(args.ref_mb * 1e6)], seed=1)[0]
    fa = os.path.join(args.tmp, 'ref.fa')
    with open(fa, 'wb') as f:
        f.write(b'>chr1\n'); f.write(ref.tobytes()); f.write(b'\n')
    rng = np.random.default_rng(9)
    reads = []
    for s in range(0, args.reads, 4096):
        c, o, _ = synth.sample_reads_concat([ref], min(4096, args.reads - s), mean_len=15000, err=0.10, seed=1000 + 7919 * (s // 4096))
        for i in range(len(o) - 1):
            sq = c[o[i]:o[i + 1]].tobytes()
            reads.append((sq, quals(len(sq), rng).tobytes()))
    per_copy = sum(2 * len(r[0]) + 16 for r in reads)
    rep = args.replicate
    while rep > 4 and per_copy * rep * 1.25 * 3.3 > shutil.disk_usage(args.tmp).free:     # inputs + the largest output must fit
        rep -= 1
    qrep = max(1, rep // 4)

    def write_fq(path, copies):
        with open(path, 'wb', buffering=1 << 24) as f:
            for rp in range(copies):
                for i, (sq, q) in enumerate(reads):
                    f.write(b'@r%d_%d\n' % (rp, i)); f.write(sq); f.write(b'\n+\n'); f.write(q); f.write(b'\n')
    fq, fq4 = os.path.join(args.tmp, 'reads.fq'), os.path.join(args.tmp, 'reads_quarter.fq')
    write_fq(fq, rep); write_fq(fq4, qrep)
    n_full, n_q = len(reads) * rep, len(reads) * qrep

    def run(kind, path):
        out = os.path.join(args.tmp, 'out.' + {'sorted': 'sorted.bam'}.get(kind, kind))
        extra = {'bam': ['--bam-writer', 'native'], 'sorted': ['--bam-writer', 'native-sort', '-workdir', os.path.join(args.tmp, 'wd')]}.get(kind, [])
        env = dict(os.environ, VMX_DRIVER_TIMING='1', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        t0 = time.time()
        pr = subprocess.run([sys.executable, '-m', 'vacmap_amd.driver', '-ref', fa, '-read', path, '-mode', 'H', '-o', out, '-t', str(args.t), '--nowriteindex',
                             '--force'] + extra, env=env, stderr=subprocess.PIPE, text=True)
        dt = time.time() - t0
        tm = {}
        for ln in pr.stderr.splitlines():
            if ln.startswith('vacmapx timing (s):'):
                tm = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in ln.split(':', 1)[1].split()}
        if pr.returncode != 0:
            sys.stderr.write(pr.stderr[-3000:])
            raise SystemExit('driver run failed (%s)' % kind)
        size = os.path.getsize(out)
        os.remove(out)
        res = {'wall_s': dt, 'loop_s': tm.get('loop'), 'writer_cpu_s': tm.get('writer_cpu'), 'assemble_write_s': tm.get('assemble_write'), 'bytes': size}
        if kind == 'sorted':                               # the driver's last line: "... index X.csi (merge of N runs, M MB of records: S s)"
            import re
            m = re.search(r'merge of (\d+) runs, ([0-9.]+) MB of records: ([0-9.]+) s', pr.stderr)
            res.update({'runs': int(m.group(1)), 'run_file_bytes': float(m.group(2)) * 1e6, 'merge_s': float(m.group(3)),
                        'merge_GBps_of_records': float(m.group(2)) / 1e3 / max(float(m.group(3)), 1e-9), 'index_bytes': os.path.getsize(out + '.csi')})
            os.remove(out + '.csi')
        return res

    def med(v):
        """median of the rounds that gave a figure (a quarter run's loop can come out longer than the full run's: no marginal rate then)"""
        v = [x for x in v if x is not None]
        return float(np.median(v)) if v else None

    rounds = []
    for rd in range(args.rounds):
        r = {}
        order = kinds if rd % 2 == 0 else kinds[::-1]
        for length, path in (('full', fq), ('quarter', fq4)):
            for kind in order:
                r['%s_%s' % (kind, length)] = run(kind, path)
                print(json.dumps({'round': rd, 'run': '%s_%s' % (kind, length), **r['%s_%s' % (kind, length)]}), flush=True)
        for kind in kinds:
            d = r[kind + '_full']['loop_s'] - r[kind + '_quarter']['loop_s']
            r[kind + '_marginal_reads_per_s'] = (n_full - n_q) / d if d > 0 else None
        base, new = kinds
        ratio = '%s_over_%s' % (new, base)
        r[ratio] = r[new + '_marginal_reads_per_s'] / r[base + '_marginal_reads_per_s'] if r[new + '_marginal_reads_per_s'] and r[base + '_marginal_reads_per_s'] else None
        rounds.append(r)
        print(json.dumps({'round': rd, base + '_marginal_reads_per_s': r[base + '_marginal_reads_per_s'], new + '_marginal_reads_per_s': r[new + '_marginal_reads_per_s'],
                          ratio: r[ratio]}), flush=True)
    res = {'reads_full': n_full, 'reads_quarter': n_q, 'rounds': rounds,
           base + '_marginal_reads_per_s_median': med([r[base + '_marginal_reads_per_s'] for r in rounds]),
           new + '_marginal_reads_per_s_median': med([r[new + '_marginal_reads_per_s'] for r in rounds]),
           ratio + '_per_round': [r[ratio] for r in rounds]}
    res[ratio + '_of_medians'] = (res[new + '_marginal_reads_per_s_median'] / res[base + '_marginal_reads_per_s_median']
                                  if res[new + '_marginal_reads_per_s_median'] and res[base + '_marginal_reads_per_s_median'] else None)
    if new == 'sorted':
        for k in ('merge_s', 'merge_GBps_of_records', 'run_file_bytes', 'runs'):
            res['sorted_full_%s_median' % k] = float(np.median([r['sorted_full'][k] for r in rounds]))
        res['sorted_full_loop_over_bam_full_loop_per_round'] = [r['sorted_full']['loop_s'] / r['bam_full']['loop_s'] for r in rounds]
    # the start-up share of a run varies by seconds between processes: the full runs' loops and the writer thread's busy time say more
    for kind in kinds:
        res[kind + '_full_loop_s_median'] = float(np.median([r[kind + '_full']['loop_s'] for r in rounds]))
        res[kind + '_full_writer_busy_s_median'] = float(np.median([r[kind + '_full']['assemble_write_s'] for r in rounds]))
    print(json.dumps({k: v for k, v in res.items() if k != 'rounds'}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, 'w'), indent=1)
    for pth in (fq, fq4, fa):
        os.remove(pth)


def _save(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, 'w'), indent=1)


def input_bench(args):
    import gzip, itertools
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_input_cases as K
    from vacmap_amd import driver as D
    from vacmap_amd.lib import Context, BamReader
    os.makedirs(args.tmp, exist_ok=True)
    ctx = Context(0)
    t0 = time.time()
    head, recs, _ = K.scale_records(int(args.gb * (1 << 30)))
    total = len(head) + sum(len(r) for r in recs)
    res = {'reads': len(recs), 'inflated_bytes': total, 'generate_s': time.time() - t0, 'files': {}}
    paths = {k: os.path.join(args.tmp, 'in_%s.bam' % k) for k in ('zlib6', 'device')}
    K.write_bgzf_zlib(paths['zlib6'], [head] + recs)
    K.write_bgzf_device(paths['device'], [head] + recs, ctx)
    del recs
    for kind, p in paths.items():
        runs = []
        for rep in range(3):                                            # the first pass grows the reader's pools and warms the page cache; the third hands out with one memcpy
            os.environ['VMX_BAM_IN_COPY_THREADS'] = '1' if rep == 2 else '4'
            t0 = time.time()
            rd = BamReader(ctx, p)
            n = 0
            for ch in iter(lambda: rd.read(4096), None):
                n += len(ch['seqs_off']) - 1
            dt = time.time() - t0
            st = rd.stats(); rd.close()
            runs.append({'reads': n, 'wall_s': dt, 'reads_per_s': n / dt, 'file_GBps': os.path.getsize(p) / dt / 1e9, 'inflated_GBps': total / dt / 1e9, 'phases': st})
        res['files'][kind] = {'file_bytes': os.path.getsize(p), 'first_pass': runs[0], 'second_pass': runs[1], 'one_copy_thread_pass': runs[2]}
        print(json.dumps({kind: runs[1]}), flush=True)
    if args.only != 'reader':
        z = paths['zlib6']
        t0 = time.time()
        n = sum(len(c['seqs_off']) - 1 for c in itertools.islice(D._bam_chunks(z, 100), 20))
        res['python_reader'] = {'reads': n, 'wall_s': time.time() - t0}
        res['python_reader']['reads_per_s'] = n / res['python_reader']['wall_s']
        raw = open(z, 'rb').read(64 << 20)
        cut = 0
        for off, m in K.split_members(raw):                # whole members only
            cut = off + len(m)
        t0 = time.time(); inf = gzip.decompress(raw[:cut]); dt = time.time() - t0
        res['host_zlib_one_thread'] = {'inflated_bytes': len(inf), 'wall_s': dt, 'inflated_GBps': len(inf) / dt / 1e9}
        ctx.close()
        pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(args.bench_steps), '--warmup', '1'], stdout=subprocess.PIPE, text=True, timeout=600)
        line = [ln for ln in pr.stdout.splitlines() if ln.startswith('{')]
        if pr.returncode == 0 and line:
            b = json.loads(line[-1])
            rps = b.get('reads_per_s') or (b.get('extra') or {}).get('reads_per_s') or b.get('value')
            res['bench_line'] = {'reads_per_s': rps, 'unit': b.get('unit'), 'value': b.get('value')}
            res['reader_over_bench_reads_per_s'] = res['files']['zlib6']['second_pass']['reads_per_s'] / rps if rps else None
        else:
            raise SystemExit('bench.py failed with status %d: nothing more is started' % pr.returncode)
        r2 = res['files']['zlib6']['second_pass']
        res['reader_over_python_reader'] = r2['reads_per_s'] / res['python_reader']['reads_per_s']
        res['inflate_in_host_zlib_threads'] = (total / max(r2['phases']['inflate_s'], 1e-9) / 1e9) / res['host_zlib_one_thread']['inflated_GBps']
    for p in paths.values():
        os.remove(p)
    _save(res, args.out)


def fastq_input_bench(args):
    """lib.FastqReader against lib.Fastx on the same bgzipped FASTQ and against Fastx on the plain text: args.rounds alternated rounds, each
    reader's second pass over its file timed (the first grows pools and warms the page cache) -> profiles/fastq_input_reader.json"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_input_cases as K
    import fastq_input_cases as F
    from vacmap_amd.lib import Context, FastqReader, Fastx
    os.makedirs(args.tmp, exist_ok=True)
    ctx = Context(0)
    t0 = time.time()
    pieces, _ = F.scale_text(int(args.gb * (1 << 30)))
    total = sum(len(x) for x in pieces)
    gz, plain = os.path.join(args.tmp, 'in.fastq.gz'), os.path.join(args.tmp, 'in.fastq')
    K.write_bgzf_zlib(gz, pieces)
    with open(plain, 'wb') as f:
        for x in pieces:
            f.write(x)
    res = {'reads': len(pieces), 'text_bytes': total, 'gz_bytes': os.path.getsize(gz), 'generate_s': time.time() - t0, 'rounds': []}
    del pieces

    def run(make):
        out = None
        for _ in range(2):                                  # the second pass counts
            t0 = time.time()
            rd = make()
            n = 0
            for ch in iter(lambda: rd.read(4096), None):
                n += len(ch['seqs_off']) - 1
            dt = time.time() - t0
            out = {'reads': n, 'wall_s': dt, 'reads_per_s': n / dt, 'inflated_GBps': total / dt / 1e9}
            if hasattr(rd, 'stats'):
                out['phases'] = rd.stats()
            rd.close()
        return out
    for _ in range(args.rounds):
        rnd = {'device_gz': run(lambda: FastqReader(ctx, gz)), 'host_gz': run(lambda: Fastx(gz, lib=ctx.lib)), 'host_plain': run(lambda: Fastx(plain, lib=ctx.lib))}
        rnd['device_over_host_gz'] = rnd['device_gz']['reads_per_s'] / rnd['host_gz']['reads_per_s']
        res['rounds'].append(rnd)
        print(json.dumps({k: v if isinstance(v, float) else v['reads_per_s'] for k, v in rnd.items()}), flush=True)
    res['device_faster_in_every_pair'] = all(r['device_over_host_gz'] > 1.0 for r in res['rounds'])
    res['pipeline_wants_GBps_of_text'] = 8.0
    ctx.close()
    os.remove(gz); os.remove(plain)
    _save(res, args.out)


def _hifi_pieces(n_bytes, wrapped, seed=17, pool=64):
    """FASTA text of at least n_bytes: 15 kb reads (2 ... 40 kb) on one line each, or wrapped at 60; read i is a rotation of pool read i mod pool"""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(15000, 4000, pool), 2000, 40000).astype(np.int64)
    seqs = [np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, int(n))] for n in lens]
    pieces, tot, i = [], 0, 0
    while tot < n_bytes:
        k = i % pool
        n = int(lens[k])
        s = np.roll(seqs[k], (i * 131) % n)
        if wrapped:
            m = n // 60
            body = np.empty((m, 61), np.uint8); body[:, :60] = s[:m * 60].reshape(m, 60); body[:, 60] = 10
            body = body.tobytes() + (s[m * 60:].tobytes() + b'\n' if m * 60 < n else b'')
        else:
            body = s.tobytes() + b'\n'
        pieces.append(b'>read%09d ch=%d\n' % (i, i % 512) + body)
        tot += len(pieces[-1]); i += 1
    return pieces


def _fasta_input_step(args):
    """child of fasta_input_bench: --only READER:PATH, two passes over the file, the second one reported"""
    from vacmap_amd.lib import Context, FastqReader, Fastx
    kind, path = args.only.split(':', 1)
    ctx = Context(0)
    out = None
    for _ in range(2):                                      # the second pass counts (the first grows pools and warms the page cache)
        t0 = time.time()
        rd = Fastx(path, lib=ctx.lib) if kind == 'host' else FastqReader(ctx, path, fasta=(kind == 'device_fasta'))
        n = bases = 0
        for ch in iter(lambda: rd.read(4096), None):
            n += len(ch['seqs_off']) - 1; bases += int(ch['seqs_off'][-1])
        out = {'reads': n, 'bases': bases, 'wall_s': time.time() - t0}
        if hasattr(rd, 'stats'):
            out['phases'] = rd.stats()
        rd.close()
    ctx.close()
    print('RESULT ' + json.dumps(out))


def fasta_input_bench(args):
    """lib.FastqReader(fasta=True) against lib.Fastx on the same bgzipped files -> profiles/fasta_reads_reader.json: (a) 15 kb reads as one-line
    FASTA and wrapped at 60 (--gb of text each, zlib level 6 members), (b) the hg38-shape assembly of tools/ref_load_bench.py (--asm-gb of bases,
    60 columns), (c) the FASTQ file of fastq-input through fasta=True against fasta=False: the price of the general parser. args.rounds
    alternated rounds; every step is a child process under --run-timeout that reads its file twice and reports the second pass. A child that
    fails or runs out of time ends the run: nothing more is started."""
    if args.only and ':' in args.only:
        return _fasta_input_step(args)
    sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import bam_input_cases as K
    import fastq_input_cases as F
    import ref_load_bench as RL
    from vacmap_amd import synth
    os.makedirs(args.tmp, exist_ok=True)
    t0 = time.time()
    files, text = {}, {}
    want = [w for w in ('hifi_line', 'hifi_wrapped', 'assembly', 'fastq') if not args.only or w in args.only.split(',')]
    for w in want:
        files[w] = os.path.join(args.tmp, 'fa_%s.gz' % w)
        if w == 'assembly':
            lens = synth.hg38_like_lengths(int(args.asm_gb * 1e9))
            plain = os.path.join(args.tmp, 'fa_assembly.fa')
            text[w] = RL.write_fasta(plain, synth.make_reference_fast(lens, seed=5), [b'chr%d synthetic' % (i + 1) for i in range(len(lens))])
            K.write_bgzf_zlib(files[w], RL.pieces_of(plain), level=6)
            os.remove(plain)
        else:
            pieces = F.scale_text(int(args.gb * (1 << 30)))[0] if w == 'fastq' else _hifi_pieces(int(args.gb * (1 << 30)), w == 'hifi_wrapped')
            text[w] = sum(len(x) for x in pieces)
            K.write_bgzf_zlib(files[w], pieces)
            del pieces
    res = {'text_bytes': text, 'gz_bytes': {w: os.path.getsize(p) for w, p in files.items()}, 'generate_s': time.time() - t0, 'rounds': []}
    print('generated in %.0f s' % res['generate_s'], flush=True)

    def step(kind, w):
        pr = subprocess.run([sys.executable, os.path.abspath(__file__), 'fasta-input', '--only', kind + ':' + files[w]], stdout=subprocess.PIPE, text=True, timeout=args.run_timeout)
        line = [ln for ln in pr.stdout.splitlines() if ln.startswith('RESULT ')]
        if pr.returncode != 0 or not line:
            raise SystemExit('%s on %s failed with status %d: nothing more is started' % (kind, w, pr.returncode))
        out = json.loads(line[-1][7:])
        out['text_GBps'] = text[w] / out['wall_s'] / 1e9; out['reads_per_s'] = out['reads'] / out['wall_s']
        return out
    try:
        for _ in range(args.rounds):
            rnd = {}
            for w in want:
                kinds = ('device_fasta', 'device_fastq') if w == 'fastq' else ('device_fasta', 'host')
                rnd[w] = {k: step(k, w) for k in kinds}
                a, b = rnd[w][kinds[0]], rnd[w][kinds[1]]
                assert a['reads'] == b['reads'] and a['bases'] == b['bases'], (w, a['reads'], b['reads'])
                rnd[w]['fasta_over_' + kinds[1]] = b['wall_s'] / a['wall_s']
                print(json.dumps({w: {k: round(rnd[w][k]['text_GBps'], 3) for k in kinds}}), flush=True)
            res['rounds'].append(rnd)
    finally:
        for p in files.values():
            if os.path.exists(p):
                os.remove(p)
    _save(res, args.out)


def tags_bench(args):
    """lib.BamReader on 15 kb reads that carry MM / ML / MN, with and without tags"""
    import struct
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_input_cases as K
    from vacmap_amd.lib import Context, BamReader
    os.makedirs(args.tmp, exist_ok=True)
    ctx = Context(0)
    head, recs, _ = K.scale_records(int(args.gb * (1 << 30)))
    rng = np.random.default_rng(23)
    aux_of = {}

    def tagged(rec):
        n = struct.unpack_from('<i', rec, 20)[0]
        if n not in aux_of:                                             # (64 read lengths in the pool: one aux region each)
            k = n // 8
            mm = b'MMZC+m?,' + b','.join(b'%d' % x for x in rng.integers(0, 12, k)) + b';\0'
            aux_of[n] = mm + b'MLBC' + struct.pack('<I', k) + rng.integers(0, 256, k).astype(np.uint8).tobytes() + b'MNi' + struct.pack('<i', n)
        return struct.pack('<i', len(rec) - 4 + len(aux_of[n])) + rec[4:] + aux_of[n]
    recs = [tagged(r) for r in recs]
    total = len(head) + sum(len(r) for r in recs)
    p = os.path.join(args.tmp, 'in_tags.bam')
    K.write_bgzf_zlib(p, [head] + recs)
    n_reads = len(recs)
    del recs
    res = {'reads': n_reads, 'inflated_bytes': total, 'file_bytes': os.path.getsize(p), 'legs': {}}
    for leg, tags in (('tags_none', None), ('tags_all', '*')):
        runs = []
        for rep in range(2):                                            # the first pass grows the reader's pools and warms the page cache
            t0 = time.time()
            rd = BamReader(ctx, p, tags=tags)
            n = cbytes = 0
            for ch in iter(lambda: rd.read(4096), None):
                n += len(ch['seqs_off']) - 1; cbytes += int(ch['comments_off'][-1])
            dt = time.time() - t0
            st = rd.stats(); rd.close()
            runs.append({'reads': n, 'wall_s': dt, 'reads_per_s': n / dt, 'inflated_GBps': total / dt / 1e9, 'comment_bytes_per_read': cbytes / max(n, 1), 'phases': st})
        res['legs'][leg] = {'first_pass': runs[0], 'second_pass': runs[1]}
        print(json.dumps({leg: runs[1]}), flush=True)
    a, b = res['legs']['tags_none']['second_pass'], res['legs']['tags_all']['second_pass']
    res['tags_all_over_tags_none_reads_per_s'] = b['reads_per_s'] / a['reads_per_s']
    w = max(b['phases']['windows'], 1)
    res['per_window_ms'] = {'inflate_tags_none': 1e3 * a['phases']['inflate_s'] / w, 'inflate_tags_all': 1e3 * b['phases']['inflate_s'] / w,
                            'decode_tags_none': 1e3 * a['phases']['decode_s'] / w, 'decode_tags_all': 1e3 * b['phases']['decode_s'] / w,
                            'note': 'decode_s holds sizes, scans, k_bam_in_decode and, with tags, both aux passes and their scan'}
    os.remove(p)
    ctx.close()
    _save(res, args.out)


def input_driver(args):
    """wait_input and loop seconds of the driver on FASTQ and on unaligned BAM (--bam-reader native) of the same reads, alternated"""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_input_cases as K
    from vacmap_amd import synth
    os.makedirs(args.tmp, exist_ok=True)
    ref = synth.make_reference([int(args.ref_mb * 1e6)], seed=1)[0]
    fa = os.path.join(args.tmp, 'ref.fa')
    with open(fa, 'wb') as f:
        f.write(b'>chr1\n'); f.write(ref.tobytes()); f.write(b'\n')
    rng = np.random.default_rng(9)
    reads = []
    for s in range(0, args.reads, 4096):
        c, o, _ = synth.sample_reads_concat([ref], min(4096, args.reads - s), mean_len=15000, err=0.10, seed=1000 + 7919 * (s // 4096))
        for i in range(len(o) - 1):
            sq = c[o[i]:o[i + 1]].tobytes()
            reads.append((sq, quals(len(sq), rng).tobytes()))
    fq, bam = os.path.join(args.tmp, 'reads.fq'), os.path.join(args.tmp, 'reads.bam')
    code = np.zeros(256, np.uint8); code[[65, 67, 71, 84, 78]] = [1, 2, 4, 8, 15]

    def records():
        yield K.bam_header('@HD\tVN:1.6\tSO:unsorted\n')
        import struct
        for rp in range(args.replicate):
            for i, (sq, q) in enumerate(reads):
                name = b'r%d_%d' % (rp, i)
                c = code[np.frombuffer(sq, np.uint8)]
                c = np.concatenate([c, np.zeros(len(c) & 1, np.uint8)])
                body = struct.pack('<iiBBHHHiiii', -1, -1, len(name) + 1, 0, 4680, 0, 4, len(sq), -1, -1, 0) + name + b'\0' + ((c[0::2] << 4) | c[1::2]).tobytes() + \
                    (np.frombuffer(q, np.uint8) - 33).tobytes()
                yield struct.pack('<i', len(body)) + body
    with open(fq, 'wb', buffering=1 << 24) as f:
        for rp in range(args.replicate):
            for i, (sq, q) in enumerate(reads):
                f.write(b'@r%d_%d\n' % (rp, i)); f.write(sq); f.write(b'\n+\n'); f.write(q); f.write(b'\n')
    K.write_bgzf_zlib(bam, records())
    n_reads = len(reads) * args.replicate

    def run(kind):
        out = os.path.join(args.tmp, 'out.sam')
        env = dict(os.environ, VMX_DRIVER_TIMING='1', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        cmd = [sys.executable, '-m', 'vacmap_amd.driver', '-ref', fa, '-read', fq if kind == 'fastq' else bam, '-mode', 'H', '-o', out, '-t', str(args.t), '--nowriteindex', '--force']
        pr = subprocess.run(cmd + (['--bam-reader', 'native'] if kind == 'ubam' else []), env=env, stderr=subprocess.PIPE, text=True, timeout=args.run_timeout)   # (a run that hangs or faults ends the bench: nothing more is started)
        tm = {}
        for ln in pr.stderr.splitlines():
            if ln.startswith('vacmapx timing (s):'):
                tm = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in ln.split(':', 1)[1].split()}
        if pr.returncode != 0:
            sys.stderr.write(pr.stderr[-3000:])
            raise SystemExit('driver run failed (%s)' % kind)
        lines = sum(1 for _ in open(out, 'rb'))
        os.remove(out)
        return {'wait_input_s': tm.get('wait_input'), 'loop_s': tm.get('loop'), 'sam_lines': lines}
    rounds = []
    for rd in range(args.rounds):
        r = {}
        for kind in (('fastq', 'ubam') if rd % 2 == 0 else ('ubam', 'fastq')):
            r[kind] = run(kind)
            print(json.dumps({'round': rd, 'kind': kind, **r[kind]}), flush=True)
        rounds.append(r)
    fw = [r['fastq']['wait_input_s'] for r in rounds]; uw = [r['ubam']['wait_input_s'] for r in rounds]
    res = {'reads': n_reads, 'fastq_bytes': os.path.getsize(fq), 'ubam_bytes': os.path.getsize(bam), 'rounds': rounds, 'fastq_wait_input_s': fw, 'ubam_wait_input_s': uw,
           'fastq_wait_input_spread_s': max(fw) - min(fw), 'ubam_wait_input_median_s': float(np.median(uw)), 'fastq_wait_input_median_s': float(np.median(fw)),
           'same_sam_lines': len({r[k]['sam_lines'] for r in rounds for k in r}) == 1}
    for pth in (fq, bam, fa):
        os.remove(pth)
    _save(res, args.out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernels', 'driver', 'sorted', 'input', 'input-driver', 'fastq-input', 'fasta-input'])
    ap.add_argument('--only', default=None); ap.add_argument('--tags', action='store_true'); ap.add_argument('--run-timeout', type=float, default=600.0); ap.add_argument('--bench-steps', type=int, default=12)
    ap.add_argument('--gb', type=float, default=2.0); ap.add_argument('--reads', type=int, default=40960); ap.add_argument('--replicate', type=int, default=8); ap.add_argument('--ref-mb', type=float, default=100.0)
    ap.add_argument('--rounds', type=int, default=3); ap.add_argument('--t', type=int, default=16); ap.add_argument('--tmp', default='/tmp/vmx_bam_bench')
    ap.add_argument('--out', default=None); ap.add_argument('--asm-gb', type=float, default=3.1)
    a = ap.parse_args()
    if a.what == 'input':
        tags_bench(a) if a.tags else input_bench(a)
    elif a.what == 'fastq-input':
        fastq_input_bench(a)
    elif a.what == 'fasta-input':
        fasta_input_bench(a)
    elif a.what == 'input-driver':
        input_driver(a)
    else:
        kernels(a) if a.what == 'kernels' else driver(a, ('bam', 'sorted')) if a.what == 'sorted' else driver(a)
