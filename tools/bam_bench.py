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


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['kernels', 'driver', 'sorted'])
    ap.add_argument('--gb', type=float, default=2.0); ap.add_argument('--reads', type=int, default=40960); ap.add_argument('--replicate', type=int, default=8); ap.add_argument('--ref-mb', type=float, default=100.0)
    ap.add_argument('--rounds', type=int, default=3); ap.add_argument('--t', type=int, default=16); ap.add_argument('--tmp', default='/tmp/vmx_bam_bench')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    kernels(a) if a.what == 'kernels' else driver(a, ('bam', 'sorted')) if a.what == 'sorted' else driver(a)
