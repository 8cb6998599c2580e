#!/usr/bin/env python3
"""The PAF emitters next to the SAM emitters on one batch (a sibling of tools/sam_device_bench.py, whose batch this is).

    python tools/paf_bench.py emitter [--reads 4096] [--calls 4] [--threads 16] [--set default|eqx_md|both] [--out profiles/paf_device.json]
        --reads ONT-shape reads of mean 15 kb over a 20 Mb reference, records from the aligner. After a warm-up call of each, paf_emit_device,
        sam_emit_device, paf_emit and sam_emit alternate in one process: text bytes, lines, wall seconds per call, the device calls' upload /
        passes / download shares, and whether the device's PAF bytes are the host's. Under
        `rocprofv3 --kernel-trace --stats -d DIR -- python tools/paf_bench.py emitter --only device` the statistics hold k_paf_lines next to
        k_sam_lines of the same session.
    python tools/paf_bench.py driver [--reads 40960] [--replicate 2] [--ref-mb 100] [--rounds 2] [--emitter device] [--tmp DIR] [--out FILE]
        the driver with -o out.sam and -o out.paf on one FASTQ file (reads of 15 kb over a --ref-mb reference, written --replicate times), alternated
        in fresh processes: read-loop seconds, emit busy time, wait_input and the output's bytes and lines.
    python tools/paf_bench.py kernels --stats DIR/.../*_kernel_stats.csv --calls N
        the k_sam_* and k_paf_* rows of such statistics per device call of each kind (N = calls of each kind, warm-up included).
"""
import argparse, csv, glob, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np


def emitter(args):
    import bam_bench
    from vacmap_amd import synth
    from vacmap_amd import lib as VL
    ctx = VL.Context(0)
    ref = synth.make_reference([20_000_000], seed=1)[0]
    idx = VL.Index.from_seqs(ctx, ['chr1'], [ref], k=15, w=10)
    sb, so, _ = synth.sample_reads_concat([ref], args.reads, mean_len=15000, err=0.10, seed=1000)
    so = np.ascontiguousarray(so, np.int64)
    rng = np.random.default_rng(9)
    qb = np.concatenate([bam_bench.quals(int(so[i + 1] - so[i]), rng) for i in range(args.reads)])
    names = [b'%08x-read%d' % (int(rng.integers(0, 1 << 31)), i) for i in range(args.reads)]
    nb = np.frombuffer(b''.join(names), np.uint8); no = np.concatenate([[0], np.cumsum([len(x) for x in names])]).astype(np.int64)
    res = {'reads': args.reads, 'bases': int(so[-1]), 'host_threads': args.threads, 'calls': args.calls, 'sets': {}}
    for tag, eqx, opts in (('default', 0, VL.SamOpts(0, 1, 0, 0, 0, 0, b'1', 0, 0)), ('eqx_md', 1, VL.SamOpts(1, 1, 0, 0, 0, 0, b'1', 0, 0))):
        if args.set not in ('both', tag):
            continue
        raw = VL.align_batch_raw(ctx, idx, ctx.lib.params('H', eqx=eqx), sb, so)
        fns = {'paf_device': lambda: VL.paf_emit_device(ctx, idx, opts, nb, no, sb, so, raw),
               'sam_device': lambda: VL.sam_emit_device(ctx, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so),
               'paf_host': lambda: VL.paf_emit(ctx.lib, idx, opts, nb, no, sb, so, raw, nthreads=args.threads),
               'sam_host': lambda: VL.sam_emit(ctx.lib, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so, nthreads=args.threads)}
        kinds = [k for k in fns if args.only != 'device' or k.endswith('_device')]
        first = {k: fns[k]() for k in kinds}                           # warm-up of each
        s = {'records': int(raw.nrec)}
        for k, v in first.items():
            s[k + '_text_bytes'] = int(v[1][-1]); s[k + '_lines'] = int(v[2])
        s['paf_over_sam_bytes'] = s['paf_device_text_bytes'] / max(1, s['sam_device_text_bytes'])
        if 'paf_host' in first:
            h, d = first['paf_host'], first['paf_device']
            s['paf_device_identical_to_host'] = bool(h[0].tobytes() == d[0].tobytes() and h[1].tolist() == d[1].tolist() and h[2:] == d[2:])
        del first
        runs = {k: [] for k in kinds}
        for _ in range(args.calls):
            for k in kinds:
                t0 = time.time()
                out = fns[k]()
                r = {'wall_s': time.time() - t0}
                if k.endswith('_device'):
                    up, ke, dn = VL.sam_emit_device_times(ctx)
                    r.update({'upload_s': up, 'passes_s': ke, 'download_s': dn})
                del out
                runs[k].append(r)
        for k, v in runs.items():
            for f in v[0].keys():
                s['%s_%s_median' % (k, f)] = float(np.median([x[f] for x in v]))
        s['runs'] = runs
        res['sets'][tag] = s
        raw.close()
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, 'w'), indent=1)
    ctx.close()


def driver(args):
    import bam_bench
    from vacmap_amd import synth
    os.makedirs(args.tmp, exist_ok=True)
    ref = synth.make_reference([int(args.ref_mb * 1e6)], seed=1)[0]
    fa = os.path.join(args.tmp, 'ref.fa')
    with open(fa, 'wb') as f:
        f.write(b'>chr1\n'); f.write(ref.tobytes()); f.write(b'\n')
    rng = np.random.default_rng(9)
    fq = os.path.join(args.tmp, 'reads.fq')
    n_reads = 0
    with open(fq, 'wb', buffering=1 << 24) as f:
        for s in range(0, args.reads, 4096):
            c, o, _ = synth.sample_reads_concat([ref], min(4096, args.reads - s), mean_len=15000, err=0.10, seed=1000 + 7919 * (s // 4096))
            for i in range(len(o) - 1):
                sq = c[o[i]:o[i + 1]].tobytes(); q = bam_bench.quals(len(sq), rng).tobytes()
                for rp in range(args.replicate):
                    f.write(b'@r%d_%d_%d\n' % (rp, s, i)); f.write(sq); f.write(b'\n+\n'); f.write(q); f.write(b'\n')
                    n_reads += 1

    def run(kind):
        out = os.path.join(args.tmp, 'out.' + kind)
        env = dict(os.environ, VMX_DRIVER_TIMING='1', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        t0 = time.time()
        pr = subprocess.run([sys.executable, '-m', 'vacmap_amd.driver', '-ref', fa, '-read', fq, '-mode', 'H', '-o', out, '-t', str(args.t), '--nowriteindex', '--force',
                             '--sam-emitter', args.emitter], env=env, stderr=subprocess.PIPE, text=True, timeout=args.run_timeout)
        dt = time.time() - t0
        if pr.returncode != 0:
            sys.stderr.write(pr.stderr[-3000:])
            raise SystemExit('driver run failed (%s)' % kind)
        tm = {}
        for ln in pr.stderr.splitlines():
            if ln.startswith('vacmapx timing (s):'):
                tm = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in ln.split(':', 1)[1].split()}
        size = os.path.getsize(out)
        with open(out, 'rb') as f:
            lines = sum(blk.count(b'\n') for blk in iter(lambda: f.read(1 << 24), b''))
        os.remove(out)
        return {'wall_s': dt, 'loop_s': tm.get('loop'), 'emit_busy_s': tm.get('job_emit'), 'wait_input_s': tm.get('wait_input'), 'bytes': size, 'lines': lines,
                'host_fallback': 'host SAM emitter' in pr.stderr}
    rounds = []
    for rd in range(args.rounds):
        r = {}
        for kind in (('sam', 'paf') if rd % 2 == 0 else ('paf', 'sam')):
            r[kind] = run(kind)
            print(json.dumps({'round': rd, 'output': kind, **r[kind]}), flush=True)
        rounds.append(r)
    res = {'reads': n_reads, 't': args.t, 'emitter': args.emitter, 'rounds': rounds}
    for kind in ('sam', 'paf'):
        for k in ('loop_s', 'emit_busy_s', 'wait_input_s', 'bytes'):
            res['%s_%s' % (kind, k)] = [r[kind][k] for r in rounds]
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, 'w'), indent=1)
    for pth in (fq, fa):
        os.remove(pth)


def kernels(args):
    paths = sorted(glob.glob(args.stats))
    if not paths:
        raise SystemExit('no file matches %s' % args.stats)
    per = {}
    for r in csv.DictReader(open(paths[0])):
        if r['Name'].startswith(('k_sam_', 'k_paf_')) and not r['Name'].startswith('k_sam_count_other'):
            per[r['Name'].split('(')[0]] = {'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) * 1e-6, 'ms_per_device_call': float(r['TotalDurationNs']) * 1e-6 / args.calls}
    print(json.dumps({'device_calls_of_each_kind': args.calls, 'kernels': per}))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['emitter', 'kernels', 'driver'])
    ap.add_argument('--reads', type=int, default=4096); ap.add_argument('--calls', type=int, default=4); ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--set', choices=['both', 'default', 'eqx_md'], default='default'); ap.add_argument('--only', choices=['both', 'device'], default='both')
    ap.add_argument('--stats'); ap.add_argument('--out')
    ap.add_argument('--replicate', type=int, default=2); ap.add_argument('--ref-mb', type=float, default=100); ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--emitter', choices=['host', 'device'], default='device'); ap.add_argument('--tmp', default='/dev/shm/paf_bench'); ap.add_argument('-t', type=int, default=16)
    ap.add_argument('--run-timeout', type=int, default=300)
    a = ap.parse_args()
    if a.what == 'driver' and a.reads == 4096:
        a.reads = 40960
    {'emitter': emitter, 'kernels': kernels, 'driver': driver}[a.what](a)
