#!/usr/bin/env python3
"""The depth-of-coverage accumulator next to the emitters on one batch (a sibling of tools/paf_bench.py, whose batch this is).

    python tools/depth_bench.py emitter [--reads 4096] [--calls 4] [--threads 16] [--set default|eqx|both] [--window 500] [--out FILE] [--fns a,b] [--package-root DIR]
        --reads ONT-shape reads of mean 15 kb over a 20 Mb reference, records from the aligner. After a warm-up call of each, these alternate in one
        process: sam_emit_device with nothing attached, sam_emit_device with an accumulator attached, Depth.add_device alone, sam_emit on --threads
        host threads, and Depth.add on as many (the second per-record pass a host run pays). Wall seconds per call, and whether the attached, the
        stand-alone and the host accumulator hold equal counts. Under
        `rocprofv3 --kernel-trace --stats -d DIR -- python tools/depth_bench.py emitter --only device` the statistics hold k_depth_add next to the
        k_sam_* kernels of the same session.
    python tools/depth_bench.py kernels --stats DIR/.../*_kernel_stats.csv --calls N
        the k_sam_*, k_paf_* and k_depth_* rows of such statistics, total and per call (N = calls that launched the kernel).
"""
import argparse, csv, glob, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np


def emitter(args):
    if args.package_root:                                  # another build's vacmap_amd (the parent commit's, for the k_sam_* baseline)
        sys.path.insert(0, args.package_root)
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
    res = {'reads': args.reads, 'bases': int(so[-1]), 'host_threads': args.threads, 'calls': args.calls, 'window': args.window, 'sets': {}}
    has_depth = hasattr(VL, 'Depth')                      # (the same script runs against a build without the accumulator: the k_sam_* baseline)
    for tag, eqx in (('default', 0), ('eqx', 1)):
        if args.set not in ('both', tag):
            continue
        opts = VL.SamOpts(0, 1, 0, 0, 0, 0, b'1', 0, 0)
        raw = VL.align_batch_raw(ctx, idx, ctx.lib.params('H', eqx=eqx), sb, so)
        att = VL.Depth.create(idx, args.window, 0, ctx=ctx) if has_depth else None
        alone = VL.Depth.create(idx, args.window, 0, ctx=ctx) if has_depth else None
        host = VL.Depth.create(idx, args.window, 0, lib=ctx.lib) if has_depth else None

        def attached():
            ctx.attach_depth(att)
            try:
                return VL.sam_emit_device(ctx, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so)
            finally:
                ctx.attach_depth(None)
        fns = {'sam_device': lambda: VL.sam_emit_device(ctx, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so)}
        if has_depth:
            fns['sam_device_attached'] = attached
            fns['depth_device'] = lambda: alone.add_device(ctx, idx, opts, nb, no, sb, so, raw)
        if args.only != 'device':
            fns['sam_host'] = lambda: VL.sam_emit(ctx.lib, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so, nthreads=args.threads)
            if has_depth:
                fns['depth_host'] = lambda: host.add(idx, opts, nb, no, sb, so, raw, nthreads=args.threads)
        if args.fns:
            fns = {k: v for k, v in fns.items() if k in args.fns.split(',')}
        for k in fns:
            fns[k]()                                       # warm-up of each
        s = {'records': int(raw.nrec)}
        runs = {k: [] for k in fns}
        for _ in range(args.calls):
            for k in fns:
                t0 = time.time()
                out = fns[k]()
                runs[k].append(time.time() - t0)
                del out
        for k, v in runs.items():
            s[k + '_wall_s_median'] = float(np.median(v)); s[k + '_wall_s'] = v
        if has_depth and not args.fns:
            a, b = att.counts()[0], alone.counts()[0]
            s['windows'] = int(len(a)); s['counted_bases_per_call'] = int(a.sum()) // (args.calls + 1)
            s['attached_equals_alone'] = bool((a == b).all())
            if 'depth_host' in fns:
                s['device_equals_host'] = bool((a == host.counts()[0]).all())
        for d in (att, alone, host):
            if d is not None:
                d.close()
        res['sets'][tag] = s
        raw.close()
    print(json.dumps(res))
    if args.out:
        json.dump(res, open(args.out, 'w'), indent=1)
    ctx.close()


def kernels(args):
    paths = sorted(glob.glob(args.stats))
    if not paths:
        raise SystemExit('no file matches %s' % args.stats)
    per = {}
    for r in csv.DictReader(open(paths[0])):
        if r['Name'].startswith(('k_sam_', 'k_paf_', 'k_depth_')) and not r['Name'].startswith('k_sam_count_other'):
            per[r['Name'].split('(')[0]] = {'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) * 1e-6, 'avg_us': float(r['TotalDurationNs']) * 1e-3 / max(1, int(r['Calls']))}
    out = {'kernels': per, 'k_sam_total_ms': sum(v['total_ms'] for k, v in per.items() if k.startswith('k_sam_'))}
    if args.calls:
        out['k_sam_ms_per_call'] = out['k_sam_total_ms'] / args.calls
    print(json.dumps(out))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['emitter', 'kernels'])
    ap.add_argument('--reads', type=int, default=4096); ap.add_argument('--calls', type=int, default=4); ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--set', choices=['both', 'default', 'eqx'], default='both'); ap.add_argument('--only', choices=['both', 'device'], default='both')
    ap.add_argument('--window', type=int, default=500); ap.add_argument('--stats'); ap.add_argument('--out'); ap.add_argument('--package-root'); ap.add_argument('--fns', help='comma-separated: only these of sam_device, sam_device_attached, depth_device, sam_host, depth_host')
    a = ap.parse_args()
    {'emitter': emitter, 'kernels': kernels}[a.what](a)
