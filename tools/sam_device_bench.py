#!/usr/bin/env python3
"""The device SAM emitter (vm_sam_emit_device, csrc/k_sam.hip) against the host emitter (vm_sam_emit).

    python tools/sam_device_bench.py emitter [--reads 4096] [--calls 5] [--threads 16] [--only device] [--out profiles/sam_device_emitter.json]
        one batch: --reads ONT-shape reads of mean 15 kb over a 20 Mb reference, records from the aligner, under the default options and under
        --eqx --MD. sam_emit at --threads threads and sam_emit_device alternate in one process after a warm-up call of each: wall seconds and
        process CPU seconds (resource.getrusage) per call, and the device call's upload / passes / download shares from the context's clocks.
        --only device: the device calls alone, for a run under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/sam_device_bench.py ...`.
        --comments: every read carries its uBAM tags as a comment of about 10 KB (MM:Z:, ML:B:C with one value per 8 bases, MN:i:, the shape of
        profiles/bam_tags_reader.json), copied by both emitters (k_sam_lines' comment stage on the device).
        --drop-every N: the records of every N-th read are taken out of the batch before the emitters see it (reads that emit no record line);
        --keep-unmapped: vm_sam_opts.keep_unmapped = 1, those reads stay as FLAG 4 lines (k_sam_unmapped on the device; profiles/sam_keep_unmapped.json).
    python tools/sam_device_bench.py kernels --set default|eqx_md --stats DIR/.../*_kernel_stats.csv --calls N [--out profiles/sam_device_kernels.json]
        sums the k_sam_* rows of the statistics of an `emitter --only device --set ...` run per batch (N = device calls of the run: --calls + 1
        warm-up; k_sam_count_other, part of the index build, left out), copies the rows to profiles/sam_device_kernel_stats_<set>.csv, compares
        with the target (10 % of a 15.3 ms step) and adds the set to --out.
    python tools/sam_device_bench.py driver [--reads 40960] [--replicate 8] [--ref-mb 100] [--rounds 3] [--tmp DIR] [--out profiles/sam_device_driver.json]
        tools/bam_bench.py driver's input (327 680 reads of 15 kb, 100 Mb reference) through the driver with --sam-emitter host and device,
        alternated in fresh processes: read-loop seconds, emit busy time, process CPU seconds (user + system of the child) and wait_input.
"""
import argparse, csv, glob, json, os, resource, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np


class _Records:
    """a batch's records without those of every n-th read: what sam_emit / sam_emit_device read of a RawBatch"""

    def __init__(self, VL, raw, n):
        keep = [i for i in range(raw.nrec) if raw.recs[i].read_idx % n != n - 1]
        self.recs = (VL.Record * max(len(keep), 1))(*[raw.recs[i] for i in keep])
        self.nrec, self.blob, self.status, self.whole = len(keep), raw.blob, raw.status, raw

    def close(self):
        self.whole.close()


STEP_MS, TARGET_MS = 15.3, 1.5            # the project's 4096-read step (BENCH_r06.json) and a tenth of it


def _save(res, out):
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, 'w'), indent=1)


def _cpu():
    r = resource.getrusage(resource.RUSAGE_SELF)
    return r.ru_utime + r.ru_stime


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
    cb = co = None
    if args.comments:
        coms = []
        for i in range(args.reads):
            n = int(so[i + 1] - so[i]); k = n // 8
            coms.append(b'MM:Z:C+m?,' + b','.join(b'%d' % x for x in rng.integers(0, 12, k)) + b';\tML:B:C,' + b','.join(b'%d' % x for x in rng.integers(0, 256, k)) + b'\tMN:i:%d' % n)
        cb = np.frombuffer(b''.join(coms), np.uint8); co = np.concatenate([[0], np.cumsum([len(x) for x in coms])]).astype(np.int64)
        del coms
    res = {'reads': args.reads, 'bases': int(so[-1]), 'host_threads': args.threads, 'calls': args.calls, 'comment_bytes': int(co[-1]) if co is not None else 0, 'sets': {}}
    ku = int(args.keep_unmapped)
    res.update({'keep_unmapped': ku, 'drop_every': args.drop_every})
    for tag, eqx, opts in (('default', 0, VL.SamOpts(0, 1, 0, 0, 0, 0, b'1', 0, ku)), ('eqx_md', 1, VL.SamOpts(1, 1, 0, 0, 0, 0, b'1', 0, ku))):
        if args.set not in ('both', tag):
            continue
        raw = VL.align_batch_raw(ctx, idx, ctx.lib.params('H', eqx=eqx), sb, so)
        if args.drop_every:
            raw = _Records(VL, raw, args.drop_every)
        blob_bytes = int(max((raw.recs[i].cigar_off + raw.recs[i].cigar_len for i in range(raw.nrec)), default=0))

        def host():
            return VL.sam_emit(ctx.lib, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so, comments=cb, com_off=co, nthreads=args.threads)

        def device():
            if cb is None:
                return VL.sam_emit_device(ctx, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so)
            return VL.sam_emit_device(ctx, idx, opts, nb, no, sb, so, raw, quals=qb, qual_off=so, comments=cb, com_off=co)
        d = device()                                                    # warm-up of each (pools, page-locked landing block)
        same = None
        if args.only != 'device':
            h = host()
            same = bool(h[0].tobytes() == d[0].tobytes() and h[1].tolist() == d[1].tolist() and h[2:] == d[2:])
        text_bytes = int(d[1][-1]); n_lines = int(d[2])
        del d
        runs = {'host': [], 'device': []}
        for _ in range(args.calls):
            for who, fn in (('host', host), ('device', device)):
                if who == 'host' and args.only == 'device':
                    continue
                c0, t0 = _cpu(), time.time()
                out = fn()
                r = {'wall_s': time.time() - t0, 'cpu_s': _cpu() - c0}
                if who == 'device':
                    up, ke, dn = VL.sam_emit_device_times(ctx)
                    r.update({'upload_s': up, 'passes_s': ke, 'download_s': dn})
                del out
                runs[who].append(r)
        s = {'records': int(raw.nrec), 'cigar_bytes': blob_bytes, 'text_bytes': text_bytes, 'lines': n_lines, 'identical_to_host': same}
        for who, v in runs.items():
            for k in (v[0].keys() if v else ()):
                s['%s_%s_median' % (who, k)] = float(np.median([x[k] for x in v]))
        s['runs'] = runs
        res['sets'][tag] = s
        raw.close()
    _save(res, args.out)
    ctx.close()


def kernels(args):
    paths = sorted(glob.glob(args.stats))
    if not paths:
        raise SystemExit('no file matches %s' % args.stats)
    # (k_sam_count_other belongs to the index build, not to a batch)
    rows = [r for r in csv.DictReader(open(paths[0])) if r['Name'].startswith('k_sam_') and not r['Name'].startswith('k_sam_count_other')]
    per = {}
    for r in rows:
        name = r['Name'].split('(')[0]
        per[name] = {'calls': int(r['Calls']), 'total_ms': float(r['TotalDurationNs']) * 1e-6, 'average_us': float(r['AverageNs']) * 1e-3, 'max_us': float(r['MaxNs']) * 1e-3}
    tot = sum(v['total_ms'] for v in per.values())
    one = {'device_calls': args.calls, 'kernels': per, 'k_sam_ms_per_batch': tot / args.calls, 'target_met': bool(tot / args.calls <= TARGET_MS)}
    res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else {'step_ms': STEP_MS, 'target_ms': TARGET_MS, 'sets': {},
                                                                                 'note': 'per option set: the k_sam_* time of a run of its own, divided by its device calls'}
    res['sets'][args.set] = one
    dst = os.path.join(ROOT, 'profiles', 'sam_device_kernel_stats_%s.csv' % args.set)
    with open(paths[0]) as f, open(dst, 'w') as g:
        for i, ln in enumerate(f):
            if i == 0 or (ln.startswith('"k_sam_') and not ln.startswith('"k_sam_count_other')):
                g.write(ln)
    _save(res, args.out)


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
    reads = []
    for s in range(0, args.reads, 4096):
        c, o, _ = synth.sample_reads_concat([ref], min(4096, args.reads - s), mean_len=15000, err=0.10, seed=1000 + 7919 * (s // 4096))
        for i in range(len(o) - 1):
            sq = c[o[i]:o[i + 1]].tobytes()
            reads.append((sq, bam_bench.quals(len(sq), rng).tobytes()))
    with open(fq, 'wb', buffering=1 << 24) as f:
        for rp in range(args.replicate):
            for i, (sq, q) in enumerate(reads):
                f.write(b'@r%d_%d\n' % (rp, i)); f.write(sq); f.write(b'\n+\n'); f.write(q); f.write(b'\n')
    n_reads = len(reads) * args.replicate
    del reads

    def run(kind):
        out = os.path.join(args.tmp, 'out.sam')
        env = dict(os.environ, VMX_DRIVER_TIMING='1', PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
        c0 = resource.getrusage(resource.RUSAGE_CHILDREN); t0 = time.time()
        pr = subprocess.run([sys.executable, '-m', 'vacmap_amd.driver', '-ref', fa, '-read', fq, '-mode', 'H', '-o', out, '-t', str(args.t), '--nowriteindex', '--force',
                             '--sam-emitter', kind], env=env, stderr=subprocess.PIPE, text=True)
        dt = time.time() - t0; c1 = resource.getrusage(resource.RUSAGE_CHILDREN)
        if pr.returncode != 0:
            sys.stderr.write(pr.stderr[-3000:])
            raise SystemExit('driver run failed (%s)' % kind)
        tm = {}
        for ln in pr.stderr.splitlines():
            if ln.startswith('vacmapx timing (s):'):
                tm = {kv.split('=')[0]: float(kv.split('=')[1]) for kv in ln.split(':', 1)[1].split()}
        import hashlib
        h = hashlib.sha256()
        with open(out, 'rb') as f:                                       # the lines behind the header (its @PG line holds the command line)
            head = f.read(1 << 20); at = 0
            while head[at:at + 1] == b'@':
                at = head.index(b'\n', at) + 1
            h.update(head[at:])
            for blk in iter(lambda: f.read(1 << 24), b''):
                h.update(blk)
        size = os.path.getsize(out); os.remove(out)
        return {'wall_s': dt, 'loop_s': tm.get('loop'), 'emit_busy_s': tm.get('job_emit'), 'wait_input_s': tm.get('wait_input'), 'cpu_s': (c1.ru_utime - c0.ru_utime) + (c1.ru_stime - c0.ru_stime),
                'bytes': size, 'sha256_without_pg': h.hexdigest(), 'host_fallback': 'host SAM emitter' in pr.stderr}
    rounds = []
    for rd in range(args.rounds):
        r = {}
        for kind in (('host', 'device') if rd % 2 == 0 else ('device', 'host')):
            r[kind] = run(kind)
            print(json.dumps({'round': rd, 'emitter': kind, **r[kind]}), flush=True)
        rounds.append(r)
    res = {'reads': n_reads, 't': args.t, 'rounds': rounds, 'same_output': all(r['host']['sha256_without_pg'] == r['device']['sha256_without_pg'] for r in rounds)}
    for kind in ('host', 'device'):
        for k in ('loop_s', 'emit_busy_s', 'cpu_s', 'wait_input_s'):
            res['%s_%s' % (kind, k)] = [r[kind][k] for r in rounds]
    _save(res, args.out)
    for pth in (fq, fa):
        os.remove(pth)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('what', choices=['emitter', 'kernels', 'driver'])
    ap.add_argument('--reads', type=int, default=None); ap.add_argument('--calls', type=int, default=5); ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--set', choices=['both', 'default', 'eqx_md'], default='both', help='emitter: the option set(s) to run; kernels: the set the statistics belong to')
    ap.add_argument('--comments', action='store_true', help='emitter: a 10 KB uBAM-tag comment on every read')
    ap.add_argument('--keep-unmapped', action='store_true', help='emitter: vm_sam_opts.keep_unmapped = 1')
    ap.add_argument('--drop-every', type=int, default=0, help='emitter: take the records of every N-th read out of the batch')
    ap.add_argument('--only', choices=['both', 'device'], default='both'); ap.add_argument('--stats'); ap.add_argument('--out')
    ap.add_argument('--replicate', type=int, default=8); ap.add_argument('--ref-mb', type=float, default=100); ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--tmp', default='/dev/shm/sam_device_bench'); ap.add_argument('-t', type=int, default=16)
    a = ap.parse_args()
    if a.reads is None:
        a.reads = 4096 if a.what == 'emitter' else 40960
    {'emitter': emitter, 'kernels': kernels, 'driver': driver}[a.what](a)
