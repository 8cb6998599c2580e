#!/usr/bin/env python
"""Loading the reference: the host FASTA parser against the device parser (vm_index_build_fasta_device, csrc/k_fasta_in.hip).

    python tools/ref_load_bench.py --gb 3.1 --rounds 3 --baseline-lib PARENT/libvacmapx.so --out profiles/ref_fasta_reader.json

writes an hg38-shape reference (synth.hg38_like_lengths, make_reference_fast) as a 60-column FASTA, its bgzipped form (zlib level 1 members)
and a plain-gzip form (members of 64 MB without the BGZF subfield), then times Index.from_fasta on them, alternated for --rounds rounds:
`host_plain` (with --baseline-lib: that build of the library, i.e. another commit's host path; else this one's), `native_plain`,
`native_bgzf`, `native_gzip`. Every build is a child process of its own under its own time limit; it builds a small reference first (warm-up:
library load, context, first allocations) and then reports the wall seconds of the timed build and, for the native reader, its phase
seconds. A child that fails or runs out of time ends the run: nothing more is started.

    python tools/ref_load_bench.py --profile-build PATH --reader native      # one build and nothing else: the program for rocprofv3 --kernel-trace --stats
"""
import argparse, gzip, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np


def write_fasta(path, contigs, names, width=60, block=64 << 20):
    """60-column FASTA; returns the pieces' sizes summed"""
    total = 0
    with open(path, 'wb') as f:
        for name, c in zip(names, contigs):
            f.write(b'>' + name + b'\n'); total += len(name) + 2
            for a in range(0, len(c), block - block % width):
                part = c[a:a + block - block % width]
                m = len(part) // width
                out = np.empty((m, width + 1), np.uint8)
                out[:, :width] = part[:m * width].reshape(m, width); out[:, width] = 10
                out.tofile(f); total += out.size
                if m * width < len(part):
                    f.write(part[m * width:].tobytes() + b'\n'); total += len(part) - m * width + 1
    return total


def pieces_of(path, size=64 << 20):
    with open(path, 'rb') as f:
        while True:
            b = f.read(size)
            if not b:
                return
            yield b


def write_gzip_members(path, src, threads=16):
    """plain gzip: one member per 64 MB piece, deflated side by side (no BGZF subfield: a reader has to inflate it in order)"""
    from concurrent.futures import ThreadPoolExecutor
    with open(path, 'wb') as f, ThreadPoolExecutor(threads) as pool:
        batch = []
        for p in pieces_of(src):
            batch.append(p)
            if len(batch) == threads:
                for m in pool.map(lambda x: gzip.compress(x, 1), batch):
                    f.write(m)
                batch = []
        for m in pool.map(lambda x: gzip.compress(x, 1), batch):
            f.write(m)


def child_other_build(args):
    """the host path of another build of the library (one that may lack the newer entry points lib.VmxLib resolves): the C-ABI through ctypes"""
    import ctypes as C
    L = C.CDLL(args.lib)
    L.vm_ctx_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]; L.vm_ctx_destroy.argtypes = [C.c_void_p]; L.vm_index_free.argtypes = [C.c_void_p]
    L.vm_index_build_fasta.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    L.vm_index_nseq.argtypes = [C.c_void_p]; L.vm_last_error.restype = C.c_char_p
    ctx = C.c_void_p()
    assert L.vm_ctx_create(0, C.byref(ctx)) == 0, L.vm_last_error()

    def build(path):
        h = C.c_void_p()
        t0 = time.perf_counter()
        assert L.vm_index_build_fasta(ctx, path.encode(), 15, 10, C.byref(h)) == 0, L.vm_last_error()
        dt = time.perf_counter() - t0
        n = L.vm_index_nseq(h)
        L.vm_index_free(h)
        return dt, n
    if args.warm:
        build(args.warm)
    dt, n = build(args.profile_build)
    L.vm_ctx_destroy(ctx)
    print('RESULT ' + json.dumps({'wall_s': dt, 'contigs': n, 'bases': None, 'stats': None}))


def child(args):
    if args.lib:
        return child_other_build(args)
    from vacmap_amd.lib import Context, Index, VmxLib
    lib = VmxLib(args.lib) if args.lib else None
    ctx = Context(0, lib=lib) if lib else Context(0)
    kw = dict(k=15, w=10)
    if args.reader == 'native':
        kw['reader'] = 'native'
    if args.warm:
        Index.from_fasta(ctx, args.warm, **kw).close()
    t0 = time.perf_counter()
    idx = Index.from_fasta(ctx, args.profile_build, **kw)
    dt = time.perf_counter() - t0
    res = {'wall_s': dt, 'contigs': idx.nseq, 'bases': int(sum(idx.lens)), 'stats': getattr(idx, 'build_stats', None)}
    idx.close(); ctx.close()
    print('RESULT ' + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gb', type=float, default=3.1); ap.add_argument('--rounds', type=int, default=3); ap.add_argument('--tmp', default='/tmp')
    ap.add_argument('--baseline-lib', default=None); ap.add_argument('--out', default=None); ap.add_argument('--limit', type=int, default=240)
    ap.add_argument('--keep', action='store_true', help='leave the generated files in --tmp (and print their paths)')
    ap.add_argument('--profile-build', default=None); ap.add_argument('--reader', default='host'); ap.add_argument('--lib', default=None); ap.add_argument('--warm', default=None)
    args = ap.parse_args()
    if args.profile_build:
        return child(args)
    from vacmap_amd import synth
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bam_input_cases as K
    t0 = time.time()
    lens = synth.hg38_like_lengths(int(args.gb * 1e9))
    names = [b'chr%d synthetic' % (i + 1) for i in range(len(lens))]
    d = os.path.join(args.tmp, 'ref_load_bench_%d' % os.getpid())
    os.makedirs(d, exist_ok=True)
    paths = {k: os.path.join(d, n) for k, n in (('plain', 'ref.fa'), ('bgzf', 'ref.bgzf.fa.gz'), ('gzip', 'ref.gzip.fa.gz'), ('warm', 'warm.fa'), ('warm_gz', 'warm.fa.gz'))}
    text_bytes = write_fasta(paths['plain'], synth.make_reference_fast(lens, seed=5), names)
    write_fasta(paths['warm'], synth.make_reference_fast([8_000_000, 2_000_000], seed=6), [b'w1', b'w2'])
    K.write_bgzf_zlib(paths['bgzf'], pieces_of(paths['plain']), level=1)
    K.write_bgzf_zlib(paths['warm_gz'], pieces_of(paths['warm']), level=1)
    write_gzip_members(paths['gzip'], paths['plain'])
    res = {'text_bytes': text_bytes, 'bases': int(sum(lens)), 'contigs': len(lens), 'file_bytes': {k: os.path.getsize(p) for k, p in paths.items()},
           'generate_s': time.time() - t0, 'baseline_lib': args.baseline_lib, 'rounds': []}
    print('generated %.2f GB of text in %.0f s' % (text_bytes / 1e9, res['generate_s']), flush=True)
    runs = [('host_plain', 'host', 'plain', args.baseline_lib, 'warm'), ('native_plain', 'native', 'plain', None, 'warm'), ('native_bgzf', 'native', 'bgzf', None, 'warm_gz'),
            ('native_gzip', 'native', 'gzip', None, 'warm')]
    ok = True
    for r in range(args.rounds):
        rnd = {}
        for name, reader, form, lib, warm in runs:
            cmd = [sys.executable, os.path.abspath(__file__), '--profile-build', paths[form], '--reader', reader, '--warm', paths[warm]] + (['--lib', lib] if lib else [])
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
            print('round %d %s: %.2f s %s' % (r, name, rnd[name]['wall_s'], json.dumps(rnd[name]['stats'])), flush=True)
        res['rounds'].append(rnd)
        if not ok:
            break
    names_ = [x[0] for x in runs]
    res['wall_s'] = {n: [rd[n]['wall_s'] for rd in res['rounds'] if n in rd] for n in names_}
    res['spread_s'] = {n: (max(v) - min(v) if v else None) for n, v in res['wall_s'].items()}
    res['complete'] = ok
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ('wall_s', 'spread_s', 'complete')}))
    if args.keep:
        print('files: ' + json.dumps(paths))
    else:
        for p in paths.values():
            os.remove(p)
        os.rmdir(d)
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
