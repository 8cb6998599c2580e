"""driver.main releases what it opened on every way out: contexts, threads and page-locked buffers. Cases: a clean run; a failure in the emit
pool, in an aligner thread, while the header is written (before the stream exists), in the writer thread, in the reader thread; and a failure
with more windows than the reader's queue holds, so that the reader is parked on the full queue when the run fails.
Runs on the CPU emulator build of the kernels (tests/emu)."""
import threading
import time

import pytest

N_READS = 8


class Injected(RuntimeError):
    pass


@pytest.fixture(scope='module')
def ctx():
    import emu_lib
    return emu_lib.context()


@pytest.fixture(scope='module')
def inputs(tmp_path_factory, ctx):
    """a two-contig 70 kb reference and 8 reads of ~1.5 kb as plain FASTQ; the same with a sixth record that is not FASTA / FASTQ; and the
    8 reads three times under different names (24 records: twelve windows of two reads)"""
    import bam_codec as B
    from vacmap_amd import synth
    d = tmp_path_factory.mktemp('release')
    contigs = synth.make_reference([50000, 20000], seed=41)
    fa = d / 'ref.fa'
    fa.write_text(''.join('>%s\n%s\n' % (n, c.tobytes().decode()) for n, c in zip(['cA', 'cB'], contigs)))
    cat, off, _ = synth.sample_reads_concat(contigs, N_READS, mean_len=1500, err=0.05, seed=42, min_len=600, max_len=2500)
    recs = ['@q%d\n%s\n+\n%s\n' % (i, cat[off[i]:off[i + 1]].tobytes().decode(), B.ont_quals(int(off[i + 1] - off[i]), 100 + i)) for i in range(N_READS)]
    good = d / 'r.fq'; good.write_text(''.join(recs))
    bad = d / 'bad.fq'; bad.write_text(''.join(r[1:] if i == 5 else r for i, r in enumerate(recs)))
    many = d / 'many.fq'; many.write_text(''.join(r.replace('@q', '@c%dq' % c, 1) for c in range(3) for r in recs))
    return fa, good, bad, many


def _fail_on_second_call(fn):
    calls = []

    def wrapped(*a, **kw):
        calls.append(1)
        if len(calls) == 2:
            raise Injected('second call')
        return fn(*a, **kw)
    return wrapped


class _FailingFile:
    """a file object whose write raises on its second call"""

    def __init__(self, f):
        self._f, self._n = f, 0

    def write(self, data):
        self._n += 1
        if self._n == 2:
            raise Injected('second write')
        return self._f.write(data)

    def __getattr__(self, name):
        return getattr(self._f, name)


@pytest.mark.parametrize('case', ['clean', 'emit', 'align', 'header', 'writer', 'reader', 'parked'])
def test_main_releases_everything(ctx, inputs, tmp_path, monkeypatch, case):
    from vacmap_amd import driver
    import vacmap_amd.lib as VL
    monkeypatch.setattr(VL, '_default', ctx.lib)
    fa, good, bad, many = inputs
    out = tmp_path / 'x.sam'

    made = []                                            # (held here, so that none is closed by the garbage collector instead of by main)
    init = VL.Context.__init__

    def init_recorded(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(VL.Context, '__init__', init_recorded)

    pinned = {'alloc': 0, 'free': 0}
    alloc, free = ctx.lib.L.vm_pinned_alloc, ctx.lib.L.vm_pinned_free

    def alloc_counted(*a):
        p = alloc(*a)
        pinned['alloc'] += bool(p)
        return p

    def free_counted(p):
        pinned['free'] += 1
        return free(p)
    monkeypatch.setattr(ctx.lib.L, 'vm_pinned_alloc', alloc_counted)
    monkeypatch.setattr(ctx.lib.L, 'vm_pinned_free', free_counted)

    if case in ('emit', 'parked'):
        monkeypatch.setattr(VL, 'sam_emit', _fail_on_second_call(VL.sam_emit))
    elif case == 'align':
        monkeypatch.setattr(VL.ResidentReads, 'align_raw', _fail_on_second_call(VL.ResidentReads.align_raw))
    elif case == 'writer':                               # the second window's lines: the writer thread is the one that fails
        monkeypatch.setattr(VL, 'blob_write_parts', _fail_on_second_call(VL.blob_write_parts))
    elif case == 'header':                               # the second header line: the output fails before the stream exists
        monkeypatch.setattr(driver, 'open', lambda *a, **kw: _FailingFile(open(*a, **kw)) if str(a[0]) == str(out) else open(*a, **kw), raising=False)

    reads, window_batches = (many, '1') if case == 'parked' else (bad if case == 'reader' else good, '2')
    if case == 'parked':                                 # two windows in memory, two in the reader's queue, eight more behind them
        monkeypatch.setenv('VMX_DRIVER_WINDOWS', '2')
    argv = ['-ref', str(fa), '-read', str(reads), '-mode', 'H', '-t', '2', '--nowriteindex', '--batch-reads', '2',
            '--window-batches', window_batches, '--inflight', '2', '-o', str(out)]
    before = set(threading.enumerate())
    res = {}

    def run():
        try:
            res['rc'] = driver.main(argv)
        except BaseException as e:
            res['exc'] = e
    th = threading.Thread(target=run)
    th.start(); th.join(120)
    assert not th.is_alive()
    if case == 'clean':
        assert res.get('rc') == 0, res
        assert len([x for x in open(out).read().split('\n') if x and not x.startswith('@')]) == N_READS
    elif case == 'reader':
        assert isinstance(res.get('exc'), VL.VmxError) and 'not FASTA/FASTQ' in str(res['exc']), res
    else:
        assert isinstance(res.get('exc'), Injected), res
    print('contexts made %d, closed %d; pinned alloc %d, free %d' % (len(made), sum(c.h is None for c in made), pinned['alloc'], pinned['free']))
    assert made and all(c.h is None for c in made)
    if case not in ('header', 'reader'):                 # the stream had started: its contexts and page-locked buffers existed
        assert len(made) > 1 and pinned['alloc'] > 0
    t_end = time.time() + 1.0
    while set(threading.enumerate()) - before and time.time() < t_end:
        time.sleep(0.02)
    assert not set(threading.enumerate()) - before
    assert pinned['alloc'] == pinned['free']
