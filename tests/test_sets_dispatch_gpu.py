"""-m gpu: every instance of the set-level Gram-sweep family (csrc/set_rows.h), by name and by the template arguments the name hides.  For
each row of tests/_sets_dispatch.py the C entry point runs between ggan_prof_reset / ggan_prof_enable with GGAN_TRACE_SETS set: the
profiler must have seen exactly the row's kernel and the helpers the row lists, once each, with the row's grids; the trace line of the
launch -- K / NS, the loader, the width, the row and block counts, the splits, the grid -- must equal the row's `expect`; and the result
must match float64 under the gate the entry already has, unchanged:
  mix_rbf_sums   both estimators within 2e-5 max(1, |ref|) (tests/test_mmd_sets_gpu.py); 'count' rows: the closed-form pair counts, exactly
  knn_radii      |r2 - ref| <= T_i, the derived float32 Gram bound _prdc_ref.tol (tests/test_prdc_gpu.py)
  ball_counts    counts inside _prdc_ref.count_brackets, minima within T_i
  knn_lists      distances within _knn_ref.row_tol, the list as a set on closed rows, position by position on pinned rows
  parzen_lse     _parzen_ref.gate, per row and bandwidth
  kmeans_assign  _kmeans_ref: the float64 argmin on every row that is not ambiguous, distances within T_i, the inertia the fp64 sum
'lattice' rows hold integers: every distance is exact in float32, so radii, counts, minima, indices and list distances must EQUAL the
reference, ties included (parzen_lse on the lattice keeps its gate: the distances are exact, the exp / log arithmetic is not).
Inputs, outputs and the workspace sit between sentinel pads -- NaN for floats, so a load outside an operand shows in the result --, the
workspace is exactly *_workspace bytes long, outputs start as NaN / -1, and afterwards every pad and every input must keep its bits.
A row whose base offset alone selects the scalar loader must also give the BITS of the aligned call on the same values: the two loaders
deliver the same floats and nothing behind them depends on VEC.  Each row prints the instance that ran and the observed fraction of each
gate on one line that starts with SETS-ROW."""
import ctypes as C
import math
import re

import numpy as np
import pytest

import _kmeans_ref
import _parzen_ref
import _prdc_ref
import _mmd_ref
import _sets_dispatch as D
from _sets_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled

pytestmark = pytest.mark.gpu

PAD = 64                                                       # elements of sentinel on either side of every buffer
_SENT = {np.dtype(np.float32): np.nan, np.dtype(np.float64): np.nan, np.dtype(np.int32): -12345}
_LINE = re.compile(r'\[ggan\] sets (\S+) k=(\d+) vec=(\d) d=(\d+)(?: m=(\d+) T=(\d+) nb=(\d+)| nq=(\d+) nc=(\d+) c0=(\d+) nbq=(\d+) nbc=(\d+))'
                   r' S=(\d+) grid=\((\d+),(\d+)\)')


def _lines(err):
    out = []
    for m in _LINE.findall(err):
        x = dict(name=m[0], k=int(m[1]), vec=int(m[2]), d=int(m[3]), S=int(m[12]), grid=(int(m[13]), int(m[14])))
        if m[4]:
            x.update(m=int(m[4]), T=int(m[5]), nb=int(m[6]))
        else:
            x.update(nq=int(m[7]), nc=int(m[8]), c0=int(m[9]), nbq=int(m[10]), nbc=int(m[11]))
        out.append(x)
    return out


class Buf:
    """a device buffer between sentinel pads; `off` more sentinel elements in front move the base off a 16-byte boundary.  values: an
    input, read-only; else an output of n elements that starts as `fill`"""
    def __init__(self, gpu, values=None, n=0, fill=np.nan, dtype=np.float32, off=0):
        import torch
        dtype = np.dtype(dtype)
        self.out = values is None
        body = np.full(n, fill, dtype) if self.out else np.ascontiguousarray(np.ravel(values), dtype)
        self.lead, self.n, self.size = PAD + off, body.size, dtype.itemsize
        self.host = np.concatenate([np.full(self.lead, _SENT[dtype], dtype), body, np.full(PAD, _SENT[dtype], dtype)])
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        assert self.dev.data_ptr() % 256 == 0 and self.p().value % 16 == (self.size * off) % 16

    def p(self):
        return C.c_void_p(self.dev.data_ptr() + self.size * self.lead)

    def get(self, shape=None):
        a = self.dev.cpu().numpy()[self.lead:self.lead + self.n]
        return a.reshape(shape) if shape is not None else a

    def intact(self):
        now = self.dev.cpu().numpy()
        same = lambda a, b: a.tobytes() == b.tobytes()
        return same(now[:self.lead], self.host[:self.lead]) and same(now[-PAD:], self.host[-PAD:]) and (self.out or same(now, self.host))


def _host(values):
    arr = (C.c_float * len(values))(*[float(v) for v in values])
    return arr, C.cast(arr, C.c_void_p)


def _call(row, gpu, off, profiled):
    """the row's entry point through the C ABI on operands at base offsets `off` -> (outputs as numpy, profiler records or None)"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L, st = _lib.load(), F._stream()
    entry = row['entry']
    m, n, d = D.dims(row)
    A, B = D.sets(row)
    bufs = []

    def new(*a, **kw):
        bufs.append(Buf(gpu, *a, **kw))
        return bufs[-1]
    bA = new(A, off=off[0])
    bB = bA if (row['same'] or entry == 'knn_radii') else new(B, off=off[1])
    k = row['k']
    nbytes = (L.ggan_mix_rbf_sums_workspace(m, n) if entry == 'mix_rbf_sums' else L.ggan_knn_radii_workspace(m, k) if entry == 'knn_radii' else
              L.ggan_ball_counts_workspace(m, n) if entry == 'ball_counts' else L.ggan_knn_lists_workspace(m, n, k) if entry == 'knn_lists' else
              L.ggan_parzen_lse_workspace(m, n, row['ns']) if entry == 'parzen_lse' else L.ggan_kmeans_workspace(m, d, n))
    assert nbytes > 0 and nbytes % 4 == 0
    ws = new(n=nbytes // 4)                                     # exactly *_workspace bytes between its pads
    if entry == 'mix_rbf_sums':
        sig, wts = D.mmd_widths(row)
        (sg, sgp), (wt, wtp) = _host(sig), _host(wts)
        o = dict(sums=new(n=3, dtype=np.float64))
        run = lambda: L.ggan_mix_rbf_sums(bA.p(), bB.p(), m, n, d, sgp, wtp, len(sig), o['sums'].p(), ws.p(), nbytes, st)
    elif entry == 'knn_radii':
        o = dict(r2=new(n=m))
        run = lambda: L.ggan_knn_radii(bA.p(), m, d, k, o['r2'].p(), ws.p(), nbytes, st)
    elif entry == 'ball_counts':
        rad = new(D.ball_radii(row).astype(np.float32))
        o = dict(cnt=new(n=m, fill=-1, dtype=np.int32), mn=new(n=m))
        run = lambda: L.ggan_ball_counts(bA.p(), bB.p(), m, n, d, rad.p(), o['cnt'].p(), o['mn'].p(), ws.p(), nbytes, st)
    elif entry == 'knn_lists':
        o = dict(idx=new(n=m * k, fill=-1, dtype=np.int32), d2=new(n=m * k))
        run = lambda: L.ggan_knn_lists(bA.p(), bB.p(), m, n, d, k, int(row['skip']), o['idx'].p(), o['d2'].p(), ws.p(), nbytes, st)
    elif entry == 'parzen_lse':
        sg, sgp = _host(D.parzen_widths(row))
        o = dict(lse=new(n=row['ns'] * m))
        run = lambda: L.ggan_parzen_lse(bA.p(), bB.p(), m, n, d, sgp, row['ns'], o['lse'].p(), ws.p(), nbytes, st)
    else:
        o = dict(assign=new(n=m, fill=-1, dtype=np.int32), dist=new(n=m), inertia=new(n=1, dtype=np.float64),
                 moved=new(n=1, fill=-1, dtype=np.int32), status=new(n=1, fill=-1, dtype=np.int32))
        run = lambda: L.ggan_kmeans_assign(bA.p(), bB.p(), m, d, n, None, o['assign'].p(), o['dist'].p(), o['inertia'].p(), o['moved'].p(), None,
                                           o['status'].p(), ws.p(), nbytes, st)

    def checked():
        rc = run()
        assert rc == 0, (rc, L.ggan_last_error())
    if profiled:
        _, recs = _profiled(checked)
    else:
        checked()
        torch.cuda.synchronize()
        recs = None
    assert all(b.intact() for b in bufs), 'an input or a sentinel pad changed'
    shapes = dict(idx=(m, k), d2=(m, k), lse=(row['ns'], m))
    return {name: b.get(shapes.get(name)) for name, b in o.items()}, recs


def _check_dispatch(row, recs, err):
    got = {}
    for rec in recs:
        got[(rec['name'], rec['grid'])] = got.get((rec['name'], rec['grid']), 0) + rec['launches']
    x = row['expect']
    want = {(row['kernel'], x['grid'][0] * x['grid'][1] * 256): 1}
    want.update({(name, g * 256): 1 for name, g in row['also']})
    assert got == want, (sorted(got.items()), sorted(want.items()))
    lines = _lines(err)
    assert len(lines) == 1 and lines[0] == dict(x, name=row['kernel']), (lines, x)


# ---- the gates: -> {what: observed fraction of its bound}; what is exact is asserted here ------------------------------------------------
def _mmd_fractions(row, out):
    m, n, d = row['shape']
    got, ref = out['sums'], D.mmd_reference(row)
    assert got.dtype == np.float64 and np.all(np.isfinite(got))
    if row['data'] == 'count':
        assert got.tolist() == ref.tolist(), (got, ref)
        return dict(counts=0.0)
    wsum, fr = float(sum(D.mmd_widths(row)[1])), {}
    for biased in (True, False):
        if not biased and min(m, n) < 2:                         # (the unbiased estimator of a one-row set does not exist)
            continue
        v, r = _mmd_ref.from_sums(got, m, n, wsum, biased), _mmd_ref.from_sums(ref, m, n, wsum, biased)
        fr['biased' if biased else 'unbiased'] = abs(v - r) / (D.MMD_GATE * max(1.0, abs(r)))
    return fr


def _radii_fractions(row, out):
    g = out['r2'].astype(np.float64)
    assert out['r2'].dtype == np.float32 and np.all(np.isfinite(g)) and np.all(g >= 0)
    if row['data'] == 'lattice':
        A, _ = D.sets(row)
        assert np.array_equal(g, D.lattice_lists(A, A, row['k'], True)[1][:, -1])
        return dict(radii=0.0)
    r = D.knn_reference(row)
    return dict(radii=float(np.max(np.abs(g - r['dist'][:, -1]) / r['T'])))


def _ball_fractions(row, out):
    A, B = D.sets(row)
    cnt, mn, rB = out['cnt'], out['mn'].astype(np.float64), D.ball_radii(row)
    assert out['cnt'].dtype == np.int32 and np.all(np.isfinite(mn))
    if row['data'] == 'lattice':
        for r0, Db in D.lattice_blocks(A, B):
            rows = slice(r0, r0 + Db.shape[0])
            assert np.array_equal(cnt[rows], (Db <= rB[None, :]).sum(1)) and np.array_equal(mn[rows], Db.min(1)), r0
        assert np.any(cnt > 0) and np.any(cnt < B.shape[0])
        return dict(counts=0.0, minima=0.0)
    Dab, T = D.d2(row), _prdc_ref.tol(A, B)
    lo, hi, rm = _prdc_ref.count_brackets(Dab, rB, T + _prdc_ref.U * rB[None, :])
    assert np.all(lo <= cnt) and np.all(cnt <= hi), np.flatnonzero((cnt < lo) | (cnt > hi))[:8]
    assert 0 < cnt.sum() < cnt.size * B.shape[0]                 # (neither trivial end)
    return dict(minima=float(np.max(np.abs(mn - rm) / T.max(1))), open_brackets=float(np.mean(lo != hi)))


def _lists_fractions(row, out):
    A, B = D.sets(row)
    idx, d2 = out['idx'], out['d2'].astype(np.float64)
    m, k = idx.shape
    assert out['idx'].dtype == np.int32 and idx.min() >= 0 and idx.max() < B.shape[0]
    assert all(len(set(r)) == k for r in idx.tolist())
    assert not row['skip'] or not np.any(idx == np.arange(m)[:, None])
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0) and np.all(np.diff(d2, axis=1) >= 0)
    if row['data'] == 'lattice':
        ref_idx, ref_d = D.lattice_lists(A, B, k, row['skip'])
        assert np.any(ref_d[:, -1] == ref_d[:, -2])              # (ties inside the lists: the lower index decides)
        assert np.array_equal(d2, ref_d)
        assert np.array_equal(idx, ref_idx), np.flatnonzero(np.any(idx != ref_idx, axis=1))[:8]
        return dict(lists=0.0)
    r = D.knn_reference(row)
    closed = r['set_closed']
    assert np.array_equal(np.sort(idx[closed], axis=1), np.sort(r['idx'][closed], axis=1))
    assert np.array_equal(idx[r['pinned']], r['idx'][r['pinned']])
    assert closed.mean() >= 1.0 - D.OPEN_ROWS_CAP and r['pinned'].any()
    return dict(lists=float(np.max(np.abs(d2 - r['dist']) / r['T'][:, None])), open_rows=float(np.mean(~closed)))


def _parzen_fractions(row, out):
    A, B = D.sets(row)
    got = out['lse'].astype(np.float64)
    sig = D.parzen_widths(row).astype(np.float32).astype(np.float64)          # (the widths the entry point was handed)
    assert out['lse'].dtype == np.float32 and np.all(np.isfinite(got))
    if row['data'] == 'lattice':
        ref = np.concatenate([_parzen_ref.lse_from_d2(Db, sig) for _, Db in D.lattice_blocks(A, B)], axis=1)
    else:
        ref = _parzen_ref.lse_from_d2(D.d2(row), sig)
    return dict(lse=float(np.max(np.abs(got - ref) / _parzen_ref.gate(ref))))


def _assign_fractions(row, out):
    X, Cn = D.sets(row)
    Dxc, T = D.d2(row), _kmeans_ref.tol(X, Cn).max(axis=1)
    amb = _kmeans_ref.ambiguous(Dxc, T)
    a, dist = out['assign'], out['dist'].astype(np.float64)
    assert out['assign'].dtype == np.int32 and a.min() >= 0 and a.max() < Cn.shape[0]
    assert int(out['status'][0]) == 0 and int(out['moved'][0]) == X.shape[0]
    assert amb.mean() <= _kmeans_ref.AMBIGUOUS_CAP
    assert np.array_equal(a[~amb], np.argmin(Dxc, axis=1)[~amb])
    dev_sum = math.fsum(dist.tolist())
    assert abs(float(out['inertia'][0]) - dev_sum) <= 1e-12 * dev_sum
    return dict(dist=float(np.max(np.abs(dist - Dxc.min(axis=1)) / T)), ambiguous=float(amb.mean()))


_FRACTIONS = dict(mix_rbf_sums=_mmd_fractions, knn_radii=_radii_fractions, ball_counts=_ball_fractions, knn_lists=_lists_fractions,
                  parzen_lse=_parzen_fractions, kmeans_assign=_assign_fractions)
_NOT_A_GATE = ('open_brackets', 'open_rows', 'ambiguous')      # shares of rows the reference leaves undecided, printed beside the fractions


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_runs_its_instance_and_matches_float64(gpu, idx, monkeypatch, capfd):
    row = ROWS[idx]
    monkeypatch.setenv('GGAN_TRACE_SETS', '1')
    capfd.readouterr()
    out, recs = _call(row, gpu, row['off'], profiled=True)
    err = capfd.readouterr().err
    _check_dispatch(row, recs, err)                                                     # (a) the instance
    fr = _FRACTIONS[row['entry']](row, out)                                             # (b) the values
    x = row['expect']
    print('SETS-ROW %s ran %s k=%d vec=%d grid=(%d,%d) | %s' % (row_id(row), row['kernel'], x['k'], x['vec'], x['grid'][0], x['grid'][1],
                                                              ' '.join('%s=%.4f' % kv for kv in sorted(fr.items()))))
    for what, f in fr.items():
        assert what in _NOT_A_GATE or f <= 1.0, (what, f)
    if any(row['off']):                                                                 # (c) the loader changes no bit
        assert x['vec'] == 0 and row['shape'][-1] % 4 == 0
        aligned, _ = _call(row, gpu, (0,) * len(row['off']), profiled=False)
        cap = capfd.readouterr()
        print(cap.out, end='')                                                          # (the SETS-ROW line stays in the report)
        line = _lines(cap.err)
        assert len(line) == 1 and line[0]['vec'] == 1, line
        for name in out:
            assert out[name].tobytes() == aligned[name].tobytes(), name


def test_public_wrappers_choose_the_loader_by_the_width_alone(gpu, monkeypatch, capfd):
    """what production runs: on ordinary torch allocations the float4 loader for d % 4 == 0 and the scalar one otherwise, whatever was
    allocated in between; and without GGAN_TRACE_SETS nothing is printed"""
    import torch
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(11)

    def run_all(d):
        junk = torch.empty(1 + int(rng.integers(1, 50)), dtype=torch.float32, device=gpu)          # (an odd-sized neighbour)
        t = lambda rows: torch.as_tensor(rng.standard_normal((rows, d)).astype(np.float32), device=gpu)
        x, y = t(130), t(67)
        F.mix_rbf_sums(x, y, _mmd_ref.SIGMAS)
        F.mix_rbf_sums(x, x, _mmd_ref.SIGMAS)
        r = F.knn_radii(x, 3)
        F.ball_counts(y, x, r)
        F.knn_lists(y, x, 5)
        F.knn_lists(x, x, 5, skip_diag=True)
        F.parzen_lse(x, y, _parzen_ref.SIGMAS)
        F.kmeans_assign(x, y[:37].contiguous())
        torch.cuda.synchronize()
        del junk
        return ['mmd_set_sums', 'mmd_set_sums', 'knn_radii', 'ball_counts', 'knn_lists', 'knn_lists', 'parzen_lse', 'kmeans_assign']
    monkeypatch.delenv('GGAN_TRACE_SETS', raising=False)
    capfd.readouterr()
    run_all(36)
    assert '[ggan] sets' not in capfd.readouterr().err
    monkeypatch.setenv('GGAN_TRACE_SETS', '1')
    for d in (36, 33, 4, 20, 3072, 131, 1):
        names = run_all(d)
        lines = _lines(capfd.readouterr().err)
        assert [x['name'] for x in lines] == names, lines
        assert all(x['vec'] == int(d % 4 == 0) and x['d'] == d for x in lines), (d, lines)
