"""-m gpu: the wide least-squares probe (csrc/probe_wide.hip) row by row of tests/_wprobe_ref.py, in the manner of test_probe_gpu.py.  A row's
calls -- moments, normal equations, factorisation, solve, the prediction of the fit rows and of the scoring rows -- run through the C ABI
between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly _wprobe_ref.launches(row): names (which carry the tile
edge, the panel step and the chunk), grids and counts.  Every buffer sits between sentinel pads, outputs start as NaN (integers as -1);
afterwards the inputs and the pads must keep their bits.  Each stage is checked against float64 from the values that stage itself read;
each check prints `WPROBEFRAC <row> <stage> <observed / bound>`, and a figure above 1 fails.  Then: repeatability, a NaN and a label out
of range in the input, an indefinite matrix given to the factorisation directly, functional, and the pass Evaluator.probe_scores with
PROBE_WIDE."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_ref as P  # noqa: E402
import _wprobe_ref as R  # noqa: E402
import test_prdc_gpu as M  # noqa: E402  (its small oracle-weight models and snapshots)
from test_conv_dispatch_gpu import _profiled  # noqa: E402
from test_knn_gpu import _labelled_dev  # noqa: E402

pytestmark = pytest.mark.gpu

_SENT = {np.dtype(np.float32): P.SENTINEL, np.dtype(np.float64): P.SENTINEL, np.dtype(np.int32): -12345}


class Buf:
    """a device buffer of float32 / float64 / int32 between PAD sentinels on either side; out: filled with `fill`, else it holds `values`"""
    def __init__(self, gpu, values=None, n=0, fill=np.nan, dtype=np.float32):
        import torch
        self.out = values is None
        body = np.full(n, fill, dtype) if self.out else np.ascontiguousarray(np.ravel(values), dtype)
        pad = np.full(P.PAD, _SENT[np.dtype(dtype)], dtype)
        self.host = np.concatenate([pad, body, pad])
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        self.n, self.size = body.size, body.itemsize

    def p(self):
        return C.c_void_p(self.dev.data_ptr() + self.size * P.PAD)

    def get(self, shape=None):
        a = self.dev.cpu().numpy()[P.PAD:P.PAD + self.n]
        return a.reshape(shape) if shape is not None else a

    def intact(self):
        now = self.dev.cpu().numpy()
        same = lambda a, b: a.tobytes() == b.tobytes()
        return same(now[:P.PAD], self.host[:P.PAD]) and same(now[-P.PAD:], self.host[-P.PAD:]) and (self.out or same(now, self.host))


def _wprobe(gpu, Z, y, Zq, yq, C_, profiled=True):
    """one fit and two predictions through the C ABI -> (outputs as numpy -- G as ggan_wprobe_normal left it, L as ggan_wprobe_factor left
    the same buffer --, profiler records, all buffers intact)"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L, S = _lib.load(), F._stream()
    (n, d), m = Z.shape, Zq.shape[0]
    assert 2 <= n <= 131072 and 1 <= m <= 131072 and 1 <= d <= R.MAX_DIM and 1 <= C_ <= P.MAX_CLASSES      # (bounds, before anything runs)
    assert y.shape == (n,) and yq.shape == (m,) and Zq.shape[1] == d
    bufs = []

    def new(*a, **kw):
        bufs.append(Buf(gpu, *a, **kw))
        return bufs[-1]
    bZ, by, bZq, byq = new(Z), new(y, dtype=np.int32), new(Zq), new(yq, dtype=np.int32)
    o = dict(mean=new(n=d), inv_std=new(n=d), W=new(n=d * C_), bias=new(n=C_), L=new(n=d * d, dtype=np.float64), R=new(n=d * C_, dtype=np.float64))
    oi = dict(counts=new(n=C_, fill=-1, dtype=np.int32), status=new(n=1, fill=-1, dtype=np.int32), pred_fit=new(n=n, fill=-1, dtype=np.int32),
              pred=new(n=m, fill=-1, dtype=np.int32), hit_fit=new(n=1, fill=-1, dtype=np.int32), hit=new(n=1, fill=-1, dtype=np.int32))
    nbytes = L.ggan_wprobe_moments_workspace(n, d, C_)
    assert nbytes > 0
    ws = new(n=(nbytes + 3) // 4)
    assert ws.p().value % 16 == 0 and o['L'].p().value % 8 == 0 and o['R'].p().value % 8 == 0
    keep = {}

    def ok(rc):
        assert rc == 0, (rc, L.ggan_last_error())

    def run():
        ok(L.ggan_wprobe_moments(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), oi['counts'].p(), oi['status'].p(), ws.p(), nbytes, S))
        ok(L.ggan_wprobe_normal(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), o['L'].p(), o['R'].p(), S))
        keep['G'] = o['L'].dev.clone()                      # (a copy on the stream, between the two calls: the factor is made in place)
        ok(L.ggan_wprobe_factor(o['L'].p(), d, float(P.RIDGE), oi['status'].p(), S))
        ok(L.ggan_wprobe_solve(o['L'].p(), o['R'].p(), oi['counts'].p(), n, d, C_, o['W'].p(), o['bias'].p(), oi['status'].p(), S))
        ok(L.ggan_wprobe_predict(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), o['W'].p(), o['bias'].p(), oi['pred_fit'].p(),
                                 oi['hit_fit'].p(), S))
        ok(L.ggan_wprobe_predict(bZq.p(), byq.p(), m, d, C_, o['mean'].p(), o['inv_std'].p(), o['W'].p(), o['bias'].p(), oi['pred'].p(),
                                 oi['hit'].p(), S))
    if profiled:
        _, recs = _profiled(run)
    else:
        run()
        torch.cuda.synchronize()
        recs = None
    shapes = dict(L=(d, d), R=(d, C_), W=(d, C_))
    out = {k: v.get(shapes.get(k)) for k, v in list(o.items()) + list(oi.items())}
    out['G'] = keep['G'].cpu().numpy()[P.PAD:P.PAD + d * d].reshape(d, d)
    return out, recs, all(b.intact() for b in bufs[:-1]) and bufs[-1].intact()      # (the workspace: its pads)


def _fractions(r, x, out, twin=None):
    """the stage checks of one fit + prediction -> {stage: observed fraction of its bound}; the exact stages are asserted here"""
    C_, f4 = r['C'], np.float32
    assert all(out[k].dtype == f4 for k in ('mean', 'inv_std', 'W', 'bias')) and all(out[k].dtype == np.float64 for k in ('G', 'R', 'L'))
    fr = {}
    fr.update(P.check_moments(x['Z'], x['y'], C_, out['mean'], out['inv_std'], out['counts']))
    fr.update(R.check_normal(x['Z'], x['y'], C_, out['mean'], out['inv_std'], out['G'], out['R']))
    assert np.array_equal(out['G'], out['G'].T)                                  # exactly symmetric
    up = np.triu(np.ones(out['G'].shape, bool), 1)
    assert np.array_equal(out['L'][up], out['G'][up])                            # the factorisation leaves the upper triangle alone
    fr.update(R.check_factor(out['G'], out['L']))
    fr.update(R.check_solve(out['G'], out['R'], out['L'], out['W']))
    assert np.array_equal(out['bias'], (out['counts'].astype(np.float64) / r['n']).astype(f4))
    for Z, y, pred, hit, what in ((x['Z'], x['y'], out['pred_fit'], out['hit_fit'], 'fit'), (x['Zq'], x['yq'], out['pred'], out['hit'], 'dev')):
        ref, closed, _, _ = R.margins(Z, out['mean'], out['inv_std'], out['W'], out['bias'], twin=twin)
        assert pred.min() >= 0 and pred.max() < C_
        assert np.array_equal(pred[closed], ref[closed]), np.flatnonzero(closed & (pred != ref))[:8]
        assert int(hit[0]) == int(np.sum(pred == y))
        fr['open rows ' + what] = (1.0 - closed.mean()) / P.OPEN_ROWS_CAP
        print('   %s: accuracy %.4f (float64 from the device fit: %.4f), %d rows below the margin, %d of them differ'
              % (what, np.mean(pred == y), np.mean(ref == y), int((~closed).sum()), int(np.sum(pred != ref))))
    return fr


@pytest.mark.parametrize('idx', range(len(R.ROWS)), ids=[R.row_id(r) for r in R.ROWS])
def test_row_runs_its_launch_plan_and_matches_float64(gpu, idx):
    r, x, ref = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    out, recs, intact = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'])
    got = {}
    for rec in recs:
        got[(rec['name'], rec['grid'])] = got.get((rec['name'], rec['grid']), 0) + rec['launches']
    print('launches %s' % sorted(got.items()))
    assert got == R.launches(r), (sorted(got.items()), sorted(R.launches(r).items()))
    assert intact, 'an input or a sentinel pad changed'
    assert int(out['status'][0]) == 0
    twin = r.get('tie')
    if twin:                       # the twin classes: the same weights bit for bit, and the higher one never wins
        a, b = twin
        assert out['W'][:, a].tobytes() == out['W'][:, b].tobytes() and out['bias'][a] == out['bias'][b]
        assert out['R'][:, a].tobytes() == out['R'][:, b].tobytes()
        assert not np.any(out['pred'] == b) and not np.any(out['pred_fit'] == b) and np.any(out['pred_fit'] == a)
    if 'const' in r:
        j = r['const']
        assert out['inv_std'][j] == 0 and np.all(out['W'][j] == 0) and np.all(out['G'][j] == 0) and np.all(out['G'][:, j] == 0)
    if 'absent' in r:
        c = r['absent']
        assert out['counts'][c] == 0 and np.all(out['W'][:, c] == 0) and not np.any(out['pred'] == c)
    fr = _fractions(r, x, out, twin)
    # end to end: the device's W against float64 from the raw inputs, measured by what float32 numpy makes of the same formula
    fr['W end to end'] = P.rel_w(out['W'], ref['W']) / (P.W_FACTOR * ref['w32_err'])
    for key in sorted(fr):
        print('WPROBEFRAC %s %s %.4g' % (R.row_id(r), key, fr[key]))
    print('   W: device %.3e, float32 numpy %.3e (relative to max |W|)' % (P.rel_w(out['W'], ref['W']), ref['w32_err']))
    assert all(v <= 1.0 for v in fr.values()), fr


def test_a_narrow_shape_agrees_with_the_narrow_chain(gpu):
    """d = 96 through both chains: the two W within the sum of their end-to-end bounds, and the same class on every row that is closed
    under both fits and whose margin exceeds twice the largest float64 score difference between them"""
    import torch
    from graphical_gan_amd import functional as F
    idx = [i for i, r in enumerate(R.ROWS) if r.get('narrow')][0]
    r, x, ref = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    t = lambda a: torch.as_tensor(np.array(a), device=gpu)
    Z, y, Zq = t(x['Z']), t(x['y']), t(x['Zq'])
    fits = F.lsq_probe_fit(Z, y, r['C'], float(P.RIDGE)), F.lsq_probe_fit_wide(Z, y, r['C'], float(P.RIDGE))
    preds = F.lsq_probe_predict(fits[0], Zq).cpu().numpy(), F.lsq_probe_predict_wide(fits[1], Zq).cpu().numpy()
    n_, w_ = ({k: getattr(f, k).cpu().numpy() for k in f._fields} for f in fits)
    assert int(n_['status'][0]) == 0 == int(w_['status'][0]) and np.array_equal(n_['counts'], w_['counts']) and np.array_equal(n_['bias'], w_['bias'])
    frac = np.max(np.abs(n_['W'].astype(np.float64) - w_['W'])) / (2 * P.W_FACTOR * ref['w32_err'] * np.max(np.abs(ref['W'])))
    print('WPROBEFRAC %s wide W against narrow W %.4g' % (R.row_id(r), frac))
    assert frac <= 1.0
    _, closed_n, sc_n = P.margins(x['Zq'], n_['mean'], n_['inv_std'], n_['W'], n_['bias'])
    _, closed_w, sc_w, margin = R.margins(x['Zq'], w_['mean'], w_['inv_std'], w_['W'], w_['bias'])
    both = closed_n & closed_w & (margin > 2 * np.max(np.abs(sc_n - sc_w), axis=1))
    print('   %d of %d rows closed under both fits' % (both.sum(), len(both)))
    assert both.mean() >= 1.0 - P.OPEN_ROWS_CAP and np.array_equal(preds[0][both], preds[1][both])
    # at one chunk the wide prediction IS the narrow kernel's arithmetic: the same record gives the same classes on every row
    assert np.array_equal(F.lsq_probe_predict(fits[1], Zq).cpu().numpy(), preds[1])


def test_a_second_call_gives_the_same_bits(gpu):
    import torch
    idx = 3
    r, x = R.ROWS[idx], R.inputs(idx)
    a, _, _ = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    junk = torch.full((1 << 18,), 3.0, device=gpu)               # (another allocation pattern in between)
    b, _, _ = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    del junk
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_nan_row_raises_the_status_word_and_nothing_else_breaks(gpu):
    idx = 0
    r, x = R.ROWS[idx], R.inputs(idx)
    Z = np.array(x['Z'])
    Z[5, 3] = np.nan
    out, _, intact = _wprobe(gpu, Z, x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    assert intact
    assert int(out['status'][0]) & P.NONFINITE and not int(out['status'][0]) & P.BAD_LABEL
    assert np.all(np.isnan(out['W']))                            # said aloud, not a half-right W
    assert np.array_equal(out['counts'], np.bincount(x['y'], minlength=r['C'])) and np.all(np.isfinite(out['bias']))
    cols = np.arange(r['d']) != 3
    mu, s, _ = P.moments(x['Z'], x['y'], r['C'])
    assert np.allclose(out['mean'][cols], mu[cols], rtol=1e-6) and np.allclose(out['inv_std'][cols], s[cols], rtol=1e-6)      # the other columns
    assert out['pred'].min() >= 0 and out['pred'].max() < r['C'] and out['pred_fit'].min() >= 0 and out['pred_fit'].max() < r['C']
    assert int(out['hit'][0]) == int(np.sum(out['pred'] == x['yq']))
    # ... and the next, clean call on the same device is clean
    again, _, _ = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    assert int(again['status'][0]) == 0 and np.all(np.isfinite(again['W']))


def test_a_label_out_of_range_is_flagged_and_counted_nowhere(gpu):
    idx = 0
    r, x = R.ROWS[idx], R.inputs(idx)
    y = np.array(x['y'])
    y[7], y[9], y[270] = r['C'], -1, 1 << 30
    out, _, intact = _wprobe(gpu, x['Z'], y, x['Zq'], x['yq'], r['C'], profiled=False)
    assert intact and int(out['status'][0]) == P.BAD_LABEL
    good = (y >= 0) & (y < r['C'])
    assert np.array_equal(out['counts'], np.bincount(y[good], minlength=r['C'])) and out['counts'].sum() == r['n'] - 3
    assert np.all(np.isfinite(out['W'])) and np.all(np.isfinite(out['G'])) and np.all(np.isfinite(out['R']))
    Zs, Y = P.standardise(x['Z'], out['mean'], out['inv_std']), np.zeros((r['n'], r['C']))
    Y[good, y[good]] = 1.0
    err, bound = np.abs(out['R'] - Zs.T @ Y / r['n']), P.gamma(P.ROW_BLOCK) * (np.abs(Zs).T @ Y) / r['n']
    print('WPROBEFRAC bad-label R %.4g' % np.max(err / bound))
    assert np.all(err <= bound)                                  # R holds the rows with a label in range, and only those


@pytest.mark.parametrize('where', [10, 150], ids=['panel0', 'panel2'])
def test_an_indefinite_matrix_is_a_status_bit_not_a_half_right_factor(gpu, where):
    """ggan_wprobe_factor on a symmetric matrix that is not positive definite (entry [where, where] pushed far below zero: the pivot of that
    column cannot be positive), directly: BAD_PIVOT, the chain ends normally with W all NaN, and the next clean call is clean"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L, S = _lib.load(), F._stream()
    d, C_, n = 200, 4, 1000
    rng = np.random.default_rng(77)
    A = rng.normal(size=(d, 300))
    A = A @ A.T / 300.0
    A[where, where] = -50.0
    bufs = [Buf(gpu, A, dtype=np.float64), Buf(gpu, rng.normal(size=(d, C_)), dtype=np.float64), Buf(gpu, np.full(C_, n // C_), dtype=np.int32),
            Buf(gpu, np.zeros(1), dtype=np.int32), Buf(gpu, n=d * C_), Buf(gpu, n=C_)]
    bA, bR, bc, bs, bW, bb = bufs
    bs.out = True                                                # (the status word is an output here, starting at 0)
    assert L.ggan_wprobe_factor(bA.p(), d, float(P.RIDGE), bs.p(), S) == 0
    assert L.ggan_wprobe_solve(bA.p(), bR.p(), bc.p(), n, d, C_, bW.p(), bb.p(), bs.p(), S) == 0
    torch.cuda.synchronize()
    assert int(bs.get()[0]) == P.BAD_PIVOT and np.all(np.isnan(bW.get())) and np.all(bb.get() == 0.25)
    bA.out = True                                                # (factored in place)
    assert all(b.intact() for b in bufs)
    if where >= R.NB:                                            # the panels before the bad one are a right factor of their block
        k = (where // R.NB) * R.NB
        fr = R.check_factor(A[:k, :k], bA.get((d, d))[:k, :k])
        print('WPROBEFRAC indefinite-%d leading factor %.4g' % (where, fr['factor']))
        assert fr['factor'] <= 1.0
    r, x = R.ROWS[0], R.inputs(0)
    again, _, _ = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    assert int(again['status'][0]) == 0 and np.all(np.isfinite(again['W']))


def test_functional_is_the_same_chain(gpu):
    """lsq_probe_fit_wide / lsq_probe_predict_wide give the bits of the C calls, as device tensors, and refuse a gradient"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    idx = 0
    r, x = R.ROWS[idx], R.inputs(idx)
    out, _, _ = _wprobe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    t = lambda a: torch.as_tensor(np.array(a), device=gpu)
    Z, y, Zq, yq = t(x['Z']), t(x['y']), t(x['Zq']), t(x['yq'])
    fit = F.lsq_probe_fit_wide(Z, y, r['C'], float(P.RIDGE))
    assert isinstance(fit, F.ProbeFit) and all(v.is_cuda for v in fit)
    for k in ('mean', 'inv_std', 'W', 'bias', 'counts', 'status'):
        assert getattr(fit, k).cpu().numpy().tobytes() == out[k].tobytes(), k
    correct, pred = F.lsq_probe_predict_wide(fit, Zq, yq, return_pred=True)
    assert correct.dtype == pred.dtype == torch.int32 and tuple(correct.shape) == (1,)
    assert np.array_equal(pred.cpu().numpy(), out['pred']) and int(correct.item()) == int(out['hit'][0])
    assert torch.equal(F.lsq_probe_predict_wide(fit, Zq), pred) and torch.equal(F.lsq_probe_predict_wide(fit, Zq, yq), correct)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.lsq_probe_fit_wide(Z.clone().requires_grad_(), y, r['C'], 0.01)
    with pytest.raises(ValueError, match='int32'):
        F.lsq_probe_fit_wide(Z, y.cpu(), r['C'], 0.01)           # a device mismatch
    with pytest.raises(ValueError, match='columns'):
        F.lsq_probe_fit(Z, y, r['C'], 0.01)                      # the narrow pair still stops at 128


# ---- the pass ----------------------------------------------------------------------------------------------------------------------------------
def _bracket(fit, fit_z, fit_y, dev_z, dev_y, classes):
    """the device's record against the float64 fit of the pass's own device rows (moments to 4 u, W end to end), then the float64 argmax
    from the record -> [(lowest, highest accuracy the margin rule allows) for dev, for fit]"""
    dev_ = {k: getattr(fit, k).cpu().numpy() for k in fit._fields}
    f = P.fit(fit_z, fit_y, classes)
    fr = P.check_moments(fit_z, fit_y, classes, dev_['mean'], dev_['inv_std'], dev_['counts'])
    fr['W end to end'] = P.rel_w(dev_['W'], f['W']) / (P.W_FACTOR * P.rel_w(P.fit32(fit_z, fit_y, classes), f['W']))
    print('   pass fit', {k: round(v, 4) for k, v in fr.items()})
    assert all(v <= 1.0 for v in fr.values()), fr
    res = []
    for Z, y in ((dev_z, dev_y), (fit_z, fit_y)):
        pred, closed, _, _ = R.margins(Z, dev_['mean'], dev_['inv_std'], dev_['W'], dev_['bias'])
        hits = pred == y
        res.append((np.sum(hits & closed) / float(len(y)), (np.sum(hits & closed) + np.sum(~closed)) / float(len(y))))
    return res


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_the_wide_pass_adds_four_rows_and_moves_nothing_else(gpu, dataset, K, mode, capsys, monkeypatch):
    import torch
    from graphical_gan_amd import evaluate, functional as F
    from graphical_gan_amd.evaluate import Evaluator
    KEYS = list(evaluate.PROBE_KEYS + evaluate.PROBE_WIDE_KEYS)
    B, n = 8, 12
    tr = M._model(gpu, dataset, B, K, mode)
    both = _labelled_dev(dataset, B, 3 * n)
    fit, dev = both[:2 * n], both[2 * n:]
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before = M._snapshot(tr.feed), np.random.get_state()[1].tobytes()
    plain, plain_got = Evaluator(tr, S).probe_scores(fit, dev, return_fit=True)
    ev = Evaluator(tr, dict(S, PROBE_WIDE=True))
    shared = M._snapshot(ev.feed)['rng_state']
    res, got = ev.probe_scores(fit, dev, return_fit=True)
    assert list(res) == KEYS and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    assert list(Evaluator(tr, S).probe_scores(fit, dev, wide=True)) == KEYS                       # the keyword is the setting
    assert (M._snapshot(tr.feed), np.random.get_state()[1].tobytes()) == before and M._snapshot(ev.feed)['rng_state'] == shared
    # the three values of today, and everything they were made from, keep their bits
    assert [res[k] for k in KEYS[:3]] == [plain[k] for k in KEYS[:3]] and list(plain) == KEYS[:3]
    for k, v in plain_got.items():
        for a, b in zip(v if isinstance(v, tuple) else [v], got[k] if isinstance(v, tuple) else [got[k]]):
            assert torch.equal(a, b), k
    c = tr.cfg
    rows_fit, rows_dev = 2 * n * B, n * B
    assert tuple(got['fit_x_rows'].shape) == (rows_fit, c.output_dim) and tuple(got['dev_x'].shape) == (rows_dev, c.output_dim)
    assert tuple(got['fit_h_rows'].shape) == (rows_fit, c.flat) and tuple(got['dev_h'].shape) == (rows_dev, c.flat)
    assert int(got['fit_x'].status.item()) == 0 == int(got['fit_h'].status.item())
    # x and h are what an independent Extractor forward on the same noise gives: the probe's own noise state, minibatch by minibatch
    ind = Evaluator(tr, S)
    with ind._guard():
        ind.feed['rng_state'] = F.noise_state(ind.device, int(S.get('SEED', 0)) + evaluate.EVAL_SEED + evaluate.PROBE_SEED)
        X, _ = ind._stage(fit[:2 * n], want_labels=True)
        for i in range(2 * n):
            at = slice(i * B, (i + 1) * B)
            tr.model.set_batch(ind.feed, X[i])
            tr.model.sample_noise(ind.feed)
            real_x = tr.model.real_x(ind.feed)
            q, h = tr.model.Extractor(real_x, eps=ind.feed['q_eps'], return_top=True) if c.agg else tr.model.Extractor(real_x, return_top=True)
            assert torch.equal(h, got['fit_h_rows'][at]) and torch.equal(real_x.float().reshape(B, -1), got['fit_x_rows'][at]), i
            assert torch.equal(q[0] if isinstance(q, tuple) else q, got['fit_z'][at]), i
    assert M._snapshot(tr.feed) == before[0]
    # the values: inside what the float64 argmax from the device's record allows (h; x where a float64 fit of its width is quick)
    host = {k: v.cpu().numpy() for k, v in got.items() if torch.is_tensor(v)}
    for (key_dev, key_fit), rec, zf, zd in ((KEYS[3:5], 'fit_x', 'fit_x_rows', 'dev_x'), (KEYS[5:7], 'fit_h', 'fit_h_rows', 'dev_h')):
        if host[zf].shape[1] > 1024:
            continue
        (lo_d, hi_d), (lo_f, hi_f) = _bracket(got[rec], host[zf], host['fit_y'], host[zd], host['dev_y'], 4)
        print(dataset, key_dev, res[key_dev], (lo_d, hi_d), key_fit, res[key_fit], (lo_f, hi_f))
        assert lo_d - 1e-12 <= res[key_dev] <= hi_d + 1e-12 and lo_f - 1e-12 <= res[key_fit] <= hi_f + 1e-12
    assert res['dev probe accuracy x'] > 0.5                     # (the images DO depend on the class, linearly)
    # every other pass logs the same values whether the wide probe ran in between or not
    quiet, mixed = Evaluator(tr, S), Evaluator(tr, dict(S, PROBE_WIDE=True))
    a1 = quiet.set_scores(dev, knn=True, mmd=True)
    mixed.probe_scores(fit, dev)
    b1 = mixed.set_scores(dev, knn=True, mmd=True)
    assert a1 == b1 and quiet.dev_costs(dev) == mixed.dev_costs(dev)
    assert M._snapshot(quiet.feed)['rng_state'] == M._snapshot(mixed.feed)['rng_state']
    # the averaged weights' names
    tr.ema_loaded, mixed.weights = True, 'ema'
    try:
        assert list(mixed.tag(mixed.probe_scores(fit, dev))) == [k + ' ema' for k in KEYS]
    finally:
        tr.ema_loaded, mixed.weights = False, 'live'
    # a width above the cap: that pair is skipped with one message, the other stays
    capsys.readouterr()
    monkeypatch.setattr(F, 'WPROBE_MAX_DIM', 600)
    res4 = Evaluator(tr, dict(S, PROBE_WIDE=True)).probe_scores(fit, dev)
    monkeypatch.undo()
    text = capsys.readouterr().out
    assert list(res4) == KEYS[:3] + KEYS[5:] and text.count('[evaluate] probe accuracy x skipped') == 1 and 'accuracy h skipped' not in text
    assert [res4[k] for k in res4] == [res[k] for k in res4]
    # a raised status word: nan and one message that names every fit, no exception
    bad = [(x, np.where(np.arange(B) == 0, -1, y)) for x, y in fit[:2 * n]]
    res3 = Evaluator(tr, dict(S, PROBE_WIDE=True)).probe_scores(bad, dev)
    text = capsys.readouterr().out
    assert list(res3) == KEYS and all(np.isnan(v) for v in res3.values())
    assert text.count('[evaluate] probe: status') == 1 and '1 (x)' in text and '1 (h)' in text
    assert M._snapshot(tr.feed) == before[0]
