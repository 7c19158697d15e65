"""-m gpu: the least-squares linear probe (csrc/probe_fit.hip) row by row of tests/_probe_ref.py.  A row's calls -- moments, normal equations,
solve, the prediction of the fit rows and of the scoring rows -- run through the C ABI between ggan_prof_reset / ggan_prof_enable; the
profiler must have seen exactly the row's launches, the normal-equations instance the row names among them, each with the work-item count
of its grid and block.  Every buffer sits between sentinel pads, outputs start as NaN (integers as -1); afterwards the inputs and the pads
must keep their bits.  The outputs are checked in the stages of _probe_ref's docstring, each against float64 from the float32 values the
stage itself read; each check prints the observed fraction of its bound, and a figure above 1 fails.  Then: repeatability, a NaN and a
label out of range in the input, and the pass Evaluator.probe_scores -- its names and values, the other passes it leaves bit-identical,
the ' ema' names, the training run it does not change."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _probe_ref as R  # noqa: E402
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)
from test_conv_dispatch_gpu import _profiled  # noqa: E402
from test_knn_gpu import _labelled_dev  # noqa: E402

pytestmark = pytest.mark.gpu

_SENT = {np.dtype(np.float32): R.SENTINEL, np.dtype(np.int32): -12345}


class Buf:
    """a device buffer of float32 / int32 between PAD sentinels on either side; out: filled with `fill`, else it holds `values`, read-only"""
    def __init__(self, gpu, values=None, n=0, fill=np.nan, dtype=np.float32):
        import torch
        self.out = values is None
        body = np.full(n, fill, dtype) if self.out else np.ascontiguousarray(np.ravel(values), dtype)
        pad = np.full(R.PAD, _SENT[np.dtype(dtype)], dtype)
        self.host = np.concatenate([pad, body, pad])
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        self.n = body.size

    def p(self):
        return C.c_void_p(self.dev.data_ptr() + 4 * R.PAD)

    def get(self, shape=None):
        a = self.dev.cpu().numpy()[R.PAD:R.PAD + self.n]
        return a.reshape(shape) if shape is not None else a

    def intact(self):
        now = self.dev.cpu().numpy()
        same = lambda a, b: a.tobytes() == b.tobytes()
        return same(now[:R.PAD], self.host[:R.PAD]) and same(now[-R.PAD:], self.host[-R.PAD:]) and (self.out or same(now, self.host))


def _probe(gpu, Z, y, Zq, yq, C_, profiled=True):
    """one fit and two predictions through the C ABI -> (outputs as numpy, profiler records, all buffers intact)"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L, S = _lib.load(), F._stream()
    (n, d), m = Z.shape, Zq.shape[0]
    assert 2 <= n <= 131072 and 1 <= m <= 131072 and 1 <= d <= R.MAX_DIM and 1 <= C_ <= R.MAX_CLASSES      # (bounds, before anything runs)
    assert y.shape == (n,) and yq.shape == (m,) and Zq.shape[1] == d
    bufs = []

    def new(*a, **kw):
        bufs.append(Buf(gpu, *a, **kw))
        return bufs[-1]
    bZ, by, bZq, byq = new(Z), new(y, dtype=np.int32), new(Zq), new(yq, dtype=np.int32)
    o = dict(mean=new(n=d), inv_std=new(n=d), G=new(n=d * d), R=new(n=d * C_), W=new(n=d * C_), bias=new(n=C_))
    oi = dict(counts=new(n=C_, fill=-1, dtype=np.int32), status=new(n=1, fill=-1, dtype=np.int32), pred_fit=new(n=n, fill=-1, dtype=np.int32),
              pred=new(n=m, fill=-1, dtype=np.int32), hit_fit=new(n=1, fill=-1, dtype=np.int32), hit=new(n=1, fill=-1, dtype=np.int32))
    nbytes = max(L.ggan_probe_moments_workspace(n, d, C_), L.ggan_probe_normal_workspace(n, d, C_))
    assert nbytes > 0
    ws = new(n=(nbytes + 3) // 4)
    assert ws.p().value % 16 == 0

    def ok(rc):
        assert rc == 0, (rc, L.ggan_last_error())

    def run():
        ok(L.ggan_probe_moments(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), oi['counts'].p(), oi['status'].p(), ws.p(), nbytes, S))
        ok(L.ggan_probe_normal(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), o['G'].p(), o['R'].p(), ws.p(), nbytes, S))
        ok(L.ggan_probe_solve(o['G'].p(), o['R'].p(), oi['counts'].p(), n, d, C_, float(R.RIDGE), o['W'].p(), o['bias'].p(), oi['status'].p(), S))
        ok(L.ggan_probe_predict(bZ.p(), by.p(), n, d, C_, o['mean'].p(), o['inv_std'].p(), o['W'].p(), o['bias'].p(), oi['pred_fit'].p(),
                                oi['hit_fit'].p(), S))
        ok(L.ggan_probe_predict(bZq.p(), byq.p(), m, d, C_, o['mean'].p(), o['inv_std'].p(), o['W'].p(), o['bias'].p(), oi['pred'].p(),
                                oi['hit'].p(), S))
    if profiled:
        _, recs = _profiled(run)
    else:
        run()
        torch.cuda.synchronize()
        recs = None
    shapes = dict(G=(d, d), R=(d, C_), W=(d, C_))
    out = {k: v.get(shapes.get(k)) for k, v in list(o.items()) + list(oi.items())}
    return out, recs, all(b.intact() for b in bufs[:-1]) and bufs[-1].intact()      # (the workspace: its pads)


def _fractions(r, x, out, twin=None):
    """the stage checks of one fit + prediction -> {stage: observed fraction of its bound}; the exact stages are asserted here"""
    C_, f4 = r['C'], np.float32
    assert all(out[k].dtype == f4 for k in ('mean', 'inv_std', 'G', 'R', 'W', 'bias'))
    fr = {}
    fr.update(R.check_moments(x['Z'], x['y'], C_, out['mean'], out['inv_std'], out['counts']))
    fr.update(R.check_normal(x['Z'], x['y'], C_, out['mean'], out['inv_std'], out['G'], out['R']))
    assert np.array_equal(out['G'], out['G'].T)
    fr.update(R.check_solve(out['G'], out['R'], out['W']))
    assert np.array_equal(out['bias'], (out['counts'].astype(np.float64) / r['n']).astype(f4))
    for Z, y, pred, hit, what in ((x['Z'], x['y'], out['pred_fit'], out['hit_fit'], 'fit'), (x['Zq'], x['yq'], out['pred'], out['hit'], 'dev')):
        ref, closed, _ = R.margins(Z, out['mean'], out['inv_std'], out['W'], out['bias'], twin=twin)
        assert pred.min() >= 0 and pred.max() < C_
        assert np.array_equal(pred[closed], ref[closed]), np.flatnonzero(closed & (pred != ref))[:8]
        assert int(hit[0]) == int(np.sum(pred == y))
        fr['open rows ' + what] = (1.0 - closed.mean()) / R.OPEN_ROWS_CAP
        print('   %s: accuracy %.4f (float64 from the device fit: %.4f), %d rows below the margin, %d of them differ'
              % (what, np.mean(pred == y), np.mean(ref == y), int((~closed).sum()), int(np.sum(pred != ref))))
    return fr


@pytest.mark.parametrize('idx', range(len(R.ROWS)), ids=[R.row_id(r) for r in R.ROWS])
def test_row_runs_its_instance_and_matches_float64(gpu, idx):
    r, x, ref = R.ROWS[idx], R.inputs(idx), R.reference(idx)
    out, recs, intact = _probe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'])
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
        assert not np.any(out['pred'] == b) and not np.any(out['pred_fit'] == b) and np.any(out['pred_fit'] == a)
    if 'const' in r:
        j = r['const']
        assert out['inv_std'][j] == 0 and np.all(out['W'][j] == 0) and np.all(out['G'][j] == 0)
    if 'absent' in r:
        c = r['absent']
        assert out['counts'][c] == 0 and np.all(out['W'][:, c] == 0) and not np.any(out['pred'] == c)
    fr = _fractions(r, x, out, twin)
    # end to end: the device's W against float64 from the raw inputs, measured by what float32 numpy makes of the same formula
    fr['W end to end'] = R.rel_w(out['W'], ref['W']) / (R.W_FACTOR * ref['w32_err'])
    for key in sorted(fr):
        print('PROBEFRAC %s %s %s %.4f' % (R.row_id(r), R.instance(r), key, fr[key]))
    print('   W: device %.3e, float32 numpy %.3e (relative to max |W|)' % (R.rel_w(out['W'], ref['W']), ref['w32_err']))
    assert all(v <= 1.0 for v in fr.values()), fr


def test_a_second_call_gives_the_same_bits(gpu):
    import torch
    idx = 3
    r, x = R.ROWS[idx], R.inputs(idx)
    a, _, _ = _probe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    junk = torch.full((1 << 18,), 3.0, device=gpu)               # (another allocation pattern in between)
    b, _, _ = _probe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    del junk
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_a_nan_row_raises_the_status_word_and_nothing_else_breaks(gpu):
    idx = 2
    r, x = R.ROWS[idx], R.inputs(idx)
    Z = np.array(x['Z'])
    Z[5, 3] = np.nan
    out, _, intact = _probe(gpu, Z, x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    assert intact
    assert int(out['status'][0]) & R.NONFINITE and not int(out['status'][0]) & R.BAD_LABEL
    assert np.all(np.isnan(out['W']))                            # said aloud, not a half-right W
    assert np.array_equal(out['counts'], np.bincount(x['y'], minlength=r['C'])) and np.all(np.isfinite(out['bias']))
    cols = np.arange(r['d']) != 3
    mu, s, _ = R.moments(x['Z'], x['y'], r['C'])
    assert np.allclose(out['mean'][cols], mu[cols], rtol=1e-6) and np.allclose(out['inv_std'][cols], s[cols], rtol=1e-6)      # the other columns
    assert out['pred'].min() >= 0 and out['pred'].max() < r['C'] and out['pred_fit'].min() >= 0 and out['pred_fit'].max() < r['C']
    assert int(out['hit'][0]) == int(np.sum(out['pred'] == x['yq']))
    # ... and the next, clean call on the same device is clean
    again, _, _ = _probe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    assert int(again['status'][0]) == 0 and np.all(np.isfinite(again['W']))


def test_a_label_out_of_range_is_flagged_and_counted_nowhere(gpu):
    idx = 1
    r, x = R.ROWS[idx], R.inputs(idx)
    y = np.array(x['y'])
    y[7], y[9], y[200] = r['C'], -1, 1 << 30
    out, _, intact = _probe(gpu, x['Z'], y, x['Zq'], x['yq'], r['C'], profiled=False)
    assert intact and int(out['status'][0]) == R.BAD_LABEL
    good = (y >= 0) & (y < r['C'])
    assert np.array_equal(out['counts'], np.bincount(y[good], minlength=r['C'])) and out['counts'].sum() == r['n'] - 3
    assert np.all(np.isfinite(out['W'])) and np.all(np.isfinite(out['G'])) and np.all(np.isfinite(out['R']))


def test_functional_is_the_same_chain(gpu):
    """lsq_probe_fit / lsq_probe_predict give the bits of the C calls, as device tensors, and refuse a gradient"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    idx = 2
    r, x = R.ROWS[idx], R.inputs(idx)
    out, _, _ = _probe(gpu, x['Z'], x['y'], x['Zq'], x['yq'], r['C'], profiled=False)
    t = lambda a: torch.as_tensor(np.array(a), device=gpu)
    Z, y, Zq, yq = t(x['Z']), t(x['y']), t(x['Zq']), t(x['yq'])
    fit = F.lsq_probe_fit(Z, y, r['C'], float(R.RIDGE))
    assert isinstance(fit, F.ProbeFit) and all(v.is_cuda for v in fit)
    for k in ('mean', 'inv_std', 'W', 'bias', 'counts', 'status'):
        assert getattr(fit, k).cpu().numpy().tobytes() == out[k].tobytes(), k
    correct, pred = F.lsq_probe_predict(fit, Zq, yq, return_pred=True)
    assert correct.dtype == pred.dtype == torch.int32 and tuple(correct.shape) == (1,)
    assert np.array_equal(pred.cpu().numpy(), out['pred']) and int(correct.item()) == int(out['hit'][0])
    assert torch.equal(F.lsq_probe_predict(fit, Zq), pred) and torch.equal(F.lsq_probe_predict(fit, Zq, yq), correct)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.lsq_probe_fit(Z.clone().requires_grad_(), y, r['C'], 0.01)
    with pytest.raises(ValueError, match='int32'):
        F.lsq_probe_fit(Z, y.cpu(), r['C'], 0.01)                # a device mismatch


# ---- the pass ----------------------------------------------------------------------------------------------------------------------------------
KEYS = ['dev probe accuracy z', 'fit probe accuracy z', 'dev probe accuracy xr']


def _restated(fit, fit_z, fit_y, dev_z, dev_y, classes):
    """the restatement of tests/_probe_ref.py on the pass's own device rows: the device's fit record against the float64 fit of those rows
    (moments to 4 u, W end to end within 4 x the float32 restatement's error), then the float64 argmax from the record on the dev and
    the fit rows -> [(lowest, highest accuracy the margin rule allows) for dev, for fit]: the two ends differ by the rows below the margin"""
    dev_ = {k: getattr(fit, k).cpu().numpy() for k in fit._fields}
    f = R.fit(fit_z, fit_y, classes)
    fr = R.check_moments(fit_z, fit_y, classes, dev_['mean'], dev_['inv_std'], dev_['counts'])
    fr['W end to end'] = R.rel_w(dev_['W'], f['W']) / (R.W_FACTOR * R.rel_w(R.fit32(fit_z, fit_y, classes), f['W']))
    print('   pass fit', {k: round(v, 4) for k, v in fr.items()})
    assert all(v <= 1.0 for v in fr.values()), fr
    res = []
    for Z, y in ((dev_z, dev_y), (fit_z, fit_y)):
        pred, closed, _ = R.margins(Z, dev_['mean'], dev_['inv_std'], dev_['W'], dev_['bias'])
        hits = pred == y
        res.append((np.sum(hits & closed) / float(len(y)), (np.sum(hits & closed) + np.sum(~closed)) / float(len(y))))
    return res


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_probe_scores_values_and_the_passes_it_leaves_alone(gpu, dataset, K, mode, capsys):
    import torch
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 12
    tr = P._model(gpu, dataset, B, K, mode)
    both = _labelled_dev(dataset, B, 3 * n)                     # one set of class prototypes: 2 n minibatches to fit on, n (+ a partial one) to score
    fit, dev = both[:2 * n], both[2 * n:]
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    ev = Evaluator(tr, S)
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before = P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']
    res, got = ev.probe_scores(fit, dev, return_fit=True)
    assert list(res) == KEYS and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    assert (P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']) == before
    c = tr.cfg
    assert tuple(got['fit_z'].shape) == (2 * n * B, c.dim_latent) == tuple(got['fit_xr_rows'].shape) and tuple(got['dev_z'].shape) == (n * B, c.dim_latent)
    host = {k: v.cpu().numpy() for k, v in got.items() if torch.is_tensor(v)}
    assert np.array_equal(host['dev_y'], np.concatenate([y for _, y in dev[:n]])) and np.array_equal(host['fit_y'], np.concatenate([y for _, y in fit[:2 * n]]))
    assert int(got['fit'].status.item()) == 0 and int(got['fit_xr'].status.item()) == 0
    for (key_dev, key_fit), rec, zf, zd in ((KEYS[:2], 'fit', 'fit_z', 'dev_z'), ((KEYS[2], None), 'fit_xr', 'fit_xr_rows', 'dev_xr')):
        (lo_d, hi_d), (lo_f, hi_f) = _restated(got[rec], host[zf], host['fit_y'], host[zd], host['dev_y'], 4)
        print(dataset, key_dev, res[key_dev], (lo_d, hi_d), key_fit, res.get(key_fit), (lo_f, hi_f))
        assert lo_d - 1e-12 <= res[key_dev] <= hi_d + 1e-12
        assert key_fit is None or lo_f - 1e-12 <= res[key_fit] <= hi_f + 1e-12
    assert res['dev probe accuracy xr'] > 0.5                    # (the images DO depend on the class, linearly)
    # the caps, at whole minibatches; a second pass draws on: its own noise state moves, the evaluator's does not
    res2, capped = Evaluator(tr, dict(S, PROBE_FIT_ROWS=5 * B + 3, PROBE_MAX_ROWS=2 * B)).probe_scores(fit, dev, return_fit=True)
    assert capped['fit_z'].shape[0] == 5 * B and capped['dev_z'].shape[0] == 2 * B and list(res2) == KEYS
    # every other pass logs the same values whether the probe ran in between or not
    plain, mixed = Evaluator(tr, S), Evaluator(tr, S)
    a1 = plain.set_scores(dev, knn=True, mmd=True)
    mixed.probe_scores(fit, dev)
    b1 = mixed.set_scores(dev, knn=True, mmd=True)
    mixed.probe_scores(fit, dev)
    assert a1 == b1 and plain.dev_costs(dev) == mixed.dev_costs(dev)
    assert P._snapshot(plain.feed)['rng_state'] == P._snapshot(mixed.feed)['rng_state']
    # the averaged weights' names
    tr.ema_loaded, mixed.weights = True, 'ema'
    try:
        assert list(mixed.tag(mixed.probe_scores(fit, dev))) == [k + ' ema' for k in KEYS]
    finally:
        tr.ema_loaded, mixed.weights = False, 'live'
    # a raised status word: nan and one message, no exception
    capsys.readouterr()
    bad = [(x, np.where(np.arange(B) == 0, -1, y)) for x, y in fit[:2 * n]]
    res3 = Evaluator(tr, S).probe_scores(bad, dev)
    out = capsys.readouterr().out
    assert list(res3) == KEYS and all(np.isnan(v) for v in res3.values()) and out.count('[evaluate] probe: status') == 1
    assert P._snapshot(tr.feed) == before[0]


def test_training_bit_identical_with_the_probe_pass(gpu, tmp_path, monkeypatch, capsys):
    from graphical_gan_amd.models import Config
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base, KNN_EVERY=2), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, KNN_EVERY=2, PROBE_EVERY=2), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    rest = lambda seen: [(n, i, v) for n, i, v in seen if n not in KEYS and n != 'time']
    assert rest(seen0) == rest(seen1)                        # the training costs AND the k-NN pass's values
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [1, 3], key
    assert all(0.0 <= v <= 1.0 for n, _, v in seen1 if n in KEYS) and not [n for n, _, _ in seen0 if n in KEYS]
    order = [n for n, i, _ in seen1 if i == 1 and n.startswith('dev ')]
    assert order.index('dev knn accuracy x') < order.index(KEYS[0])                  # after the set-level scores
    # synthetic minibatches have no labels: one message, no pass
    capsys.readouterr()
    S = dict(DATASET='mnist', BATCH_SIZE=8, ITERS=2, LOG_EVERY=1, MODE='ali', SYNTHETIC='force', PROBE_EVERY=1)
    _, _, _, seen = P._train(S, Config('mnist', batch_size=8, n_coms=0, mode='ali', dim=8, dim_latent=16))
    assert capsys.readouterr().out.count('[run] dev probe accuracy skipped') == 1 and not [n for n, _, _ in seen if 'probe' in n]
