"""-m gpu: the softmax cross-entropy and the class-score kernels (csrc/class_score.hip) case by case of tests/_cls_ref.py.  A case's call runs
through the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the case's two launches, each with the
work-item count of its grid and block.  Every buffer sits between sentinel pads, outputs start as NaN (integers as -1); afterwards the
inputs and the pads must keep their bits.  Values are gated as _cls_ref's docstring says, each check prints the observed fraction of its
bound.  Then: repeatability, the status bits, the shapes the entry points refuse, and functional.SoftmaxXent / softmax_xent / class_score."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cls_ref as R  # noqa: E402
from test_conv_dispatch_gpu import _profiled  # noqa: E402
from test_probe_gpu import Buf  # noqa: E402

pytestmark = pytest.mark.gpu


def _launches(recs):
    got = {}
    for rec in recs:
        got[(rec['name'], rec['grid'])] = got.get((rec['name'], rec['grid']), 0) + rec['launches']
    return got


def _call(gpu, bufs_of, run, profiled):
    """bufs_of(new) -> the case's buffers (the workspace last); run(L, stream) makes the call -> (rc, profiler records, buffers intact)"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L, S = _lib.load(), F._stream()
    bufs = []

    def new(*a, **kw):
        bufs.append(Buf(gpu, *a, **kw))
        return bufs[-1]
    named = bufs_of(new, L)
    if profiled:
        rc, recs = _profiled(lambda: run(L, S, named))
    else:
        rc, recs = run(L, S, named), None
        torch.cuda.synchronize()
    return rc, recs, all(b.intact() for b in bufs), named


def _xent(gpu, x, y, profiled=False):
    B, C = x.shape
    assert 1 <= B <= R.MAX_BATCH and 2 <= C <= R.MAX_CLASSES and y.shape == (B,)          # (bounds, before anything runs)

    def bufs_of(new, L):
        nbytes = L.ggan_softmax_xent_workspace(B, C)
        assert nbytes > 0
        d = dict(x=new(x), y=new(y, dtype=np.int32), loss=new(n=1), dl=new(n=B * C), hits=new(n=1, fill=-1, dtype=np.int32),
                 status=new(n=1, fill=-1, dtype=np.int32), ws=new(n=(nbytes + 3) // 4), nbytes=nbytes)
        assert d['ws'].p().value % 16 == 0
        return d

    def run(L, S, b):
        return L.ggan_softmax_xent_fwd_grad(b['x'].p(), b['y'].p(), B, C, b['loss'].p(), b['dl'].p(), b['hits'].p(), b['status'].p(), b['ws'].p(),
                                            b['nbytes'], S)
    rc, recs, intact, b = _call(gpu, bufs_of, run, profiled)
    assert rc == 0
    out = dict(loss=b['loss'].get(), dl=b['dl'].get((B, C)), hits=b['hits'].get(), status=b['status'].get())
    return out, recs, intact


def _score(gpu, x, S_, profiled=False):
    N, C = x.shape
    assert 1 <= S_ <= R.MAX_SPLITS and S_ <= N <= R.MAX_ROWS and 2 <= C <= R.MAX_CLASSES

    def bufs_of(new, L):
        nbytes = L.ggan_class_score_workspace(N, C, S_)
        assert nbytes > 0
        d = dict(x=new(x), scores=new(n=S_), stats=new(n=4), status=new(n=1, fill=-1, dtype=np.int32), ws=new(n=(nbytes + 3) // 4), nbytes=nbytes)
        assert d['ws'].p().value % 16 == 0
        return d

    def run(L, S, b):
        return L.ggan_class_score(b['x'].p(), N, C, S_, b['scores'].p(), b['stats'].p(), b['status'].p(), b['ws'].p(), b['nbytes'], S)
    rc, recs, intact, b = _call(gpu, bufs_of, run, profiled)
    assert rc == 0
    return dict(scores=b['scores'].get(), stats=b['stats'].get(), status=b['status'].get()), recs, intact


XENT_CASES = [(B, C, s) for (B, C) in R.XENT_ROWS for s in R.XENT_SCALES]


@pytest.mark.parametrize('B,C,scale', XENT_CASES, ids=[R.xent_id(*c) for c in XENT_CASES])
def test_xent_case_runs_its_launches_and_matches_float64(gpu, B, C, scale):
    x, y, t = R.xent_inputs(B, C, scale)
    out, recs, intact = _xent(gpu, x, y, profiled=True)
    got = _launches(recs)
    print('launches %s' % sorted(got.items()))
    assert got == R.xent_launches(B), (sorted(got.items()), sorted(R.xent_launches(B).items()))
    assert intact, 'an input or a sentinel pad changed'
    assert int(out['status'][0]) == 0
    loss, dl, hits = R.xent(x, y)
    assert int(out['hits'][0]) == hits and np.argmax(x[t]) != y[t]              # exact: no arithmetic decides a hit; the tied row is none
    assert out['dl'].dtype == np.float32 and np.all(np.isfinite(out['dl']))
    fr = {'loss': R.fraction(out['loss'][0], loss),
          'dlogits': float(np.max(np.abs(out['dl'].astype(np.float64) - dl))) / R.dl_gate(B, C),
          'row sums': float(np.max(np.abs(out['dl'].astype(np.float64).sum(axis=1)))) / (C * R.dl_gate(B, C))}
    for key in sorted(fr):
        print('CLSFRAC xent %s %s %.4f' % (R.xent_id(B, C, scale), key, fr[key]))
    assert all(v <= 1.0 for v in fr.values()), fr


def test_xent_a_second_call_gives_the_same_bits(gpu):
    import torch
    x, y, _ = R.xent_inputs(4099, 7, 80.0)
    a, _, _ = _xent(gpu, x, y)
    junk = torch.full((1 << 18,), 3.0, device=gpu)               # (another allocation pattern in between)
    b, _, _ = _xent(gpu, x, y)
    del junk
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize('bad', [-1, 'C'])
def test_xent_a_label_out_of_range_raises_bit_1(gpu, bad):
    B, C = 257, 64
    x, y, _ = R.xent_inputs(B, C, 1.0)
    y = np.array(y)
    y[130] = C if bad == 'C' else bad
    out, _, intact = _xent(gpu, x, y)
    assert intact and int(out['status'][0]) == R.BAD_LABEL and np.isnan(out['loss'][0])
    # dlogits is written all the same: the flagged row's one-hot is empty, every other row is as before
    ref = np.exp(R.log_softmax(x)) / B
    good = np.arange(B) != 130
    ref[np.arange(B)[good], y[good]] -= 1.0 / B
    assert np.max(np.abs(out['dl'].astype(np.float64) - ref)) <= R.dl_gate(B, C)
    # ... and the next, clean call on the same device is clean
    y[130] = 0
    again, _, _ = _xent(gpu, x, y)
    assert int(again['status'][0]) == 0 and np.isfinite(again['loss'][0])


def test_xent_an_inf_logit_raises_bit_2(gpu):
    B, C = 100, 10
    x, y, _ = R.xent_inputs(B, C, 1.0)
    x = np.array(x)
    x[41, 3] = np.inf
    out, _, intact = _xent(gpu, x, y)
    assert intact and int(out['status'][0]) == R.NONFINITE and np.isnan(out['loss'][0])
    rows = np.arange(B) != 41
    _, dl, _ = R.xent(np.delete(x, 41, axis=0), np.delete(y, 41))
    assert np.max(np.abs(out['dl'][rows].astype(np.float64) - dl * (B - 1) / B)) <= R.dl_gate(B, C)      # the other rows, untouched


def test_entry_points_refuse_shapes_out_of_range_before_any_launch(gpu):
    import ctypes as C
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = C.c_void_p(256)                                           # (never dereferenced: the refusal comes first)

    def refused(fn):
        rc, recs = _profiled(fn)
        assert rc < 0 and recs == [], (rc, recs)
        return L.ggan_last_error()
    for B, Cc in ((0, 10), (65537, 10), (8, 1), (8, 65)):
        assert L.ggan_softmax_xent_workspace(B, Cc) == 0
        msg = refused(lambda: L.ggan_softmax_xent_fwd_grad(p, p, B, Cc, p, p, p, p, p, 1 << 20, None))
        assert b'ggan_softmax_xent_fwd_grad' in msg and b'classes' in msg
    for N, Cc, S_ in ((100, 10, 0), (5, 10, 6), (100, 10, 65), (100, 1, 10), (100, 65, 10), ((1 << 20) + 1, 10, 10)):
        assert L.ggan_class_score_workspace(N, Cc, S_) == 0
        msg = refused(lambda: L.ggan_class_score(p, N, Cc, S_, p, p, p, p, 1 << 30, None))
        assert b'ggan_class_score' in msg and b'splits' in msg
    assert b'workspace' in refused(lambda: L.ggan_softmax_xent_fwd_grad(p, p, 8, 10, p, p, p, p, p, 0, None))
    assert b'workspace' in refused(lambda: L.ggan_class_score(p, 100, 10, 10, p, p, p, p, 0, None))


@pytest.mark.parametrize('N,C,S,scale', R.SCORE_ROWS, ids=[R.score_id(*c) for c in R.SCORE_ROWS])
def test_score_case_runs_its_launches_and_matches_float64(gpu, N, C, S, scale):
    x = R.score_inputs(N, C, S, scale)
    out, recs, intact = _score(gpu, x, S, profiled=True)
    got = _launches(recs)
    print('launches %s' % sorted(got.items()))
    assert got == R.score_launches(N, S), (sorted(got.items()), sorted(R.score_launches(N, S).items()))
    assert intact, 'an input or a sentinel pad changed'
    assert int(out['status'][0]) == 0
    scores, mean, std, h_row, h_marg = R.class_score(x, S)
    fr = {'scores': R.fraction(out['scores'], scores), 'mean': R.fraction(out['stats'][0], mean), 'std': R.fraction(out['stats'][1], std),
          'row entropy': R.fraction(out['stats'][2], h_row), 'marginal entropy': R.fraction(out['stats'][3], h_marg)}
    for key in sorted(fr):
        print('CLSFRAC score %s %s %.4f' % (R.score_id(N, C, S, scale), key, fr[key]))
    assert all(v <= 1.0 for v in fr.values()), fr
    again, _, _ = _score(gpu, x, S)
    for k in out:
        assert out[k].tobytes() == again[k].tobytes(), k


def test_score_a_nan_logit_gives_status_2_and_nan_everywhere(gpu):
    N, C, S = 1003, 10, 10
    x = np.array(R.score_inputs(N, C, S, 3.0))
    x[555, 2] = np.nan
    out, _, intact = _score(gpu, x, S)
    assert intact and int(out['status'][0]) == R.NONFINITE
    assert np.all(np.isnan(out['scores'])) and np.all(np.isnan(out['stats']))


def test_functional_is_the_same_call_and_differentiates_once(gpu):
    import torch
    from graphical_gan_amd import functional as F, _lib
    assert (F.CLS_MAX_CLASSES, F.CLS_MAX_SPLITS, F.CLS_MAX_BATCH, F.CLS_SCORE_MAX_ROWS) == (R.MAX_CLASSES, R.MAX_SPLITS, R.MAX_BATCH, R.MAX_ROWS)
    assert (F.CLS_BAD_LABEL, F.CLS_NONFINITE) == (R.BAD_LABEL, R.NONFINITE)
    B, C = 100, 10
    x, y, _ = R.xent_inputs(B, C, 1.0)
    out, _, _ = _xent(gpu, x, y)
    t = lambda a: torch.as_tensor(np.array(a), device=gpu)
    X, Y = t(x), t(y)
    loss, hits, status = F.softmax_xent(X, Y)
    assert loss.dim() == 0 and loss.is_cuda and hits.dtype == status.dtype == torch.int32
    assert loss.cpu().numpy().tobytes() == out['loss'].tobytes() and int(hits.item()) == int(out['hits'][0]) and int(status.item()) == 0
    # autograd.grad of the loss is the reference's dlogits; a seed other than 1 scales it
    ref_loss, ref_dl, _ = R.xent(x, y)
    Xg = X.clone().requires_grad_()
    loss_g = F.SoftmaxXent.apply(Xg, Y)[0]
    (g,) = torch.autograd.grad(loss_g, Xg, retain_graph=True)
    assert g.cpu().numpy().tobytes() == out['dl'].tobytes()
    assert np.max(np.abs(g.double().cpu().numpy() - ref_dl)) <= R.dl_gate(B, C)
    (g3,) = torch.autograd.grad(loss_g, Xg, grad_outputs=torch.full((), 3.0, device=gpu), retain_graph=True)
    assert np.array_equal(g3.cpu().numpy(), np.float32(3.0) * out['dl'])
    # a second differentiation says what is missing
    (g1,) = torch.autograd.grad(loss_g, Xg, create_graph=True)
    assert g1.requires_grad
    with pytest.raises(NotImplementedError, match='SoftmaxXent'):
        torch.autograd.grad(g1.sum(), Xg)
    # the score
    N, Cs, S, scale = R.SCORE_ROWS[2]
    xs = R.score_inputs(N, Cs, S, scale)
    sc, _, _ = _score(gpu, xs, S)
    rec = F.class_score(t(xs), S)
    assert isinstance(rec, F.ClassScore) and all(v.is_cuda for v in rec) and tuple(rec.scores.shape) == (S,) and rec.mean.dim() == 0
    assert rec.scores.cpu().numpy().tobytes() == sc['scores'].tobytes() and int(rec.status.item()) == 0
    got = np.array([rec.mean.item(), rec.std.item(), rec.row_entropy.item(), rec.marginal_entropy.item()], np.float32)
    assert got.tobytes() == sc['stats'].tobytes()
    # no CPU path, no backward, the bounds
    with pytest.raises(_lib.GganError):
        F.softmax_xent(X.cpu(), Y.cpu())
    with pytest.raises(_lib.GganError):
        F.class_score(t(xs).cpu(), S)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.class_score(t(xs).requires_grad_(), S)
    with pytest.raises(ValueError, match='int32'):
        F.softmax_xent(X, Y.cpu())
    with pytest.raises(ValueError, match='splits'):
        F.class_score(t(xs), 65)
    with pytest.raises(ValueError, match='classes'):
        F.softmax_xent(torch.zeros(4, 65, device=gpu), torch.zeros(4, dtype=torch.int32, device=gpu))


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------------
def test_the_device_fit_follows_the_float64_restatement_and_solves_the_task(gpu):
    """The task of _cls_ref (four quadrants, 512 fit rows, 256 held out, 32 steps): the float64 restatement reaches 100 % held-out accuracy with
    every top-two logit margin above 1 (measured on the CPU: the smallest is 12.89), so the device fit must reach 100 % too; its first 20
    per-step losses stay within 4 x the float32-against-float64 gap of the CPU restatement (7.34e-7, at step 2: the gate is 2.94e-6).
    Most of that gap is the float32 bias-corrected step size of Adam's first steps (csrc/optim.hip: adam_lr_t), not summation order:
    _cls_ref.py says what it consists of."""
    import torch
    from graphical_gan_amd import optim
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.classifier import ImageClassifier
    ref = R.fit_reference('float64')
    assert ref['accuracy'] == 1.0 and ref['margin'] > 1.0                     # the condition on the case
    fx, fy, hx, hy = R.fit_task()
    t = lambda a: torch.as_tensor(np.array(a), device=gpu)
    registry, optimizers = dict(lib.named_params()), dict(optim._optimizers)
    cls = ImageClassifier(R.fit_config(), R.FIT_CLASSES, R.FIT_SEED, device=gpu)
    losses = cls.fit([(t(x), t(y)) for x, y in R.fit_batches(fx, fy)], R.FIT_EPOCHS)
    assert losses.is_cuda and tuple(losses.shape) == (len(ref['losses']),)
    assert lib.named_params() == registry and optim._optimizers == optimizers and int(cls.opt.step.item()) == len(ref['losses'])
    assert (cls.fit_rows, cls.epochs) == (R.FIT_ROWS, R.FIT_EPOCHS)
    losses = losses.cpu().numpy().astype(np.float64)
    held = [(t(x), t(y)) for x, y in R.fit_batches(hx, hy)]
    lg, ft = cls.logits(t(hx), features=True)
    assert tuple(lg.shape) == (R.FIT_HELD, R.FIT_CLASSES) and tuple(ft.shape) == (R.FIT_HELD, 128) and not lg.requires_grad
    lg = lg.cpu().numpy()
    top = np.sort(lg, axis=1)
    print('CLSFIT held-out accuracy %.4f, smallest margin %.3f (float64: %.3f); largest logit gap to float64 %.3e'
          % (np.mean(np.argmax(lg, 1) == hy), np.min(top[:, -1] - top[:, -2]), ref['margin'], np.max(np.abs(lg - ref['held_logits']))))
    gaps = np.abs(losses[:R.FIT_TRAJECTORY] - ref['losses'][:R.FIT_TRAJECTORY])
    print('CLSFRAC fit trajectory %.4f (largest gap %.3e at step %d, gate %.3e)' % (gaps.max() / R.FIT_LOSS_GATE, gaps.max(), int(gaps.argmax()), R.FIT_LOSS_GATE))
    assert cls.accuracy(held) == 1.0 and np.array_equal(np.argmax(lg, 1), hy)
    assert gaps.max() <= R.FIT_LOSS_GATE, (gaps.max(), R.FIT_LOSS_GATE)
    # minibatch independence: a row's logits do not depend on who else is in the minibatch (no BatchNorm).  Not to the bit -- the products'
    # launch plans, and so their summation orders, follow the row count --, but within the roundoff of the longest sum, 512 terms
    alone, among = cls.logits(t(hx[:8])).cpu().numpy().astype(np.float64), lg[:8].astype(np.float64)
    assert np.max(np.abs(alone - among)) <= 512 * R.U32 * np.max(np.abs(among)), np.max(np.abs(alone - among))
    other = cls.logits(t(np.concatenate([hx[:8], 1.0 - hx[8:32]]))).cpu().numpy().astype(np.float64)      # the same rows among other company
    assert np.max(np.abs(other[:8] - among)) <= 512 * R.U32 * np.max(np.abs(among))


# ---- the pass ----------------------------------------------------------------------------------------------------------------------------------
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)
from test_knn_gpu import _labelled_dev  # noqa: E402

KEYS = ['dev classifier score x', 'dev classifier score std x', 'dev classifier score data', 'dev classifier accuracy', 'dev classifier frechet x']


def _settings(B, mode, K, **more):
    return dict(dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, CLS_SAMPLES=7 * B + 3, CLS_MAX_ROWS=5 * B, CLS_SPLITS=3, CLS_FIT_ROWS=10 * B, CLS_EPOCHS=2), **more)


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_classifier_scores_values_and_the_passes_it_leaves_alone(gpu, dataset, K, mode, capsys, tmp_path, monkeypatch):
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd.evaluate import Evaluator
    monkeypatch.delenv('GGAN_CLS_CKPT', raising=False)
    B, n = 8, 6
    tr = P._model(gpu, dataset, B, K, mode)
    both = _labelled_dev(dataset, B, 3 * n)
    fit, dev = both[:2 * n], both[2 * n:]
    S = _settings(B, mode, K)
    ev = Evaluator(tr, S)
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before = P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']
    res, got = ev.classifier_scores(fit, dev, return_sets=True)
    assert list(res) == KEYS and all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    assert (P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']) == before
    cls = got['classifier']
    assert ev.cls_fits == 1 and cls.classes == 4 and cls.fit_rows == 10 * B and cls.epochs == 2 and cls.held_out == res['dev classifier accuracy']
    assert tuple(got['logits_x'].shape) == (7 * B, 4) and tuple(got['features_x'].shape) == (7 * B, 128)
    assert tuple(got['logits_data'].shape) == (5 * B, 4) and tuple(got['features_data'].shape) == (5 * B, 128)
    host = {k: v.cpu().numpy() for k, v in got.items() if torch.is_tensor(v)}
    assert np.array_equal(host['labels'], np.concatenate([y for _, y in dev[:5]]))
    # each value is what the restatement gives from the returned logits and labels
    sx, mx, sdx, hrx, hmx = R.class_score(host['logits_x'], 3)
    sd, md, _, hrd, hmd = R.class_score(host['logits_data'], 3)
    fr = {'score x': R.fraction(res[KEYS[0]], mx), 'score std x': R.fraction(res[KEYS[1]], sdx), 'score data': R.fraction(res[KEYS[2]], md),
          'scores x': R.fraction(host['scores_x'], sx), 'scores data': R.fraction(host['scores_data'], sd),
          'entropies': max(R.fraction([v.item() for v in got['entropies_x']], [hrx, hmx]), R.fraction([v.item() for v in got['entropies_data']], [hrd, hmd]))}
    for key in sorted(fr):
        print('CLSFRAC pass %s %s %.4f' % (dataset, key, fr[key]))
    assert all(v <= 1.0 for v in fr.values()), fr
    assert res[KEYS[3]] == float(np.mean(np.argmax(host['logits_data'], axis=1) == host['labels']))
    fd, st = F.frechet_distance(got['features_data'], got['features_x'][:5 * B])
    assert int(st.item()) == 0 and res[KEYS[4]] == float(fd[0].item())
    print(dataset, res)
    # the second firing does not refit: the same classifier, the same weights, fresh noise
    theta = cls.opt.theta.clone()
    res2, got2 = ev.classifier_scores(fit, dev, return_sets=True)
    assert ev.cls_fits == 1 and got2['classifier'] is cls and torch.equal(cls.opt.theta, theta)
    assert torch.equal(got2['logits_data'], got['logits_data']) and not torch.equal(got2['logits_x'], got['logits_x'])
    assert res2[KEYS[3]] == res[KEYS[3]] and res2[KEYS[2]] == res[KEYS[2]]
    # every other pass logs the same values whether the classifier pass ran in between or not
    plain, mixed = Evaluator(tr, S), Evaluator(tr, S)
    a1 = plain.set_scores(dev, knn=True, mmd=True)
    mixed.classifier_scores(fit, dev)
    b1 = mixed.set_scores(dev, knn=True, mmd=True)
    mixed.classifier_scores(fit, dev)
    assert a1 == b1 and plain.dev_costs(dev) == mixed.dev_costs(dev) and plain.frechet_scores(dev) == mixed.frechet_scores(dev)
    # ... the passes with a noise state of their own included, fired twice so that their states have moved
    for _ in range(2):
        a2, a3 = plain.probe_scores(fit, dev), plain.swd_scores(dev)
        mixed.classifier_scores(fit, dev)
        assert mixed.probe_scores(fit, dev) == a2 and mixed.swd_scores(dev) == a3
    assert plain.set_scores(dev, prdc=True, rec=True) == mixed.set_scores(dev, prdc=True, rec=True)
    assert P._snapshot(plain.feed)['rng_state'] == P._snapshot(mixed.feed)['rng_state']
    # with a file: it appears, and a fresh evaluator that loads it reproduces the first one's values bit for bit without fitting
    path = str(tmp_path / 'cls.npz')
    monkeypatch.setenv('GGAN_CLS_CKPT', path)
    first = Evaluator(tr, S)
    r1 = first.classifier_scores(fit, dev)
    assert os.path.exists(path) and first.cls_fits == 1 and r1 == res                 # (the same seed: the same fit and the same noise as ev's first call)
    with np.load(path) as z:
        assert 'classifier/meta' in z.files and 'classifier/Conv1.Filters' in z.files and 'accuracy=%s' % r1[KEYS[3]] in list(z['classifier/meta'])
    second = Evaluator(tr, S)
    r2 = second.classifier_scores([fit[0]], dev)                                      # (the fit rows are not even looked at)
    assert second.cls_fits == 0 and r2 == r1
    monkeypatch.delenv('GGAN_CLS_CKPT')
    # the averaged weights' names
    tr.ema_loaded, mixed.weights = True, 'ema'
    try:
        assert list(mixed.tag(mixed.classifier_scores(fit, dev))) == [k + ' ema' for k in KEYS] and mixed.cls_fits == 1
    finally:
        tr.ema_loaded, mixed.weights = False, 'live'
    # a raised status word: nan and one message, no exception
    capsys.readouterr()
    bad = [(x, np.where(np.arange(B) == 0, -1, y)) for x, y in dev[:5]]
    res3 = mixed.classifier_scores(fit, bad)
    out = capsys.readouterr().out
    assert list(res3) == KEYS and np.isnan(res3[KEYS[3]]) and out.count('[evaluate] classifier: status') == 1
    assert P._snapshot(tr.feed) == before[0]


def test_training_bit_identical_with_the_classifier_pass_and_the_flag_prints_the_rows(gpu, tmp_path, monkeypatch, capsys):
    from graphical_gan_amd import checkpoint, evaluate
    from graphical_gan_amd.models import Config
    monkeypatch.delenv('GGAN_CLS_CKPT', raising=False)
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    small = dict(CLS_SAMPLES=3 * B, CLS_MAX_ROWS=2 * B, CLS_SPLITS=2, CLS_FIT_ROWS=4 * B, CLS_EPOCHS=1)
    base = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base, KNN_EVERY=2), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, KNN_EVERY=2, CLS_EVERY=2, **small), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1) and not any('classifier' in k.lower() for k in w1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    rest = lambda seen: [(n, i, v) for n, i, v in seen if n not in KEYS and n != 'time']
    assert rest(seen0) == rest(seen1)                        # the training costs AND the k-NN pass's values
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [1, 3], key
    assert not [n for n, _, _ in seen0 if n in KEYS]
    # the checkpoint does not hold the classifier; evaluate --cls prints the five rows
    ckpt = str(tmp_path / 'params.npz')
    checkpoint.save(ckpt, tr1)
    with np.load(ckpt) as z:
        assert not any('classifier' in k for k in z.files)
    P._fresh()
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=K, BATCH_SIZE=B, **small)
    capsys.readouterr()
    res = evaluate.main([ckpt, '--script', 'gmgan_inference_mnist', '--cls'] + ['--set=%s=%s' % kv for kv in over.items()])
    out = capsys.readouterr().out
    assert all(k in res and ('%s\t' % k) in out for k in KEYS)
    plain = evaluate.main([ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()])
    assert not any(k in plain for k in KEYS) and all(plain[k] == res[k] for k in plain)
    # GGAN_EMA_EVAL=ema: the ' ema' names and no others; =both: both sets of names from ONE fitted classifier
    from graphical_gan_amd import run
    from graphical_gan_amd.classifier import ImageClassifier
    fits, fit = [], ImageClassifier.fit
    monkeypatch.setattr(ImageClassifier, 'fit', lambda self, *a, **kw: (fits.append(1), fit(self, *a, **kw))[1])
    monkeypatch.setenv('GGAN_EMA_DECAY', '0.9')
    monkeypatch.setenv('GGAN_CLS_EVERY', '2')
    for which, names in (('ema', [k + ' ema' for k in KEYS]), ('both', KEYS + [k + ' ema' for k in KEYS])):
        monkeypatch.setenv('GGAN_EMA_EVAL', which)
        S = dict(base, ITERS=2, **small)
        S.update(run.ema_settings('gmgan_inference_mnist'))
        S.update(run.classifier_settings('gmgan_inference_mnist'))
        assert S['EMA_EVAL'] == which and S['CLS_EVERY'] == 2
        del fits[:]
        _, _, _, seen = P._train(S, cfg())
        assert [n for n, i, _ in seen if 'classifier' in n] == names and all(i == 1 for n, i, _ in seen if 'classifier' in n)
        assert len(fits) == 1
    for k in ('GGAN_EMA_DECAY', 'GGAN_EMA_EVAL', 'GGAN_CLS_EVERY'):
        monkeypatch.delenv(k)
    # synthetic minibatches have no labels: one message, no pass
    capsys.readouterr()
    S = dict(DATASET='mnist', BATCH_SIZE=8, ITERS=2, LOG_EVERY=1, MODE='ali', SYNTHETIC='force', CLS_EVERY=1)
    _, _, _, seen = P._train(S, Config('mnist', batch_size=8, n_coms=0, mode='ali', dim=8, dim_latent=16))
    assert capsys.readouterr().out.count('[run] dev classifier score skipped') == 1 and not [n for n, _, _ in seen if 'classifier' in n]
