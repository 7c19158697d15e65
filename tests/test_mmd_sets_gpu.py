"""-m gpu: the set-level mixture-of-RBF sums (csrc/mmd_sets.hip) against the float64 direct-difference restatement tests/_mmd_ref.py --
values, exact pair coverage, the same-pointer case, repeatability, agreement with the fused minibatch op --, the differentiable unbiased
estimator, and the dev-set MMD pass: its sets, its values, the Trainer it leaves untouched, the training it does not change, the CLI.

The value gate is the project's existing one for this quantity (test_mix_rbf_mmd2_fused_op): |v - ref| <= 2e-5 max(1, |ref|)."""
import ctypes as C
import functools
import gzip
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _mmd_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(2, 2, 1),               # minimum
          (5, 9, 16),              # the fused op's own shape
          (130, 67, 33),           # X / Y boundary inside a tile, ragged rows and k, rows that are not 16-byte aligned
          (257, 300, 131),         # several tile pairs each way, past the fused op's 512 rows
          (192, 160, 3072)]        # long k loop; data in [0.6, 1]: large common norms


def _gate(v, ref):
    return abs(v - ref) <= 2e-5 * max(1.0, abs(ref))


@functools.lru_cache(maxsize=None)
def _case(m, n, d):
    """(x, y, float64 sums) of a shape, computed once per run and never written to"""
    rng = np.random.default_rng(1000 * m + 10 * n + d)
    if d == 3072:
        x = (0.6 + 0.4 * rng.random((m, d))).astype(np.float32)
        y = (0.6 + 0.4 * rng.random((n, d)) ** 1.25).astype(np.float32)
    else:
        x = (rng.standard_normal((m, d)) * 1.5).astype(np.float32)
        y = (rng.standard_normal((n, d)) + 0.3).astype(np.float32)
    s = R.sums3(x, y)
    for a in (x, y, s):
        a.setflags(write=False)
    return x, y, s


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32), device=dev)          # (a copy: the shared cases are read-only)


# ---- 1. values -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', SHAPES)
def test_sums_and_both_estimators_against_float64(gpu, m, n, d):
    from graphical_gan_amd import functional as F
    from graphical_gan_amd import tflib as lib
    x, y, s = _case(m, n, d)
    tx, ty = _t(x, gpu), _t(y, gpu)
    got = F.mix_rbf_sums(tx, ty, R.SIGMAS)
    assert got.dtype.is_floating_point and got.element_size() == 8 and tuple(got.shape) == (3,) and got.is_cuda
    g = got.cpu().numpy()
    print('sums', (m, n, d), g, s)
    for biased in (True, False):
        ref = R.from_sums(s, m, n, 6.0, biased)
        v = R.from_sums(g, m, n, 6.0, biased)
        print(' biased' if biased else ' unbiased', v, ref, abs(v - ref))
        assert _gate(v, ref), (biased, v, ref)
    # the public route: a 0-dim float32 device tensor (the unbiased estimator always, the biased one beyond the fused op's rows)
    u = lib.objs.mmd.mix_rbf_mmd2(tx, ty, biased=False)
    assert u.dim() == 0 and u.is_cuda and str(u.dtype) == 'torch.float32'
    assert _gate(float(u), R.from_sums(s, m, n, 6.0, False))
    if m + n > 512:
        b = lib.objs.mmd.mix_rbf_mmd2(tx, ty, biased=True)
        assert b.dim() == 0 and _gate(float(b), R.from_sums(s, m, n, 6.0, True))
    # one pair more or less would show: the smallest kernel value moves an estimator by more than the gate
    if m > 2:
        x64, y64 = x.astype(np.float64), y.astype(np.float64)
        kmin = min(R._kernel(x64[:8], y64, R.SIGMAS, [1.0] * 6).min(), R._kernel(x64[:8], x64, R.SIGMAS, [1.0] * 6).min())
        assert kmin / (m * max(m, n)) > 2e-5 * max(1.0, abs(R.from_sums(s, m, n, 6.0, True)))


# ---- 2. exact coverage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', [(130, 67, 33), (257, 300, 131), (1, 1, 5),
                                   (4100, 4000, 33)])          # 64 blocks, 33 steps in 32 splits: split 0 also takes the half step t = 32
def test_every_pair_counted_exactly_once(gpu, m, n, d):
    """sigma = 1e6 makes every kernel value exactly sum(wts) = 7: the sums are then pair counts"""
    from graphical_gan_amd import functional as F
    if d == 5:
        x, y = np.ones((1, 5), np.float32), np.full((1, 5), 2.0, np.float32)
    elif m > 1000:                   # (rows alone: the counts are closed-form, the float64 sums of _case are not needed)
        rng = np.random.default_rng(1000 * m + 10 * n + d)
        x, y = rng.standard_normal((m, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
    else:
        x, y, _ = _case(m, n, d)
    got = F.mix_rbf_sums(_t(x, gpu), _t(y, gpu), (1e6,) * 3, (1., 2., 4.)).cpu().numpy()
    assert got.tolist() == [7.0 * m * (m - 1), 7.0 * n * (n - 1), 7.0 * m * n], got


# ---- 3. same pointer -------------------------------------------------------------------------------------------------------------
def test_x_and_y_the_same_pointer(gpu):
    from graphical_gan_amd import functional as F
    from graphical_gan_amd import tflib as lib
    m, d = 130, 33
    x = _case(130, 67, 33)[0]
    tx = _t(x, gpu)
    w = (1., 2., 4., 1., .5, 3.)
    s = F.mix_rbf_sums(tx, tx, R.SIGMAS, w).cpu().numpy()
    ref = R.sums3(x, x, R.SIGMAS, w)
    assert abs((s[2] - s[0]) - m * sum(w)) <= 1e-3 * m * sum(w), s
    assert abs(R.from_sums(s, m, m, sum(w), True)) < 1e-5
    assert _gate(R.from_sums(s, m, m, sum(w), False), R.from_sums(ref, m, m, sum(w), False))
    assert abs(float(lib.objs.mmd.mix_rbf_mmd2(tx, tx, wts=w, biased=True))) < 1e-5            # (the fused op, as before)
    u = float(lib.objs.mmd.mix_rbf_mmd2(tx, tx, wts=w, biased=False))
    assert _gate(u, R.from_sums(ref, m, m, sum(w), False))


# ---- 4. repeatability ------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu):
    import torch
    from graphical_gan_amd import functional as F
    x, y, _ = _case(257, 300, 131)
    tx, ty = _t(x, gpu), _t(y, gpu)
    a = F.mix_rbf_sums(tx, ty, R.SIGMAS)
    junk = torch.full((1 << 16,), 3.0, device=gpu)               # (another allocation pattern in between)
    b = F.mix_rbf_sums(tx, ty, R.SIGMAS)
    del junk
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---- 5. the fused minibatch op -----------------------------------------------------------------------------------------------------
def test_agrees_with_the_fused_op(gpu):
    from graphical_gan_amd import functional as F
    from graphical_gan_amd import tflib as lib
    m = n = 64
    rng = np.random.default_rng(64 + 128)
    x, y = (rng.standard_normal((m, 128)) * 1.5).astype(np.float32), (rng.standard_normal((n, 128)) + 0.3).astype(np.float32)
    tx, ty = _t(x, gpu), _t(y, gpu)
    old = float(lib.objs.mmd.mix_rbf_mmd2(tx, ty))                                           # biased, m + n <= 512: the fused op
    new = float(F.mmd2_from_sums(F.mix_rbf_sums(tx, ty, R.SIGMAS), m, n, 6.0, True))
    assert _gate(new, old), (new, old)
    assert _gate(new, R.mmd2(x, y, biased=True))


# ---- 6. the differentiable unbiased estimator ----------------------------------------------------------------------------------------
def _raw_fused(gpu, tx, ty, gout):
    """the two EXISTING entry points, called directly: (value, dX, dY)"""
    import torch
    from graphical_gan_amd import _lib
    L = _lib.load()
    (m, d), n = tx.shape, ty.shape[0]
    sg = (C.c_float * 6)(*R.SIGMAS)
    out = torch.empty((), device=gpu)
    scratch = torch.empty((m + n,), device=gpu)
    dx, dy = torch.empty_like(tx), torch.empty_like(ty)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(L.ggan_mix_rbf_mmd2_fwd(p(tx), p(ty), m, n, d, sg, None, 6, p(out), p(scratch), st), 'fwd')
    _lib.check(L.ggan_mix_rbf_mmd2_bwd(p(tx), p(ty), m, n, d, sg, None, 6, p(gout), p(dx), p(dy), st), 'bwd')
    return out, dx, dy


@pytest.mark.parametrize('m,n,d', [(64, 64, 128), (5, 9, 16)])
def test_unbiased_estimator_is_differentiable_at_training_sizes(gpu, m, n, d):
    import torch
    from graphical_gan_amd import tflib as lib
    rng = np.random.default_rng(m + d)
    x, y = rng.standard_normal((m, d)) * 1.5, rng.standard_normal((n, d)) + 0.3
    # float64 reference: a CPU composition from direct differences, differentiated by torch.autograd
    X = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    Y = torch.tensor(y, dtype=torch.float64, requires_grad=True)

    def K(A, B):
        D = ((A[:, None, :] - B[None, :, :]) ** 2).sum(-1)
        return sum(torch.exp(-D / (2.0 * sg * sg)) for sg in R.SIGMAS)
    Kxx, Kyy, Kxy = K(X, X), K(Y, Y), K(X, Y)
    ref = ((Kxx.sum() - torch.trace(Kxx)) / (m * (m - 1)) + (Kyy.sum() - torch.trace(Kyy)) / (n * (n - 1)) - 2 * Kxy.sum() / (m * n))
    rx, ry = torch.autograd.grad(ref * 3.0, [X, Y])
    assert abs(float(ref.detach()) - R.mmd2(x, y, biased=False)) <= 1e-12
    # the existing biased op, recorded from its entry points BEFORE the new ones have run
    tx0, ty0 = _t(x, gpu), _t(y, gpu)
    three = torch.full((), 3.0, device=gpu)
    rec = [t.clone() for t in _raw_fused(gpu, tx0, ty0, three)]

    tx, ty = _t(x, gpu).requires_grad_(True), _t(y, gpu).requires_grad_(True)
    v = lib.objs.mmd.mix_rbf_mmd2(tx, ty, biased=False)
    assert v.requires_grad and v.dim() == 0
    print('unbiased', float(v.detach()), float(ref.detach()))
    assert _gate(float(v.detach()), float(ref.detach()))
    dx, dy = torch.autograd.grad(v * 3.0, [tx, ty])
    rel = lambda a, r: float((a.double().cpu() - r).abs().max() / (r.abs().max() + 1e-30))
    print(' grads', rel(dx, rx), rel(dy, ry))
    assert rel(dx, rx) < 1e-4 and rel(dy, ry) < 1e-4
    # one side only
    (dy1,) = torch.autograd.grad(lib.objs.mmd.mix_rbf_mmd2(tx.detach(), ty, biased=False) * 3.0, [ty])
    assert torch.equal(dy1, dy)
    # ... and the biased op still gives what its entry points gave: through the public route, and called directly again
    b = lib.objs.mmd.mix_rbf_mmd2(tx, ty)
    bx, by = torch.autograd.grad(b * 3.0, [tx, ty])
    again = _raw_fused(gpu, tx0, ty0, three)
    for got in ((b.detach(), bx, by), again):
        for a, r in zip(got, rec):
            assert torch.equal(a, r)
    assert _gate(float(b.detach()), R.mmd2(x, y, biased=True))
    assert abs(float(b.detach()) - float(v.detach())) > 1e-4                       # (two different estimators)


# ---- helpers: a small model with oracle weights ------------------------------------------------------------------------------------
def _fresh():
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd import optim
    optim.reset_optimizers()
    lib.delete_all_params()


def _model(gpu, dataset, B, K, mode, dim=8, dl=16):
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    from oracle import nets as N
    ocfg = N.Cfg(dataset, batch_size=B, n_coms=K, dim=dim, dim_latent=dl)
    P0 = N.init_params(ocfg, seed=0)
    rng = np.random.default_rng(7)
    for k in P0:
        if P0[k].ndim <= 2 and ('Biases' in k or k.endswith('.b') or 'offset' in k):
            P0[k] = (0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
        if k.endswith('.scale'):
            P0[k] = (1 + 0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
    _fresh()
    tr = Trainer(Config(dataset, batch_size=B, n_coms=K, mode=mode, dim=dim, dim_latent=dl), device=gpu, graph=False)
    tr.load_params(P0)
    return tr


def _snapshot(feed):
    import torch
    return {k: v.detach().cpu().numpy().tobytes() for k, v in feed.items() if torch.is_tensor(v)}


# ---- 7. the pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset,K,mode', [('cifar10', 5, 'local_ep'), ('mnist', 0, 'ali')])
def test_mmd_scores_sets_values_and_an_untouched_trainer(gpu, dataset, K, mode):
    import torch
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 4
    tr = _model(gpu, dataset, B, K, mode)
    rng = np.random.default_rng(21)
    if dataset == 'mnist':
        xs = [rng.random((B, 784), dtype=np.float32) for _ in range(n)]
    else:
        xs = [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]
    dev = [(x, np.zeros(B, np.int64)) for x in xs] + [(xs[0][:B - 1], np.zeros(B - 1))]          # (a partial minibatch: dropped)
    ev = Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K), keep_noise=True)
    tr.model.sample_noise(tr.feed)                 # (the Trainer's buffers hold something to compare)
    torch.cuda.synchronize()
    before = _snapshot(tr.feed)
    assert 'rng_state' in before
    res, sets = ev.mmd_scores(dev, return_sets=True)
    torch.cuda.synchronize()
    assert _snapshot(tr.feed) == before            # feed buffers and noise state: byte for byte
    assert tr.feed['rng_state'].data_ptr() != ev.feed['rng_state'].data_ptr()
    assert sorted(res) == ['dev mmd x', 'dev mmd z'] and all(isinstance(v, float) for v in res.values())
    c = tr.cfg
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z=(n * B, c.dim_latent), pz=(n * B, c.dim_latent),
                                                                 x=(n * B, c.output_dim), gx=(n * B, c.output_dim))
    assert all(v.is_cuda for v in sets.values())
    host = {k: v.cpu().numpy() for k, v in sets.items()}
    for name, a, b in (('dev mmd z', 'z', 'pz'), ('dev mmd x', 'x', 'gx')):
        ref = R.mmd2(host[a], host[b], biased=False)
        print(name, res[name], ref)
        assert _gate(res[name], ref), (name, res[name], ref)
    # the sets are what the nets give on each minibatch (per-minibatch BatchNorm statistics), rebuilt here on a feed of the test's own
    feed = tr.model.feed_buffers(gpu)
    with torch.no_grad(), tr.model.single_stream():
        for i in range(n):
            rows = slice(i * B, (i + 1) * B)
            tr.model.set_batch(feed, torch.as_tensor(xs[i]).to(gpu))
            real_x = tr.model.real_x(feed)
            assert torch.equal(sets['x'][rows], real_x.float())
            assert torch.equal(sets['z'][rows], tr.model.Extractor(real_x))
            assert torch.equal(sets['gx'][rows], tr.model.Generator(sets['pz'][rows].clone()).float())
            kept = ev.kept[i]
            if K:
                pz = tr.model.HyperGenerator(torch.as_tensor(kept['k_onehot']).to(gpu), torch.as_tensor(kept['p_z_noise']).to(gpu))
                assert torch.equal(sets['pz'][rows], pz)
            else:
                assert np.array_equal(host['pz'][rows], kept['p_z_noise'])
    assert len(ev.kept) == n and not np.array_equal(host['pz'][:B], host['pz'][B:2 * B])         # fresh prior draws per minibatch
    # MMD_MAX_ROWS caps the sets at whole minibatches
    ev2 = Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, MMD_MAX_ROWS=2 * B + 3))
    res2, capped = ev2.mmd_scores(dev, return_sets=True)
    assert capped['z'].shape[0] == 2 * B and sorted(res2) == sorted(res)
    assert sorted(ev2.mmd_scores(dev)) == sorted(res)                 # (without the sets: the dict alone)


# ---- 8. training unaffected ------------------------------------------------------------------------------------------------------
def _data_on_disk(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    mk = lambda n: (rng.random((n, 784), dtype=np.float32), rng.integers(0, 10, size=n))
    with gzip.open(str(tmp_path / 'mnist.pkl.gz'), 'wb') as f:
        pickle.dump((mk(64), mk(24), mk(20)), f)
    monkeypatch.setenv('GGAN_MNIST', str(tmp_path / 'mnist.pkl.gz'))
    for i in list(range(1, 6)) + ['t']:
        name = 'test_batch' if i == 't' else 'data_batch_%d' % i
        with open(str(tmp_path / name), 'wb') as f:
            pickle.dump({'data': rng.integers(0, 256, size=(16, 3072)).astype(np.uint8), 'labels': list(rng.integers(0, 10, size=16))}, f)


def _train(S, cfg):
    from graphical_gan_amd import run, optim
    from graphical_gan_amd import tflib as lib
    _fresh()
    seen = []
    orig = lib.plot.plot
    it0 = lib.plot._iter[0]

    def rec(name, value):
        seen.append((name, lib.plot._iter[0] - it0, float(value)))
        orig(name, value)
    lib.plot.plot = rec
    try:
        tr = run.train(S, cfg)
    finally:
        lib.plot.plot = orig
    w = tr.get_params()
    adam = {}
    for key, o in optim._optimizers.items():
        adam[key[0]] = (o.step.cpu().numpy().copy(), o.m.cpu().numpy().copy(), o.v.cpu().numpy().copy())
    return tr, w, adam, seen


@pytest.mark.parametrize('dataset', ['cifar10', 'mnist'])
def test_training_bit_identical_with_the_mmd_pass(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    _data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=6, LOG_EVERY=3, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = _train(dict(base), cfg())
    tr1, w1, a1, seen1 = _train(dict(base, MMD_EVERY=2), cfg())
    if dataset == 'cifar10':    # (int32 loader data: the host-fed ring and one graph replay per iteration, with the pass in between)
        assert getattr(tr1, '_feeder', None) is not None and tr1._iter_graph is not None
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    train_keys = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev ') and n != 'time']
    assert train_keys(seen0) == train_keys(seen1)            # the logged training costs too
    at = lambda name: [i for n, i, _ in seen1 if n == name]
    assert at('dev mmd z') == [1, 3, 5] and at('dev mmd x') == [1, 3, 5]
    assert all(np.isfinite(v) for n, _, v in seen1 if n.startswith('dev mmd'))
    assert not [n for n, _, _ in seen0 if n.startswith('dev ')]
    assert not [n for n, _, _ in seen1 if n.startswith('dev ') and not n.startswith('dev mmd')]      # (no other pass was switched on)


# ---- 9. CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_two_rows_of_the_live_evaluator(gpu, tmp_path, monkeypatch, capsys):
    from graphical_gan_amd import checkpoint, run, evaluate
    from graphical_gan_amd.evaluate import Evaluator
    from graphical_gan_amd.engine import Trainer
    _data_on_disk(tmp_path, monkeypatch)
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=5, BATCH_SIZE=8)
    S = run.reference_block('gmgan_inference_mnist', **over)
    _fresh()
    tr = Trainer(run.config(S), device=gpu, graph=False)
    for it in range(2):
        tr.iteration(it, iter(tr.model.synthetic_ring(gpu, n=4) * 2))
    ckpt = str(tmp_path / 'params_2.npz')
    checkpoint.save(ckpt, tr)
    np.random.seed(5)
    dev, test = run.eval_sets(S, tr.model, gpu)
    ev = Evaluator(tr, S)                          # the passes in evaluate_once's order: they share ONE stream of noise draws
    ev.dev_costs(dev)
    ev.cluster_accuracy(test)
    live = ev.mmd_scores(dev)
    _fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--mmd'])
    out = capsys.readouterr().out
    assert res['dev mmd z'] == live['dev mmd z'] and res['dev mmd x'] == live['dev mmd x']
    for k in ('dev mmd z', 'dev mmd x'):
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    _fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if not k.startswith('dev mmd'))
    assert all(plain[k] == res[k] for k in plain)
