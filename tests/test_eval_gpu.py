"""-m gpu: the evaluation passes (graphical_gan_amd/evaluate.py) on the HIP path -- the posterior / clustering-accuracy kernels against
a float64 restatement, dev costs and the sample grid against the oracle on the same weights, batches and noise, training left
bit-identical by passes run in the middle of it, and the checkpoint CLI."""
import gzip
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _fresh():
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd import optim
    optim.reset_optimizers()
    lib.delete_all_params()


# ---- 1. kernel parity ------------------------------------------------------------------------------------------------------------
def _posterior_case(K, B, D, seed):
    rng = np.random.default_rng(seed)
    N = 3 * B + 7                                   # not a multiple of B: the last launch has 7 rows
    s = np.float32(np.sqrt(10.0 / D))               # logits O(10)
    mu = (s * rng.standard_normal((K, D))).astype(np.float32)
    z = (s * rng.standard_normal((N, D))).astype(np.float32)
    mu[0] += 2.0                                     # a far component: rows sitting on it saturate (p = 1.0 exactly)
    z[[3, 11, B + 1]] = mu[0]
    z[[5, B + 2, 2 * B + 4]] = z[1]                 # duplicated rows: equal probabilities in every column
    return z, mu


@pytest.mark.parametrize('K,B', [(5, 50), (30, 64), (50, 50), (8192, 64)])
def test_posterior_assign_and_accuracy_kernels(gpu, K, B):
    import torch
    from graphical_gan_amd import functional as F, _lib
    from graphical_gan_amd import evaluate as E
    assert K <= _lib.POSTERIOR_MAX_K
    D = 128
    z, mu = _posterior_case(K, B, D, K + B)
    N = z.shape[0]
    log_pi = float(np.log(np.float32(1.0) / np.float32(K)))
    zt, mt = torch.as_tensor(z, device=gpu), torch.as_tensor(mu, device=gpu)
    assign = torch.full((N,), -1, dtype=torch.int32, device=gpu)
    colbest = torch.zeros((K,), dtype=torch.int64, device=gpu)
    probs = torch.empty((N, K), dtype=torch.float32, device=gpu)
    for r0 in range(0, N, B):
        r1 = min(N, r0 + B)
        F.gmm_posterior_assign_(zt[r0:r1], mt, log_pi, r0, assign, colbest, probs[r0:r1])
    labels = np.random.default_rng(1).integers(0, 10, size=N).astype(np.int32)
    correct = torch.zeros((1,), dtype=torch.int32, device=gpu)
    F.cluster_accuracy_(assign, torch.as_tensor(labels, device=gpu), colbest, correct)
    torch.cuda.synchronize()
    P = probs.cpu().numpy()
    A = assign.cpu().numpy()
    keys = colbest.cpu().numpy().view(np.uint64)
    # float64 softmax of the logits
    lg = -0.5 * ((z.astype(np.float64)[:, None, :] - mu.astype(np.float64)[None]) ** 2).sum(-1) + log_pi
    P64 = np.exp(lg - lg.max(1, keepdims=True))
    P64 /= P64.sum(1, keepdims=True)
    assert np.abs(P - P64).max() <= 1e-5
    srt = np.sort(P64, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 1e-5
    assert clear.sum() >= N // 2
    assert (A[clear] == np.argmax(P64, axis=1)[clear]).all()
    assert (A == np.argmax(P, axis=1)).all()                      # first index on the kernel's own ties
    # column argmax: exactly np.argmax over the kernel's own fp32 probabilities, lowest row on ties
    assert P[3, 0] == 1.0 and P[11, 0] == 1.0                     # (saturated rows: a tie at p = 1.0)
    assert (keys == E.column_keys(P)).all()
    rows = (0xFFFFFFFF - (keys & np.uint64(0xFFFFFFFF))).astype(np.int64)
    assert (rows == np.argmax(P, axis=0)).all() and rows[0] == 3
    # the match count: the host restatement of the reference's loop, exactly
    c = int(correct.cpu().numpy()[0])
    assert c == E.decode_cluster_accuracy(A, labels, keys)
    if K <= 1000:           # (beyond, the reference loop's +1000 relabelling collides with cluster indices: evaluate.host_cluster_accuracy)
        assert np.float32(c / float(N)) == np.float32(E.host_cluster_accuracy(P, labels))


def test_all_zero_column_decodes_to_row_zero(gpu):
    """a component whose probabilities all underflow to 0.0f labels itself with row 0's label (np.argmax of an all-zero column)"""
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd import evaluate as E
    K, D, N = 4, 8, 20
    mu = np.zeros((K, D), np.float32)
    mu[3] = 100.0                                    # nothing comes near component 3: exp(-.5 * 8e4) == 0 in fp32
    z = np.random.default_rng(0).standard_normal((N, D)).astype(np.float32) * 0.1
    assign = torch.empty((N,), dtype=torch.int32, device=gpu)
    colbest = torch.zeros((K,), dtype=torch.int64, device=gpu)
    probs = torch.empty((N, K), dtype=torch.float32, device=gpu)
    F.gmm_posterior_assign_(torch.as_tensor(z, device=gpu), torch.as_tensor(mu, device=gpu), 0.0, 0, assign, colbest, probs)
    labels = (np.arange(N) % 3).astype(np.int32) + 5
    correct = torch.zeros((1,), dtype=torch.int32, device=gpu)
    F.cluster_accuracy_(assign, torch.as_tensor(labels, device=gpu), colbest, correct)
    P, keys = probs.cpu().numpy(), colbest.cpu().numpy().view(np.uint64)
    assert (P[:, 3] == 0).all()
    assert int(0xFFFFFFFF - (int(keys[3]) & 0xFFFFFFFF)) == 0
    assert int(correct.cpu().numpy()[0]) == E.decode_cluster_accuracy(assign.cpu().numpy(), labels, keys)
    assert np.float32(int(correct.cpu().numpy()[0]) / N) == np.float32(E.host_cluster_accuracy(P, labels))


# ---- helpers: a small model with oracle weights ----------------------------------------------------------------------------------
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
    return ocfg, P0, tr


def _images(dataset, n, B, rng):
    if dataset == 'mnist':
        return [rng.random((B, 784), dtype=np.float32) for _ in range(n)]
    return [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]


# ---- 2. dev costs ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset,K,mode', [('mnist', 4, 'local_ep'), ('cifar10', 5, 'local_epce'), ('cifar10', 0, 'ali'),
                                            ('cifar10', 0, 'alice')])
def test_dev_costs_match_oracle(gpu, dataset, K, mode):
    from graphical_gan_amd.evaluate import Evaluator
    from oracle import step as S, tape as tp, nets as N, objs as OJ
    B = 6 if dataset == 'mnist' else 8
    ocfg, P0, tr = _model(gpu, dataset, B, K, mode)
    rng = np.random.default_rng(11)
    xs = _images(dataset, 3, B, rng)
    dev = [(x, np.zeros(B, np.int64)) for x in xs] + [(xs[0][:B - 1], np.zeros(B - 1))]     # (a partial minibatch: dropped)
    ev = Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K), keep_noise=True)
    res = ev.dev_costs(dev)
    assert len(ev.kept) == 3
    gens, recs = [], []
    for x, kept in zip(xs, ev.kept):
        feed = {('real_x' if dataset == 'mnist' else 'real_x_int'): x, 'p_z_noise': kept['p_z_noise']}
        if K:
            feed['k_idx'] = np.argmax(kept['k_onehot'], axis=1)
            feed['gumbel_u'] = kept['gumbel_u']
        Pt = {k: tp.T(np.asarray(v, np.float64)) for k, v in P0.items()}
        out = S.forward(ocfg, Pt, feed, mode)
        gens.append(float(out['gen_cost'].v))
        if mode in ('local_epce', 'alice'):          # (step.forward folds the penalty into gen_cost: restated as it builds it)
            r = OJ.distance(out['real_x'], N.Generator(ocfg, Pt, out['q_z']), 'l2')
            if mode == 'alice':
                r = tp.add(r, OJ.distance(out['p_z'], N.Extractor(ocfg, Pt, out['fake_x']), 'l2'))
            recs.append(float(r.v))
    rel = lambda a, b: abs(a - b) / max(1e-6, abs(b))
    assert rel(res['dev gen cost'], np.mean(gens)) <= 5e-5, (res, np.mean(gens))
    if mode in ('local_epce', 'alice'):
        assert rel(res['dev rec cost'], np.mean(recs)) <= 5e-5
        assert rel(res['dev reg cost'], np.mean(gens) - np.mean(recs)) <= 5e-5
    else:
        assert 'dev rec cost' not in res
    # fresh noise per dev batch, and a noise state of the evaluator's own
    assert not np.array_equal(ev.kept[0]['p_z_noise'], ev.kept[1]['p_z_noise'])
    assert tr.feed['rng_state'].data_ptr() != ev.feed['rng_state'].data_ptr()


# ---- 3. training unaffected ------------------------------------------------------------------------------------------------------
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
def test_training_bit_identical_with_eval_passes(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    _data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=8, LOG_EVERY=4, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = _train(dict(base), cfg())
    if dataset == 'cifar10':    # (int32 loader data: the host-fed ring and one graph replay per iteration)
        assert getattr(tr0, '_feeder', None) is not None and tr0._iter_graph is not None
    out = tmp_path / 'out'
    tr1, w1, a1, seen1 = _train(dict(base, DEV_EVERY=2, ACCURACY_EVERY=3, SAMPLE_EVERY=4, OUT_DIR=str(out)), cfg())
    if dataset == 'cifar10':
        assert getattr(tr1, '_feeder', None) is not None and tr1._iter_graph is not None
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    train_keys = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith(('dev ', 'testing ')) and n != 'time']
    assert train_keys(seen0) == train_keys(seen1)            # the logged training costs too
    at = lambda name: [i for n, i, _ in seen1 if n == name]
    assert at('dev gen cost') == [1, 3, 5, 7]
    assert at('testing accuracy') == [2, 5]
    assert all(0.0 <= v <= 1.0 for n, _, v in seen1 if n == 'testing accuracy')
    assert not [n for n, _, _ in seen0 if n.startswith(('dev ', 'testing '))]
    pngs = sorted(p.name for p in out.iterdir() if p.suffix == '.png')
    assert '3_samples_local_ep.png' in pngs and '7_samples_local_ep.png' in pngs, pngs


# ---- 4. grid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset,K,n_vis', [('cifar10', 5, 50), ('mnist', 5, 500)])
def test_sample_grid_matches_oracle(gpu, dataset, K, n_vis, tmp_path):
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd.evaluate import Evaluator
    from oracle import nets as N, tape as tp
    ocfg, P0, tr = _model(gpu, dataset, 8, K, 'local_ep')
    ev = Evaluator(tr, dict(BATCH_SIZE=8, MODE='local_ep', N_COMS=K, N_VIS=n_vis))
    if n_vis > 128:          # (the fused Generator head takes at most 128 rows: the Linear + Batchnorm fallback runs)
        from graphical_gan_amd import tflib as lib
        w = lib.param('Generator.Input.W')
        assert not F.LinearBatchNormRows.usable(torch.zeros((n_vis, 16), device=gpu), w)
    grid = ev.sample_grid()
    assert grid.shape == (n_vis, ocfg.output_dim)
    Pt = {k: tp.T(np.asarray(v, np.float64)) for k, v in P0.items()}
    noise = ev.fixed_noise.cpu().numpy().astype(np.float64)
    onehot = np.tile(np.eye(K), (n_vis // K, 1))
    ref = N.Generator(ocfg, Pt, N.HyperGenerator(ocfg, Pt, tp.T(onehot), tp.T(noise))).v
    assert np.abs(grid - ref).max() <= 1e-5, np.abs(grid - ref).max()
    cols = grid.reshape(n_vis // K, K, -1)
    for j in range(K):                # column j of the saved grid: component j
        assert np.array_equal(cols[:, j], grid[j::K])
    paths = ev.save_images(str(tmp_path), 9)
    assert paths[0].endswith('9_samples_local_ep.png')
    # the fixed noise is drawn once: a second grid is the same
    assert np.array_equal(ev.sample_grid(), grid)


# ---- 5. CLI ----------------------------------------------------------------------------------------------------------------------
def test_cli_scores_a_checkpoint_as_the_live_evaluator(gpu, tmp_path, monkeypatch):
    from graphical_gan_amd import checkpoint, run, evaluate
    from graphical_gan_amd.evaluate import Evaluator
    _data_on_disk(tmp_path, monkeypatch)
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=5, BATCH_SIZE=8)
    S = run.reference_block('gmgan_inference_mnist', **over)
    _fresh()
    from graphical_gan_amd.engine import Trainer
    tr = Trainer(run.config(S), device=gpu, graph=False)
    for it in range(3):          # (a few steps on synthetic minibatches: the optimizers exist, the weights moved)
        tr.iteration(it, iter(tr.model.synthetic_ring(gpu, n=4) * 2))
    ckpt = str(tmp_path / 'params_3.npz')
    checkpoint.save(ckpt, tr)
    np.random.seed(5)
    _, test = run.eval_sets(S, tr.model, gpu)
    live = Evaluator(tr, S).cluster_accuracy(test)
    _fresh()
    np.random.seed(5)
    res = evaluate.main([ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()])
    assert res['testing accuracy'] == live
    assert 'dev gen cost' in res and np.isfinite(res['dev gen cost'])
