"""-m gpu: the k-NN-ball ops (csrc/knn_sets.hip: functional.knn_radii / ball_counts / prdc) against the float64 direct-difference
restatement tests/_prdc_ref.py -- radii, self-exclusion by index, exactness and ties on an integer lattice, exact pair coverage, count
brackets, the four scores end to end, repeatability --, and the dev-set precision / recall / density / coverage pass: its values, the
Trainer it leaves untouched, the sets it shares with the MMD pass, the training it does not change, the CLI.

Tolerance (derived in _prdc_ref, not measured): a float32 Gram-form distance is within T_ij = (2 d + 4) 2^-23 (|a_i|^2 + |b_j|^2) of the
exact one, a k-th order statistic moves by at most the largest perturbation of its row; counts are bracketed by the pairs at least /
at most that far inside their ball, and a row whose bracket is closed must match exactly (test_prdc_cpu asserts how few are open)."""
import gzip
import os
import pickle
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _prdc_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ['dev %s %s' % (what, space) for space in ('z', 'x') for what in ('precision', 'recall', 'density', 'coverage')]


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32), device=dev)          # (a copy: the shared cases are read-only)


def _rows(n, d):
    """a set of n rows of width d out of the shared cases"""
    if (n, d) == (2, 1):
        return np.array([[0.5], [2.0]], np.float32)
    return {(9, 16): R.case(5, 9, 16)[1], (130, 33): R.case(130, 67, 33)[0], (300, 131): R.case(257, 300, 131)[1],
            (192, 3072): R.case(192, 160, 3072)[0]}[(n, d)]


def _inside(got, b):
    return all(lo <= g <= hi for g, lo, hi in zip(got, b['lo'], b['hi']))


# ---- 1. radii --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d,ks', [(2, 1, (1,)),                 # minimum
                                    (9, 16, (1, 3)),              # a ragged tile
                                    (130, 33, (1, 3, 5)),         # the row-block boundary at 128; rows that are not 16-byte aligned
                                    (300, 131, (1, 5, 8)),        # several candidate blocks and splits; the longest list
                                    (192, 3072, (3,))])           # the long k loop
def test_radii_against_float64(gpu, n, d, ks):
    from graphical_gan_amd import functional as F
    Z = _rows(n, d)
    D, T = R.d2(Z, Z), R.tol(Z, Z).max(1)
    tz = _t(Z, gpu)
    for k in ks:
        got = F.knn_radii(tz, k)
        assert got.is_cuda and str(got.dtype) == 'torch.float32' and tuple(got.shape) == (n,)
        g = got.cpu().numpy().astype(np.float64)
        ref = R.radii_from(D, k)
        print('radii', (n, d, k), 'max err', np.abs(g - ref).max(), 'bound', T.max(), 'rel', (np.abs(g - ref) / T).max())
        assert np.all(np.isfinite(g)) and np.all(g >= 0)
        assert np.all(np.abs(g - ref) <= T), (k, np.abs(g - ref).max())


# ---- 2. self-exclusion by index -----------------------------------------------------------------------------------------------------
def test_self_left_out_by_index_duplicates_count(gpu):
    from graphical_gan_amd import functional as F
    Z = np.array(_rows(130, 33))
    Z[129] = Z[0]                     # (another row block)
    Z[5] = Z[0]
    D, T = R.d2(Z, Z), R.tol(Z, Z).max(1)
    tz = _t(Z, gpu)
    for k in (1, 2):
        g = F.knn_radii(tz, k).cpu().numpy().astype(np.float64)
        ref = R.radii_from(D, k)
        assert all(ref[i] == 0.0 for i in (0, 5, 129))
        assert all(0.0 <= g[i] <= T[i] for i in (0, 5, 129)), (k, g[[0, 5, 129]])          # the two twins, not the row itself
        assert np.all(np.abs(g - ref) <= T)
    g, ref = F.knn_radii(tz, 3).cpu().numpy().astype(np.float64), R.radii_from(D, 3)
    assert all(ref[i] > 100 * T[i] for i in (0, 5, 129))                                  # (a real neighbour: far outside the tolerance)
    assert np.all(np.abs(g - ref) <= T)


# ---- 3. exactness on a lattice --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', [(130, 67, 33), (257, 300, 16),
                                   (5800, 5800, 16)])           # 46 blocks each way in 45 splits: split 0 walks a second, ragged tile
def test_integer_lattice_is_exact_ties_included(gpu, m, n, d):
    """integer entries: every product and sum is exact in float32, so everything must EQUAL the reference -- the test of `<=` at a tie and
    of the multiset rule (equal distances are plentiful)"""
    from graphical_gan_amd import functional as F
    X, Y = R.lattice(m, n, d)
    k = 3
    tx, ty = _t(X, gpu), _t(Y, gpu)
    r_x, r_y = R.radii(X, k), R.radii(Y, k)
    assert np.array_equal(F.knn_radii(tx, k).cpu().numpy().astype(np.float64), r_x)
    assert np.array_equal(F.knn_radii(ty, k).cpu().numpy().astype(np.float64), r_y)
    Dxy = R.d2(X, Y)
    assert np.any(Dxy == r_y[None, :]) and np.any(Dxy.T == r_x[None, :])                 # the reference sees exact ties at the threshold
    for A, B, rB, ta, tb in ((Y, X, r_x, ty, tx), (X, Y, r_y, tx, ty)):
        cnt, mn = F.ball_counts(ta, tb, _t(rB, gpu))
        rc, rm = R.ball_counts(A, B, rB)
        assert str(cnt.dtype) == 'torch.int32' and str(mn.dtype) == 'torch.float32'
        assert np.array_equal(cnt.cpu().numpy(), rc) and np.array_equal(mn.cpu().numpy().astype(np.float64), rm)
    got = F.prdc(tx, ty, k).cpu().numpy()
    assert tuple(got.tolist()) == R.prdc(X, Y, k), (got, R.prdc(X, Y, k))


# ---- 4. every pair seen exactly once ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', [(130, 67, 33), (257, 300, 131), (1, 1, 5), (5800, 5800, 16)])          # (the last: two tiles per workgroup)
def test_every_pair_seen_exactly_once(gpu, m, n, d):
    import torch
    from graphical_gan_amd import functional as F
    A, B = (np.ones((1, 5), np.float32), np.full((1, 5), 2.0, np.float32)) if d == 5 else R.case(m, n, d)
    ta, tb = _t(A, gpu), _t(B, gpu)
    for a, b in ((ta, tb), (tb, ta)):
        cnt, _ = F.ball_counts(a, b, torch.full((b.shape[0],), 3e38, device=gpu))
        assert cnt.cpu().tolist() == [b.shape[0]] * a.shape[0]
        cnt, _ = F.ball_counts(a, b, torch.full((b.shape[0],), -1.0, device=gpu))
        assert cnt.cpu().tolist() == [0] * a.shape[0]


# ---- 5. counts and minima against the reference's radii ----------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', R.CASES)
def test_ball_counts_inside_their_brackets(gpu, m, n, d):
    from graphical_gan_amd import functional as F
    X, Y = R.case(m, n, d)
    Dxx, Dyy, Dxy = R.case_d2(m, n, d)
    k = 3
    Txy = R.tol(X, Y)
    for A, B, D, rB, T in ((Y, X, Dxy.T, R.radii_from(Dxx, k), Txy.T), (X, Y, Dxy, R.radii_from(Dyy, k), Txy)):
        r32 = rB.astype(np.float32)
        lo, hi, rm = R.count_brackets(D, rB, T + R.U * rB[None, :])
        cnt, mn = F.ball_counts(_t(A, gpu), _t(B, gpu), _t(r32, gpu))
        cnt, mn = cnt.cpu().numpy(), mn.cpu().numpy().astype(np.float64)
        print('counts', (A.shape[0], B.shape[0], d), 'open brackets', int(np.sum(lo != hi)), 'min err / bound', (np.abs(mn - rm) / T.max(1)).max())
        assert np.all(lo <= cnt) and np.all(cnt <= hi), np.flatnonzero((cnt < lo) | (cnt > hi))
        assert np.all(np.abs(mn - rm) <= T.max(1))
        assert 0 < cnt.sum() < cnt.size * B.shape[0]                                        # (neither trivial end)


# ---- 6. the four scores end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', R.CASES)
def test_prdc_end_to_end(gpu, m, n, d):
    from graphical_gan_amd import functional as F
    X, Y = R.case(m, n, d)
    tx, ty = _t(X, gpu), _t(Y, gpu)
    for k in (1, 3, 5):
        if k > min(m, n) - 1:
            continue
        got = F.prdc(tx, ty, k)
        assert got.is_cuda and str(got.dtype) == 'torch.float64' and tuple(got.shape) == (4,)
        got = got.cpu().tolist()
        b = R.score_brackets(X, Y, k, doubled=True, D=R.case_d2(m, n, d))
        print('prdc', (m, n, d, k), got, b['lo'], b['hi'])
        assert _inside(got, b), (k, got, b['lo'], b['hi'])


# ---- 7. repeatability --------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu):
    import torch
    from graphical_gan_amd import functional as F
    X, Y = R.case(257, 300, 131)
    tx, ty = _t(X, gpu), _t(Y, gpu)
    r = F.knn_radii(tx, 5)

    def run():
        cnt, mn = F.ball_counts(ty, tx, r)
        return [v.cpu().numpy().tobytes() for v in (F.knn_radii(tx, 5), cnt, mn, F.prdc(tx, ty, 5))]
    a = run()
    junk = torch.full((1 << 16,), 3.0, device=gpu)               # (another allocation pattern in between)
    b = run()
    del junk
    assert a == b


# ---- helpers: a small model with oracle weights (as tests/test_mmd_sets_gpu.py) --------------------------------------------------------
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


# ---- 8. the pass -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset,K,mode', [('cifar10', 5, 'local_ep'), ('mnist', 0, 'ali')])
def test_prdc_scores_values_shared_sets_and_an_untouched_trainer(gpu, dataset, K, mode):
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
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    ev = Evaluator(tr, S, keep_noise=True)
    tr.model.sample_noise(tr.feed)                 # (the Trainer's buffers hold something to compare)
    torch.cuda.synchronize()
    before = _snapshot(tr.feed)
    assert 'rng_state' in before
    res, sets = ev.prdc_scores(dev, return_sets=True)
    torch.cuda.synchronize()
    assert _snapshot(tr.feed) == before            # feed buffers and noise state: byte for byte
    assert list(res) == KEYS and all(isinstance(v, float) for v in res.values())
    c = tr.cfg
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z=(n * B, c.dim_latent), pz=(n * B, c.dim_latent),
                                                                 x=(n * B, c.output_dim), gx=(n * B, c.output_dim))
    assert len(ev.kept) == n
    host = {k: v.cpu().numpy() for k, v in sets.items()}
    for space, a, b in (('z', 'z', 'pz'), ('x', 'x', 'gx')):
        br = R.score_brackets(host[a], host[b], 5, doubled=True)
        got = [res['dev %s %s' % (what, space)] for what in ('precision', 'recall', 'density', 'coverage')]
        print(dataset, space, got, br['lo'], br['hi'])
        assert _inside(got, br), (space, got, br['lo'], br['hi'])
    # PRDC_K reaches the op; PRDC_MAX_ROWS caps the sets at whole minibatches
    ev2 = Evaluator(tr, dict(S, PRDC_MAX_ROWS=2 * B + 3, PRDC_K=2))
    res2, capped = ev2.prdc_scores(dev, return_sets=True)
    assert capped['z'].shape[0] == 2 * B and list(res2) == KEYS
    hc = {k: v.cpu().numpy() for k, v in capped.items()}
    assert _inside([res2['dev %s z' % w] for w in ('precision', 'recall', 'density', 'coverage')], R.score_brackets(hc['z'], hc['pz'], 2))
    assert list(ev2.prdc_scores(dev)) == KEYS                          # (without the sets: the dict alone)
    # both passes at once: ONE build of the sets, no noise draws beyond those of the MMD pass alone, and its two values unchanged
    alone, both = Evaluator(tr, S, keep_noise=True), Evaluator(tr, S, keep_noise=True)
    assert _snapshot(alone.feed)['rng_state'] == _snapshot(both.feed)['rng_state']
    mmd_alone, sets_alone = alone.mmd_scores(dev, return_sets=True)
    builds, build = [], both._score_sets
    both._score_sets = lambda *a, **kw: (builds.append(1), build(*a, **kw))[1]
    res_both, sets_both = both.set_scores(dev, mmd=True, prdc=True, return_sets=True)
    assert len(builds) == 1 and len(both.kept) == n
    assert list(res_both) == ['dev mmd z', 'dev mmd x'] + KEYS
    assert all(res_both[k] == mmd_alone[k] for k in mmd_alone)
    assert _snapshot(alone.feed)['rng_state'] == _snapshot(both.feed)['rng_state']
    assert all(torch.equal(sets_alone[k], sets_both[k]) for k in sets_alone)
    prdc_alone = Evaluator(tr, S).prdc_scores(dev)                    # ... and the eight values are those of the PRDC pass alone
    assert all(res_both[k] == prdc_alone[k] for k in KEYS)
    assert _snapshot(tr.feed) == before


# ---- 9. training unaffected ------------------------------------------------------------------------------------------------------
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
def test_training_bit_identical_with_the_prdc_pass(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    _data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=6, LOG_EVERY=3, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = _train(dict(base), cfg())
    tr1, w1, a1, seen1 = _train(dict(base, PRDC_EVERY=2), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    train_keys = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev ') and n != 'time']
    assert train_keys(seen0) == train_keys(seen1)            # the logged training costs too
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [1, 3, 5], key
    assert all(np.isfinite(v) and 0.0 <= v for n, _, v in seen1 if n in KEYS)
    assert not [n for n, _, _ in seen0 if n.startswith('dev ')]
    assert not [n for n, _, _ in seen1 if n.startswith('dev ') and n not in KEYS]      # (no dev mmd, no other pass was switched on)


# ---- 10. CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_eight_rows_of_the_live_evaluator(gpu, tmp_path, monkeypatch, capsys):
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
    live = ev.set_scores(dev, mmd=True, prdc=True)
    _fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--mmd', '--prdc'])
    out = capsys.readouterr().out
    for k in ['dev mmd z', 'dev mmd x'] + KEYS:
        assert res[k] == live[k], k
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    _fresh()
    np.random.seed(5)
    only = evaluate.main(args + ['--prdc'])        # the same sets either way: the eight values do not depend on the MMD flag
    assert [k for k in only if k.startswith('dev ') and (k in KEYS or 'mmd' in k)] == KEYS
    assert all(only[k] == live[k] for k in KEYS)
    _fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in only if k not in KEYS)
    assert all(plain[k] == only[k] for k in plain)
