"""gpu: the sliced Wasserstein distance on the device against the float64 reference tests/_swd_ref.py over its grid -- the op on given projections
(gate a), the whole op through the projection (gate b) --, the bitwise properties, non-finite input as a status, the pass
Evaluator.swd_scores on sets rebuilt here from the same seeds, run.train with the pass switched on beside `dev mmd`, and the CLI."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _swd_ref as R  # noqa: E402
import test_mmd_sets_gpu as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a)).to(dev)


def _bits(*tensors):
    return b''.join(t.cpu().numpy().tobytes() for t in tensors)


# ---- gate (a): the op on given projections ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_the_op_on_given_projections_against_the_reference(gpu, kind):
    """sliced_wasserstein_projected against the float64 reference on the same float32 arrays, over the whole grid and both exponents:
    |per - ref| <= (m + n + 4) 2^-52 ref and exactly 0 where ref is 0 -- derived, not measured: the differences are exact in fp64 and
    every term is nonnegative, so the fp64 sum of at most m + n terms is off by at most that many roundings --; values within the same
    bound plus one rounding of the root; values[0] <= values[1]; status 0; two calls give the same bits"""
    from graphical_gan_amd import functional as F
    worst, worst_v = 0.0, 0.0
    for k, m, n, L in R.cases((kind,)):
        x, y = R.sets(k, m, n, L)
        xd = _t(x, gpu)
        yd = xd if y is x else _t(y, gpu)
        for p in R.PS:
            rv, rper = R.case_reference(k, m, n, L, p)
            v, per, st = F.sliced_wasserstein_projected(xd, yd, p)
            v2, per2, st2 = F.sliced_wasserstein_projected(xd, yd, p)
            assert v.dtype.is_floating_point and v.element_size() == 8 and tuple(v.shape) == (2,) and tuple(per.shape) == (L,) and per.element_size() == 8
            assert tuple(st.shape) == (1,) and st.element_size() == 4 and not st.dtype.is_floating_point
            assert _bits(v, per, st) == _bits(v2, per2, st2), (R.case_id(k, m, n, L), p)
            v, per = v.cpu().numpy(), per.cpu().numpy()
            ident = (R.case_id(k, m, n, L), p)
            assert int(st.item()) == 0, ident
            err = np.abs(per - rper)
            assert np.all(per[rper == 0] == 0) and np.all(err <= R.per_bound(m, n) * rper), (ident, float(np.max(err / np.maximum(rper, 1e-300))))
            errv = np.abs(v - rv)
            assert np.all(v[rv == 0] == 0) and np.all(errv <= R.values_bound(m, n) * rv), (ident, v, rv)
            assert v[0] <= v[1], ident
            if np.any(rper > 0):
                worst = max(worst, float(np.max(err[rper > 0] / rper[rper > 0]) / R.per_bound(m, n)))
                worst_v = max(worst_v, float(np.max(errv[rv > 0] / rv[rv > 0]) / R.values_bound(m, n)))
    print(kind, 'gate (a): the largest error is %.3f of its bound on per, %.3f on values' % (worst, worst_v))


# ---- gate (b): the whole op -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', [1, 3, 16, 127, 128, 784, 3072])
def test_the_whole_op_against_the_float64_projections(gpu, d):
    """sliced_wasserstein(x, y, theta, p) against the reference on the float64 projections of the same float32 inputs.  delta = the largest
    difference between F.Gemm's projections (existing code, not under test) and those; W_p is a metric and moving every point by at most
    delta moves a measure by at most delta, so |W_p(l) - ref W_p(l)| <= 2 delta for every direction, for unequal sizes too, and through
    the p-mean and the max over directions -- plus the op's own fp64 rounding on the projections it was given, gate (a)'s relative bound
    (some 1e-13 of the distance: all there is at d = 1, where a unit direction is +-1, F.Gemm is exact and delta is 0); delta itself is held to the textbook dot-product bound d 2^-24 max|x_row| max|theta_col|,
    which catches a wrong transpose the first inequality alone would forgive.  A set against itself gives exactly 0."""
    import torch
    from graphical_gan_amd import functional as F
    L = 64
    rng = np.random.default_rng(1000 + d)
    theta = rng.normal(size=(d, L))
    theta = (theta / np.sqrt(np.sum(theta * theta, axis=0, keepdims=True))).astype(np.float32)
    td = _t(theta, gpu)
    for m, n in ((257, 257), (1000, 999)):
        x = rng.random((m, d), dtype=np.float32)
        y = (0.8 * rng.random((n, d), dtype=np.float32) + 0.15 * rng.random((1, d), dtype=np.float32)).astype(np.float32)
        xd, yd = _t(x, gpu), _t(y, gpu)
        proj = [F.Gemm.apply(a, td, None, False, False, F.ACT_NONE, 0.0).cpu().numpy().astype(np.float64) for a in (xd, yd)]
        p64 = [a.astype(np.float64) @ theta.astype(np.float64) for a in (x, y)]
        delta = max(float(np.max(np.abs(a - b))) for a, b in zip(proj, p64))
        ceiling = d * 2.0 ** -24 * max(float(np.max(np.sqrt(np.sum(a.astype(np.float64) ** 2, axis=1)))) for a in (x, y)) * \
            float(np.max(np.sqrt(np.sum(theta.astype(np.float64) ** 2, axis=0))))
        assert delta <= ceiling, (m, n, delta, ceiling)
        for p in R.PS:
            rv, rper = R.reference(p64[0], p64[1], p)
            v, per, st = F.sliced_wasserstein(xd, yd, td, p)
            v, per = v.cpu().numpy(), per.cpu().numpy()
            assert int(st.item()) == 0 and per.shape == (L,)
            e_per = float(np.max(np.abs(per ** (1.0 / p) - rper ** (1.0 / p))))
            e_val = float(np.max(np.abs(v - rv)))
            print('d %d, %d x %d, p %d: delta %.3e (ceiling %.3e), largest error per direction %.3e, of values %.3e; sliced distance %.3e'
                  % (d, m, n, p, delta, ceiling, e_per, e_val, rv[0]))
            own = R.values_bound(m, n) * float(np.max(rper)) ** (1.0 / p)      # gate (a)'s share: at d = 1 the projection is exact, delta is 0
            assert e_per <= 2 * delta + own and e_val <= 2 * delta + own, (m, n, p, e_per, e_val, delta)
            v0, per0, st0 = F.sliced_wasserstein(xd, xd, td, p)
            assert int(st0.item()) == 0 and not torch.any(per0 != 0) and not torch.any(v0 != 0)
            v1, per1, _ = F.sliced_wasserstein(xd, xd.clone(), td, p)
            assert not torch.any(per1 != 0) and not torch.any(v1 != 0)


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n', [(1000, 999), (4097, 4097)])
def test_permuted_rows_and_swapped_sets_give_the_same_bits(gpu, m, n):
    """the result depends on the multiset of each column only: rows of px and of py permuted independently give the same bits of per and
    values; at m = n so do the two sets swapped"""
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(m)
    for kind in ('gauss', 'ties'):
        x, y = R.sets(kind, m, n, 64)
        for p in R.PS:
            want = _bits(*F.sliced_wasserstein_projected(_t(x, gpu), _t(y, gpu), p))
            got = _bits(*F.sliced_wasserstein_projected(_t(x[rng.permutation(m)], gpu), _t(y[rng.permutation(n)], gpu), p))
            assert got == want, (kind, p)
            if m == n:
                assert _bits(*F.sliced_wasserstein_projected(_t(y, gpu), _t(x, gpu), p)) == want, (kind, p)


@pytest.mark.parametrize('m,n,L', [(257, 300, 33), (65, 64, 1), (1000, 999, 3)])
def test_views_and_odd_offsets_give_the_bits_of_the_contiguous_copy(gpu, m, n, L):
    import torch
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(L)
    x, y = _t(rng.normal(size=(m, L)).astype(np.float32), gpu), _t(rng.normal(size=(n, L)).astype(np.float32), gpu)
    wide = torch.zeros((m, L + 3), dtype=torch.float32, device=gpu)
    wide[:, 1:L + 1] = x
    view = wide[:, 1:L + 1]                                   # a non-contiguous view
    buf = torch.zeros((n * L + 1,), dtype=torch.float32, device=gpu)
    buf[1:] = y.reshape(-1)
    odd = buf[1:].view(n, L)                                  # contiguous, at an odd element offset of its storage
    assert not view.is_contiguous() and odd.is_contiguous() and odd.storage_offset() == 1 and odd.data_ptr() % 8 == 4
    for p in R.PS:
        want = _bits(*F.sliced_wasserstein_projected(x, y, p))
        assert _bits(*F.sliced_wasserstein_projected(view, odd, p)) == want
        assert _bits(*F.sliced_wasserstein_projected(odd, view, p)) == _bits(*F.sliced_wasserstein_projected(y, x, p))


@pytest.mark.parametrize('m,n', [(257, 257), (1000, 999)])
def test_columns_taken_out_of_a_wide_array_keep_their_bits(gpu, m, n):
    """L = 1 and L = 3 columns taken out of an L = 64 array give the bits those columns had inside it: a direction's value does not depend
    on its neighbours or on the stride"""
    from graphical_gan_amd import functional as F
    x, y = (_t(a, gpu) for a in R.sets('gauss', m, n, 64))
    for p in R.PS:
        _, per, _ = F.sliced_wasserstein_projected(x, y, p)
        for lo, hi in ((0, 1), (37, 38), (63, 64), (10, 13), (61, 64)):
            v, part, st = F.sliced_wasserstein_projected(x[:, lo:hi], y[:, lo:hi], p)
            assert _bits(part) == _bits(per[lo:hi]) and int(st.item()) == 0, (p, lo, hi)
            top = float(per[lo:hi].max())
            assert tuple(part.shape) == (hi - lo,) and float(v[1]) == (top if p == 1 else math.sqrt(top))


# ---- bad input ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [0, 1])
@pytest.mark.parametrize('bad', [float('nan'), float('inf'), float('-inf')])
def test_a_non_finite_value_is_a_status(gpu, bad, which):
    """a NaN, a +inf or a -inf in either set, in one column of three: SWD_NONFINITE in the status word and NaN in every output -- no
    exception, and the next call is clean"""
    import torch
    from graphical_gan_amd import functional as F
    x, y = (_t(a, gpu) for a in R.sets('gauss', 257, 257, 3))
    a, b = x.clone(), y.clone()
    (a, b)[which][200, 1] = bad
    v, per, st = F.sliced_wasserstein_projected(a, b, 2)
    assert int(st.item()) == F.SWD_NONFINITE and torch.isnan(v).all() and torch.isnan(per).all()
    v, per, st = F.sliced_wasserstein_projected(x, y, 2)
    assert int(st.item()) == 0 and torch.isfinite(v).all() and torch.isfinite(per).all()


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,dl', [('local_ep', 16), ('vegan', 8)])
def test_swd_scores_values_sets_and_an_untouched_trainer(gpu, mode, dl):
    """a tiny gmgan trainer, three dev minibatches and a partial one, eight directions: the four keys in order; the values are
    functional.sliced_wasserstein_projected on sets rebuilt here from the same seeds, with bit-equal projections; x is the full pixel
    space (3072 columns); the Trainer's feed and the evaluator's shared noise state are as they were"""
    import torch
    from graphical_gan_amd import functional as F, evaluate as E
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    B, K, n, seed, L = 4, 5, 3, 11, 8
    P._fresh()
    tr = Trainer(Config('cifar10', batch_size=B, n_coms=K, mode=mode, dim=8, dim_latent=dl, bn=False if mode == 'vegan' else None), device=gpu,
                 graph=False, seed=4321)
    rng = np.random.default_rng(3)
    xs = [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]
    dev = xs + [xs[0][:B - 1]]                                 # (unlabelled; a partial minibatch: dropped)
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, N_VIS=2 * K, SEED=seed, SWD_DIRS=L)
    ev = E.Evaluator(tr, S)
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before, shared = P._snapshot(tr.feed), ev.feed['rng_state'].cpu().numpy().tobytes()
    res, sets = ev.swd_scores(dev, return_sets=True)
    torch.cuda.synchronize()
    assert P._snapshot(tr.feed) == before and ev.feed['rng_state'].cpu().numpy().tobytes() == shared
    assert tuple(res) == E.SWD_KEYS and all(isinstance(v, float) and np.isfinite(v) and v >= 0 for v in res.values()), res
    assert res['dev swd z'] <= res['dev swd max z'] and res['dev swd x'] <= res['dev swd max x']
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z_proj=(n * B, L), pz_proj=(n * B, L), x_proj=(n * B, L), gx_proj=(n * B, L),
                                                                 theta_z=(dl, L), theta_x=(3072, L))
    assert ev.last_seconds > 0
    # the directions and the sets again, on a feed and a noise state of the test's own
    c, model = tr.cfg, tr.model
    draw = np.random.RandomState(seed + E.EVAL_SEED + E.SWD_SEED)
    thetas = []
    for d in (dl, c.output_dim):
        t = draw.normal(size=(d, L))
        t = t / np.sqrt(np.sum(t * t, axis=0, keepdims=True))
        assert np.allclose(np.sum(t * t, axis=0), 1.0, rtol=0, atol=1e-12)
        thetas.append(_t(t.astype(np.float32), gpu))
    assert torch.equal(thetas[0], sets['theta_z']) and torch.equal(thetas[1], sets['theta_x'])
    feed = model.feed_buffers(gpu)
    feed['rng_state'] = F.noise_state(gpu, seed + E.EVAL_SEED + E.SWD_SEED)
    gemm = lambda a, t: F.Gemm.apply(a.float().contiguous(), t, None, False, False, F.ACT_NONE, 0.0)
    unit = lambda x: gemm(F.Axpby.apply(x.float().reshape(B, -1).contiguous(), None, 0.5, 0.0, 0.5), thetas[1])
    mine = {k: [] for k in ('z_proj', 'pz_proj', 'x_proj', 'gx_proj')}
    pzs = []
    with torch.no_grad(), model.single_stream():
        for i in range(n):
            model.set_batch(feed, _t(xs[i], gpu))
            model.sample_noise(feed)
            real_x = model.real_x(feed)
            q = model.Extractor(real_x, eps=feed['q_eps']) if c.agg else model.Extractor(real_x)
            mine['z_proj'].append(gemm(q[0] if isinstance(q, tuple) else q, thetas[0]))
            mine['x_proj'].append(unit(real_x))
            pz = model.HyperGenerator(feed['k_onehot'], feed['p_z_noise']).clone()
            pzs.append(pz)
            mine['pz_proj'].append(gemm(pz, thetas[0]))
            mine['gx_proj'].append(unit(model.Generator(pz)))
        mine = {k: torch.cat(v) for k, v in mine.items()}
        for k in mine:
            assert torch.equal(sets[k], mine[k]), k
        p = E.SWD_P
        (vz, _, sz), (vx, _, sx) = F.sliced_wasserstein_projected(mine['z_proj'], mine['pz_proj'], p), F.sliced_wasserstein_projected(mine['x_proj'], mine['gx_proj'], p)
    assert int(sz.item()) == 0 and int(sx.item()) == 0
    assert [res[k] for k in E.SWD_KEYS] == [float(vz[0]), float(vz[1]), float(vx[0]), float(vx[1])]
    assert not torch.equal(pzs[0], pzs[1])                     # fresh prior draws per minibatch
    # against float64 on the rebuilt sets, for the record of what the keys mean
    ref = R.reference(mine['x_proj'].cpu().numpy(), mine['gx_proj'].cpu().numpy(), p)[0]
    assert abs(res['dev swd x'] - ref[0]) <= R.values_bound(n * B, n * B) * ref[0] and abs(res['dev swd max x'] - ref[1]) <= R.values_bound(n * B, n * B) * ref[1]
    # a second pass goes on in the pass's own stream of draws; SWD_MAX_ROWS caps the sets at whole minibatches; SWD_P = 1 is another number
    assert ev.swd_scores(dev) != res
    ev2 = E.Evaluator(tr, dict(S, SWD_MAX_ROWS=2 * B + 1))
    res2, capped = ev2.swd_scores(dev, return_sets=True)
    assert capped['z_proj'].shape[0] == 2 * B and torch.equal(capped['x_proj'], sets['x_proj'][:2 * B]) and tuple(res2) == E.SWD_KEYS
    res1 = E.Evaluator(tr, dict(S, SWD_P=1)).swd_scores(dev)
    assert tuple(res1) == E.SWD_KEYS and res1['dev swd x'] <= res['dev swd x'] * (1 + 1e-12) and res1['dev swd x'] != res['dev swd x']


def test_a_raised_status_gives_nan_and_one_message(gpu, capsys):
    """a dev image with a NaN pixel (MNIST minibatches are float32): four nan rows and one message, no exception"""
    from graphical_gan_amd import evaluate as E
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    B = 4
    P._fresh()
    tr = Trainer(Config('mnist', batch_size=B, n_coms=0, mode='ali', dim=8, dim_latent=16), device=gpu, graph=False, seed=1)
    rng = np.random.default_rng(0)
    dev = [rng.random((B, 784), dtype=np.float32) for _ in range(2)]
    dev[1][2, 300] = np.nan
    capsys.readouterr()
    res = E.Evaluator(tr, dict(BATCH_SIZE=B, MODE='ali', N_COMS=0, SWD_DIRS=8)).swd_scores(dev)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'swd' in ln]
    assert tuple(res) == E.SWD_KEYS and all(math.isnan(v) for v in res.values()), res
    assert len(lines) == 1 and lines[0].startswith('[evaluate] swd: status 1 (z) / 1 (x)') and 'non-finite' in lines[0]


# ---- run.train --------------------------------------------------------------------------------------------------------------------------------
def test_training_and_dev_mmd_bit_identical_with_the_swd_pass(gpu, tmp_path, monkeypatch):
    """a few iterations with MMD_EVERY alone, then with SWD_EVERY added: the `dev mmd` values, the logged training costs, the final weights
    and the optimizers' state are bit-identical -- the pass draws from a noise state of its own --, and the four names are logged"""
    from graphical_gan_amd.models import Config
    from graphical_gan_amd import evaluate as E
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=6, LOG_EVERY=3, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K, MMD_EVERY=2,
                SWD_DIRS=16)
    cfg = lambda: Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16)
    _, w0, a0, seen0 = P._train(dict(base), cfg())
    _, w1, a1, seen1 = P._train(dict(base, SWD_EVERY=2), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    rest = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev swd') and n != 'time']
    assert rest(seen0) == rest(seen1) and [n for n, _, _ in seen0 if n.startswith('dev mmd')]
    assert not [n for n, _, _ in seen0 if n.startswith('dev swd')]
    for it in (1, 3, 5):
        got = [n for n, i, _ in seen1 if i == it and n.startswith('dev ')]
        assert got == ['dev mmd z', 'dev mmd x'] + list(E.SWD_KEYS), (it, got)
    assert all(np.isfinite(v) and v >= 0 for n, _, v in seen1 if n.startswith('dev swd'))


def test_the_names_end_in_ema_on_the_averaged_weights_and_follow_the_frechet_pass(gpu, tmp_path, monkeypatch):
    from graphical_gan_amd.models import Config
    from graphical_gan_amd import evaluate as E
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    S = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=2, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K, SWD_EVERY=2,
             FRECHET_EVERY=2, SWD_DIRS=16, EMA_DECAY=0.5, EMA_EVAL='ema')
    _, _, _, seen = P._train(S, Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16))
    dev = [(n, i) for n, i, _ in seen if n.startswith('dev ')]
    assert dev == [(k + ' ema', 1) for k in E.FRECHET_KEYS + E.SWD_KEYS]


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_four_rows_and_moves_no_other(gpu, tmp_path, monkeypatch, capsys):
    """evaluate CKPT --swd: the four rows of a live evaluator on the restored weights, printed; every other row as without the flag"""
    from graphical_gan_amd import checkpoint, run, evaluate
    from graphical_gan_amd.engine import Trainer
    P._data_on_disk(tmp_path, monkeypatch)
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=5, BATCH_SIZE=8, SWD_DIRS=16)
    S = run.reference_block('gmgan_inference_mnist', **over)
    P._fresh()
    tr = Trainer(run.config(S), device=gpu, graph=False)
    for it in range(2):
        tr.iteration(it, iter(tr.model.synthetic_ring(gpu, n=4) * 2))
    ckpt = str(tmp_path / 'params_2.npz')
    checkpoint.save(ckpt, tr)
    np.random.seed(5)
    dev, _ = run.eval_sets(S, tr.model, gpu)
    live = evaluate.Evaluator(tr, S).swd_scores(dev)           # (a noise state of its own: whatever ran before it)
    P._fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--swd'])
    out = capsys.readouterr().out
    for k in evaluate.SWD_KEYS:
        assert res[k] == live[k] and '%s\t%s' % (k, live[k]) in out.splitlines(), k
    P._fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if not k.startswith('dev swd'))
    assert all(plain[k] == res[k] for k in plain)
