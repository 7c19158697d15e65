"""gpu: the Frechet distance on the device against the float64 reference tests/_frechet_ref.py over its grid -- the fp64 stage alone fed numpy's
moments (gate a), the whole op from float32 rows (gate b) and its moments --, the bitwise properties, non-finite input as a status, the pass
Evaluator.frechet_scores on sets rebuilt here from the same seeds, and run.train with the pass switched on beside `dev mmd`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _frechet_ref as R  # noqa: E402
import test_mmd_sets_gpu as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a)).to(dev)


def _stage(dev, m1, S1, m2, S2):
    """ggan_frechet_distance through the C ABI on float64 moments -> (values [4], status)"""
    import torch
    from graphical_gan_amd import _lib
    from graphical_gan_amd.functional._core import _p, _stream
    L = _lib.load()
    t = [_t(np.ascontiguousarray(a, np.float64), dev) for a in (m1, S1, m2, S2)]
    d = m1.shape[0]
    out = torch.full((4,), -1.0, dtype=torch.float64, device=dev)
    st = torch.full((1,), -1, dtype=torch.int32, device=dev)
    nbytes = L.ggan_frechet_distance_workspace(d)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    _lib.check(L.ggan_frechet_distance(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), d, _p(out), _p(st), _p(ws), nbytes, _stream()), 'ggan_frechet_distance')
    return out.cpu().numpy(), int(st.item())


# ---- gate (a): the fp64 stage alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_the_fp64_stage_against_the_reference(gpu, kind):
    """ggan_frechet_distance fed the float64 moments numpy computed: abs(fd - ref) / (tr S1 + tr S2 + |dmu|^2) within four times the largest
    value seen over the grid on one MI355X (3.2e-7, at 'self' n = 2 d = 127: the reference's own error at rank 1, which the float64 model
    of the kernel's route shows to the digit -- test_frechet_cpu.py); the three parts are held to the same bound; a set against itself is 0"""
    worst = 0.0
    for k, n, d in R.cases((kind,)):
        x, y = R.sets(k, n, d)
        ref = R.case_reference(k, n, d)
        v, st = _stage(gpu, *(R.moments(x) + R.moments(y)))
        err = R.rel_err(v, ref)
        parts = float(np.max(np.abs(v[1:] - ref[1:]))) / max(R.scale_of(ref), 1e-300)
        worst = max(worst, err, parts)
        assert st == 0 and err <= R.FP64_STAGE_BOUND and parts <= R.FP64_STAGE_BOUND, (R.case_id(k, n, d), err, parts, st)
        assert v[0] == v[1] + v[2] - v[3]
        if k == 'self':
            assert abs(v[0]) <= 1e-9 * v[2] and v[1] == 0, (R.case_id(k, n, d), v)
    print(kind, 'gate (a): worst %.3e of bound %.3e' % (worst, R.FP64_STAGE_BOUND))


# ---- gate (b): the whole op, and its moments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', R.KINDS)
def test_the_whole_op_and_its_moments_against_the_reference(gpu, kind):
    """functional.frechet_distance from the float32 rows within four times the largest value seen over the grid on one MI355X (1.4e-6, at
    'short' n = 600 d = 127), itself below 256 * 2^-24 -- all an fp32 sum over a block of 256 rows can explain; mean and covariance entry
    by entry against float64 under the same bound, the covariance relative to sqrt(S_ii S_jj) (exactly 0 where that is 0: a constant
    column), the mean relative to sqrt(S_ii) or its own size; two calls give the same bits"""
    from graphical_gan_amd import functional as F
    assert R.WHOLE_OP_BOUND <= R.WHOLE_OP_CEILING
    worst, worst_cov = 0.0, 0.0
    for k, n, d in R.cases((kind,)):
        x, y = R.sets(k, n, d)
        ref = R.case_reference(k, n, d)
        xd, yd = _t(x, gpu), _t(y, gpu)
        v, st = F.frechet_distance(xd, yd)
        v2, st2 = F.frechet_distance(xd, yd)
        assert v.dtype.is_floating_point and v.element_size() == 8 and tuple(v.shape) == (4,) and tuple(st.shape) == (1,) and st.element_size() == 4
        assert v.cpu().numpy().tobytes() == v2.cpu().numpy().tobytes() and int(st.item()) == int(st2.item()) == 0, R.case_id(k, n, d)
        err = R.rel_err(v.cpu().numpy(), ref)
        worst = max(worst, err)
        assert err <= R.WHOLE_OP_BOUND, (R.case_id(k, n, d), err)
        for rows, rd in ((x, xd), (y, yd)):
            mu, S = R.moments(rows)
            mean, cov = (a.cpu().numpy() for a in F.frechet_moments(rd))
            assert mean.dtype == np.float64 and cov.dtype == np.float64 and cov.shape == (d, d)
            sd = np.sqrt(np.diag(S))
            den = np.outer(sd, sd)
            assert np.all((cov - S)[den == 0] == 0), R.case_id(k, n, d)
            e = float(np.max(np.abs(cov - S)[den > 0] / den[den > 0])) if np.any(den > 0) else 0.0
            em = float(np.max(np.abs(mean - mu) / np.maximum(sd, np.abs(mu))))
            worst_cov = max(worst_cov, e)
            assert e <= R.WHOLE_OP_BOUND and em <= R.WHOLE_OP_BOUND, (R.case_id(k, n, d), e, em)
            assert np.array_equal(cov, cov.T)
    print(kind, 'gate (b): worst %.3e, covariance %.3e, of bound %.3e (ceiling %.3e)' % (worst, worst_cov, R.WHOLE_OP_BOUND, R.WHOLE_OP_CEILING))


# ---- bitwise properties ---------------------------------------------------------------------------------------------------------------------
def test_rows_permuted_inside_one_block_give_the_same_mean_bits(gpu):
    """the block's column sums run in fp64, and the fp64 sum of 256 float32 values of a bounded exponent spread (here multiples of 2^-10
    below 16) is exact in any order.  Not required across blocks, nor of values whose sum does not fit 53 bits."""
    from graphical_gan_amd import functional as F
    x = np.round(np.array(R.sets('gauss', 256, 33)[0]) * 1024.0) / 1024.0
    perm = np.random.default_rng(5).permutation(256)
    a, b = F.frechet_moments(_t(x.astype(np.float32), gpu))[0], F.frechet_moments(_t(x[perm].astype(np.float32), gpu))[0]
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize('n,d', [(257, 33), (300, 128)])
def test_views_and_odd_offsets_give_the_bits_of_the_contiguous_copy(gpu, n, d):
    import torch
    from graphical_gan_amd import functional as F
    x, y = (_t(a, gpu) for a in R.sets('gauss', 600, d))
    x, y = x[:n], y[:n]
    want = F.frechet_distance(x, y)[0].cpu().numpy().tobytes()
    wide = torch.zeros((n, d + 3), dtype=torch.float32, device=gpu)
    wide[:, 1:d + 1] = x
    view = wide[:, 1:d + 1]                                   # a non-contiguous view
    buf = torch.zeros((n * d + 1,), dtype=torch.float32, device=gpu)
    buf[1:] = y.reshape(-1)
    odd = buf[1:].view(n, d)                                  # contiguous, at an odd element offset of its storage
    assert not view.is_contiguous() and odd.is_contiguous() and odd.storage_offset() == 1 and odd.data_ptr() % 8 == 4
    assert F.frechet_distance(view, odd)[0].cpu().numpy().tobytes() == want
    for a, b in ((x, view), (y, odd)):
        for p, q in zip(F.frechet_moments(a), F.frechet_moments(b)):
            assert torch.equal(p, q)


# ---- bad input ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_a_non_finite_entry_is_a_status(gpu, bad):
    """a NaN or an inf in either set: FRECHET_NONFINITE in the status word and NaN values -- no exception, and the next call is clean"""
    import torch
    from graphical_gan_amd import functional as F
    x, y = (_t(a, gpu) for a in R.sets('gauss', 257, 33))
    for which in (0, 1):
        a, b = x.clone(), y.clone()
        (a, b)[which][200, 7] = bad
        v, st = F.frechet_distance(a, b)
        assert int(st.item()) & F.FRECHET_NONFINITE and not int(st.item()) & F.FRECHET_NOT_CONVERGED
        assert torch.isnan(v).all()
    v, st = F.frechet_distance(x, y)
    assert int(st.item()) == 0 and torch.isfinite(v).all()


# ---- the pass ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,dl', [('local_ep', 16), ('vegan', 8)])
def test_frechet_scores_values_sets_and_an_untouched_trainer(gpu, mode, dl):
    """a tiny gmgan trainer, three dev minibatches and a partial one: the four keys; the values are functional.frechet_distance on sets
    rebuilt here from the same seeds; xr is 128 wide whatever DIM_LATENT is (8 under vegan); the Trainer's feed and the evaluator's shared
    noise state are as they were"""
    import torch
    from graphical_gan_amd import functional as F, evaluate as E
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    B, K, n, seed = 4, 5, 3, 11
    P._fresh()
    tr = Trainer(Config('cifar10', batch_size=B, n_coms=K, mode=mode, dim=8, dim_latent=dl, bn=False if mode == 'vegan' else None), device=gpu,
                 graph=False, seed=4321)
    rng = np.random.default_rng(3)
    xs = [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]
    dev = xs + [xs[0][:B - 1]]                                 # (unlabelled; a partial minibatch: dropped)
    ev = E.Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, N_VIS=2 * K, SEED=seed))
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before, shared = P._snapshot(tr.feed), ev.feed['rng_state'].cpu().numpy().tobytes()
    res, sets = ev.frechet_scores(dev, return_sets=True)
    torch.cuda.synchronize()
    assert P._snapshot(tr.feed) == before and ev.feed['rng_state'].cpu().numpy().tobytes() == shared
    assert tuple(res) == E.FRECHET_KEYS and all(isinstance(v, float) and np.isfinite(v) for v in res.values()), res
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z=(n * B, dl), pz=(n * B, dl), xr=(n * B, 128), gxr=(n * B, 128))
    assert ev.last_seconds > 0 and res['dev frechet mean z'] >= 0 and res['dev frechet mean xr'] >= 0
    # the sets again, on a feed and a noise state of the test's own
    c, model = tr.cfg, tr.model
    feed = model.feed_buffers(gpu)
    feed['rng_state'] = F.noise_state(gpu, seed + E.EVAL_SEED + E.FRECHET_SEED)
    proj = np.random.RandomState(seed + E.EVAL_SEED + E.FRECHET_SEED).normal(size=(c.output_dim, 128)) / np.sqrt(float(c.output_dim))
    proj = _t(proj.astype(np.float32), gpu)
    unit = lambda x: F.Gemm.apply(F.Axpby.apply(x.float().reshape(B, -1).contiguous(), None, 0.5, 0.0, 0.5), proj, None, False, False, F.ACT_NONE, 0.0)
    mine = {k: [] for k in sets}
    with torch.no_grad(), model.single_stream():
        for i in range(n):
            model.set_batch(feed, _t(xs[i], gpu))
            model.sample_noise(feed)
            real_x = model.real_x(feed)
            q = model.Extractor(real_x, eps=feed['q_eps']) if c.agg else model.Extractor(real_x)
            mine['z'].append((q[0] if isinstance(q, tuple) else q).clone())
            mine['xr'].append(unit(real_x))
            pz = model.HyperGenerator(feed['k_onehot'], feed['p_z_noise']).clone()
            mine['pz'].append(pz)
            mine['gxr'].append(unit(model.Generator(pz)))
        mine = {k: torch.cat(v) for k, v in mine.items()}
        for k in sets:
            assert torch.equal(sets[k], mine[k]), k
        (vz, sz), (vx, sx) = F.frechet_distance(mine['z'], mine['pz']), F.frechet_distance(mine['xr'], mine['gxr'])
    assert int(sz.item()) == 0 and int(sx.item()) == 0
    want = [float(vz[0]), float(vz[1]), float(vx[0]), float(vx[1])]
    assert [res[k] for k in E.FRECHET_KEYS] == want
    assert not torch.equal(mine['pz'][:B], mine['pz'][B:2 * B])         # fresh prior draws per minibatch
    # a second pass goes on in the pass's own stream of draws; FRECHET_MAX_ROWS caps the sets at whole minibatches
    assert ev.frechet_scores(dev) != res
    ev2 = E.Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, N_VIS=2 * K, SEED=seed, FRECHET_MAX_ROWS=2 * B + 1))
    res2, capped = ev2.frechet_scores(dev, return_sets=True)
    assert capped['z'].shape[0] == 2 * B and torch.equal(capped['xr'], sets['xr'][:2 * B]) and tuple(res2) == E.FRECHET_KEYS


def test_a_raised_status_gives_nan_and_one_message(gpu, capsys):
    """a dev image with a NaN pixel (MNIST minibatches are float32): nan rows and one message naming the bits, no exception"""
    import torch
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
    res = E.Evaluator(tr, dict(BATCH_SIZE=B, MODE='ali', N_COMS=0)).frechet_scores(dev)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if 'frechet' in ln]
    assert tuple(res) == E.FRECHET_KEYS and all(np.isnan(v) for v in res.values()), res
    assert len(lines) == 1 and 'status 1 (z) / 1 (xr)' in lines[0] and 'non-finite' in lines[0] and 'did not converge' in lines[0]


# ---- run.train --------------------------------------------------------------------------------------------------------------------------------
def test_training_and_dev_mmd_bit_identical_with_the_frechet_pass(gpu, tmp_path, monkeypatch):
    """a few iterations with MMD_EVERY alone, then with FRECHET_EVERY added: the `dev mmd` values, the logged training costs, the final weights
    and the optimizers' state are bit-identical -- the pass draws from a noise state of its own --, and the four names are logged"""
    from graphical_gan_amd.models import Config
    from graphical_gan_amd import evaluate as E
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=6, LOG_EVERY=3, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K, MMD_EVERY=2)
    cfg = lambda: Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16)
    _, w0, a0, seen0 = P._train(dict(base), cfg())
    _, w1, a1, seen1 = P._train(dict(base, FRECHET_EVERY=2), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    rest = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev frechet') and n != 'time']
    assert rest(seen0) == rest(seen1) and [n for n, _, _ in seen0 if n.startswith('dev mmd')]
    assert not [n for n, _, _ in seen0 if n.startswith('dev frechet')]
    for it in (1, 3, 5):
        got = [n for n, i, _ in seen1 if i == it and n.startswith('dev ')]
        assert got == ['dev mmd z', 'dev mmd x'] + list(E.FRECHET_KEYS), (it, got)
    assert all(np.isfinite(v) for n, _, v in seen1 if n.startswith('dev frechet'))


def test_the_names_end_in_ema_on_the_averaged_weights(gpu, tmp_path, monkeypatch):
    from graphical_gan_amd.models import Config
    from graphical_gan_amd import evaluate as E
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    S = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=2, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K, FRECHET_EVERY=2,
             EMA_DECAY=0.5, EMA_EVAL='ema')
    _, _, _, seen = P._train(S, Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16))
    dev = [(n, i) for n, i, _ in seen if n.startswith('dev ')]
    assert dev == [(k + ' ema', 1) for k in E.FRECHET_KEYS]


# ---- CLI ----------------------------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_four_rows_and_moves_no_other(gpu, tmp_path, monkeypatch, capsys):
    """evaluate CKPT --frechet: the four rows of a live evaluator on the restored weights, printed; every other row as without the flag"""
    from graphical_gan_amd import checkpoint, run, evaluate
    from graphical_gan_amd.engine import Trainer
    P._data_on_disk(tmp_path, monkeypatch)
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=5, BATCH_SIZE=8)
    S = run.reference_block('gmgan_inference_mnist', **over)
    P._fresh()
    tr = Trainer(run.config(S), device=gpu, graph=False)
    for it in range(2):
        tr.iteration(it, iter(tr.model.synthetic_ring(gpu, n=4) * 2))
    ckpt = str(tmp_path / 'params_2.npz')
    checkpoint.save(ckpt, tr)
    np.random.seed(5)
    dev, _ = run.eval_sets(S, tr.model, gpu)
    live = evaluate.Evaluator(tr, S).frechet_scores(dev)       # (a noise state of its own: whatever ran before it)
    P._fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--frechet'])
    out = capsys.readouterr().out
    for k in evaluate.FRECHET_KEYS:
        assert res[k] == live[k] and '%s\t%s' % (k, live[k]) in out.splitlines(), k
    P._fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if not k.startswith('dev frechet'))
    assert all(plain[k] == res[k] for k in plain)
