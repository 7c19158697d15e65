"""-m gpu: the straight-through MODE_K values of the mixture scripts (gmgan_inference_cifar10.py:164-171) on the HIP path.

  * ggan_gmm_latent_st_fwd / _bwd against a float64 numpy restatement: logits, the soft assignment, the argmax (first index on a
    tie), the forward value k = (h - v) + v bit for bit, both backward rules;
  * the reference's own runs (tests/golden/reference_trace_mode_k.json) replayed through engine.Trainer;
  * step graphs against eager steps, and the evaluator's dev gen cost against a live forward pass.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import test_reference_trace_cpu as RC
import test_reference_trace_gpu as RG
from oracle import reftrace as RT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = json.load(open(os.path.join(HERE, 'golden', 'reference_trace_mode_k.json')))
STC, ST = 'STRAIGHT_THROUGHT_CONCRETE', 'STRAIGHT_THROUGHT'
MARGIN = 1e-3                     # relative top-two gap above which float32 and float64 must pick the same index


def _fresh():
    from graphical_gan_amd import tflib as lib, optim
    optim.reset_optimizers()
    lib.delete_all_params()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _gap(v):
    top = np.sort(v, axis=-1)[:, ::-1]
    return (top[:, 0] - top[:, 1]) / np.maximum(np.abs(top[:, 0]), 1e-30)


def _fwd(mode, z, mu, u, log_pi, temp):
    import torch
    from graphical_gan_amd import _lib
    B, K = z.shape[0], mu.shape[0]
    dev = torch.device('cuda:0')
    zt, mt = torch.as_tensor(z, device=dev), torch.as_tensor(mu, device=dev)
    ut = torch.as_tensor(u, device=dev) if mode == STC else None
    logits = torch.full((B, K), np.nan, device=dev)
    k = torch.full((B, K), np.nan, device=dev)
    soft = torch.full((B, K), np.nan, device=dev) if mode == STC else None
    L = _lib.load()
    assert L.ggan_gmm_latent_st_fwd(_p(zt), _p(mt), _p(ut), _p(logits), _p(k), _p(soft), B, K, z.shape[1], log_pi, temp,
                                    _lib.MODE_K[mode], None) == 0, L.ggan_last_error()
    torch.cuda.synchronize()
    return logits.cpu().numpy(), k.cpu().numpy(), (soft.cpu().numpy() if soft is not None else None)


def _st_value(v):
    """TF's float32 stop_gradient(h - v) + v, h = one_hot(argmax v) (np.argmax: the first index on a tie)"""
    h = np.zeros_like(v)
    h[np.arange(v.shape[0]), np.argmax(v, axis=1)] = 1
    return (h - v) + v


def _gumbel64(u):
    u = u.astype(np.float64)
    return -np.log(-np.log(u + 1e-20) + 1e-20)


def _softmax64(x):
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


@pytest.mark.parametrize('mode', [STC, ST])
@pytest.mark.parametrize('B', [6, 50, 64])
@pytest.mark.parametrize('K', [5, 30, 50, 256])
def test_st_forward_against_float64(gpu, mode, K, B):
    D, temp = 128, 0.1
    rng = np.random.default_rng(K * 1000 + B)
    z = rng.standard_normal((B, D)).astype(np.float32)
    mu = rng.standard_normal((K, D)).astype(np.float32)
    u = rng.random((B, K), dtype=np.float32)
    log_pi = float(np.log(np.float32(1.0) / np.float32(K)))
    logits, k, soft = _fwd(mode, z, mu, u, log_pi, temp)
    l64 = -0.5 * ((z.astype(np.float64)[:, None, :] - mu.astype(np.float64)[None]) ** 2).sum(-1) + log_pi
    assert np.abs(logits - l64).max() <= 1e-5 * max(1.0, np.abs(l64).max()), np.abs(logits - l64).max()
    if mode == STC:
        # the soft assignment from the kernel's own logits (their float32 rounding is pinned above) and its float32 (logits + g) / temp:
        # within 1e-5, plus what one float32 ulp of that softmax input (|x| ~ 10 D: ~1e-4) moves s by -- the kernel's logf and numpy's
        # log may round g apart by an ulp
        x32 = (logits + _gumbel64(u).astype(np.float32)) * np.float32(1.0 / temp)
        s64 = _softmax64(x32.astype(np.float64))
        ulp = np.spacing(np.abs(x32).max(axis=1, keepdims=True)).astype(np.float64)
        assert np.all(np.abs(soft - s64) <= 1e-5 + 4 * ulp * np.maximum(soft, s64))
        v32, v64 = soft, _softmax64((l64 + _gumbel64(u)) / temp)
    else:
        v32, v64 = logits, l64
    # the forward value, bit for bit: (h - v) + v in float32 from the kernel's own v, exactly 0 off the argmax
    assert np.array_equal(k.view(np.int32), _st_value(v32).view(np.int32))
    hot = np.argmax(v32, axis=1)
    off = np.ones_like(k, bool)
    off[np.arange(B), hot] = False
    assert np.all(k[off] == 0.0)
    if mode == ST:
        assert np.abs(k[~off] - 1.0).max() <= 4e-5          # (an ulp of |logits| ~ D: not exactly 1)
    # the argmax agrees with float64 wherever the top two are apart
    clear = _gap(v64) >= MARGIN
    assert clear.sum() >= B // 2
    assert np.array_equal(hot[clear], np.argmax(v64, axis=1)[clear])


@pytest.mark.parametrize('mode', [STC, ST])
@pytest.mark.parametrize('K', [5, 256])
def test_st_forward_ties_take_the_first_index(gpu, mode, K):
    """two components with the same logit (ST) / the same softmax output (STC) at the top of every row: the lower index wins, within
    one wave and across waves"""
    D, B = 128, 4
    rng = np.random.default_rng(5)
    z = np.zeros((B, D), np.float32)
    u = np.full((B, K), 0.5, np.float32)
    base = (0.1 * rng.standard_normal(D)).astype(np.float32)
    for lo, hi in ([(1, 2), (0, 4), (3, 1)] if K == 5 else [(3, 200), (70, 130), (250, 10)]):
        mu = (3.0 + rng.standard_normal((K, D))).astype(np.float32)   # far from z = 0 ...
        mu[lo], mu[hi] = base, -base                                  # ... but two at the same distance: equal logits, bit for bit
        logits, k, soft = _fwd(mode, z, mu, u, 0.0, 0.1)
        v = soft if mode == STC else logits
        assert np.all(v[:, lo] == v[:, hi]) and np.all(v[:, lo] == v.max(axis=1)), (lo, hi)
        first = min(lo, hi)
        assert np.all(np.argmax(v, axis=1) == first)
        assert np.array_equal(k.view(np.int32), _st_value(v).view(np.int32))
        assert np.all(k[:, max(lo, hi)] == 0.0) and np.all(k[:, first] != 0.0)


def _bwd(entry, mode, z, mu, kk, gl, gk, want_dz, want_dmu, temp=0.1):
    import torch
    from graphical_gan_amd import _lib
    dev = torch.device('cuda:0')
    B, D, K = z.shape[0], z.shape[1], mu.shape[0]
    t = lambda a: torch.as_tensor(a, device=dev) if a is not None else None
    dz = torch.full((B, D), np.nan, device=dev) if want_dz else None
    dmu = torch.full((K, D), np.nan, device=dev) if want_dmu else None
    zt, mt, kt, glt, gkt = t(z), t(mu), t(kk), t(gl), t(gk)
    L = _lib.load()
    if entry == 'concrete':
        rc = L.ggan_gmm_latent_bwd(_p(zt), _p(mt), _p(kt), _p(glt), _p(gkt), _p(dz), _p(dmu), B, K, D, temp, None)
    else:
        rc = L.ggan_gmm_latent_st_bwd(_p(zt), _p(mt), _p(kt), _p(glt), _p(gkt), _p(dz), _p(dmu), B, K, D, temp, _lib.MODE_K[mode], None)
    assert rc == 0, L.ggan_last_error()
    torch.cuda.synchronize()
    return (dz.cpu().numpy() if dz is not None else None), (dmu.cpu().numpy() if dmu is not None else None)


@pytest.mark.parametrize('B,K', [(6, 5), (64, 30), (50, 256)])
def test_stc_backward_is_the_concrete_backward_on_the_soft_assignment(gpu, B, K):
    D = 128
    rng = np.random.default_rng(B + K)
    z = rng.standard_normal((B, D)).astype(np.float32)
    mu = rng.standard_normal((K, D)).astype(np.float32)
    u = rng.random((B, K), dtype=np.float32)
    _, _, soft = _fwd(STC, z, mu, u, float(np.log(np.float32(1.0) / np.float32(K))), 0.1)
    gl = rng.standard_normal((B, K)).astype(np.float32)
    gk = rng.standard_normal((B, K)).astype(np.float32)
    a = _bwd('concrete', STC, z, mu, soft, gl, gk, True, True)
    b = _bwd('st', STC, z, mu, soft, gl, gk, True, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('B,K', [(6, 5), (64, 30), (50, 50), (64, 256)])
def test_st_backward_against_float64(gpu, B, K):
    """dlogits = g_logits + g_k (k = stop_gradient(h - logits) + logits), then dz = -sum_j dlog (z - mu_j), dmu_j = sum_b dlog (z_b - mu_j);
    each of g_logits / g_k / dz / dmu may be NULL"""
    D = 128
    rng = np.random.default_rng(3 * B + K)
    z = rng.standard_normal((B, D)).astype(np.float32)
    mu = rng.standard_normal((K, D)).astype(np.float32)
    gl = rng.standard_normal((B, K)).astype(np.float32)
    gk = rng.standard_normal((B, K)).astype(np.float32)
    diff = z.astype(np.float64)[:, None, :] - mu.astype(np.float64)[None]          # [B, K, D]
    for use_gl, use_gk, want_dz, want_dmu in [(1, 1, 1, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0)]:
        dlog = (gl.astype(np.float64) if use_gl else 0) + (gk.astype(np.float64) if use_gk else 0)
        dz, dmu = _bwd('st', ST, z, mu, None, gl if use_gl else None, gk if use_gk else None, want_dz, want_dmu)
        if want_dz:
            ref = -(dlog[:, :, None] * diff).sum(1)
            assert np.abs(dz - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), (use_gl, use_gk)
        else:
            assert dz is None
        if want_dmu:
            ref = (dlog[:, :, None] * diff).sum(0)
            assert np.abs(dmu - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max()), (use_gl, use_gk)


# ---- the reference's runs -------------------------------------------------------------------------------------------------------
def _roles(key, t):
    """random-node roles of a mode's trace: under STRAIGHT_THROUGHT there is no Gumbel draw to find"""
    script, mode, mode_k = key.split(':')
    consts = dict(t['constants'], **t.get('script_constants', {}))
    ocfg, mode = RC.image_cfg('%s:%s' % (script, mode), consts)
    roles, missing = RC.roles_for(ocfg, mode, t['random_nodes'])
    if mode_k == ST:
        assert 'gumbel_u' not in [r[0] for r in roles.values()]
        missing = [m for m in missing if m[1] != 'gumbel_u']
    assert not missing, missing
    return ocfg, mode, consts, roles


@pytest.mark.parametrize('key', sorted(TRACE))
def test_hip_path_replays_the_reference_mode_k_run(gpu, key):
    import torch
    from graphical_gan_amd.engine import Trainer
    t = TRACE[key]
    mode_k = key.split(':')[2]
    ocfg, mode, consts, roles = _roles(key, t)
    _fresh()
    cfg = RG._image_config(':'.join(key.split(':')[:2]), consts)
    cfg.mode_k = mode_k
    tr = Trainer(cfg, device=gpu, graph=False, inject_noise=True)
    assert ('gumbel_u' in tr.feed) == (mode_k != ST)
    W0 = {n: RT.det_weight(n, shp, np.float32) for n, shp in zip(t['names'], t['shapes'])}
    tr.load_params(W0)
    runs = [r for r in t['runs'] if r['train']]
    feeds = [RC.make_feed(ocfg, mode, t, r, roles)[0] for r in runs]
    tr.set_feed(feeds[0])
    first = runs[0]['train'][0]
    ref_grads = dict(zip(t['names'], t['first_grads']))
    which = 'disc' if first['optimizer'] == 1 else 'gen'
    out = tr.model.forward(tr.feed, which)
    c = float(out[which + '_cost'].detach())
    assert abs(c - first['cost']) <= 2e-5 * max(1.0, abs(first['cost'])), (key, c, first['cost'])
    opt = out[which + '_train_op'].optimizer
    grads = [(g[0] + g[1]) if isinstance(g, tuple) else g for g in opt.compute_gradients(out[which + '_cost'])]
    gmax = max(d[1] for d in ref_grads.values() if d is not None)
    for p, g in zip(opt.params, grads):
        ref = ref_grads.get(p.param_name)
        if ref is None:
            assert g is None or float(g.abs().max()) == 0.0, p.param_name
            continue
        mine = RT.digest(p.param_name, g.detach().cpu().numpy())
        scale = max(ref[1], 1e-2 * gmax)
        assert np.abs(np.asarray(mine[2:]) - np.asarray(ref[2:])).max() <= 3e-4 * scale, (key, p.param_name, mine[:2], ref[:2])
        assert abs(mine[0] - ref[0]) <= 3e-4 * max(ref[0], scale), (key, p.param_name, 'l2', mine[0], ref[0])
    del out, grads
    # the loop through engine.Trainer: every fetched cost (the generator steps differentiate through the estimator), the final weights
    tr.load_params(W0)
    it_feeds, j, it = iter(feeds), 0, 0
    while j < len(runs):
        res = tr.iteration(it, it_feeds)
        for name in (['gen_cost'] if it > 0 else []) + ['disc_cost'] * cfg.critic_iters:
            rec = runs[j]['train'][0]
            v = float(res[name])
            assert abs(v - rec['cost']) <= 2e-3 * max(1.0, abs(rec['cost'])), (key, 'run', runs[j]['run'], name, v, rec['cost'])
            j += 1
        it += 1
    P = tr.get_params()
    gall = max(g for g in t['gmax'] if g is not None)
    for n, shape, gs, dg in zip(t['names'], t['shapes'], t['gmax'], t['final']):
        if gs is not None and gs < 1e-9 * gall:
            continue                                     # (a mathematically zero gradient: Adam random-walks the tensor on rounding noise)
        _final_check(key, n, P[n], dg, W0[n], t['final_samples'])
    _fresh()
    torch.cuda.synchronize()


def _final_check(key, name, mine, ref_digest, w0, count):
    """test_reference_trace_gpu._final_check on the `count` entries this fixture keeps: ||P - P_ref|| <= 0.02 ||P_ref - P_0|| + an fp32
    floor on the sampled entries, the norm to 1e-4"""
    m = RT.digest(name, mine, count)
    assert abs(m[0] - ref_digest[0]) <= 1e-4 * max(ref_digest[0], 1e-3) + 1e-6, (key, name, m[0], ref_digest[0])
    start = w0.astype(np.float64).ravel()[RT.sample_positions(name, w0.size, count)]
    ref, got = np.asarray(ref_digest[2:]), np.asarray(m[2:])
    floor = 4e-7 * (np.abs(ref).max() + 1e-3) * np.sqrt(count)
    assert np.linalg.norm(got - ref) <= 0.02 * np.linalg.norm(ref - start) + floor, (key, name, 'entries')


# ---- step graphs, evaluation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode_k', ['CONCRETE', STC, ST])
@pytest.mark.parametrize('dataset,K,B', [('cifar10', 30, 64), ('mnist', 30, 50)])
def test_step_graph_matches_eager(gpu, mode_k, dataset, K, B):
    """a few iterations as step graphs and as eager steps: bit-identical costs and weights.  (The two nets passes stay on one stream: run
    side by side inside a graph, their convolutions are planned for fewer workgroups and sum in another order -- the costs then differ in
    the last bits, in every MODE_K, CONCRETE included.)"""
    import torch
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    finals = []
    for graph in (False, True):
        _fresh()
        np.random.seed(0)
        tr = Trainer(Config(dataset, batch_size=B, n_coms=K, mode='local_ep', mode_k=mode_k), device=gpu, graph=graph, seed=4321)
        assert tr.model.cfg.mode_k == mode_k
        tr.model.fork_nets = False
        batches = iter(tr.model.synthetic_ring(gpu, n=5, seed=99) * 40)
        for it in range(4):
            res = tr.iteration(it, batches)
        tr.flush()
        torch.cuda.synchronize()
        finals.append(({k: v.copy() for k, v in tr.get_params().items()}, {k: float(v) for k, v in res.items()}))
    assert finals[0][1] == finals[1][1]
    assert all(np.isfinite(v) for v in finals[0][1].values())
    for k in finals[0][0]:
        assert np.array_equal(finals[0][0][k], finals[1][0][k]), k
    _fresh()


def test_dev_costs_use_the_models_estimator(gpu):
    """Evaluator.dev_costs under STRAIGHT_THROUGHT: the mean of what a live forward(feed, 'gen') gives on the same batches and noise"""
    import torch
    from graphical_gan_amd import run
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.evaluate import Evaluator
    S = run.reference_block('gmgan_inference_cifar10', MODE='local_epce', MODE_K=ST, BATCH_SIZE=8, N_COMS=6, DIM=16)
    _fresh()
    tr = Trainer(run.config(S), device=gpu, graph=False, inject_noise=True)
    assert tr.model.cfg.mode_k == ST and 'gumbel_u' not in tr.feed
    rng = np.random.default_rng(3)
    xs = [rng.integers(0, 256, size=(8, 3072)).astype(np.int32) for _ in range(3)]
    ev = Evaluator(tr, S, keep_noise=True)
    assert 'gumbel_u' not in ev.feed
    res = ev.dev_costs([(x, np.zeros(8, np.int64)) for x in xs])
    vals = np.zeros((3, 2), np.float32)
    with torch.no_grad():
        for i, (x, kept) in enumerate(zip(xs, ev.kept)):
            assert 'gumbel_u' not in kept
            tr.set_feed({'real_x_int': x, 'p_z_noise': kept['p_z_noise'], 'k_idx': np.argmax(kept['k_onehot'], axis=1)})
            out = tr.model.forward(tr.feed, 'gen')
            vals[i, 0] = float(out['gen_cost'])
            vals[i, 1] = float(out['rec_penalty'])
            tr.model.join_side()
    assert res['dev gen cost'] == float(np.mean(vals[:, 0])), (res, vals)
    assert res['dev rec cost'] == float(np.mean(vals[:, 1]))
    _fresh()
