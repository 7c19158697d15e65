"""-m gpu: the mixture scripts' global-critic MODEs (gmgan_inference_cifar10.py:39: ali, alice, vegan) on the HIP path.

  * the Linear on concat([z, k], 1) whose split is off the product kernels' tile grid (DIM_LATENT = 8: functional.Gemm2 through
    ggan_gemm_split's staged operands) against float64, forward and both gradients;
  * the reference's own runs (tests/golden/reference_trace_gmgan_global.json) replayed through engine.Trainer: registered parameters,
    the order of the optimizer runs, every run's cost, the first step's gradients, the final weights;
  * step graphs against eager steps; the evaluator's passes and a checkpoint round trip; the launch census of a step.
"""
import json
import os
import types

import numpy as np
import pytest

import test_reference_trace_cpu as RC
import test_reference_trace_gpu as RG
import test_mode_k_gpu as MK
from oracle import reftrace as RT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = json.load(open(os.path.join(HERE, 'golden', 'reference_trace_gmgan_global.json')))
ST = 'STRAIGHT_THROUGHT'
MODES = ('ali', 'alice', 'vegan')
_fresh = MK._fresh


# ---- the Linear on [z | k] ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', [0, 1])
@pytest.mark.parametrize('M,K1,K2', [(12, 8, 5), (100, 8, 30), (128, 8, 50), (16, 16, 5), (128, 128, 30), (12, 3, 1)])
def test_pair_input_linear_off_the_tile_grid_against_float64(gpu, M, K1, K2, act):
    """[a1 | a2] @ w + b (+ LeakyReLU) with a1 of 8 / 16 / 3 columns (staged by the library) and of 128 (read in place): the product and
    the gradients to both inputs, the weight and the bias against float64.  Bound: the rounding of a float32 dot product of n terms,
    n * 2^-24 * sum |terms|, times 8 for the order of summation the kernels are free to choose."""
    import torch
    from graphical_gan_amd import functional as F
    N = 512
    rng = np.random.default_rng(M * 1000 + K1 * 10 + K2)
    a1, a2 = rng.standard_normal((M, K1)).astype(np.float32), rng.standard_normal((M, K2)).astype(np.float32)
    w = (rng.standard_normal((K1 + K2, N)) / np.sqrt(K1 + K2)).astype(np.float32)
    b = (0.1 * rng.standard_normal(N)).astype(np.float32)
    g = rng.standard_normal((M, N)).astype(np.float32)
    t = lambda a: torch.as_tensor(a, device=gpu).requires_grad_(True)
    ta1, ta2, tw, tb = t(a1), t(a2), t(w), t(b)
    assert F.Gemm2.usable(ta1, ta2) and F.Gemm2.aligned(ta1, ta2) == (K1 % 64 == 0)
    out = F.Gemm2.apply(ta1, ta2, tw, tb, act, 0.2)
    d1, d2, dw, db = torch.autograd.grad(out, [ta1, ta2, tw, tb], grad_outputs=torch.as_tensor(g, device=gpu))
    torch.cuda.synchronize()
    A = np.concatenate([a1, a2], 1).astype(np.float64)
    W, G = w.astype(np.float64), g.astype(np.float64)
    pre = A @ W + b
    ref = np.where(pre > 0, pre, 0.2 * pre) if act else pre
    assert np.all(np.abs(pre) > 1e-6)                                   # (no pre-activation within rounding of the kink)
    Gp = G * np.where(pre > 0, 1.0, 0.2) if act else G
    eps = 2.0 ** -24

    def close(got, want, n, mag):
        err = np.abs(got.detach().cpu().numpy().astype(np.float64) - want)
        assert np.all(err <= 8 * n * eps * mag + 1e-30), (err.max(), (8 * n * eps * mag).min())
    K = K1 + K2
    close(out, ref, K + 1, np.abs(A) @ np.abs(W) + np.abs(b))
    dA, magA = Gp @ W.T, np.abs(Gp) @ np.abs(W.T)
    close(d1, dA[:, :K1], N, magA[:, :K1])
    close(d2, dA[:, K1:], N, magA[:, K1:])
    close(dw, A.T @ Gp, M, np.abs(A.T) @ np.abs(Gp))
    close(db, Gp.sum(0), M, np.abs(Gp).sum(0))


# ---- the reference's runs -----------------------------------------------------------------------------------------------------------
def _case(key):
    """(trace, product Config, the feeds of the runs with a train op, those runs) of a fixture case"""
    t = TRACE[key]
    script, mode = key.split(':')[:2]
    consts = dict(t['constants'], **t.get('script_constants', {}))
    cfg = RG._image_config('%s:%s' % (script, mode), consts)
    cfg.mode_k = t['mode_k']
    # what tests/test_reference_trace_cpu.roles_for / make_feed read of a configuration.  The mixture scripts draw the same random
    # nodes in all of these MODEs -- hyper_p_z, hyper_p_k, the Gumbel noise, celebA's dequantisation -- and none for a critic
    ocfg = types.SimpleNamespace(B=cfg.B, K=cfg.K, dim_latent=cfg.dim_latent, dataset=cfg.dataset, output_dim=cfg.output_dim, z_samples=100)
    roles, missing = RC.roles_for(ocfg, 'ali', t['random_nodes'])
    if t['mode_k'] == ST:
        assert 'gumbel_u' not in [r[0] for r in roles.values()]
        missing = [m for m in missing if m[1] != 'gumbel_u']
    assert not missing, missing
    runs = [r for r in t['runs'] if r['train']]
    for r in runs:                   # every random node the reference evaluated in a run has a role here
        assert {d[0] for d in r['draws']} <= set(roles), (key, r['draws'])
    feeds = [RC.make_feed(ocfg, 'ali', t, r, roles)[0] for r in runs]
    return t, cfg, feeds, runs


@pytest.mark.parametrize('key', sorted(TRACE))
def test_hip_path_replays_the_reference_global_critic_run(gpu, key):
    """test_mode_k_gpu.test_hip_path_replays_the_reference_mode_k_run on the global-critic fixture, with its tolerances (the float64
    shim against the float32 HIP path: cost 2e-5 on the initial weights and 2e-3 along the run, gradient digests 3e-4 of the tensor's
    scale, final weights by _final_check); every run's cost is compared, also each of vegan's five critic steps."""
    import torch
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.engine import Trainer
    t, cfg, feeds, runs = _case(key)
    _fresh()
    tr = Trainer(cfg, device=gpu, graph=False, inject_noise=True)
    assert ('gumbel_u' in tr.feed) == (t['mode_k'] != ST) and not [k for k in tr.feed if k.startswith('dn_')]
    assert cfg.critic_iters == t['critic_iters']
    # the registered parameters are the reference's, by name and shape: both step kinds built on the initial feed
    tr.set_feed(feeds[0])
    for which in ('disc', 'gen'):
        tr.model.forward(tr.feed, which)
        tr.model.join_side()
    ours = {n: list(p.shape) for n, p in lib.named_params().items()}
    theirs = dict(zip(t['names'], t['shapes']))
    assert ours == theirs, (sorted(set(ours) ^ set(theirs)), [k for k in ours if k in theirs and ours[k] != theirs[k]])
    W0 = {n: RT.det_weight(n, shp, np.float32) for n, shp in theirs.items()}
    tr.load_params(W0)
    # the order of the optimizer runs: critic steps alone, then generator step + critic steps
    order, it = [], 0
    while len(order) < len(runs):
        order += ([0] if it > 0 else []) + [1] * cfg.critic_iters
        it += 1
    assert [r['train'][0]['optimizer'] for r in runs] == order[:len(runs)] and len(order) == len(runs)
    # the first run (a critic step) on the initial weights: cost and every gradient digest, None where the reference has none
    first = runs[0]['train'][0]
    assert first['optimizer'] == 1
    ref_grads = dict(zip(t['names'], t['first_grads']))
    out = tr.model.forward(tr.feed, 'disc')
    c = float(out['disc_cost'].detach())
    print(key, 'first cost', c, first['cost'])
    assert abs(c - first['cost']) <= 2e-5 * max(1.0, abs(first['cost'])), (key, c, first['cost'])
    opt = out['disc_train_op'].optimizer
    assert sorted(p.param_name for p in opt.params) == sorted(n for n in t['names'] if n.startswith('Discriminator'))
    grads = [(g[0] + g[1]) if isinstance(g, tuple) else g for g in opt.compute_gradients(out['disc_cost'])]
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
    # the generator side has no gradient in the reference's critic step: none of it is in the critic's var_list here either
    assert not [n for n, d in ref_grads.items() if d is None and n.startswith('Discriminator')]
    del out, grads
    tr.model.join_side()
    # the loop, step by step through engine.Trainer: every fetched cost, then the final weights
    tr.load_params(W0)
    for r, feed in zip(runs, feeds):
        rec = r['train'][0]
        tr.set_feed(feed)
        v = float(tr.step('gen' if rec['optimizer'] == 0 else 'disc'))
        print(key, 'run', r['run'], rec['optimizer'], v, rec['cost'])
        assert abs(v - rec['cost']) <= 2e-3 * max(1.0, abs(rec['cost'])), (key, 'run', r['run'], rec['optimizer'], v, rec['cost'])
    tr.flush()
    P = tr.get_params()
    gall = max(g for g in t['gmax'] if g is not None)
    for n, shape, gs, dg in zip(t['names'], t['shapes'], t['gmax'], t['final']):
        if gs is not None and gs < 1e-9 * gall:
            continue                                     # (a mathematically zero gradient: Adam random-walks the tensor on rounding noise)
        MK._final_check(key, n, P[n], dg, W0[n], t['final_samples'])
    _fresh()
    torch.cuda.synchronize()


# ---- step graphs ----------------------------------------------------------------------------------------------------------------------
def _full(dataset, B, K, mode):
    from graphical_gan_amd.models import Config
    thin = mode == 'vegan'
    return Config(dataset, batch_size=B, n_coms=K, mode=mode, dim_latent=8 if thin else 128, bn=False if thin else None)


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dataset,K,B', [('cifar10', 30, 64), ('mnist', 30, 50)])
def test_step_graph_matches_eager(gpu, mode, dataset, K, B):
    """test_mode_k_gpu.test_step_graph_matches_eager in the global-critic MODEs: three iterations (vegan: 5 + 6 + 6 steps, so that both step
    kinds are replayed from their graphs) as step graphs and as eager steps give bit-identical costs and weights.  The two nets passes
    stay on one stream, as there."""
    import torch
    from graphical_gan_amd.engine import Trainer
    finals = []
    for graph in (False, True):
        _fresh()
        np.random.seed(0)
        tr = Trainer(_full(dataset, B, K, mode), device=gpu, graph=graph, seed=4321)
        assert tr.cfg.critic == ('latent' if mode == 'vegan' else 'global')
        tr.model.fork_nets = False
        batches = iter(tr.model.synthetic_ring(gpu, n=5, seed=99) * 40)
        for it in range(3):
            res = tr.iteration(it, batches)
        tr.flush()
        torch.cuda.synchronize()
        finals.append(({k: v.copy() for k, v in tr.get_params().items()}, {k: float(v) for k, v in res.items()}))
    assert finals[0][1] == finals[1][1] and set(finals[0][1]) == {'gen_cost', 'disc_cost'}
    assert all(np.isfinite(v) for v in finals[0][1].values())
    for k in finals[0][0]:
        assert np.array_equal(finals[0][0][k], finals[1][0][k]), k
    _fresh()


# ---- everything above the step -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', MODES)
def test_evaluator_passes_and_checkpoint(gpu, mode, tmp_path):
    """one small trainer per MODE, its average of the generator-side weights on: the due passes return the documented keys with finite
    values -- dev rec / reg cost only where the MODE has a reconstruction term --, the sample grid has one column per component, the
    reconstruction pairs, clustering accuracy, a set-level score and the probe run, and a checkpoint round-trips, ema/gen/* included."""
    import torch
    from graphical_gan_amd import checkpoint
    from graphical_gan_amd.models import Config
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.evaluate import Evaluator
    B, K, dl = 8, 5, (8 if mode == 'vegan' else 16)
    mk = lambda: Trainer(Config('cifar10', batch_size=B, n_coms=K, mode=mode, dim=8, dim_latent=dl, bn=False if mode == 'vegan' else None),
                         device=gpu, graph=True, seed=4321, ema_decay=0.9)
    _fresh()
    np.random.seed(0)
    tr = mk()
    batches = iter(tr.model.synthetic_ring(gpu, n=5, seed=99) * 40)
    for it in range(3):
        res = tr.iteration(it, batches)
    assert set(res) == {'gen_cost', 'disc_cost'} and all(np.isfinite(float(v)) for v in res.values())
    rng = np.random.default_rng(3)
    dev = [(rng.integers(0, 256, size=(B, 3072)).astype(np.int32), rng.integers(0, 10, size=B)) for _ in range(4)]
    ev = Evaluator(tr, dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, N_VIS=2 * K, PROBE_FIT_ROWS=2 * B))
    costs = ev.dev_costs(dev)
    want = {'dev gen cost'} | ({'dev rec cost', 'dev reg cost'} if mode in ('alice', 'vegan') else set())
    assert set(costs) == want and all(np.isfinite(v) for v in costs.values()), costs
    grid = ev.sample_grid()
    assert grid.shape == (2 * K, 3072) and np.all(np.isfinite(grid)) and np.abs(grid).max() <= 1.0
    assert np.array_equal(ev.fixed_k.cpu().numpy(), np.tile(np.eye(K, dtype=np.float32), (2, 1)))    # (row r is component r % K: one per column)
    real, rec = ev.reconstructions(dev[0])
    assert real.shape == rec.shape == (B, 3072) and np.all(np.isfinite(rec))
    acc = ev.cluster_accuracy(dev)
    assert 0.0 <= acc <= 1.0
    scores = ev.set_scores(dev, mmd=True)
    assert scores and all(np.isfinite(v) for v in scores.values()), scores
    probe = ev.probe_scores(dev[:2], dev[2:])
    assert probe and all(np.isfinite(v) for v in probe.values()), probe
    paths = ev.save_images(str(tmp_path), 0)
    assert len(paths) == 2 and all(os.path.getsize(p) > 0 for p in paths)
    # the checkpoint: parameters, both optimizers' state, the average -- restored into a fresh trainer bit for bit
    path = str(tmp_path / 'ckpt.npz')
    keys = checkpoint.save(path, tr)
    assert 'ema/gen/Generator.Hyper.Mu' in keys and 'ema/gen/decay' in keys and 'adam/gen/step' in keys and 'adam/disc/step' in keys
    assert not [k for k in keys if k.startswith('ema/gen/Discriminator')]
    PA, EA = tr.get_params(), tr.get_params(weights='ema')
    assert any(not np.array_equal(PA[n], EA[n]) for n in EA)
    res_a = tr.iteration(3, batches)
    tr.flush()
    PA2 = {k: v.copy() for k, v in tr.get_params().items()}
    _fresh()
    np.random.seed(0)
    tr2 = mk()
    b2 = iter(tr2.model.synthetic_ring(gpu, n=5, seed=99) * 40)
    for it in range(3):
        tr2.iteration(it, b2)
    checkpoint.restore(path, tr2)
    P2, E2 = tr2.get_params(), tr2.get_params(weights='ema')
    assert sorted(P2) == sorted(PA) and all(np.array_equal(P2[n], PA[n]) for n in PA)
    assert sorted(E2) == sorted(EA) and all(np.array_equal(E2[n], EA[n]) for n in EA)
    res_b = tr2.iteration(3, b2)
    tr2.flush()
    torch.cuda.synchronize()
    assert {k: float(v) for k, v in res_a.items()} == {k: float(v) for k, v in res_b.items()}
    P3 = tr2.get_params()
    assert all(np.array_equal(P3[n], PA2[n]) for n in PA2)
    _fresh()


# ---- the launch census -----------------------------------------------------------------------------------------------------------------
# aten operators that launch nothing: allocations, views and aliases.  Every other operator torch runs on a device tensor during a step
# (a copy, a fill, an addition, a concatenation ...) is torch-composed work on the step path.
_NO_LAUNCH = {'empty.memory_format', 'empty_like.default', 'empty_strided.default', 'new_empty.default', 'new_empty_strided.default',
              'view.default', '_unsafe_view.default', 'reshape.default', '_reshape_alias.default', 'view_as.default', 'detach.default',
              'alias.default', 'slice.Tensor', 'select.int', 'as_strided.default', 'set_.source_Storage_storage_offset',
              'set_.source_Storage', 't.default', 'transpose.int', 'permute.default', 'expand.default', 'unsqueeze.default',
              'squeeze.default', 'squeeze.dim', 'split.Tensor', 'unbind.int', 'lift_fresh.default', 'is_same_size.default',
              'sym_size.int', 'sym_numel.default', 'sym_stride.int', 'sym_storage_offset.default', 'is_pinned.default',
              'record_stream.default', '_local_scalar_dense.default'}


def _census(fn):
    """the aten operators with a device tensor among their arguments or results that run during fn() (forward and backward threads
    alike), beyond _NO_LAUNCH, with their counts; and the library entry points fn() called, {name: calls}"""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from torch.utils._pytree import tree_leaves
    from graphical_gan_amd import _lib
    seen = {}

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types_, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            name = str(func).replace('aten.', '', 1)
            on_dev = any(torch.is_tensor(x) and x.is_cuda for x in tree_leaves((args, kwargs or {}, out)))
            if on_dev and name not in _NO_LAUNCH:
                seen[name] = seen.get(name, 0) + 1
            return out
    L, calls = _lib.load(), {}
    names = [n for n in _lib.SIGNATURES if n not in ('ggan_version', 'ggan_last_error')]
    saved = {n: getattr(L, n) for n in names}

    def counted(name, entry):
        def call(*a):
            calls[name] = calls.get(name, 0) + 1
            return entry(*a)
        return call
    for n in names:
        setattr(L, n, counted(n, saved[n]))
    try:
        with Watch():
            fn()
            torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(L, n, saved[n])
    return seen, calls


def _crop_operators(gpu):
    """what torch itself runs for the MNIST Generator's crop out[:, :, :7, :7] (gmgan_inference_mnist.py:179, models.Generator) and its
    backward, found by running that expression alone: the crop is a slice and a copy in every MODE of the MNIST scripts, local_ep
    included, and no part of the critics.  The census of an MNIST step may hold these operators, once per Generator pass, and no other."""
    import torch
    x = torch.zeros(2, 3, 8, 8, device=gpu, requires_grad=True)
    g = torch.ones(2, 3, 7, 7, device=gpu)

    def crop():
        y = x[:, :, :7, :7].contiguous()
        torch.autograd.grad(y, [x], grad_outputs=g)
    seen, calls = _census(crop)
    assert not calls and 'clone.default' in seen
    return seen


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('dataset,K,B', [('cifar10', 30, 64), ('mnist', 30, 50)])
def test_a_step_is_library_launches_only(gpu, mode, dataset, K, B):
    """both step kinds of each new MODE at the scripts' sizes, issued as the capture issues them (eager steps behind the warm-up): torch
    runs no operator on a device tensor but allocations and views -- every launch of the step is an entry point of this library.  Read
    from the operators torch dispatches (forward, backward, pack and update) and from the library's call records, the way
    test_step_gpu's fused_launches checks count entry points.  MNIST: but for the Generator's crop (_crop_operators), at most twice -- a
    step runs the Generator on p_z and, with a reconstruction term, on q_z."""
    import torch
    from graphical_gan_amd.engine import Trainer
    crop = _crop_operators(gpu) if dataset == 'mnist' else {}
    _fresh()
    np.random.seed(0)
    tr = Trainer(_full(dataset, B, K, mode), device=gpu, graph=False, seed=4321)
    batches = iter(tr.model.synthetic_ring(gpu, n=5, seed=99) * 40)
    for it in range(2):                                   # (both step kinds built, the optimizers exist)
        tr.iteration(it, batches)
    for which in ('disc', 'gen'):
        tr.set_batch(next(batches))
        seen, calls = _census(lambda: tr.step(which))
        n = sum(calls.values())
        print(dataset, mode, which, 'library calls', n, 'torch operators', seen, 'crop', crop)
        # (a step is at least the noise launch, the Extractor's four layers, the critic's three and their backward, pack and update)
        assert n >= 10, (which, calls)
        # the pair-input Linear on [z | k] went through the two-source product, and MODE ali's one head took its cost as a hint: the
        # head's own forward and backward entry points ran once each, the launch that carries an unhinted head's backward did not
        assert calls.get('ggan_gemm_split', 0) >= 1, (which, calls)
        if mode == 'ali':
            assert (calls.get('ggan_critic_head_fwd_bce'), calls.get('ggan_critic_head_bwd_tail'), calls.get('ggan_bce_heads_bwd')) == (1, 1, None), calls
        extra = {k: v for k, v in seen.items() if v > 2 * crop.get(k, 0)}
        assert not extra, (dataset, mode, which, extra)
    tr.flush()
    torch.cuda.synchronize()
    _fresh()
