"""-m gpu: BatchNorm in the state-space scripts (BN_FLAG, ssgan_inference_moving_mnist.py:31-34) on the HIP path.

  * ggan_bn_split_fwd_train / ggan_bn_split_bwd_act (functional.BatchNormGroupedTrain) against float64 torch, forward and backward,
    groups 1 and 2, act none / relu / lrelu, rows and NCHW layouts, at the full-size shapes of the nets and at awkward ones;
  * variance of inputs with a large mean, bit-identical reruns and graph replays, the data-gradient skip of trailing groups;
  * the reference's own BN_FLAG = True runs (tests/golden/reference_trace_ssgan_bn.json) replayed through engine.Trainer;
  * step graphs against eager steps, and a few full-size iterations.
"""
import json
import os

import numpy as np
import pytest

from oracle import reftrace as RT

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TRACE = json.load(open(os.path.join(HERE, 'golden', 'reference_trace_ssgan_bn.json')))
ACTS = {'none': 0, 'lrelu': 1, 'relu': 2}


def _fresh():
    from graphical_gan_amd import tflib as lib, optim
    optim.reset_optimizers()
    lib.delete_all_params()


def _ref(x, scale, offset, act, groups, eps=1e-5):
    """float64 torch: each of `groups` leading parts normalised with its own biased batch statistics"""
    import torch
    N, C = x.shape[0], x.shape[1]
    xg = x.reshape(groups, N // groups, C, -1)
    mean = xg.mean(dim=(1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = (xg - mean) / torch.sqrt(var + eps) * scale.reshape(1, 1, C, 1) + offset.reshape(1, 1, C, 1)
    if act == 'relu':
        y = torch.relu(y)
    elif act == 'lrelu':
        y = torch.maximum(0.2 * y, y)
    return y.reshape(x.shape)


def _run(gpu, shape, groups, act, mean=0.0, seed=0, grad_rows=None):
    import torch
    from graphical_gan_amd import functional as F
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = (torch.randn(shape, generator=g, dtype=torch.float64) + mean).float().double()     # (the float64 side sees the float32 inputs)
    sc = 1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    of = 0.2 * torch.randn(C, generator=g, dtype=torch.float64)
    gy = torch.randn(shape, generator=g, dtype=torch.float64)
    xs = [t.to(gpu, torch.float32).requires_grad_(True) for t in (x, sc, of)]
    y = F.BatchNormGroupedTrain.apply(xs[0], xs[1], xs[2], 1e-5, ACTS[act], 0.2, groups, grad_rows)
    gx, gs, go = torch.autograd.grad(y, xs, gy.to(gpu, torch.float32))
    return (x, sc, of, gy), (y.detach(), gx, gs, go)


def _close(got, ref, tol, what):
    got = got.double().cpu()
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max()) + 1e-30
    assert err <= tol * scale, (what, err, scale)


SHAPES = [
    (65536, 64), (8192, 128), (1024, 256),                          # the 3dcnn critic's volumes as [rows, C] (B 32, LEN 16, DIM 32)
    (1024, 64, 16, 16), (512, 32, 32, 32),                          # the frame critic's BN2, the frame generator's BN4
    (1000, 40), (30, 3, 5, 7), (2, 37), (2, 5, 3, 3), (4098, 33),   # C not a multiple of 32, ragged slabs, one row per group
]


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('groups', [1, 2])
@pytest.mark.parametrize('act', sorted(ACTS))
def test_grouped_bn_matches_float64(gpu, shape, groups, act):
    import torch
    (x, sc, of, gy), (y, gx, gs, go) = _run(gpu, shape, groups, act)
    xr, scr, ofr = (t.clone().requires_grad_(True) for t in (x, sc, of))
    yr = _ref(xr, scr, ofr, act, groups)
    gxr, gsr, gor = torch.autograd.grad(yr, (xr, scr, ofr), gy)
    _close(y, yr.detach(), 2e-6, 'y')
    _close(gx, gxr, 5e-5, 'gx')
    _close(gs, gsr, 5e-5, 'gscale')
    _close(go, gor, 5e-5, 'goffset')


@pytest.mark.parametrize('shape', [(65536, 64), (512, 32, 32, 32), (30, 3, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_grouped_bn_variance_with_large_mean(gpu, shape):
    """mean 1e3, std 1: E[x^2] - E[x]^2 in float32 would lose the variance to cancellation (an error of ~1e6 * 6e-8 = 0.06 on a
    variance of 1, ~3 % of every output); the slab means + Chan's merge stay within 2e-5 of |y| -- the float32 mean itself is only
    known to half an ulp of 1e3 (3e-5), which bounds any float32 kernel here"""
    import torch
    # (no activation: a LeakyReLU mask flips wherever the affine output lies within the mean's rounding of zero -- a kink, not the
    #  variance, decides those entries)
    (x, sc, of, gy), (y, gx, gs, go) = _run(gpu, shape, 2, 'none', mean=1e3)
    xr, scr, ofr = (t.clone().requires_grad_(True) for t in (x, sc, of))
    yr = _ref(xr, scr, ofr, 'none', 2)
    gxr, gsr, _ = torch.autograd.grad(yr, (xr, scr, ofr), gy)
    _close(y, yr.detach(), 2e-5, 'y')
    _close(gx, gxr, 1e-4, 'gx')
    _close(gs, gsr, 1e-4, 'gscale')


@pytest.mark.parametrize('shape', [(65536, 64), (1024, 64, 16, 16)], ids=lambda s: 'x'.join(map(str, s)))
def test_grouped_bn_bit_identical_reruns_and_graph_replay(gpu, shape):
    import torch
    from graphical_gan_amd import functional as F
    torch.manual_seed(0)
    x = torch.randn(shape, device=gpu)
    sc, of = torch.rand(shape[1], device=gpu) + .5, torch.randn(shape[1], device=gpu)
    gy = torch.randn(shape, device=gpu)

    def step():
        xs = [t.clone().requires_grad_(True) for t in (x, sc, of)]
        y = F.BatchNormGroupedTrain.apply(xs[0], xs[1], xs[2], 1e-5, 1, 0.2, 2, None)
        return (y.detach(),) + torch.autograd.grad(y, xs, gy)
    a, b = step(), step()
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()                                   # (the workspace of this stream exists before capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = step()
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, out):
        assert torch.equal(u, v)


@pytest.mark.parametrize('shape', [(4096, 64), (64, 32, 8, 8)], ids=lambda s: 'x'.join(map(str, s)))
def test_grouped_bn_skips_trailing_data_gradient(gpu, shape):
    """grad_rows = the first group: its gx as without the skip, the second group's gx left as it was, scale / offset gradients
    unchanged -- and without parameter gradients the trailing gy is not read (NaN there changes nothing)"""
    import torch
    from graphical_gan_amd import _lib
    from graphical_gan_amd.functional import _core as K
    torch.manual_seed(1)
    N, C = shape[0], shape[1]
    HW = int(np.prod(shape[2:])) if len(shape) > 2 else 1
    x = torch.randn(shape, device=gpu)
    sc, of = torch.rand(C, device=gpu) + .5, torch.randn(C, device=gpu)
    gy = torch.randn(shape, device=gpu)
    mean, inv = torch.empty((2, C), device=gpu), torch.empty((2, C), device=gpu)
    y = torch.empty_like(x)
    L, ws, p = K._L(), K.workspace(x.device), K._p
    _lib.check(L.ggan_bn_split_fwd_train(p(x), p(sc), p(of), p(y), p(mean), p(inv), N, C, HW, 2, 1e-5, 1, 0.2, p(ws), ws.numel(),
                                         K._stream()), 'fwd')

    def bwd(gyv, gx_groups, want_params):
        gx = torch.full_like(x, 7.0)
        gs = torch.full((C,), 7.0, device=gpu) if want_params else None
        go = torch.full((C,), 7.0, device=gpu) if want_params else None
        _lib.check(L.ggan_bn_split_bwd_act(p(x), p(gyv), 1, 0.2, p(sc), p(of), p(mean), p(inv), p(gx), p(gs), p(go), p(None), N, C, HW,
                                           2, gx_groups, p(ws), ws.numel(), K._stream()), 'bwd')
        return gx, gs, go
    full = bwd(gy, 2, True)
    skip = bwd(gy, 1, True)
    h = N // 2
    assert torch.equal(skip[0][:h], full[0][:h])
    assert bool((skip[0][h:] == 7.0).all())
    assert torch.equal(skip[1], full[1]) and torch.equal(skip[2], full[2])
    gy_nan = gy.clone()
    gy_nan[h:] = float('nan')
    lean = bwd(gy_nan, 1, False)
    assert torch.equal(lean[0][:h], full[0][:h])
    assert bool((lean[0][h:] == 7.0).all())


def test_grouped_bn_refuses_a_double_backward(gpu):
    import torch
    from graphical_gan_amd import functional as F
    x = torch.randn(8, 4, device=gpu, requires_grad=True)
    sc, of = torch.ones(4, device=gpu, requires_grad=True), torch.zeros(4, device=gpu, requires_grad=True)
    y = F.BatchNormGroupedTrain.apply(x, sc, of, 1e-5, 0, 0.0, 2, None)
    with pytest.raises(NotImplementedError):
        torch.autograd.grad((y * y).sum(), x, create_graph=True)


def test_sync_group_refuses_grouped_bn(gpu):
    import torch
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.tflib.ops import batchnorm as BN
    _fresh()
    old = BN._SYNC_GROUP
    BN._SYNC_GROUP = object()          # (any process group: the refusal comes before it is used)
    try:
        with pytest.raises(NotImplementedError):
            lib.ops.batchnorm.Batchnorm('T.BN', [0, 1, 2, 3], torch.randn(2, 2, 3, 3, 4, device=gpu), groups=2)
    finally:
        BN._SYNC_GROUP = old
        _fresh()


# ---- the reference's runs ---------------------------------------------------------------------------------------------------
def _ss_case(t):
    """(constructor keywords, runs with a train op, feeds of those runs): test_reference_trace_cpu.ss_case on this fixture"""
    c = dict(t['script_constants'], **t['constants'])
    chairs = c.get('N_C', 0) == 0
    kw = dict(batch_size=c['BATCH_SIZE'], length=c['LEN'], dim=c['DIM'], dim_op=c['DIM_OP'], dim_g=c['DIM_LATENT_G'], dim_l=c['DIM_LATENT_L'],
              n_c=c.get('N_C', 0), channels=3 if chairs else 1, op_dyn_mode='res_w' if chairs else 'res', mode=c['MODE'],
              ali_mode=t['ali_mode'] or 'concat_x', bn_g=True, bn_e=True, bn_d=True)
    B, n_c, dim_l, dim_g = kw['batch_size'], kw['n_c'], kw['dim_l'], kw['dim_g']
    order = {('normal', (B, dim_l)): ['p_z_l_0', 'epsilon'], ('normal', (B, dim_g)): ['p_z_g'], ('categorical', (B,)): ['p_y_idx']}
    roles, seen = {}, {}
    for nid, kind, shape in t['random_nodes']:
        sig = (kind, tuple(shape))
        i = seen.get(sig, 0)
        seen[sig] = i + 1
        if sig in order and i < len(order[sig]):
            roles[nid] = (order[sig][i], kind, tuple(shape))
    runs = [r for r in t['runs'] if r['train']]
    feeds = []
    for j, r in enumerate(runs):
        d = [x for x in r['feeds'] if x['stream']][0]
        assert d['index'] == j
        x = RT.det_batch(d['stream'], d['index'], (d['spec'][0], tuple(d['spec'][1])))
        feed = {'real_x_unit': x.astype(np.float64)}
        y = np.zeros((B, n_c), np.float32)
        if n_c:
            y[np.arange(B), RT.det_batch(d['stream'] + '/y', d['index'], ('label', B, n_c))] = 1
        feed['real_y'] = y
        feed['p_y'] = np.zeros((B, n_c), np.float32)
        assert set(x[0] for x in r['draws']) <= set(roles), r['draws']
        for nid, (name, kind, shape) in roles.items():
            v = RT.det_noise(r['run'], nid, kind, shape, n_c or None)
            if name == 'p_y_idx':
                feed['p_y'][np.arange(B), v] = 1
            else:
                feed[name] = v
        feeds.append(feed)
    return kw, runs, feeds


def _final_check(key, name, mine, ref_digest, w0, count):
    """test_mode_k_gpu._final_check: ||P - P_ref|| <= 0.02 ||P_ref - P_0|| + an fp32 floor on the kept entries, the norm to 1e-4"""
    m = RT.digest(name, mine, count)
    assert abs(m[0] - ref_digest[0]) <= 1e-4 * max(ref_digest[0], 1e-3) + 1e-6, (key, name, m[0], ref_digest[0])
    start = w0.astype(np.float64).ravel()[RT.sample_positions(name, w0.size, count)]
    ref, got = np.asarray(ref_digest[2:]), np.asarray(m[2:])
    floor = 4e-7 * (np.abs(ref).max() + 1e-3) * np.sqrt(count)
    assert np.linalg.norm(got - ref) <= 0.02 * np.linalg.norm(ref - start) + floor, (key, name, 'entries')


@pytest.mark.parametrize('key', sorted(TRACE))
def test_hip_path_replays_the_reference_bn_run(gpu, key):
    """test_reference_trace_gpu.test_hip_path_replays_the_state_space_reference_run with BN_FLAG = True: the product registry is the
    reference's (names, shapes), the first run's cost and gradients, every cost of the loop, the weights after the last run"""
    import torch
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    t = TRACE[key]
    kw, runs, feeds = _ss_case(t)
    cfg = SSConfig(dataset='chairs' if 'chairs' in key else 'moving_mnist', **kw)
    _fresh()                                       # the registry the nets build on their own: the reference's names and shapes
    tr = Trainer(cfg, device=gpu, graph=False, inject_noise=True, model=StateSpaceGAN(cfg))
    tr.set_feed(feeds[0])
    for which in ('disc', 'gen'):
        tr.model.forward(tr.feed, which)
    assert {n: list(p.shape) for n, p in lib.named_params().items()} == dict(zip(t['names'], t['shapes'])), key
    _fresh()
    tr = Trainer(cfg, device=gpu, graph=False, inject_noise=True, model=StateSpaceGAN(cfg))
    W0 = {n: RT.det_weight(n, shp, np.float32) for n, shp in zip(t['names'], t['shapes'])}
    tr.load_params(W0)
    tr.set_feed(feeds[0])
    first = runs[0]['train'][0]
    ref_grads = dict(zip(t['names'], t['first_grads']))
    which = 'disc' if first['optimizer'] == 1 else 'gen'
    out = tr.model.forward(tr.feed, which)
    c = float(out[which + '_cost'].detach())
    assert abs(c - first['cost']) <= 2e-5 * max(1.0, abs(first['cost'])), (key, c, first['cost'])
    opt = out[which + '_train_op'].optimizer
    grads = torch.autograd.grad(out[which + '_cost'], opt.params, allow_unused=True)
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
    tr.load_params(W0)
    it_feeds, j, it = iter(feeds), 0, 0
    while j < len(runs):
        res = tr.iteration(it, it_feeds)
        for name in (['gen_cost'] if it > 0 else []) + ['disc_cost']:
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


# ---- step graphs, full size -------------------------------------------------------------------------------------------------
def _trainer(gpu, graph, mode, ali_mode, B, L, dim, bn=True):
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    _fresh()
    np.random.seed(0)
    cfg = SSConfig(batch_size=B, length=L, dim=dim, mode=mode, ali_mode=ali_mode, bn_g=bn, bn_e=bn, bn_d=bn)
    return Trainer(cfg, device=gpu, graph=graph, seed=4321, model=StateSpaceGAN(cfg))


def _adam_states():
    from graphical_gan_amd import optim
    return [(k[0], o.state_dict()) for k, o in sorted(optim._optimizers.items(), key=lambda kv: kv[0][0])]


@pytest.mark.parametrize('mode,ali_mode', [('local_ep', 'concat_x'), ('ali', '3dcnn')])
def test_bn_step_graph_matches_eager(gpu, mode, ali_mode):
    """4 iterations (the first eager in both, as the Trainer rehearses; then 3 graph replays) with the nets on two streams
    (fork_nets): bit-identical weights and Adam state"""
    import torch
    finals = []
    for graph in (False, True):
        tr = _trainer(gpu, graph, mode, ali_mode, 4, 4, 8)
        assert tr.model.fork_nets
        ring = tr.model.synthetic_ring(gpu)
        feeds = iter(ring * 4)
        for it in range(4):
            tr.iteration(it, feeds)
        torch.cuda.synchronize()
        finals.append((tr.get_params(), _adam_states()))
    (pa, sa), (pb, sb) = finals
    assert pa.keys() == pb.keys()
    for n in pa:
        assert np.array_equal(pa[n], pb[n]), n
    assert [r for r, _ in sa] == [r for r, _ in sb]
    for (r, a), (_, b) in zip(sa, sb):
        for k in a:
            assert torch.equal(a[k], b[k]), (r, k)
    _fresh()


@pytest.mark.parametrize('mode,ali_mode', [('local_ep', 'concat_x'), ('ali', '3dcnn')])
def test_bn_full_size_iterations_stay_finite(gpu, mode, ali_mode):
    import torch
    tr = _trainer(gpu, True, mode, ali_mode, 32, 16, 32)
    feeds = iter(tr.model.synthetic_ring(gpu) * 4)
    for it in range(5):
        res = tr.iteration(it, feeds)
        for k in ('gen_cost', 'disc_cost'):
            if k in res:
                assert np.isfinite(float(res[k])), (it, k, res[k])
    torch.cuda.synchronize()
    _fresh()
