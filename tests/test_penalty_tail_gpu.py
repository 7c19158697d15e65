"""-m gpu: the wali-gp penalty pass's shortened tail -- ggan_head_seed_fwd and functional.HeadInputGrad against the plain
composition they replace (bit for bit; second order also at TOL2 of tests/test_second_order_gpu.py against float64), ggan_gp_penalty_fwd_grad against the two launches it stands for (bit for
bit), and one critic step on both routes (GGAN_NO_PENALTY_SEED), eager and as a captured graph.
"""
import ctypes as C

import numpy as np
import pytest

from test_ops_gpu import TOL, _rel, _t
from test_second_order_gpu import TOL2, _check2, _masked, _np, registry  # noqa: F401  (registry: a fixture)

pytestmark = pytest.mark.gpu

ALPHA = 0.2
SEED_CASES = [(1, 1), (3, 5), (64, 512), (7, 515)]


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _at(a, off, gpu, pad=3, fill=777.0):
    """the array on the device, `off` floats behind a 16-byte boundary, inside a buffer filled with `fill` -> (view, whole buffer)"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    buf = torch.full((off + a.size + pad,), fill, dtype=torch.float32, device=gpu)
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.as_tensor(a))
    assert view.data_ptr() % 16 == 4 * off
    return view, buf


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _seed_operands(M, H, with_u, rng):
    """h with +0, -0, negatives and denormals of both signs; w_out with 0 and -0 (H == 1: -0 alone)"""
    h = rng.standard_normal((M, H)).astype(np.float32)
    special = np.array([0.0, -0.0, -1.5, 1e-40, -1e-40], dtype=np.float32)
    n = min(h.size, special.size)
    h.reshape(-1)[:n] = special[:n] if h.size > 1 else special[1:2]
    w_out = rng.standard_normal((H, 1)).astype(np.float32)
    w_out[-1, 0] = -0.0
    if H >= 3:
        w_out[-2, 0] = 0.0
    u = rng.standard_normal(M).astype(np.float32) if with_u else None
    return h, w_out, u


@pytest.mark.parametrize('off', [0, 1])
@pytest.mark.parametrize('with_u', [False, True], ids=['ones', 'u'])
@pytest.mark.parametrize('M,H', SEED_CASES)
def test_head_seed_fwd_is_the_one_deep_product_and_act_bwd(gpu, M, H, with_u, off):
    """ggan_head_seed_fwd == Gemm(u[:, None], w_out, tb=True) -> ActBwd, bit for bit (signed zeros included), on 16-byte aligned operands
    (H a multiple of 4: float4 accesses) and one float behind a boundary (scalar accesses); nothing written outside gpre"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    h, w_out, u = _seed_operands(M, H, with_u, np.random.default_rng(100 * M + H))
    tu = _t(u if with_u else np.ones(M, np.float32), gpu)
    ref = F.ActBwd.apply(F.Gemm.apply(tu.view(M, 1), _t(w_out, gpu), None, False, True, F.ACT_NONE, 0.0), _t(h, gpu), F.ACT_LRELU, ALPHA)
    (dh, _), (dw, _), (du, _) = _at(h, off, gpu), _at(w_out, off, gpu), _at(u if with_u else np.zeros(M), off, gpu)
    out, buf = _at(np.zeros((M, H)), off, gpu)
    _lib.check(_lib.load().ggan_head_seed_fwd(M, H, _p(du if with_u else None), _p(dh), _p(dw), ALPHA, _p(out), _stream()), 'ggan_head_seed_fwd')
    torch.cuda.synchronize()
    assert _same_bits(out, ref), float((out - ref).abs().max())
    assert float((buf[:off] - 777.0).abs().sum()) == 0.0 and float((buf[off + M * H:] - 777.0).abs().sum()) == 0.0


@pytest.mark.parametrize('M,K1,K2,H', [(5, 64, 3, 12), (64, 128, 64, 512)])
def test_head_input_grad_against_the_composition(gpu, registry, M, K1, K2, H):
    """functional.HeadInputGrad against LinearLReLULinear(differentiable=True) + autograd.grad under data_grad_only on the same operands:
    d_a1 bit for bit; the gradients of <d_a1, v> w.r.t. w and w_out at TOL2 of the float64 tape and equal to the composition's bit for
    bit (TOL asked for; they are the composition's own launches); none w.r.t. b, a1, a2; and no third derivative"""
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd.tflib.ops.linear import LinearLReLULinear
    from oracle import tape as tp
    lib = registry
    rng = np.random.default_rng(M + H)
    x1, x2 = rng.standard_normal((M, K1)).astype(np.float32), rng.standard_normal((M, K2)).astype(np.float32)
    LinearLReLULinear('T.1', K1 + K2, H, 'T.2', (_t(x1, gpu), _t(x2, gpu)), differentiable=True)
    P = {n: lib.param(n) for n in ('T.1.W', 'T.1.b', 'T.2.W', 'T.2.b')}
    with torch.no_grad():
        P['T.1.b'].copy_(_t(0.3 * rng.standard_normal(H), gpu))
        P['T.2.b'].copy_(_t(0.3 * rng.standard_normal(1), gpu))
    val = {n: _np(p).astype(np.float64) for n, p in P.items()}
    v = _t(rng.standard_normal((M, K1)), gpu)
    # the composition
    c1, c2 = _t(x1, gpu).requires_grad_(True), _t(x2, gpu).requires_grad_(True)
    d_hat = LinearLReLULinear('T.1', K1 + K2, H, 'T.2', (c1, c2), differentiable=True)
    with F.data_grad_only():
        (g_old,) = torch.autograd.grad(d_hat, [c1], grad_outputs=F.cached_const(1.0, d_hat.shape, gpu), create_graph=True)
    old = torch.autograd.grad((g_old * v).sum(), [P['T.1.W'], P['T.2.W']])
    # the op
    a1, a2 = _t(x1, gpu).requires_grad_(True), _t(x2, gpu).requires_grad_(True)
    with F.data_grad_only():         # (as the penalty pass calls it: the hint is for backward passes, the forward ignores it)
        g_new = F.HeadInputGrad.apply(a1, a2, P['T.1.W'], P['T.1.b'], P['T.2.W'], ALPHA)
    assert g_new.requires_grad and _same_bits(g_new, g_old), float((g_new - g_old).abs().max())
    new = torch.autograd.grad((g_new * v).sum(), [P['T.1.W'], P['T.2.W'], P['T.1.b'], a1, a2], allow_unused=True)
    for n, got in zip(('T.1.b', 'a1', 'a2'), new[2:]):
        assert got is None or float(got.abs().max()) == 0.0, n
    # float64: the tail with the kernel's own activation mask, differentiated twice
    hid = _np(F.Gemm2.apply(_t(x1, gpu), _t(x2, gpu), P['T.1.W'], P['T.1.b'], F.ACT_LRELU, ALPHA))
    R = dict(x1=tp.T(x1.astype(np.float64)), x2=tp.T(x2.astype(np.float64)))
    Wt = {n: tp.T(a) for n, a in val.items()}
    pre = tp.add(tp.matmul(tp.concat([R['x1'], R['x2']], 1), Wt['T.1.W']), tp.reshape(Wt['T.1.b'], (1, H)))
    yr = tp.reshape(tp.add(tp.matmul(_masked(pre, hid, 'lrelu', ALPHA), Wt['T.2.W']), tp.reshape(Wt['T.2.b'], (1, 1))), (M,))
    (r1,) = tp.grad(tp.reduce_sum(yr), [R['x1']])
    assert _rel(_np(g_new).astype(np.float64), r1.v) < TOL
    refs = tp.grad(tp.reduce_sum(tp.mul(r1, tp.T(_np(v).astype(np.float64)))), [Wt['T.1.W'], Wt['T.2.W']])
    for n, got, was, ref in zip(('T.1.W', 'T.2.W'), new[:2], old, refs):
        _check2(('HeadInputGrad', n), got, ref)
        e = _rel(_np(got), _np(was))
        print('HeadInputGrad', (M, K1, K2, H), n, 'vs composition', e)
        assert e < TOL, (n, e)
        # (the same launches on the same operands: not only close -- a gradient that differs in its last bits moves the weights of a long run)
        assert _same_bits(got.reshape(was.shape), was), (n, e)
    with pytest.raises(RuntimeError):
        g3 = F.HeadInputGrad.apply(a1, a2, P['T.1.W'], P['T.1.b'], P['T.2.W'], ALPHA)
        (d3,) = torch.autograd.grad((g3 * v).sum(), [P['T.2.W']], create_graph=True)
        torch.autograd.grad(d3.sum(), [P['T.1.W']])


@pytest.mark.parametrize('B,D', [(1, 1), (3, 255), (2, 257), (64, 3072), (2, 4097)])
def test_gp_fwd_grad_keeps_its_bits(gpu, B, D):
    """ggan_gp_penalty_fwd_grad == ggan_gp_penalty_fwd + ggan_gp_penalty_bwd with a unit seed: slopes, penalty and gradient bit for bit,
    twice in a row (the arrival counter is back at zero), at one thread, just under and over one pass of the workgroup, the critic's
    row and a row of more than 16 passes.  (The kernel is as it was: a variant that kept the row in registers measured no gain on the
    headline, profiles/r07_notes.md; whoever tries again has this check.)"""
    import torch
    from graphical_gan_amd import _lib
    L = _lib.load()
    g = _t(np.random.default_rng(B * 7 + D).standard_normal((B, D)), gpu)
    new = lambda *s: torch.full(s, 555.0, dtype=torch.float32, device=gpu)
    sl0, pen0, gg0, one = new(B), new(1), new(B, D), torch.ones(1, dtype=torch.float32, device=gpu)
    _lib.check(L.ggan_gp_penalty_fwd(_p(g), _p(sl0), _p(pen0), B, D, 10.0, _stream()), 'ggan_gp_penalty_fwd')
    _lib.check(L.ggan_gp_penalty_bwd(_p(g), _p(sl0), _p(one), _p(gg0), B, D, 10.0, _stream()), 'ggan_gp_penalty_bwd')
    arrive = torch.zeros(1, dtype=torch.int32, device=gpu)
    for rep in range(2):
        sl, pen, gg = new(B), new(1), new(B, D)
        _lib.check(L.ggan_gp_penalty_fwd_grad(_p(g), _p(sl), _p(pen), _p(gg), _p(arrive), B, D, 10.0, _stream()), 'ggan_gp_penalty_fwd_grad')
        torch.cuda.synchronize()
        assert int(arrive[0]) == 0, rep
        assert _same_bits(sl, sl0) and _same_bits(pen, pen0) and _same_bits(gg, gg0), rep


# ---- one critic step of wali-gp on both routes ------------------------------------------------------------------------------------------
_STEP = {}


def _critic_step(gpu, monkeypatch, seeded, graph):
    """the last critic step of a few wali-gp iterations at fixed weights (learning rate 0) and a fixed feed, as step graphs or as the same
    launches issued eagerly (Trainer.eager_as_captured): interpolates, the penalty pass's conv activations, g, the penalty and the
    packed gradient bucket.  Computed once per (route, graph) and shared by the tests below."""
    key = (seeded, graph)
    if key in _STEP:
        return _STEP[key]
    import contextlib
    import torch
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.optim import _optimizers
    from oracle import step as S
    from test_step_gpu import _fresh, _mk
    if seeded:
        monkeypatch.delenv('GGAN_NO_PENALTY_SEED', raising=False)
    else:
        monkeypatch.setenv('GGAN_NO_PENALTY_SEED', '1')
    B = 8
    ocfg, P0, cfg, tr = _mk('cifar10', B, 0, 'wali-gp', 8, 16, True, graph, gpu)
    feed = S.make_feed(ocfg, np.random.default_rng(11), 'wali-gp')
    feeds = iter([feed] * 64)
    J = lib.objs.gan_inference
    entry, rec = J.gradient_penalty, dict(calls=0)

    def spy(critic, *a, input_grad=None, **kw):
        def note(fn):
            def f(x, z):
                rec['x_hat'], rec['z_hat'] = x.detach(), z.detach()
                return fn(x, z)
            return f
        gp = entry(note(critic), *a, input_grad=note(input_grad) if input_grad is not None else None, **kw)
        rec['seeded'], rec['gp'], rec['g'] = input_grad is not None, gp.detach(), gp.grad_fn.saved_tensors[0].detach()
        rec['calls'] += 1
        return gp
    monkeypatch.setattr(J, 'gradient_penalty', spy)
    try:
        tr.iteration(0, feeds)                   # eager first calls: the optimizers come into being
        tr.iteration(1, feeds)
        for o in _optimizers.values():
            o.lr = 0.0                           # the weights stay put: every later critic step is the same step on both routes
        tr.load_params(P0)
        tr.set_feed(feed)
        tr.flush()
        tr.drop_graphs()
        lib.TAPS[0] = []
        with (contextlib.nullcontext() if graph else tr.eager_as_captured()):
            for it in (2, 3, 4):                 # capture, then replays | the same launches eagerly
                tr.iteration(it, feeds)
        taps, lib.TAPS[0] = lib.TAPS[0], None
        tr.flush()
        torch.cuda.synchronize()
    finally:
        lib.TAPS[0] = None
        monkeypatch.setattr(J, 'gradient_penalty', entry)
    assert rec['calls'] > 0 and rec['seeded'] == seeded
    acts = {n: t for _, n, t in taps if n.startswith('Discriminator.') and t.shape[0] == B}     # (the last penalty pass's; the main pass has 2B rows)
    assert len(acts) == 3, sorted(acts)
    opt = next(o for k, o in _optimizers.items() if k[0] == 'disc')
    out = dict(x_hat=rec['x_hat'].clone(), z_hat=rec['z_hat'].clone(), g=rec['g'].clone(), gp=rec['gp'].clone().reshape(1),
               bucket=opt.g.clone(), **{n: t.clone() for n, t in acts.items()})
    assert all(bool(torch.isfinite(t).all()) for t in out.values()) and float(out['g'].abs().max()) > 0
    del tr
    _fresh()
    _STEP[key] = out
    return out


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
def test_critic_step_seeded_route_against_the_composition(gpu, monkeypatch, graph):
    """GGAN_NO_PENALTY_SEED=1 against the default route: interpolates, penalty-pass activations, g, the penalty and the packed gradient
    bucket bit for bit"""
    old = _critic_step(gpu, monkeypatch, False, graph)
    new = _critic_step(gpu, monkeypatch, True, graph)
    assert sorted(old) == sorted(new)
    for k in old:
        assert _same_bits(new[k], old[k]), (k, float((new[k] - old[k]).abs().max()))
    e = _rel(_np(new['bucket']), _np(old['bucket']))
    print('bucket vs composition', graph, e)
    assert e < TOL, e


@pytest.mark.parametrize('seeded', [True, False], ids=['seeded', 'composition'])
def test_critic_step_graph_equals_eager(gpu, monkeypatch, seeded):
    """the captured step graph against the same launches issued eagerly: everything bit for bit, the bucket included"""
    eager = _critic_step(gpu, monkeypatch, seeded, False)
    graph = _critic_step(gpu, monkeypatch, seeded, True)
    for k in eager:
        assert _same_bits(graph[k], eager[k]), (k, float((graph[k] - eager[k]).abs().max()))


def test_training_run_ends_at_the_same_weights_on_both_routes(gpu, monkeypatch):
    """a few wali-gp iterations as step graphs with the optimizers' real learning rates: costs and every weight bit for bit between
    GGAN_NO_PENALTY_SEED=1 and the default route -- what a long run ends at does not depend on the route"""
    import torch
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models import Config
    from test_step_gpu import _fresh
    finals = []
    for seeded in (False, True):
        if seeded:
            monkeypatch.delenv('GGAN_NO_PENALTY_SEED', raising=False)
        else:
            monkeypatch.setenv('GGAN_NO_PENALTY_SEED', '1')
        _fresh()
        np.random.seed(0)
        tr = Trainer(Config('cifar10', batch_size=16, n_coms=0, mode='wali-gp', dim=16, dim_latent=32), device=gpu, graph=True, seed=4321)
        batches = iter(tr.model.synthetic_ring(gpu, n=5, seed=99) * 60)
        for it in range(4):
            res = tr.iteration(it, batches)
        tr.flush()
        torch.cuda.synchronize()
        finals.append(({k: v.copy() for k, v in tr.get_params().items()}, {k: float(v) for k, v in res.items()}))
        del tr
    _fresh()
    assert finals[0][1] == finals[1][1] and all(np.isfinite(v) for v in finals[1][1].values())
    for k in finals[0][0]:
        assert np.array_equal(finals[0][0][k], finals[1][0][k]), k
