"""-m gpu: the gradient-penalty double backward, op by op and at the step, against the float64 oracle tape (oracle.tape, closed under
differentiation).

Every op check is one Hessian-vector product (_hvp): with probes u, v, the first derivative g = d<u, f(x, theta)>/dx is taken with
create_graph=True (inside functional.data_grad_only() where the gradient-penalty pass runs it there), then L = <v, g> is differentiated
w.r.t. x, theta and u.  g is held to the first-order tolerance of tests/test_ops_gpu.py (TOL, TOL_LONG for long sums), every second-order
result to TOL2 = 1e-4 of its largest reference entry ("GP second-order <= 1e-4").  Errors go to GGAN_TEST_REPORT like
every _rel.

Kinks: for ops with a LeakyReLU / ReLU the reference takes its activation mask from the kernel's own fp32 forward output, and at most
a handful of units may differ from the float64 mask -- a near-zero pre-activation neither makes the test flaky nor hides a wrong mask.
"""
import contextlib
import os

import numpy as np
import pytest

from _kinks import _kink_samples
from test_ops_gpu import _REPORT, GEMM_CASES, TOL, TOL_LONG, _rel, _t

pytestmark = pytest.mark.gpu

TOL2 = 1e-4
MAX_FLIPS = 8          # units whose fp32 activation branch may differ from the float64 one


@pytest.fixture(params=[0, 1], ids=['mfma', 'naive'])
def plain(request, gpu):
    from graphical_gan_amd import functional as F
    F.force_plain(request.param)
    yield request.param
    F.force_plain(0)


@pytest.fixture
def registry(gpu):
    from graphical_gan_amd import tflib as lib
    lib.delete_all_params()
    yield lib
    lib.delete_all_params()


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _check2(tag, got, ref):
    """a second-order result at TOL2 of max |ref|; a mathematically zero one must be absent or exactly zero"""
    if ref is None or not np.abs(ref.v).max() > 0:
        assert got is None or float(got.abs().max()) == 0.0, (tag, 'expected no second-order term', None if got is None else float(got.abs().max()))
        return
    assert got is not None, (tag, 'second-order term missing')
    e = _rel(_np(got).reshape(ref.v.shape), ref.v)
    assert e <= TOL2, (tag, e)


def _hvp(gpu, inputs, dev_fn, ref_fn, inner, outer, seed, tol1=TOL, params=(), data_only=False, lib=None):
    """inputs {name: float32 array}; dev_fn({name: tensor}) -> output tensor (HIP ops); ref_fn({name: tape.T}, fp32 output) -> tape.T.
    inner: names of the first derivative (create_graph=True, under data_grad_only if data_only); outer: names L = <v, g> is
    differentiated by ('u' = the probe u).  params: inputs made registry parameters (tflib.param: what data_grad_only may skip)."""
    import torch
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    rng = np.random.default_rng(seed)
    dev = {}
    for k, a in inputs.items():
        if k in params:
            dev[k] = lib.param('SecondOrder.%s' % k, np.asarray(a, np.float32))
        else:
            dev[k] = _t(a, gpu).requires_grad_(True)
    y = dev_fn(dev)
    u = rng.standard_normal(tuple(y.shape))
    vs = {k: rng.standard_normal(np.shape(inputs[k])) for k in inner}
    tu = _t(u, gpu).requires_grad_(True)
    with (F.data_grad_only() if data_only else contextlib.nullcontext()):
        gs = torch.autograd.grad(y, [dev[k] for k in inner], grad_outputs=tu, create_graph=True)
    L = None
    for k, g in zip(inner, gs):
        term = (g * _t(vs[k], gpu).view(g.shape)).sum()
        L = term if L is None else L + term
    seconds = torch.autograd.grad(L, [tu if k == 'u' else dev[k] for k in outer], allow_unused=True)

    R = {k: tp.T(np.asarray(a, np.float64).reshape(np.shape(a))) for k, a in inputs.items()}
    U = tp.T(u)
    yr = ref_fn(R, _np(y))
    grs = tp.grad(tp.reduce_sum(tp.mul(yr, U)), [R[k] for k in inner])
    Lr = None
    for k, g in zip(inner, grs):
        term = tp.reduce_sum(tp.mul(g, tp.T(vs[k])))
        Lr = term if Lr is None else tp.add(Lr, term)
    srs = tp.grad(Lr, [U if k == 'u' else R[k] for k in outer])
    assert _rel(_np(y).reshape(yr.v.shape), yr.v) < TOL_LONG, ('forward', _rel(_np(y).reshape(yr.v.shape), yr.v))
    for k, g, gr in zip(inner, gs, grs):
        e = _rel(_np(g).reshape(gr.v.shape), gr.v)
        assert e < tol1, ('first order', k, e)
    for k, s, sr in zip(outer, seconds, srs):
        _check2(('second order', k), s, sr)
    return y, gs, seconds


def _masked(pre, y_dev, act, alpha):
    """activation with the mask taken from the kernel's fp32 output y_dev; asserts the float64 mask differs in a handful of units"""
    from oracle import tape as tp
    on = y_dev.reshape(pre.v.shape) > 0
    flips = int(np.count_nonzero(on != (pre.v > 0)))
    assert flips <= MAX_FLIPS, ('activation mask differs from float64 in %d units' % flips)
    return tp.mul(pre, tp.T(np.where(on, 1.0, alpha if act == 'lrelu' else 0.0)))


def _act_ref(pre, y_dev, act):
    from oracle import tape as tp
    if act in ('lrelu', 'relu'):
        return _masked(pre, y_dev, act, 0.2)
    return {'none': lambda p: p, 'tanh': tp.tanh, 'sigmoid': tp.sigmoid}[act](pre)


ACTS = {'none': (0, 0.0), 'lrelu': (1, 0.2), 'relu': (2, 0.0), 'tanh': (3, 0.0), 'sigmoid': (4, 0.0)}


def _prof_names(L, fn):
    import torch
    from graphical_gan_amd import _lib
    L.ggan_prof_reset()
    L.ggan_prof_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
    finally:
        L.ggan_prof_enable(0)
    names = [x['name'] for x in _lib.prof_report()]
    L.ggan_prof_reset()
    return r, names


# ---------------------------------------------------------------------------------------------------------------------------------
# ConvFwd at the critics' layer shapes
# ---------------------------------------------------------------------------------------------------------------------------------
def _critic_layers():
    """(dataset, N, Ci, H, Co, act) of every models.Discriminator conv layer at the scripts' widths (5x5, stride 2, SAME)"""
    from graphical_gan_amd.models import Config
    out = []
    for ds, N in (('cifar10', 64), ('mnist', 50)):
        c = Config(ds, batch_size=N)
        ch, S = c.C, c.S
        for i in range(c.nl):
            co = c.dim * 2 ** i
            out.append((ds, N, ch, S, co, 'none' if (c.critic_deep and c.bn and i > 0) else 'lrelu'))   # (BatchNorm follows: no epilogue)
            ch, S = co, -(-S // 2)
    return out


CRITIC_LAYERS = _critic_layers()
CONV_CASES = [(ds, N, Ci, H, Co, act, 5, 2) for ds, N, Ci, H, Co, act in CRITIC_LAYERS] + [('k3s1', 8, 16, 9, 24, 'lrelu', 3, 1)]


def test_critic_layers_are_the_scripts_shapes():
    assert [c[:5] for c in CRITIC_LAYERS] == [('cifar10', 64, 3, 32, 64), ('cifar10', 64, 64, 16, 128), ('cifar10', 64, 128, 8, 256),
                                              ('mnist', 50, 1, 28, 64), ('mnist', 50, 64, 14, 128), ('mnist', 50, 128, 7, 256)]


def _conv_case(gpu, lib, case, route, seed):
    """one ConvFwd layer (bias, activation) through _hvp.  route 'data_only': w, b registry parameters, first derivative w.r.t. x
    under data_grad_only (ConvDgradMasked for lrelu); 'composition': first derivatives w.r.t. x, w and b (ActBwd + ConvWgrad +
    ChanSum + ConvDgrad, differentiated once more)"""
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    ds, N, Ci, H, Co, act, k, s = case
    rng = np.random.default_rng(seed)
    geom = F.conv_geom(N, Ci, H, H, Co, k, s, 'SAME')
    a, alpha = ACTS[act]
    inputs = dict(x=rng.standard_normal((N, Ci, H, H)).astype(np.float32),
                  w=(rng.standard_normal((k, k, Ci, Co)) / np.sqrt(k * k * Ci)).astype(np.float32),
                  b=(0.3 * rng.standard_normal(Co)).astype(np.float32))

    def dev_fn(d):
        return F.ConvFwd.apply(d['x'], d['w'], d['b'], geom, a, alpha)

    def ref_fn(R, y):
        pre = tp.add(tp.conv2d(R['x'], R['w'], s, 'SAME'), tp.reshape(R['b'], (1, Co, 1, 1)))
        return _act_ref(pre, y, act)
    if route == 'data_only':
        return _hvp(gpu, inputs, dev_fn, ref_fn, ['x'], ['x', 'w', 'b', 'u'], seed + 1, TOL_LONG, params=('w', 'b'), data_only=True, lib=lib)
    return _hvp(gpu, inputs, dev_fn, ref_fn, ['x', 'w', 'b'], ['x', 'w', 'b', 'u'], seed + 1, TOL_LONG)


@pytest.mark.parametrize('route', ['data_only', 'composition'])
@pytest.mark.parametrize('case', CONV_CASES, ids=lambda c: '%s-%d-%d-%d-%d-%s-k%ds%d' % c)
def test_conv_layer_second_order(gpu, plain, registry, case, route):
    """ConvFwd (5x5 stride 2 SAME at the critics' own shapes, and a 3x3 stride-1 geometry) differentiated twice, on the planned kernels
    and on the plain ones (force_plain); the launches are checked to be the intended kernels"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    _, names = _prof_names(L, lambda: _conv_case(gpu, registry, case, route, sum(case[1:5])))
    ds, N, Ci, H, Co, act, k, s = case
    conv = [n for n in names if any(p in n for p in ('corr_kernel', 'thin_', 'dg16', 'wgrad', 'conv_', 'gemm'))]
    if plain:
        assert not [n for n in conv if 'naive' not in n], ('planned kernel under force_plain', names)
    elif k == 5:         # (other geometries are the plain kernels' by design: test_ops_gpu.test_conv_other_geometry_uses_plain_kernels)
        assert not [n for n in names if 'naive' in n], ('fell back to the plain kernels', names)
        if Ci <= 4:
            assert any(n.startswith('thin_') for n in names), ('thin-channel kernels did not run', names)
        if route == 'data_only' and act == 'lrelu' and k == 5:
            # ConvDgradMasked: the mask rides in the data-gradient staging, the MFMA (thin) epilogue and the filter-gradient staging
            assert 'act_bwd' not in names, ('masked launch fell back to conv + act_bwd', names)


@pytest.mark.parametrize('route', ['data_only', 'composition'])
@pytest.mark.parametrize('case', [c for c in CONV_CASES if c[2] >= 64 and c[0] == 'cifar10'], ids=lambda c: '%s-%d-%d-%d-%d-%s-k%ds%d' % c)
def test_conv_layer_second_order_dg16(gpu, registry, case, route, monkeypatch):
    """the same checks with the 16-channel data-gradient kernel forced (GGAN_DG16_FORCE), and its launch asserted"""
    from graphical_gan_amd import _lib
    monkeypatch.setenv('GGAN_DG16', '1')
    monkeypatch.setenv('GGAN_DG16_FORCE', '1')
    L = _lib.load()
    _, names = _prof_names(L, lambda: _conv_case(gpu, registry, case, route, 3 + sum(case[1:5])))
    # the exact instances: tile columns min(Wo, 16) + 8 slab columns; 16-channel tiles (KQ 4: these grids are below the default plan)
    Wo = -(-case[3] // 2)
    expect = ['dg16_kernel<%d, 4, %s>' % (min(Wo, 16) + 8, m) for m in ('false', 'true')]
    dg16 = [n for n in names if n.startswith('dg16_kernel<')]
    assert dg16 and all(n in expect for n in dg16), (names, expect)


# ---------------------------------------------------------------------------------------------------------------------------------
# Gemm, Gemm2 / Gemm2Dgrad
# ---------------------------------------------------------------------------------------------------------------------------------
GEMM2_SHAPES = [(64, 512, 158), (128, 512, 4608), (128, 512, 512), (128, 158, 512), (50, 30, 7), (65, 67, 33), (64, 1, 512)]
assert all(s in GEMM_CASES for s in GEMM2_SHAPES)
GEMM_VARIANTS = [(True, a) for a in ACTS] + [(False, 'none')]


@pytest.mark.parametrize('bias,act', GEMM_VARIANTS, ids=['%s-%s' % ('bias' if b else 'nobias', a) for b, a in GEMM_VARIANTS])
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize('mnk', GEMM2_SHAPES, ids=lambda c: '%d-%d-%d' % c)
def test_gemm_first_and_second_order(gpu, mnk, ta, tb, bias, act):
    """functional.Gemm: first derivatives of all three operands (every transposed backward branch) and the second-order products"""
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    M, N, K = mnk
    rng = np.random.default_rng(M * 7 + N * 3 + K + 100 * ta + 10 * tb)
    inputs = dict(a=rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32),
                  b=(rng.standard_normal((N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32))
    if bias:
        inputs['bias'] = (0.3 * rng.standard_normal(N)).astype(np.float32)
    a_, alpha = ACTS[act]

    def dev_fn(d):
        return F.Gemm.apply(d['a'], d['b'], d.get('bias'), bool(ta), bool(tb), a_, alpha)

    def ref_fn(R, y):
        A = tp.transpose(R['a'], (1, 0)) if ta else R['a']
        B = tp.transpose(R['b'], (1, 0)) if tb else R['b']
        pre = tp.matmul(A, B)
        if bias:
            pre = tp.add(pre, tp.reshape(R['bias'], (1, N)))
        return _act_ref(pre, y, act)
    names = ['a', 'b'] + (['bias'] if bias else [])
    _hvp(gpu, inputs, dev_fn, ref_fn, names, names + ['u'], M + N + K, TOL_LONG if K >= 4096 or M >= 4096 else TOL)


@pytest.mark.parametrize('M,K1,K2,N', [(128, 4096, 512, 512), (37, 64, 36, 70), (64, 192, 64, 256)])
@pytest.mark.parametrize('halves', ['both', 'first', 'second'])
def test_gemm2_data_gradient_second_order(gpu, M, K1, K2, N, halves):
    """Gemm2 -> (Gemm2Dgrad under create_graph) -> d/dw of the squared data gradient, against float64: e = gm w^T with
    gm = g * act'(pre) gives d(|e1|^2 + |e2|^2)/dw = 2 e^T gm.  With one half only, the other reaches Gemm2Dgrad's backward
    undefined (a zero operand): the penalty differentiates w.r.t. x_hat only."""
    import torch
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(M + K1 + K2 + len(halves))
    a1, a2 = rng.standard_normal((M, K1)), rng.standard_normal((M, K2))
    w = rng.standard_normal((K1 + K2, N)) / np.sqrt(K1 + K2)
    b = rng.standard_normal(N)
    g = rng.standard_normal((M, N))
    t1, t2 = _t(a1, gpu).requires_grad_(True), _t(a2, gpu).requires_grad_(True)
    tw, tb = _t(w, gpu).requires_grad_(True), _t(b, gpu).requires_grad_(True)
    y = F.Gemm2.apply(t1, t2, tw, tb, F.ACT_LRELU, 0.2)
    pre = np.concatenate([a1, a2], 1) @ w + b
    on = _np(y) > 0
    assert np.count_nonzero(on != (pre > 0)) <= MAX_FLIPS
    gm = g * np.where(on, 1.0, 0.2)
    e = gm @ w.T
    e1, e2 = torch.autograd.grad(y, [t1, t2], grad_outputs=_t(g, gpu), create_graph=True)
    assert _rel(_np(e1), e[:, :K1]) < TOL and _rel(_np(e2), e[:, K1:]) < TOL
    loss = {'both': (e1 * e1).sum() + (e2 * e2).sum(), 'first': (e1 * e1).sum(), 'second': (e2 * e2).sum()}[halves]
    em = e.copy()
    if halves == 'first':
        em[:, K1:] = 0
    elif halves == 'second':
        em[:, :K1] = 0
    hw, h1, h2 = torch.autograd.grad(loss, [tw, t1, t2], allow_unused=True)
    assert _rel(_np(hw), 2 * em.T @ gm) <= TOL2, _rel(_np(hw), 2 * em.T @ gm)
    assert h1 is None and h2 is None         # (the mask is piecewise constant: no second derivative w.r.t. the data)


# ---------------------------------------------------------------------------------------------------------------------------------
# activations, reductions, pointwise
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('act', ['lrelu', 'relu', 'tanh', 'sigmoid'])
def test_activation_second_order(gpu, act):
    """ActFwd -> ActBwd -> ActBwd.backward: the tanh / sigmoid second derivatives (d_ref), zero for the piecewise-linear ones, at
    large |x| as well"""
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(len(act))
    x = (rng.standard_normal(4099) * 3).astype(np.float32)
    x[:8] = [20, -20, 12, -12, 6, -6, 0.5, -0.5]
    a, alpha = ACTS[act]
    _hvp(gpu, dict(x=x), lambda d: F.ActFwd.apply(d['x'], a, alpha), lambda R, y: _act_ref(R['x'], y, act), ['x'], ['x', 'u'], 17)


def test_reductions_and_pointwise_second_order(gpu):
    """ColSum (both launch shapes), ChanSum, RowLerp and Axpby on a create_graph tape"""
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    rng = np.random.default_rng(23)
    for rows, cols in ((64, 512), (9000, 33)):
        _hvp(gpu, dict(x=rng.standard_normal((rows, cols)).astype(np.float32)), lambda d: F.ColSum.apply(d['x']),
             lambda R, y: tp.reduce_sum(R['x'], (0,)), ['x'], ['x', 'u'], rows, TOL_LONG)
    _hvp(gpu, dict(x=rng.standard_normal((50, 128, 7, 7)).astype(np.float32)), lambda d: F.ChanSum.apply(d['x']),
         lambda R, y: tp.reduce_sum(R['x'], (0, 2, 3)), ['x'], ['x', 'u'], 3, TOL_LONG)
    al = rng.uniform(size=64).astype(np.float32)
    _hvp(gpu, dict(x=rng.standard_normal((64, 3072)).astype(np.float32), y=rng.standard_normal((64, 3072)).astype(np.float32)),
         lambda d: F.RowLerp.apply(d['x'], d['y'], _t(al, gpu)),
         lambda R, y: tp.add(R['x'], tp.mul(tp.T(al.astype(np.float64).reshape(64, 1)), tp.add(R['y'], tp.neg(R['x'])))),
         ['x', 'y'], ['x', 'y', 'u'], 4)
    _hvp(gpu, dict(x=rng.standard_normal((64, 128)).astype(np.float32), y=rng.standard_normal((64, 128)).astype(np.float32)),
         lambda d: F.Axpby.apply(d['x'], d['y'], 0.7, -1.3, 0.25),
         lambda R, y: tp.add(tp.add(tp.scale(R['x'], 0.7), tp.scale(R['y'], -1.3)), tp.T(np.full((64, 128), 0.25))),
         ['x', 'y'], ['x', 'y', 'u'], 5)


def test_critic_tail_differentiable_composition(gpu, registry):
    """tflib LinearLReLULinear(differentiable=True) on a pair of inputs (the wali-gp penalty pass's critic tail): second order
    against float64 under data_grad_only, and its first derivatives equal to the fused CriticHead's on the same operands"""
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd.tflib.ops.linear import LinearLReLULinear
    from oracle import tape as tp
    lib = registry
    rng = np.random.default_rng(29)
    M, K1, K2, H = 64, 128, 64, 512
    x1, x2 = rng.standard_normal((M, K1)).astype(np.float32), rng.standard_normal((M, K2)).astype(np.float32)
    LinearLReLULinear('T.1', K1 + K2, H, 'T.2', (_t(x1, gpu), _t(x2, gpu)), differentiable=True)
    P = {n: lib.param(n) for n in ('T.1.W', 'T.1.b', 'T.2.W', 'T.2.b')}
    with torch.no_grad():
        P['T.1.b'].copy_(_t(0.3 * rng.standard_normal(H), gpu))
        P['T.2.b'].copy_(_t(0.3 * rng.standard_normal(1), gpu))
    v = {n: _np(p).astype(np.float64) for n, p in P.items()}
    hid = _np(F.Gemm2.apply(_t(x1, gpu), _t(x2, gpu), P['T.1.W'], P['T.1.b'], F.ACT_LRELU, 0.2))    # the kernel's own hidden layer

    def ref_fn(R, y):
        pre = tp.add(tp.matmul(tp.concat([R['x1'], R['x2']], 1), tp.T(v['T.1.W'])), tp.T(v['T.1.b'].reshape(1, H)))
        h = _masked(pre, hid, 'lrelu', 0.2)
        return tp.reshape(tp.add(tp.matmul(h, tp.T(v['T.2.W'])), tp.T(v['T.2.b'].reshape(1, 1))), (M,))
    dev_fn = lambda d: LinearLReLULinear('T.1', K1 + K2, H, 'T.2', (d['x1'], d['x2']), differentiable=True)
    y, gs, _ = _hvp(gpu, dict(x1=x1, x2=x2), dev_fn, ref_fn, ['x1', 'x2'], ['x1', 'x2', 'u'], 31, data_only=True)
    # (w.r.t. the tail's weights: second order through the same tape)
    d1, d2 = _t(x1, gpu).requires_grad_(True), _t(x2, gpu).requires_grad_(True)
    u = _t(rng.standard_normal(M), gpu)
    vv = (_t(rng.standard_normal((M, K1)), gpu), _t(rng.standard_normal((M, K2)), gpu))
    with F.data_grad_only():
        g1, g2 = torch.autograd.grad(dev_fn(dict(x1=d1, x2=d2)), [d1, d2], grad_outputs=u, create_graph=True)
    got = torch.autograd.grad((g1 * vv[0]).sum() + (g2 * vv[1]).sum(), list(P.values()), allow_unused=True)
    R = dict(x1=tp.T(x1.astype(np.float64)), x2=tp.T(x2.astype(np.float64)))
    Wt = {n: tp.T(a) for n, a in v.items()}
    pre = tp.add(tp.matmul(tp.concat([R['x1'], R['x2']], 1), Wt['T.1.W']), tp.reshape(Wt['T.1.b'], (1, H)))
    yr = tp.reshape(tp.add(tp.matmul(_masked(pre, hid, 'lrelu', 0.2), Wt['T.2.W']), tp.reshape(Wt['T.2.b'], (1, 1))), (M,))
    r1, r2 = tp.grad(tp.reduce_sum(tp.mul(yr, tp.T(_np(u).astype(np.float64)))), [R['x1'], R['x2']])
    Lr = tp.add(tp.reduce_sum(tp.mul(r1, tp.T(_np(vv[0]).astype(np.float64)))), tp.reduce_sum(tp.mul(r2, tp.T(_np(vv[1]).astype(np.float64)))))
    for n, g_, r in zip(P, got, tp.grad(Lr, [Wt[n] for n in P])):
        _check2(('tail', n), g_, r)
    # the fused (once-differentiable) head: same first derivatives
    f1, f2 = _t(x1, gpu).requires_grad_(True), _t(x2, gpu).requires_grad_(True)
    lf = LinearLReLULinear('T.1', K1 + K2, H, 'T.2', (f1, f2))
    assert _rel(_np(lf), _np(y)) < TOL
    h1, h2 = torch.autograd.grad(lf, [f1, f2], grad_outputs=u)
    assert _rel(_np(h1), _np(g1)) < TOL and _rel(_np(h2), _np(g2)) < TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# data_grad_only
# ---------------------------------------------------------------------------------------------------------------------------------
def _mini_critic(F, P, x, geoms):
    """conv(lrelu) -> conv(lrelu) -> Gemm(lrelu) -> Gemm: the penalty pass's layer kinds, P registry parameters"""
    h = F.ConvFwd.apply(x, P['c1.W'], P['c1.b'], geoms[0], F.ACT_LRELU, 0.2)
    h = F.ConvFwd.apply(h, P['c2.W'], P['c2.b'], geoms[1], F.ACT_LRELU, 0.2)
    h = F.Gemm.apply(h.reshape(h.shape[0], -1), P['l1.W'], P['l1.b'], False, False, F.ACT_LRELU, 0.2)
    return F.Gemm.apply(h, P['l2.W'], P['l2.b'], False, False, F.ACT_NONE, 0.0).reshape(-1)


def test_data_grad_only_skips_parameter_gradients_only(gpu, registry, monkeypatch):
    """Under data_grad_only the inner gradient and the second-order parameter gradients equal the unhinted run's (<= 1e-5), and the
    inner grad call makes no filter-gradient, channel-sum or column-sum launch; without the hint it does"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    lib = registry
    rng = np.random.default_rng(37)
    N = 16
    geoms = [F.conv_geom(N, 3, 32, 32, 32, 5, 2), F.conv_geom(N, 32, 16, 16, 64, 5, 2)]
    shapes = {'c1.W': (5, 5, 3, 32), 'c1.b': (32,), 'c2.W': (5, 5, 32, 64), 'c2.b': (64,), 'l1.W': (64 * 64, 128), 'l1.b': (128,),
              'l2.W': (128, 1), 'l2.b': (1,)}
    P = {n: lib.param('Mini.' + n, (rng.standard_normal(s) / np.sqrt(np.prod(s[:-1]) if len(s) > 1 else 3)).astype(np.float32))
         for n, s in shapes.items()}
    x = _t(rng.standard_normal((N, 3, 32, 32)), gpu)
    u, v = _t(rng.standard_normal(N), gpu), _t(rng.standard_normal((N, 3, 32, 32)), gpu)
    L_ = _lib.load()
    watched = ('ggan_conv2d_bwd_filter', 'ggan_conv2d_bwd_filter_act', 'ggan_conv2d_bwd_filter_parts', 'ggan_chansum', 'ggan_colsum',
               'ggan_colsum_tall', 'ggan_gemm_colsum', 'ggan_act_bwd_chansum')
    res, counts = {}, {}
    for hinted in (False, True):
        calls = dict.fromkeys(watched, 0)
        orig = {n: getattr(L_, n) for n in watched}

        def counted(name):
            def f(*a):
                calls[name] += 1
                return orig[name](*a)
            return f
        xd = x.clone().requires_grad_(True)
        y = _mini_critic(F, P, xd, geoms)
        for n in watched:
            monkeypatch.setattr(L_, n, counted(n))
        try:
            with (F.data_grad_only() if hinted else contextlib.nullcontext()):
                (g,) = torch.autograd.grad(y, [xd], grad_outputs=u, create_graph=True)
            torch.cuda.synchronize()
        finally:
            for n in watched:
                monkeypatch.setattr(L_, n, orig[n])
        counts[hinted] = dict(calls)
        sec = torch.autograd.grad((g * v).sum(), list(P.values()), allow_unused=True)
        res[hinted] = (_np(g), [_np(s) for s in sec])
    assert sum(counts[True].values()) == 0, counts[True]
    assert counts[False]['ggan_conv2d_bwd_filter'] > 0 and counts[False]['ggan_colsum'] + counts[False]['ggan_chansum'] > 0, counts[False]
    assert _rel(res[True][0], res[False][0]) <= 1e-5
    for n, a, b in zip(P, res[True][1], res[False][1]):
        assert (a is None) == (b is None), n
        if b is not None and np.abs(b).max() > 0:
            assert _rel(a, b) <= 1e-5, n


@pytest.mark.parametrize('which', ['weight', 'bias'])
@pytest.mark.parametrize('tb', [0, 1])
def test_data_grad_only_keeps_the_non_parameter_operand(gpu, registry, which, tb):
    """Gemm.backward's mixed branches: only one of weight and bias is a registry parameter; the other operand's gradient is still
    produced under data_grad_only, and is right (first and second order against float64)"""
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    rng = np.random.default_rng(41 + tb)
    M, K, N = 64, 96, 40
    inputs = dict(x=rng.standard_normal((M, K)).astype(np.float32),
                  w=(rng.standard_normal((N, K) if tb else (K, N)) / np.sqrt(K)).astype(np.float32),
                  b=(0.3 * rng.standard_normal(N)).astype(np.float32))
    params = ('b',) if which == 'weight' else ('w',)
    data = 'w' if which == 'weight' else 'b'

    def ref_fn(R, y):
        W = tp.transpose(R['w'], (1, 0)) if tb else R['w']
        return _act_ref(tp.add(tp.matmul(R['x'], W), tp.reshape(R['b'], (1, N))), y, 'lrelu')
    _hvp(gpu, inputs, lambda d: F.Gemm.apply(d['x'], d['w'], d['b'], False, bool(tb), F.ACT_LRELU, 0.2), ref_fn, ['x', data],
         ['x', 'w', 'b', 'u'], 43, params=params, data_only=True, lib=registry)


def test_data_grad_only_keeps_a_data_dependent_weight_slot(gpu, registry):
    """a weight slot fed with a product of two activations is differentiated under data_grad_only (functional._is_param); the
    parameter in the same layers is not"""
    import torch
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    rng = np.random.default_rng(47)
    M, K, N = 32, 48, 24
    inputs = dict(x=rng.standard_normal((M, K)).astype(np.float32), p=rng.standard_normal((K, 8)).astype(np.float32),
                  q=rng.standard_normal((8, N)).astype(np.float32), b=(0.3 * rng.standard_normal(N)).astype(np.float32))

    def dev_fn(d):
        w = F.Gemm.apply(d['p'], d['q'], None, False, False, F.ACT_TANH, 0.0)        # data-dependent weight
        return F.Gemm.apply(d['x'], w, d['b'], False, False, F.ACT_SIGMOID, 0.0)

    def ref_fn(R, y):
        w = tp.tanh(tp.matmul(R['p'], R['q']))
        return tp.sigmoid(tp.add(tp.matmul(R['x'], w), tp.reshape(R['b'], (1, N))))
    _hvp(gpu, inputs, dev_fn, ref_fn, ['x', 'p', 'q'], ['x', 'p', 'q', 'b', 'u'], 53, params=('b',), data_only=True, lib=registry)
    b = registry.param('SecondOrder.b')
    x = _t(inputs['x'], gpu).requires_grad_(True)
    with F.data_grad_only():          # (the hint is for create_graph calls: a plain backward takes the fused launches, which form both)
        gx, gb = torch.autograd.grad(dev_fn(dict(x=x, p=_t(inputs['p'], gpu), q=_t(inputs['q'], gpu), b=b)), [x, b], allow_unused=True,
                                     grad_outputs=_t(rng.standard_normal((M, N)), gpu), create_graph=True)
    assert gx is not None and gb is None      # (the parameter's gradient is the one skipped)


# ---------------------------------------------------------------------------------------------------------------------------------
# BatchNorm at the MNIST critic's shapes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(50, 128, 7, 7), (50, 256, 4, 4)])
def test_batchnorm_second_order_mnist_critic(gpu, shape):
    """BatchNormTrain NCHW + LeakyReLU (the MNIST critic's Discriminator.BN2 / BN3) differentiated twice"""
    from graphical_gan_amd import functional as F
    from oracle import tape as tp
    rng = np.random.default_rng(shape[1])
    Cc = shape[1]
    inputs = dict(x=(rng.standard_normal(shape) * 1.3 + 0.2).astype(np.float32), s=(1 + 0.3 * rng.standard_normal(Cc)).astype(np.float32),
                  o=(0.2 * rng.standard_normal(Cc)).astype(np.float32))

    def ref_fn(R, y):
        return _act_ref(tp.batchnorm_train(R['x'], R['s'], R['o'], [0, 2, 3], 1e-5), y, 'lrelu')
    _hvp(gpu, inputs, lambda d: F.BatchNormTrain.apply(d['x'], d['s'], d['o'], 1e-5, F.ACT_LRELU, 0.2), ref_fn, ['x'],
         ['x', 's', 'o', 'u'], 59, TOL_LONG)


# ---------------------------------------------------------------------------------------------------------------------------------
# step level: the penalty on its own, and the gradient bucket a critic step trains with
# ---------------------------------------------------------------------------------------------------------------------------------
GP_CASES = [('cifar10', 8, 0, 'wali-gp', 8, 16), ('mnist', 6, 0, 'wali-gp', 8, 16), ('svhn', 8, 0, 'vegan-wgan-gp', 8, 16),
            ('cifar10', 8, 0, 'vegan-wgan-gp', 8, 16), ('cifar10', 8, 0, 'wali-gp', None, 128), ('mnist', 8, 0, 'wali-gp', None, 128)]


def _report(v):
    """an observed relative error to GGAN_TEST_REPORT, as test_ops_gpu._rel writes them"""
    if _REPORT is not None:
        with open(_REPORT, 'a') as f:
            f.write('%s %.3e\n' % (os.environ.get('PYTEST_CURRENT_TEST', '?').split(' ')[0], v))


def _check_grads(tag, names, grads, ogs, tol, kink_log):
    """every parameter gradient at tol of max |ref|, with test_step_gpu's allowance for a provable, rare near-kink"""
    gmax = max(np.abs(og.v).max() for og in ogs if og is not None)
    for n, g, og in zip(names, grads, ogs):
        if og is None:
            assert g is None or float(np.abs(g).max()) == 0.0, (tag, n)
            continue
        ref = og.v
        err = np.abs(np.asarray(g).reshape(ref.shape) - ref)
        scale = max(np.abs(ref).max(), 1e-2 * gmax)
        _report(err.max() / scale)
        if err.max() <= tol * scale:
            continue
        kinks = _kink_samples(kink_log)
        assert 1 <= len(kinks) <= 8, (tag, n, err.max(), scale, 'deviation without a provable (and rare) near-kink', kinks)
        l2 = np.linalg.norm(err) / (np.linalg.norm(ref) + 1e-30)
        assert np.median(err) <= tol * scale and l2 <= 2e-3, (tag, n, err.max(), np.median(err), l2, scale)


def _oracle(ocfg, P0, mode, seed=11):
    from oracle import step as S, tape as tp
    feed = S.make_feed(ocfg, np.random.default_rng(seed), mode)
    Pt = {k: tp.T(v.astype(np.float64)) for k, v in P0.items()}
    tp.KINK_LOG = kink_log = []
    try:
        oout = S.forward(ocfg, Pt, feed, mode)
    finally:
        tp.KINK_LOG = None
    return feed, Pt, oout, kink_log


@pytest.mark.parametrize('case', GP_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_gradient_penalty_alone(gpu, case):
    """the penalty term of the critic cost on its own: value (1e-5), its gradient w.r.t. every critic parameter (1e-4, through the
    second leaves the penalty pass uses), and the Wasserstein part disc_cost - gp (1e-4)"""
    import torch
    from graphical_gan_amd import tflib as lib
    from oracle import tape as tp
    from test_step_gpu import _mk
    dataset, B, K, mode, dim, dl = case
    ocfg, P0, cfg, tr = _mk(dataset, B, K, mode, dim, dl, True, False, gpu)
    feed, Pt, oout, kink_log = _oracle(ocfg, P0, mode)
    tr.set_feed(feed)
    out = tr.model.forward(tr.feed)
    gp, ogp = out['gradient_penalty'], oout['gradient_penalty']
    _report(abs(float(gp.detach()) - float(ogp.v)) / max(1.0, abs(float(ogp.v))))
    assert abs(float(gp.detach()) - float(ogp.v)) <= 1e-5 * max(1.0, abs(float(ogp.v))), (float(gp.detach()), float(ogp.v))
    ow = float(oout['disc_cost'].v) - float(ogp.v)
    w = float(out['disc_cost'].detach()) - float(gp.detach())
    assert abs(w - ow) <= 1e-4 * max(1.0, abs(ow)), (w, ow)
    opt = out['disc_train_op'].optimizer
    names = [p.param_name for p in opt.params]
    extra = [lib.second_leaf_for(p) for p in opt.params]
    leaves = list(opt.params) + [e for e in extra if e is not None]
    gs = torch.autograd.grad(gp, leaves, allow_unused=True, retain_graph=True)
    grads, j = [], len(opt.params)
    for i, e in enumerate(extra):
        g = _np(gs[i])
        if e is not None:
            g2 = _np(gs[j])
            j += 1
            g = g2 if g is None else (g if g2 is None else g + g2)
        grads.append(g)
    ogs = tp.grad(ogp, [Pt[n] for n in names])
    _check_grads(('gp', case), names, grads, ogs, 1e-4, kink_log)


@pytest.mark.parametrize('case', GP_CASES, ids=lambda c: '-'.join(str(x) for x in c))
def test_critic_step_gradient_bucket(gpu, case):
    """what trains: one critic step through Trainer._fwd_bwd (deferred filter-gradient slabs, pack_, the late penalty term, the unit
    seed), its packed gradient bucket against the oracle's disc-cost gradient at 1e-4"""
    import torch
    from oracle import tape as tp
    from test_step_gpu import _mk
    dataset, B, K, mode, dim, dl = case
    ocfg, P0, cfg, tr = _mk(dataset, B, K, mode, dim, dl, True, False, gpu)
    feed, Pt, oout, kink_log = _oracle(ocfg, P0, mode)
    tr.set_feed(feed)
    cost, opt, keep = tr._fwd_bwd('disc', fuse_update=False)
    torch.cuda.synchronize()
    oc = float(oout['disc_cost'].v)
    assert abs(float(cost) - oc) <= 1e-5 * max(1.0, abs(oc)), (float(cost), oc)
    names = [p.param_name for p in opt.params]
    grads = [_np(opt.g[o:o + n].view(p.shape)) for p, (o, n) in zip(opt.params, opt.slots)]
    ogs = tp.grad(oout['disc_cost'], [Pt[n] for n in names])
    _check_grads(('bucket', case), names, grads, ogs, 1e-4, kink_log)
