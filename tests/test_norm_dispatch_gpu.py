"""-m gpu: every kernel instance of the normalisation family (csrc/bn.hip, csrc/linear_bn.hip), by name.  For each row of
tests/_norm_dispatch.py the row's entry point runs between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the
row's launches -- every label, as often as the row says, with the row's grid -- and every output must match the float64 oracle tape
evaluated on the float32-rounded inputs.  Operands sit in NaN-filled buffers (at the row's base offset) and the outputs of the rows that
call a C entry point start as NaN inside NaN padding, so a read outside an operand, an element no workgroup stores and a store outside
an output all show (the rows that go through autograd -- bwd_bwd, split -- get their outputs from the autograd functions).

Bounds (the project's own): TOL of max|ref| for gradients, save_mean and save_invstd, and for the Linear output h; 1e-5 of max|ref| for
y (test_batchnorm); 5e-5 for the second-order outputs (test_batchnorm_second_derivative); the split rows keep
test_grouped_bn_matches_float64's.  The rows with a constant channel compare y, gx and save_invstd channel by channel: that channel's
invstd is 1 / sqrt(eps), about 316, and would otherwise set the scale for its neighbours.

Two outputs are mathematically zero and are held absolutely, at three times the worst difference measured over the rows (the margin
test_ops_gpu.py holds over observed error): gx_chansum, against the float64 sum of the device's own gx (CHANSUM_ABS), and the bias
gradient of the Linear + BatchNorm backward, against its float64 reference (DB_ABS).

No masked row is decided by a kink: _norm_dispatch.inputs() / split_inputs() keep every float64 pre-activation MARGIN away from zero
(test_norm_dispatch_cpu.py asserts it without a GPU), and no element is left out of any comparison."""
import ctypes as C

import numpy as np
import pytest

import _norm_dispatch as D
from _norm_dispatch import ROWS, row_id, dims
from test_conv_dispatch_gpu import _profiled
from test_gemm_dispatch_gpu import _dev, _p
from test_ops_gpu import TOL, _rel, _t

pytestmark = pytest.mark.gpu

CHANSUM_ABS = 2.5e-5           # 3 x 8.4e-6, the worst |gx_chansum - sum(gx)| over the rows on MI355X (bn_bwd_nchw_k, 16389 elements per
#                                channel, |gx| up to 2.1; the other kernels: reg4_k<256> 4.6e-6, reg4_k<1024> 7.4e-6, reg_k 6.7e-6)
DB_ABS = 1.7e-5                # 3 x 5.5e-6, the worst |db| over the rows on MI355X (linear_bn_rows_bwd_k<8>, 112 rows; <4> 3.3e-6, <16> 3.9e-6):
#                                the sum over the rows of a BatchNorm data gradient, |gh| up to ~3
_GUARDS = []                   # (buffer, floats in front of the output, floats of the output) of every _out() of the running test


def _out(shape, gpu, off=0, band=0):
    """a NaN-filled float32 output, `off` floats into its buffer; `band` (a multiple of 4) more NaN floats on each side"""
    import torch
    n = int(np.prod(shape))
    assert band % 4 == 0
    buf = torch.full((band + off + n + 4 + band,), float('nan'), dtype=torch.float32, device=gpu)
    off += band
    view = buf[off:off + n].view(shape)
    assert view.data_ptr() % 16 == (4 * off) % 16
    _GUARDS.append((buf, off, n))
    return view


def _check_guards():
    """the NaN padding in front of and behind every output is still NaN: nothing was stored outside an output"""
    import torch
    for buf, off, n in _GUARDS:
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n:]).all()), ('a store outside an output', off, n, buf[:off], buf[off + n:])


def _null():
    return C.c_void_p(None)


def _run_fwd(row, gpu, inp, ref):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    N, Cc, HW = dims(row)
    x, sc, of = _dev(inp['x'], gpu), _dev(inp['scale'], gpu), _dev(inp['offset'], gpu)
    y, m, iv = _out(x.shape, gpu), _out((Cc,), gpu), _out((Cc,), gpu)
    rc = L.ggan_bn_fwd_train(_p(x), _p(sc), _p(of), _p(y), _p(m), _p(iv), N, Cc, HW, D.EPS, D.ACTS.index(row['act']), row['alpha'], F._stream())
    assert rc == 0, rc
    return [('y', y, ref['y'], 1e-5), ('save_mean', m, ref['save_mean'], TOL), ('save_invstd', iv, ref['save_invstd'], TOL)]


def _run_bwd(row, gpu, inp, ref):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    N, Cc, HW = dims(row)
    ox, og, ogx, oy = row['off']
    act = D.ACTS.index(row['act'])
    x, gy = _dev(inp['x'], gpu, ox), _dev(inp['gy'], gpu, og)
    yref = _dev(inp['y'], gpu, oy) if act else None
    sc, m, iv = _dev(inp['scale'], gpu), _dev(inp['save_mean'], gpu), _dev(inp['save_invstd'], gpu)
    gx, gs, go = _out(x.shape, gpu, ogx), _out((Cc,), gpu), _out((Cc,), gpu)
    cs = _out((Cc,), gpu) if row['chansum'] else None
    rc = L.ggan_bn_bwd_act(_p(x), _p(gy), _p(yref), act, row['alpha'], _p(sc), _p(m), _p(iv), _p(gx), _p(gs), _p(go), _p(cs), N, Cc, HW,
                           F._stream())
    assert rc == 0, rc
    outs = [('gx', gx, ref['gx'], TOL), ('gscale', gs, ref['gscale'], TOL), ('goffset', go, ref['goffset'], TOL)]
    if cs is not None:
        outs.append(('gx_chansum', cs, gx, None))
    return outs


def _run_sync(row, gpu, inp, ref):
    """as test_sync_batchnorm_entry_points: the batch cut into `world` replicas, the statistics rows gathered by hand"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    N, Cc, HW = dims(row)
    world, act, st = row['world'], D.ACTS.index(row['act']), F._stream()
    n = N // world
    cut = lambda a: [_dev(a[r * n:(r + 1) * n], gpu) for r in range(world)]
    xs, gys = cut(inp['x']), cut(inp['gy'])
    sc, of = _dev(inp['scale'], gpu), _dev(inp['offset'], gpu)
    stats = _out((world, 2, Cc), gpu)
    for r in range(world):
        assert L.ggan_bn_sync_stats(_p(xs[r]), _p(stats[r]), n, Cc, HW, st) == 0
    ys, means, invs = [], [], []
    for r in range(world):
        y, m, iv = _out(xs[r].shape, gpu), _out((Cc,), gpu), _out((Cc,), gpu)
        assert L.ggan_bn_sync_apply(_p(xs[r]), _p(stats), world, _p(sc), _p(of), _p(y), _p(m), _p(iv), n, Cc, HW, D.EPS, act, row['alpha'], st) == 0
        ys.append(y); means.append(m); invs.append(iv)
    outs = [('y', torch.cat(ys), ref['y'], 1e-5)]
    for r in range(world):
        outs += [('save_mean[%d]' % r, means[r], ref['save_mean'], TOL), ('save_invstd[%d]' % r, invs[r], ref['save_invstd'], TOL)]
    if len(row['launches']) == 2:
        return outs
    sums = _out((world, 2, Cc), gpu)
    yp = lambda r: _p(ys[r]) if act else _null()
    for r in range(world):
        assert L.ggan_bn_sync_bwd_stats(_p(xs[r]), _p(gys[r]), yp(r), act, row['alpha'], _p(means[r]), _p(invs[r]), _p(sums[r]), n, Cc, HW, st) == 0
    gxs, gss, gos = [], [], []
    for r in range(world):
        gx, gs, go = _out(xs[r].shape, gpu), _out((Cc,), gpu), _out((Cc,), gpu)
        assert L.ggan_bn_sync_bwd_apply(_p(xs[r]), _p(gys[r]), yp(r), act, row['alpha'], _p(sc), _p(means[r]), _p(invs[r]), _p(sums), world, r,
                                        _p(gx), _p(gs), _p(go), n, Cc, HW, st) == 0
        gxs.append(gx); gss.append(gs); gos.append(go)
    assert all(torch.isfinite(g).all() for g in gss + gos)
    return outs + [('gx', torch.cat(gxs), ref['gx'], TOL), ('gscale', sum(g.double() for g in gss), ref['gscale'], TOL),
                   ('goffset', sum(g.double() for g in gos), ref['goffset'], TOL)]


def _run_bwd_bwd(row, gpu, inp, ref):
    """as test_batchnorm_second_derivative: L = sum(w * d(sum(g0 * BN(x)))/dx) differentiated w.r.t. x, g0 and scale"""
    import torch
    from graphical_gan_amd import functional as F
    tx, ts, to, tg = (_t(inp[k], gpu).requires_grad_(True) for k in ('x', 'scale', 'offset', 'gy'))
    y = F.BatchNormTrain.apply(tx, ts, to, D.EPS, D.ACTS.index(row['act']), row['alpha'])
    (gx,) = torch.autograd.grad(y, [tx], grad_outputs=tg, create_graph=True)
    dx, dg, ds = torch.autograd.grad((gx * _t(inp['h'], gpu)).sum(), [tx, tg, ts])
    return [('y', y.detach(), ref['y'], 1e-5), ('gx', gx.detach(), ref['gx'], TOL), ('gx2', dx, ref['gx2'], 5e-5), ('ggy', dg, ref['ggy'], 5e-5),
            ('gscale2', ds, ref['gscale2'], 5e-5)]


def _run_lin_fwd(row, gpu, inp, ref):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    M, K, N = row['shape']
    x, w, b, sc, of = (_dev(inp[k], gpu) for k in ('x', 'w', 'b', 'scale', 'offset'))
    h, y, m, iv = _out((M, N), gpu), _out((M, N), gpu), _out((N,), gpu), _out((N,), gpu)
    rc = L.ggan_linear_bn_rows_fwd(_p(x), _p(w), _p(b), _p(sc), _p(of), _p(h), _p(y), _p(m), _p(iv), M, K, N, D.EPS, D.ACTS.index(row['act']),
                                   row['alpha'], F._stream())
    assert rc == 0, rc
    return [('h', h, ref['h'], TOL), ('y', y, ref['y'], 1e-5), ('save_mean', m, ref['save_mean'], TOL), ('save_invstd', iv, ref['save_invstd'], TOL)]


def _run_lin_bwd(row, gpu, inp, ref):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    M, K, N = row['shape']
    act = D.ACTS.index(row['act'])
    x, gy, h, sc, m, iv = (_dev(inp[k], gpu) for k in ('x', 'gy', 'h', 'scale', 'save_mean', 'save_invstd'))
    yref = _dev(inp['y'], gpu) if act else None
    dw, db, ds, do = _out((K, N), gpu), _out((N,), gpu), _out((N,), gpu), _out((N,), gpu)
    rc = L.ggan_linear_bn_rows_bwd(_p(x), _p(gy), _p(h), _p(yref), _p(sc), _p(m), _p(iv), _p(dw), _p(db), _p(ds), _p(do), M, K, N, act, row['alpha'],
                                   F._stream())
    assert rc == 0, rc
    assert np.abs(ref['db']).max() < 1e-12                      # (mathematically zero: it feeds a BatchNorm)
    return [('dw', dw, ref['dw'], TOL), ('db', db, ref['db'], ('abs', DB_ABS)), ('dscale', ds, ref['dscale'], TOL), ('doffset', do, ref['doffset'], TOL)]


def _run_split(row, gpu, seed):
    """through BatchNormGroupedTrain as test_grouped_bn_matches_float64 runs it, against its float64 torch reference and at its bounds"""
    import torch
    from graphical_gan_amd import functional as F
    from test_ssgan_bn_gpu import _ref
    x, sc, of, gy = (torch.from_numpy(a).double() for a in D.split_inputs(row, seed))
    if row['act'] in D.MASKS:
        lo = float(_ref(x, sc, of, 'none', row['groups']).abs().min())
        assert lo >= D.MARGIN, lo
    xs = [t.to(gpu, torch.float32).requires_grad_(True) for t in (x, sc, of)]
    y = F.BatchNormGroupedTrain.apply(xs[0], xs[1], xs[2], D.EPS, D.ACTS.index(row['act']), row['alpha'], row['groups'], None)
    gx, gs, go = torch.autograd.grad(y, xs, gy.to(gpu, torch.float32))
    xr, scr, ofr = (t.clone().requires_grad_(True) for t in (x, sc, of))
    yr = _ref(xr, scr, ofr, row['act'], row['groups'])
    gxr, gsr, gor = torch.autograd.grad(yr, (xr, scr, ofr), gy)
    n = lambda t: t.detach().numpy()
    return [('y', y.detach(), n(yr), 2e-6), ('gx', gx, n(gxr), 5e-5), ('gscale', gs, n(gsr), 5e-5), ('goffset', go, n(gor), 5e-5)]


_RUN = dict(bn_fwd=_run_fwd, bn_bwd=_run_bwd, sync=_run_sync, bwd_bwd=_run_bwd_bwd, lin_fwd=_run_lin_fwd, lin_bwd=_run_lin_bwd)


def _check_launches(row, recs):
    """exactly the row's labels; each as often as the row says, every record of it with the row's grid"""
    want = {l[0]: l for l in row['launches']}
    assert len(want) == len(row['launches'])
    assert sorted(set(r['name'] for r in recs)) == sorted(want), ([(r['name'], r['launches'], r['grid']) for r in recs], row['launches'])
    for name, launch in want.items():
        mine = [r for r in recs if r['name'] == name]
        print('%s launches %s grid %s' % (name, [r['launches'] for r in mine], [r['grid'] for r in mine]))
        assert sum(r['launches'] for r in mine) == launch[1], (mine, launch)
        assert all(r['grid'] == D.threads(launch) for r in mine), (mine, launch, D.threads(launch))


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_runs_its_kernel_and_matches_float64(gpu, idx):
    from graphical_gan_amd import functional as F
    row = ROWS[idx]
    del _GUARDS[:]
    F.workspace(gpu)                     # (allocated and zeroed outside the profiled region)
    if row['entry'] == 'split':
        results, recs = _profiled(lambda: _run_split(row, gpu, 7000 + idx))
    else:
        inp, ref = D.inputs(row, 7000 + idx)
        if row['act'] in D.MASKS:
            assert D.margin(row, ref) >= D.MARGIN, D.margin(row, ref)
        results, recs = _profiled(lambda: _RUN[row['entry']](row, gpu, inp, ref))
    _check_launches(row, recs)                                                          # (a)
    _check_guards()
    if row['const'] is not None and row['entry'] == 'bn_fwd':      # a power-of-two count of 0.5: sum and mean exact, so y is the offset itself
        got, c = {what: t.cpu().numpy() for what, t, _, _ in results}, row['const']
        assert got['save_mean'][c] == 0.5 and np.all(got['y'][:, c] == inp['offset'][c]), (got['save_mean'][c], inp['offset'][c])
    for what, got, want, tol in results:                                               # (b)
        got = got.double().cpu().numpy()
        assert np.all(np.isfinite(got)), (what, 'elements nobody stored or not finite: %d' % int((~np.isfinite(got)).sum()))
        if what == 'gx_chansum':                   # against the float64 sum of the device's own gx
            own = want.double().cpu().numpy().sum(axis=(0, 2))
            e = float(np.abs(got - own).max())
            print('NORM %s gx_chansum abs %.3e (bound %.1e, largest |gx| %.3e)' % (row['launches'][-1][0], e, CHANSUM_ABS, float(np.abs(want.cpu().numpy()).max())))
            assert e <= CHANSUM_ABS, (what, e, CHANSUM_ABS)
            continue
        want = np.asarray(want, dtype=np.float64).reshape(got.shape)
        if row['const'] is not None and what in ('y', 'gx', 'save_invstd'):      # channel by channel
            for c in range(dims(row)[1]):
                gc, wc = (got[:, c], want[:, c]) if got.ndim > 1 else (got[c:c + 1], want[c:c + 1])
                e = _rel(gc, wc)
                print('NORM %s %s[channel %d] rel %.3e (tol %.0e)' % (row['launches'][-1][0], what, c, e, tol))
                assert e < tol, (what, c, e, tol)
            continue
        if isinstance(tol, tuple):                 # an absolute bound (the Linear + BatchNorm rows)
            e = float(np.abs(got - want).max())
            print('NORM %s %s abs %.3e (bound %.3e) rel %.3e' % (row['launches'][-1][0], what, e, tol[1], _rel(got, want)))
            assert e <= tol[1], (what, e, tol[1])
        else:
            e = _rel(got, want)
            print('NORM %s %s rel %.3e (tol %.0e)' % (row['launches'][-1][0], what, e, tol))
            assert e < tol, (what, e, tol)
