"""-m gpu: every kernel instance of the conv2d family, by name.  For each row of tests/_conv_dispatch.py the op runs through
graphical_gan_amd.functional under the row's launch plan and environment; the profiler must have seen exactly the row's kernel (and
the helper kernels the row lists) with the grid the row's split-K count implies, and the result must match the float64 oracle within
the figures of test_ops_gpu.py (TOL for forward and data gradients, TOL_LONG for filter gradients).  What a kernel name cannot show --
wave layout, pixel tile, slab unit, split count, XCD tile order, slab table -- is read from the GGAN_TRACE_CONV line of
conv_corr.hip's plan_and_launch."""
import ctypes as C
import re

import numpy as np
import pytest

from _conv_dispatch import ROWS, row_id
from test_ops_gpu import TOL, TOL_LONG, _rel, _t

pytestmark = pytest.mark.gpu

_PLAN_RE = re.compile(r'\[ggan\] plan (\S+) mode=(\d) cfg=(\d) tile=\((\d+),(\d+),(\d+)\) xq=(\d) SK=(\d+) xcd_p=(\d) grid=\((\d+),(\d+),(\d+)\) (table|no-table)')


def _plans(err):
    return [dict(mode=int(m[1]), cfg=int(m[2]), tile=(int(m[3]), int(m[4]), int(m[5])), xq=int(m[6]), sk=int(m[7]), xcd_p=int(m[8]),
                 grid=(int(m[9]), int(m[10]), int(m[11])), table=m[12] == 'table') for m in _PLAN_RE.findall(err)]


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _profiled(fn):
    """fn() between ggan_prof_reset / ggan_prof_enable(1) and a synchronise -> (fn's result, prof_report records)"""
    import torch
    from graphical_gan_amd import _lib
    L = _lib.load()
    L.ggan_prof_reset()
    L.ggan_prof_enable(1)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        L.ggan_prof_enable(0)
    recs = _lib.prof_report()
    L.ggan_prof_reset()
    return out, recs


def _run_op(row, gpu, seed):
    """-> [(what, device result as numpy, float64 reference, tolerance)], run inside the row's launch plan"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    from oracle import ops as O
    L = _lib.load()
    op = row['op']
    N, Ci, H, W, Co, pad = row['geom']
    geom = F.conv_geom(N, Ci, H, W, Co, 5, 2, pad)
    Ho, Wo = geom[5], geom[6]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Ci, H, W)).astype(np.float32)
    w = (rng.standard_normal((5, 5, Ci, Co)) / np.sqrt(25 * Ci)).astype(np.float32)
    gy = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)
    yref = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)       # continuous: the derivative's value at 0 is not compared
    assert np.all(yref != 0.0)
    b_o, b_i = rng.standard_normal(Co).astype(np.float32), rng.standard_normal(Ci).astype(np.float32)
    x64, w64, gy64 = x.astype(np.float64), w.astype(np.float64), gy.astype(np.float64)
    slope = np.where(yref > 0, 1.0, 0.2)
    ws = F.workspace(gpu)
    tx, tw, tg, tr = _t(x, gpu), _t(w, gpu), _t(gy, gpu), _t(yref, gpu)
    st = F._stream()
    if op == 'fwd':
        y = F.ConvFwd.apply(tx, tw, _t(b_o, gpu), geom, F.ACT_NONE, 0.0)
        return [('y', y.cpu().numpy(), O.conv2d(x64, w64, 2, pad) + b_o.reshape(1, -1, 1, 1), TOL)]
    if op == 'fwd_masked':
        y = torch.empty((N, Co, Ho, Wo), device=gpu)
        g = F._geom(geom)
        rc = L.ggan_conv2d_fwd_masked(C.byref(g), _ptr(tx), _ptr(tw), _ptr(y), _ptr(tr), F.ACT_LRELU, 0.2, _ptr(ws), ws.numel(), st)
        assert rc == 0, rc
        return [('y', y.cpu().numpy(), O.conv2d(x64, w64, 2, pad) * slope, TOL)]
    if op == 'fwd_cast':
        from graphical_gan_amd.tflib.ops import act as A
        ring = torch.as_tensor(rng.integers(0, 256, size=(2, N, Ci * H * W)).astype(np.int32), device=gpu)
        x_int = torch.zeros((N, Ci * H * W), dtype=torch.int32, device=gpu)
        ca, cb = torch.ones(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
        pend = A.cast_scale(x_int, 255., 2., noise=None, ring=(ring, ca, cb, 0), defer=True)
        y = F.ConvFwd.apply(pend.reshape(-1, Ci, H, W), tw, _t(b_o, gpu), geom, F.ACT_NONE, 0.0)
        assert pend.done
        xs = 2.0 * (ring[1].cpu().numpy().astype(np.float64) / 255.0 - 0.5).reshape(N, Ci, H, W)
        return [('x', pend.out.cpu().numpy().reshape(N, Ci, H, W), xs, TOL),
                ('y', y.cpu().numpy(), O.conv2d(xs, w64, 2, pad) + b_o.reshape(1, -1, 1, 1), TOL)]
    if op == 'dgrad':
        gx = F.ConvDgrad.apply(tg, tw, None, geom, F.ACT_NONE, 0.0)
        return [('gx', gx.cpu().numpy(), O.conv2d_bwd_data(gy64, w64, (H, W), 2, pad), TOL)]
    if op == 'dgrad_bias_act':
        gx = F.ConvDgrad.apply(tg, tw, _t(b_i, gpu), geom, F.ACT_RELU, 0.0)
        return [('gx', gx.cpu().numpy(), np.maximum(O.conv2d_bwd_data(gy64, w64, (H, W), 2, pad) + b_i.reshape(1, -1, 1, 1), 0.0), TOL)]
    if op == 'dgrad_masked':
        gx = F.ConvDgradMasked.apply(tg, tr, tw, geom, F.ACT_LRELU, 0.2)
        return [('gx', gx.cpu().numpy(), O.conv2d_bwd_data(gy64 * slope, w64, (H, W), 2, pad), TOL)]
    if op == 'wgrad':
        gw = F.ConvWgrad.apply(tx, tg, geom)
        return [('gw', gw.cpu().numpy(), O.conv2d_bwd_filter(x64, gy64, 5, 2, pad), TOL_LONG)]
    ref_w, ref_b = O.conv2d_bwd_filter(x64, gy64 * slope, 5, 2, pad), (gy64 * slope).sum((0, 2, 3))
    g = F._geom(geom)
    if op == 'wgrad_act':
        gw, gb = torch.empty((5, 5, Ci, Co), device=gpu), torch.empty((Co,), device=gpu)
        rc = L.ggan_conv2d_bwd_filter_act(C.byref(g), _ptr(tx), _ptr(tg), _ptr(tr), F.ACT_LRELU, 0.2, _ptr(gw), _ptr(gb), _ptr(ws), ws.numel(), st)
        assert rc == 0, rc
        return [('gw', gw.cpu().numpy(), ref_w, TOL_LONG), ('gb', gb.cpu().numpy(), ref_b, TOL_LONG)]
    assert op == 'wgrad_parts', op
    elems = 25 * Ci * Co
    cap = 64 * (elems + Co)
    part = torch.empty(cap, device=gpu)
    n, stride = C.c_int(0), C.c_size_t(0)
    rc = L.ggan_conv2d_bwd_filter_parts(C.byref(g), _ptr(tx), _ptr(tg), _ptr(tr), F.ACT_LRELU, 0.2, 1, _ptr(part), cap, C.byref(n), C.byref(stride), st)
    assert rc == 0 and n.value == row['sk'] and stride.value == elems + Co, (rc, n.value, stride.value)
    flat = torch.zeros(elems + Co, device=gpu)
    step = torch.zeros(1, dtype=torch.int32, device=gpu)
    rc = L.ggan_pack_parts((C.c_void_p * 1)(part.data_ptr()), (C.c_size_t * 1)(elems + Co), (C.c_size_t * 1)(0), (C.c_int * 1)(n.value),
                           (C.c_size_t * 1)(stride.value), 1, _ptr(flat), _ptr(step), st)
    assert rc == 0, rc
    out = flat.cpu().numpy()
    return [('gw', out[:elems].reshape(5, 5, Ci, Co), ref_w, TOL_LONG), ('gb', out[elems:], ref_b, TOL_LONG)]


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_runs_its_kernel_and_matches_float64(gpu, idx, monkeypatch, capfd):
    from graphical_gan_amd import functional as F
    row = ROWS[idx]
    for k in ('GGAN_DG16', 'GGAN_DG16_FORCE', 'GGAN_DG16_KQ', 'GGAN_NO_THIN', 'GGAN_WGRAD_SPLIT', 'GGAN_WGRAD_W4', 'GGAN_FWD_SK', 'GGAN_DGRAD_SK',
              'GGAN_WGRAD_SK'):
        monkeypatch.delenv(k, raising=False)
    for k, v in row['env'].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('GGAN_TRACE_CONV', '1')
    F.workspace(gpu)                     # (allocated and zeroed outside the profiled region)
    capfd.readouterr()

    def call():
        with F.target_workgroups(row['target']):
            return _run_op(row, gpu, 1000 + idx)
    results, recs = _profiled(call)
    err = capfd.readouterr().err
    # (a) exactly the row's kernel, and the helpers it lists
    names = sorted(set(r['name'] for r in recs))
    assert names == sorted(set((row['kernel'],) + tuple(row['also']))), (names, row)
    main = [r for r in recs if r['name'] == row['kernel']]
    assert len(main) == 1 and main[0]['launches'] == 1, main
    print('%s grid %d' % (row['kernel'], main[0]['grid']))
    assert main[0]['grid'] == row['tiles'] * row['sk'] * row['block'], (main[0]['grid'], row['tiles'], row['sk'], row['block'])
    if 'plan' in row:
        plans = _plans(err)
        assert len(plans) == 1, err
        p = plans[0]
        print('plan %r' % (p,))
        assert {k: p[k] for k in ('cfg', 'tile', 'xq', 'xcd_p')} == row['plan'] and p['sk'] == row['sk'], (p, row)
        gx, gy_, gz = p['grid']
        assert gx * gy_ * gz == row['tiles'] * row['sk']
        if p['xcd_p']:
            assert (gx * gy_) % 8 == 0 and gx % p['xcd_p'] == 0 and gy_ % (8 // p['xcd_p']) == 0
    else:
        assert '[ggan] plan' not in err, err
    # (b) float64
    for what, got, ref, tol in results:
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        e = _rel(got, ref)
        print('%s rel %.3e (tol %.0e)' % (what, e, tol))
        assert e < tol, (what, e, tol)


def test_forward_computes_its_slab_descriptors_when_first_launched_under_capture(gpu, monkeypatch, capfd):
    """The forward DMA path reads its slab offsets from a per-geometry table built on the host; fwd_slab_table returns NULL when a
    geometry is first launched during stream capture, and the kernel then computes the offsets itself.  One ConvFwd of a geometry no other
    test of this module uses is captured alone in a single-stream graph (no parallel branches), replayed, and then run eagerly (now with
    the table): the two results must be bit-identical and match float64."""
    import torch
    from graphical_gan_amd import functional as F
    from oracle import ops as O
    for k in ('GGAN_FWD_SK', 'GGAN_NO_THIN'):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('GGAN_TRACE_CONV', '1')
    case, target = (3, 12, 20, 20, 40), 8
    assert all(tuple(r['geom'][:5]) != case for r in ROWS)
    N, Ci, H, W, Co = case
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N, Ci, H, W)).astype(np.float32)
    w = (rng.standard_normal((5, 5, Ci, Co)) / np.sqrt(25 * Ci)).astype(np.float32)
    b = rng.standard_normal(Co).astype(np.float32)
    ref = O.conv2d(x.astype(np.float64), w.astype(np.float64), 2, 'SAME') + b.reshape(1, -1, 1, 1)
    geom = F.conv_geom(N, Ci, H, W, Co, 5, 2, 'SAME')
    tx, tw, tb = _t(x, gpu), _t(w, gpu), _t(b, gpu)
    stream = torch.cuda.Stream(device=gpu)
    stream.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(stream), F.target_workgroups(target):
        # warm-up with another geometry: the stream's workspace, the kernels' LDS attributes
        wg = F.conv_geom(4, 12, 12, 12, 40, 5, 2, 'SAME')
        F.ConvFwd.apply(torch.zeros((4, 12, 12, 12), device=gpu), torch.zeros((5, 5, 12, 40), device=gpu), None, wg, F.ACT_NONE, 0.0)
        torch.cuda.synchronize()
        capfd.readouterr()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            y_cap = F.ConvFwd.apply(tx, tw, tb, geom, F.ACT_NONE, 0.0)
        captured = _plans(capfd.readouterr().err)
        graph.replay()
        torch.cuda.synchronize()
        y_graph = y_cap.cpu().numpy().copy()
        y_eager = F.ConvFwd.apply(tx, tw, tb, geom, F.ACT_NONE, 0.0)
        torch.cuda.synchronize()
        eager = _plans(capfd.readouterr().err)
    y_eager = y_eager.cpu().numpy()
    print('captured %r\neager %r' % (captured, eager))
    assert len(captured) == 1 and len(eager) == 1                                    # one launch each: a one-node graph
    assert captured[0]['table'] is False and eager[0]['table'] is True
    assert captured[0]['sk'] == 1 and {k: v for k, v in captured[0].items() if k != 'table'} == {k: v for k, v in eager[0].items() if k != 'table'}
    assert captured[0]['cfg'] == 4 and captured[0]['xq'] == 4 and captured[0]['tile'] == (1, 6, 10)      # two tile positions per image
    e1, e2 = _rel(y_graph, ref), _rel(y_eager, ref)
    print('rel %.3e %.3e' % (e1, e2))
    assert np.array_equal(y_graph, y_eager)
    assert e1 < TOL and e2 < TOL, (e1, e2)
