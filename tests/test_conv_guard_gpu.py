"""-m gpu: what every conv2d row runs inside.  The rows of tests/_conv_dispatch.py, the non-square EXTRA_ROWS and the MISALIGNED rows of
tests/_conv_guard.py run through their C entry points with every float operand in its own NaN-filled buffer (a band of at least one
image plane and 1024 floats on each side), the int32 ring of fwd_cast inside bands of 2^30, outputs that start as NaN inside bands of
the same width, and a workspace that is NaN behind its zero head.  The profiler must have seen the row's kernel and helpers with the
row's grid (and the row's plan line for corr_kernel), exactly as test_conv_dispatch_gpu.py asks; then _conv_guard.check() reads the
whole buffers: bands untouched, every output element finite, the workspace head zero and exactly the row's slabs written, the result
within TOL / TOL_LONG of the float64 oracle ('gauss') or equal to it ('exact').  Masked ops run with LeakyReLU and with ReLU on a mask
reference that has exact +0 and -0 entries.  CONV_GUARD_REPORT=<file> appends what each run launched and its relative errors."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import _conv_guard as G
from _conv_guard import ALL_ROWS, guard_id
from test_conv_dispatch_gpu import _profiled, _plans
from test_gemm_dispatch_gpu import _dev, _p
from test_norm_dispatch_gpu import _out, _GUARDS

pytestmark = pytest.mark.gpu

_REPORT = os.environ.get('CONV_GUARD_REPORT')
_SWITCHES = ('GGAN_DG16', 'GGAN_DG16_FORCE', 'GGAN_DG16_KQ', 'GGAN_NO_THIN', 'GGAN_WGRAD_SPLIT', 'GGAN_WGRAD_W4', 'GGAN_FWD_SK', 'GGAN_DGRAD_SK',
             'GGAN_WGRAD_SK')
CASES = [(r, d) for r in ALL_ROWS for d in G.data_sets(r)]


def _workspace(gpu):
    """-> (buffer, bytes): GGAN_WS_RESERVED zero bytes, then NaN"""
    import torch
    head = G.WS_RESERVED // 4
    buf = torch.full((head + G.WS_FLOATS,), float('nan'), dtype=torch.float32, device=gpu)
    buf[:head].zero_()
    return buf, 4 * buf.numel()


def _run(row, gpu, inp):
    """-> dict(rc, n_parts, stride, ws, part): the row's entry point on banded operands; the outputs are the _GUARDS entries, in `names`"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    op = row['op']
    N, Ci, H, W, Co, pad = row['geom']
    geom = F.conv_geom(N, Ci, H, W, Co, 5, 2, pad)
    Ho, Wo = geom[5], geom[6]
    bw = G.band(row)
    dev = lambda name: _dev(inp[name], gpu, 1 if row.get('off') == name else 0, band=bw)
    out = lambda shape: _out(shape, gpu, band=bw)
    act = {None: F.ACT_NONE, 'lrelu': F.ACT_LRELU, 'relu': F.ACT_RELU}[inp['mask']]
    alpha = inp['alpha'] if inp['mask'] == 'lrelu' else 0.0
    ws, wsb = _workspace(gpu)
    st = F._stream()
    g = F._geom(geom)
    res = dict(ws=ws, names=[], keep=[])
    if op == 'fwd':
        x, w, b = dev('x'), dev('w'), dev('b_o')
        y = out((N, Co, Ho, Wo))
        res.update(rc=L.ggan_conv2d_fwd(C.byref(g), _p(x), _p(w), _p(b), _p(y), F.ACT_NONE, 0.0, _p(ws), wsb, st), names=['y'])
    elif op == 'fwd_masked':
        x, w, r = dev('x'), dev('w'), dev('yref')
        y = out((N, Co, Ho, Wo))
        res.update(rc=L.ggan_conv2d_fwd_masked(C.byref(g), _p(x), _p(w), _p(y), _p(r), act, alpha, _p(ws), wsb, st), names=['y'])
    elif op == 'fwd_cast':
        ring = inp['ring']
        rbuf = torch.full((bw + ring.size + bw,), G.RING_BAND, dtype=torch.int32, device=gpu)
        rview = rbuf[bw:bw + ring.size]
        rview.copy_(torch.from_numpy(np.ascontiguousarray(ring).reshape(-1)))
        ca, cb = torch.ones(1, dtype=torch.int32, device=gpu), torch.zeros(1, dtype=torch.int32, device=gpu)
        w, b = dev('w'), dev('b_o')
        xo, y = out((N, Ci, H, W)), out((N, Co, Ho, Wo))
        res.update(rc=L.ggan_conv2d_fwd_cast_ring(C.byref(g), _p(rview), 2, _p(ca), _p(cb), 0, _p(None), 255.0, 2.0, _p(xo), _p(w), _p(b), _p(y),
                                                  F.ACT_NONE, 0.0, st), names=['x', 'y'], ws=None, keep=[rbuf, ca, cb])
    elif op in ('dgrad', 'dgrad_bias_act'):
        gy, w = dev('gy'), dev('w')
        b = dev('b_i') if op == 'dgrad_bias_act' else None
        gx = out((N, Ci, H, W))
        res.update(rc=L.ggan_conv2d_bwd_data(C.byref(g), _p(gy), _p(w), _p(b), _p(gx), F.ACT_RELU if b is not None else F.ACT_NONE, 0.0, _p(ws),
                                             wsb, st), names=['gx'])
    elif op == 'dgrad_masked':
        gy, r, w = dev('gy'), dev('yref'), dev('w')
        gx = out((N, Ci, H, W))
        res.update(rc=L.ggan_conv2d_bwd_data_act(C.byref(g), _p(gy), _p(r), act, alpha, _p(w), _p(gx), _p(ws), wsb, st), names=['gx'])
    elif op == 'wgrad':
        x, gy = dev('x'), dev('gy')
        gw = out((5, 5, Ci, Co))
        res.update(rc=L.ggan_conv2d_bwd_filter(C.byref(g), _p(x), _p(gy), _p(gw), _p(None), _p(ws), wsb, st), names=['gw'])
    elif op == 'wgrad_act':
        x, gy, r = dev('x'), dev('gy'), dev('yref')
        gw = out((5, 5, Ci, Co))
        gb = None if row.get('nobias') else out((Co,))
        res.update(rc=L.ggan_conv2d_bwd_filter_act(C.byref(g), _p(x), _p(gy), _p(r), act, alpha, _p(gw), _p(gb), _p(ws), wsb, st),
                   names=['gw'] if gb is None else ['gw', 'gb'])
    else:
        assert op == 'wgrad_parts', op
        x, gy, r = dev('x'), dev('gy'), dev('yref')
        elems = 25 * Ci * Co
        cap = G.PARTS_CAP * (elems + Co)
        part = out((cap,))
        pg = _GUARDS.pop()
        n, stride = C.c_int(0), C.c_size_t(0)
        rc = L.ggan_conv2d_bwd_filter_parts(C.byref(g), _p(x), _p(gy), _p(r), act, alpha, 1, _p(part), cap, C.byref(n), C.byref(stride), st)
        res.update(rc=rc, n_parts=n.value, stride=stride.value, part=pg, ws=None)
        if rc == 0 and n.value * stride.value <= cap:
            flat = out((elems + Co,))
            step = torch.zeros(1, dtype=torch.int32, device=gpu)
            rc = L.ggan_pack_parts((C.c_void_p * 1)(part.data_ptr()), (C.c_size_t * 1)(elems + Co), (C.c_size_t * 1)(0), (C.c_int * 1)(n.value),
                                   (C.c_size_t * 1)(stride.value), 1, _p(flat), _p(step), st)
            res.update(rc=rc, names=['flat'], keep=[step])
    return res


def _check_launches(row, recs, err):
    """the row's kernel and helpers with the row's grid, and its plan line: what test_conv_dispatch_gpu.py asserts"""
    names = sorted(set(r['name'] for r in recs))
    assert names == sorted(set((row['kernel'],) + tuple(row['also']))), (names, [(r['name'], r['grid']) for r in recs], _plans(err), row)
    main = [r for r in recs if r['name'] == row['kernel']]
    assert len(main) == 1 and main[0]['launches'] == 1, main
    assert main[0]['grid'] == row['tiles'] * row['sk'] * row['block'], (main[0]['grid'], row['tiles'], row['sk'], row['block'])
    if 'plan' in row:
        plans = _plans(err)
        assert len(plans) == 1, err
        p = plans[0]
        assert {k: p[k] for k in ('cfg', 'tile', 'xq', 'xcd_p')} == row['plan'] and p['sk'] == row['sk'], (p, row)
        gx, gy_, gz = p['grid']
        assert gx * gy_ * gz == row['tiles'] * row['sk']
        if p['xcd_p']:
            assert (gx * gy_) % 8 == 0 and gx % p['xcd_p'] == 0 and gy_ % (8 // p['xcd_p']) == 0
    else:
        assert '[ggan] plan' not in err, err


@pytest.mark.parametrize('idx', range(len(CASES)), ids=['%s-%s' % (guard_id(r), d) for r, d in CASES])
def test_row_inside_guard_bands(gpu, idx, monkeypatch, capfd):
    from graphical_gan_amd import functional as F
    row, data = CASES[idx]
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in row['env'].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('GGAN_TRACE_CONV', '1')
    for mask in G.masks(row):
        inp = G.inputs(row, data, mask)
        ref = G.reference(row, inp)
        del _GUARDS[:]
        capfd.readouterr()

        def call():
            with F.target_workgroups(row['target']):
                return _run(row, gpu, inp)
        res, recs = _profiled(call)
        err = capfd.readouterr().err
        host = lambda t: t.cpu().numpy()
        bufs = dict(out={name: (host(buf), off, ref[name].shape if name != 'flat' else (n,)) for name, (buf, off, n) in zip(res['names'], _GUARDS)},
                    ws=host(res['ws']) if res['ws'] is not None else None)
        if 'part' in res:
            bufs['part'] = (host(res['part'][0]), res['part'][1], res['part'][2])
        seen = dict(id=guard_id(row), data=data, mask=mask, rc=res['rc'], launches=[(r['name'], r['launches'], r['grid']) for r in recs],
                    plans=_plans(err), n_parts=res.get('n_parts'))
        errs, failure = None, None
        try:
            assert res['rc'] == 0, res['rc']
            _check_launches(row, recs, err)
            errs = G.check(row, data, bufs, dict(ref=ref, n_parts=res.get('n_parts'), stride=res.get('stride')))
        except AssertionError as e:
            failure = e
        if _REPORT:
            with open(_REPORT, 'a') as f:
                f.write(json.dumps(dict(seen, errs=errs, failed=str(failure)[:400] if failure else None)) + '\n')
        print('%s %s %s: %s %s' % (guard_id(row), data, mask, seen['launches'], errs))
        if failure is not None:
            raise failure
        del _GUARDS[:]
