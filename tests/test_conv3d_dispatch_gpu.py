"""-m gpu: every kernel instance of the 3-D convolution family (csrc/conv3d.hip), by name.  For each row of tests/_conv3d_dispatch.py
the row's C entry point runs between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the row's launches -- every
label, as often as the row says, with the row's grid -- and every output must be finite and within TOL (5e-6 of max|ref|, the bound
test_conv3d_entry_points holds this family to) of the float64 oracle evaluated on the float32-rounded inputs.  Operands sit in
NaN-filled buffers, outputs start as NaN inside NaN padding, and the workspace behind its reserved (zero) head is NaN too: after the
call exactly the row's SK slabs of it are finite, which is how a test reads the split the kernel ran.  The layout kernels (im2col3d /
col2im3d) and the wide-volume rows (FASTDIV_ROWS: data -1, 0, 1, every sum exact in float32) are compared by equality.  A refused row
returns non-zero, launches nothing and leaves its output NaN.  No element is left out of any comparison; gy is an input of the
gradient rows, so no activation kink decides anything."""
import ctypes as C

import numpy as np
import pytest

import _conv3d_dispatch as D
from _conv3d_dispatch import ROWS, FASTDIV_ROWS, row_id, geometry
from test_conv_dispatch_gpu import _profiled
from test_gemm_dispatch_gpu import _dev, _p
from test_norm_dispatch_gpu import _out, _check_guards, _GUARDS
from test_ops_gpu import TOL, _rel

pytestmark = pytest.mark.gpu

RUN = [r for r in ROWS if not r['run']]
OWN = ('conv3d_igemm_k<', 'im2col3d', 'col2im3d')        # labels of conv3d.hip's own launches


def _workspace(row, gpu):
    """-> (buffer or None, bytes): GGAN_WS_RESERVED zero bytes, then the row's float count of NaN, then NaN padding"""
    import torch
    if row['ws'] is None:
        return None, 0
    head = D.WS_RESERVED // 4
    buf = torch.full((head + row['ws'] + 4,), float('nan'), dtype=torch.float32, device=gpu)
    buf[:head].zero_()
    return buf, D.WS_RESERVED + 4 * row['ws']


def _check_workspace(row, buf, out_elems):
    """the reserved head is still zero, exactly SK slabs behind it were written (none when SK = 1), the rest is still NaN"""
    import torch
    if buf is None:
        return
    head, used = D.WS_RESERVED // 4, (row['plan']['SK'] * out_elems if row['plan'] and row['plan']['SK'] > 1 else 0)
    assert used <= row['ws'], (used, row['ws'])
    assert bool((buf[:head] == 0).all()), 'the reserved head of the workspace was written'
    assert bool(torch.isfinite(buf[head:head + used]).all()), 'fewer slabs written than the row says'
    assert bool(torch.isnan(buf[head + used:]).all()), 'more of the workspace written than the row says'


def _dims(row):
    return (C.c_int * 10)(*row['dims'])


def _run(row, gpu, inp):
    """-> (rc, [(output name, device tensor)], workspace buffer, result elements per slab)"""
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    N, Ll, H, W, Ci, Co, fl, fs, sl, s = row['dims']
    (Lo, Ho, Wo), _ = geometry(row['dims'])
    off = lambda name: 1 if name in row['off'] else 0
    dev = lambda name: _dev(inp[name], gpu, off(name))
    e, st, dims = row['entry'], F._stream(), _dims(row)
    ws, wsb = _workspace(row, gpu)
    if e == 'fwd':
        x, w, b = dev('x'), dev('w'), (_dev(inp['b'], gpu) if row['bias'] else None)
        y = _out((N, Lo, Ho, Wo, Co), gpu, off('y'))
        rc = L.ggan_conv3d_fwd(dims, _p(x), _p(w), _p(b), _p(y), D.ACTS.index(row['act']), row['alpha'], _p(ws), wsb, st)
        return rc, [('y', y)], ws, y.numel()
    if e == 'wgrad':
        x, gy = dev('x'), dev('gy')
        gw = _out((fl, fs, fs, Ci, Co), gpu, off('gw'))
        rc = L.ggan_conv3d_wgrad(dims, _p(x), _p(gy), _p(gw), _p(ws), wsb, st)
        return rc, [('gw', gw)], ws, gw.numel()
    if e == 'dgrad':
        gy, w = dev('gy'), dev('w')
        gx = _out((N, Ll, H, W, Ci), gpu, off('gx'))
        return L.ggan_conv3d_dgrad(dims, _p(gy), _p(w), _p(gx), st), [('gx', gx)], None, 0
    if e == 'im2col':
        x = dev('x')
        col = _out((N * Lo * Ho * Wo, fl * fs * fs * Ci), gpu, off('col'))
        return L.ggan_im2col3d(dims, _p(x), _p(col), st), [('col', col)], None, 0
    col = dev('col')
    gx = _out((N, Ll, H, W, Ci), gpu, off('gx'))
    return L.ggan_col2im3d(dims, _p(col), _p(gx), st), [('gx', gx)], None, 0


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


@pytest.mark.parametrize('idx', range(len(RUN)), ids=[row_id(r) for r in RUN])
def test_row_runs_its_kernel_and_matches_float64(gpu, idx):
    import torch
    row = RUN[idx]
    del _GUARDS[:]
    inp = D.inputs(row)
    ref = D.reference(row, inp) if not row['refused'] else {}
    (rc, outs, ws, out_elems), recs = _profiled(lambda: _run(row, gpu, inp))
    _check_guards()
    if row['refused']:
        assert rc != 0 and recs == [], (rc, recs)
        assert all(bool(torch.isnan(t).all()) for _, t in outs), 'a refused call wrote its output'
        _check_workspace(dict(row, plan=None), ws, 0)
        return
    assert rc == 0, rc
    _check_launches(row, recs)
    _check_workspace(row, ws, out_elems)
    for what, t in outs:
        got, want = t.double().cpu().numpy(), ref[what]
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.all(np.isfinite(got)), (what, 'elements nobody stored or not finite: %d' % int((~np.isfinite(got)).sum()))
        if row['entry'] in ('im2col', 'col2im'):
            assert np.array_equal(got, want), (what, int((got != want).sum()))
            continue
        e = _rel(got, want)
        print('CONV3D %s %s rel %.3e (tol %.0e)' % (row['launches'][0][0], what, e, TOL))
        assert e <= TOL, (what, e, TOL)
        if row['entry'] == 'dgrad':                # voxels no tap reaches: exact zeros out of the NaN-filled gx
            assert np.all(got[want == 0] == 0), 'a voxel without a tap is not exactly zero'


def _own(recs):
    return [r for r in recs if r['name'].startswith(OWN)]


def _wrong_rows(got, want, width):
    """rows (leading index of the [rows, width] view) where got differs from want"""
    bad = np.flatnonzero((got.reshape(-1, width) != want.reshape(-1, width)).any(axis=1))
    return bad[:8].tolist(), int(bad.size)


@pytest.mark.parametrize('idx', range(len(FASTDIV_ROWS)), ids=[row_id(r) for r in FASTDIV_ROWS])
def test_wide_volume_is_exact(gpu, idx):
    """Wo = 4096 and 258 output rows of that width: row / 4096 by FastDiv is one too large at rows 1 052 671 and 1 056 767 (the last
    voxels of h = 256 and 257), which then decode to w = -1 and gather zeros -- a forward output that is the bias alone, a data
    gradient of zeros, two terms missing from every filter-gradient sum.  ggan_conv3d_igemm_ok must not admit the geometry:
    functional.conv3d takes the patch route, and every result equals the float64 reference exactly (data -1, 0, 1)."""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    row = FASTDIV_ROWS[idx]
    N, Ll, H, W, Ci, Co, fl, fs, sl, s = row['dims']
    inp = D.inputs(row)
    ref = D.reference(row, inp)
    what = list(ref)[0]
    width = dict(y=Co, gw=Co, gx=Ci)[what]
    F.workspace(gpu)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=gpu)
    tx, tw, tb, tgy = t(inp['x']), t(inp['w']), t(inp['b'].reshape(1, 1, 1, 1, Co)), t(inp['gy'])

    def through_autograd(grad_rows=None):
        x = tx.clone().requires_grad_(row['entry'] == 'dgrad')
        w = tw.clone().requires_grad_(row['entry'] == 'wgrad')
        y = F.conv3d(x, w, tb if row['bias'] else None, sl, s, grad_rows=grad_rows)
        if row['entry'] == 'fwd':
            return y.detach()
        return torch.autograd.grad(y, (x if row['entry'] == 'dgrad' else w,), tgy)[0]
    variants = [('functional.conv3d', through_autograd)]
    if row['entry'] == 'dgrad':
        variants.append(('functional.conv3d grad_rows', lambda: through_autograd(N)))
    for name, fn in variants:
        got, recs = _profiled(fn)
        got = got.double().cpu().numpy()
        bad, nbad = _wrong_rows(got, ref[what], width)
        print('CONV3D wide %s %s: %d wrong rows %s; launches %s' % (name, what, nbad, bad, [(r['name'], r['launches'], r['grid']) for r in _own(recs)]))
        assert np.all(np.isfinite(got)) and nbad == 0, (name, what, nbad, bad)
        assert sorted((r['name'], r['launches'], r['grid']) for r in _own(recs)) == sorted((l[0], l[1], D.threads(l)) for l in row['launches']), (_own(recs), row['launches'])
    if L.ggan_conv3d_igemm_ok(_dims(row), D.KIND[row['entry']]):         # whatever the library admits must be right: the C entry point itself
        del _GUARDS[:]
        (rc, outs, ws, _), recs = _profiled(lambda: _run(dict(row, ws=D.BIG if row['entry'] != 'dgrad' else None), gpu, inp))
        _check_guards()
        got = outs[0][1].double().cpu().numpy()
        bad, nbad = _wrong_rows(got, ref[what], width)
        print('CONV3D wide %s %s: rc %d, %d wrong rows %s; launches %s' % (D.ENTRY[row['entry']], what, rc, nbad, bad, [(r['name'], r['grid']) for r in recs]))
        assert rc == 0 and np.all(np.isfinite(got)) and nbad == 0, (D.ENTRY[row['entry']], what, rc, nbad, bad)
