"""-m gpu: every path of the optimizer tail (csrc/optim.hip: pack_k, pack_adam_k, adam_k<false>, adam_k<true>, rmsprop_k), row by
row of tests/_optim_dispatch.py.  The row's entry point runs through the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler
must have seen exactly the row's launches, each with the work-item count of the row's grid and block (a record holds that product, not
the grid's shape); the pointers handed over must have exactly the alignment the row states
(which is what decides float4 or scalar inside the kernels, where the profiler cannot look); every output is checked in the stages of
_optim_dispatch's docstring -- flat bitwise, m and v against float64 from the float32 inputs, theta against float64 from the device's own
m and v -- and every buffer is sentinel-filled in front, behind and between the slots: whatever lies outside the launched tensors, and
every source, must be bit-unchanged.  Each check prints the worst observed fraction of its bound; a figure above 1 fails."""
import ctypes as C

import numpy as np
import pytest

import _optim_dispatch as D
from _optim_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled

pytestmark = pytest.mark.gpu


def _up(host, gpu):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(host)).to(gpu)
    assert t.data_ptr() % 16 == 0
    return t


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _p(t, floats=0):
    return C.c_void_p(t.data_ptr() + 4 * floats) if t is not None else C.c_void_p(None)


def _check_launches(row, recs):
    """exactly the row's labels; every (label, work-items per launch) as often as the row says"""
    want = {(l[0], D.threads(l)): l[1] for l in row['launches']}
    assert len(want) == len(row['launches'])
    got = {}
    for r in recs:
        got[(r['name'], r['grid'])] = got.get((r['name'], r['grid']), 0) + r['launches']
    print('launches %s' % sorted(got.items()))
    assert got == want, (sorted(got.items()), sorted(want.items()))


# ---- ggan_pack_adam / ggan_pack_parts2 -------------------------------------------------------------------------------------------------------
def _sources(row, inp, gpu):
    """-> per tensor (device buffer of src or None, of src2 or None, their host images); the pointers have the row's alignment"""
    out = []
    for t, s1, s2 in zip(row['tensors'], inp['src'], inp['src2']):
        h1 = D.src_host(t['size'], t['parts'], t['stride'], t['soff'], s1)[0] if s1 is not None else None
        h2 = D.src_host(t['size'], t['parts2'], t['stride2'], t['soff2'], s2)[0] if s2 is not None else None
        d1, d2 = (_up(h, gpu) if h is not None else None for h in (h1, h2))
        assert (d1 is not None) == t['src'] and (d2 is not None) == (t['parts2'] > 0)
        for d, off in ((d1, t['soff']), (d2, t['soff2'])):
            assert d is None or (d.data_ptr() + 4 * off) % 16 == (4 * off) % 16
        out.append((d1, d2, h1, h2))
    return out


def _table_args(row, lo, hi, srcs, offs):
    tens = row['tensors'][lo:hi]
    k = len(tens)
    arr = lambda ct, vals: (ct * k)(*vals)
    s1 = arr(C.c_void_p, [(srcs[lo + i][0].data_ptr() + 4 * t['soff']) if t['src'] else None for i, t in enumerate(tens)])
    sizes, off = arr(C.c_size_t, [t['size'] for t in tens]), arr(C.c_size_t, offs[lo:hi])
    parts, strides = arr(C.c_int, [t['parts'] for t in tens]), arr(C.c_size_t, [t['stride'] for t in tens])
    if not any(t['parts2'] for t in tens):
        return s1, sizes, off, parts, strides, None, None, None, k
    s2 = arr(C.c_void_p, [(srcs[lo + i][1].data_ptr() + 4 * t['soff2']) if t['parts2'] else None for i, t in enumerate(tens)])
    return s1, sizes, off, parts, strides, s2, arr(C.c_int, [max(t['parts2'], 1) for t in tens]), arr(C.c_size_t, [t['stride2'] for t in tens]), k


def _run_pack_rows(row, gpu, inp):
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    adam = row['entry'] == 'pack_adam'
    offs, total = D.layout(row['tensors'])
    for t, off in zip(row['tensors'], offs):                                # (bounds, before anything runs)
        assert D.PAD <= off and off + t['size'] + 4 <= total and off % 4 == t['slot']
    srcs = _sources(row, inp, gpu)
    flat = _up(np.full(total, D.SENTINEL), gpu)
    state = [_up(inp[k], gpu) for k in ('theta', 'm', 'v')] if adam else []
    bufs = [flat] + state
    for b, (t, off) in ((b, to) for b in bufs for to in zip(row['tensors'], offs)):
        assert (b.data_ptr() + 4 * off) % 16 == (4 * t['slot']) % 16
    step = torch.tensor([row['step0']], dtype=torch.int32, device=gpu)
    arrive = torch.zeros(D.ARRIVE_INTS, dtype=torch.int32, device=gpu)
    segs = D.segments(row) if adam else [(0, len(row['tensors']), True)] * row['repeat']
    lr, b1, b2, eps = row['hyper'] if adam else (0, 0, 0, 0)

    def run():
        shots = [([b.clone() for b in bufs], int(step.item()))]
        for lo, hi, counted in segs:
            s1, sizes, off, parts, strides, s2, p2, st2, k = _table_args(row, lo, hi, srcs, offs)
            if adam:
                rc = L.ggan_pack_adam(s1, sizes, off, parts, strides, s2, p2, st2, k, _p(flat), _p(state[0]), _p(state[1]), _p(state[2]), _p(step),
                                      _p(arrive if counted else None), lr, b1, b2, eps, row['gscale'], F._stream())
            else:
                rc = L.ggan_pack_parts2(s1, sizes, off, parts, strides, s2, p2, st2, k, _p(flat), _p(step if row['bump'] else None), F._stream())
            assert rc == 0, (rc, L.ggan_last_error())
            torch.cuda.synchronize()
            shots.append(([b.clone() for b in bufs], int(step.item())))
            assert int(arrive.abs().max()) == 0, 'arrival counters not left at zero'
        return shots
    shots, recs = _profiled(run)
    _check_launches(row, recs)
    worst = dict(m=0.0, v=0.0, theta=0.0, theta_at_0=0.0)
    for li, (lo, hi, counted) in enumerate(segs):
        (before, step_b), (after, step_a) = shots[li], shots[li + 1]
        before, after = [b.cpu().numpy() for b in before], [b.cpu().numpy() for b in after]
        # the counter: once per completed update (pack: once per launch that was given it)
        assert step_a == step_b + (1 if (counted and (adam or row['bump'])) else 0), (li, step_b, step_a)
        t_ord = step_b + 1
        assert not adam or t_ord == D.ordinal(row, li), (li, t_ord, D.ordinal(row, li))
        inside = np.zeros(total, bool)
        for t, off in list(zip(row['tensors'], offs))[lo:hi]:
            inside[off:off + t['size']] = True
        for name, b, a in zip(('flat', 'theta', 'm', 'v'), before, after):
            assert _same_bits(b[~inside], a[~inside]), 'launch %d stored outside its tensors in %s' % (li, name)
        plans = D.tensor_plans(row, lo, hi)
        for k in range(lo, hi):
            t, off, plan = row['tensors'][k], offs[k], plans[k - lo]
            n = t['size']
            sl = slice(off, off + n)
            g32 = D.flat_sum(inp['src'][k], inp['src2'][k], n)
            bad = np.flatnonzero(after[0][sl].view(np.uint32) != g32.view(np.uint32))
            assert bad.size == 0, ('flat', li, k, plan, bad[:8], after[0][sl][bad[:8]], g32[bad[:8]])
            if not adam:
                continue
            fr = D.adam_fractions(g32, before[1][sl], before[2][sl], before[3][sl], after[1][sl], after[2][sl], after[3][sl], t_ord, row['hyper'],
                                  row['gscale'])
            print('OPTIM pack_adam launch %d tensor %d n=%d %s chunk %d wgs %d..%d tail %s: fractions of the bound m %.4f v %.4f theta %.4f (at zero weights %.4f)'
                  % (li, k, n, plan['path'], plan['chunk'], plan['first'], plan['last'], plan['tail'], fr['m'], fr['v'], fr['theta'], fr['theta_at_0']))
            for key in worst:
                worst[key] = max(worst[key], fr[key])
            assert D.within(fr), (li, k, plan, fr)
            still = (g32 == 0) & (before[2][sl] == 0) & (before[3][sl] == 0)
            assert _same_bits(before[1][sl][still], after[1][sl][still]), 'g = m = v = 0 moved a weight'
    for d1, d2, h1, h2 in srcs:                                           # read-only inputs
        assert (d1 is None or _same_bits(d1.cpu().numpy(), h1)) and (d2 is None or _same_bits(d2.cpu().numpy(), h2))
    if adam:
        print('OPTIM %s worst fraction of the bound: m %.4f v %.4f theta %.4f (at zero weights %.4f)'
              % (row_id(row), worst['m'], worst['v'], worst['theta'], worst['theta_at_0']))
    elif not row['bump']:
        assert shots[-1][1] == row['step0']


# ---- ggan_adam_step (+ ggan_adam_advance), ggan_adam_step_counted, ggan_rmsprop_step ------------------------------------------------------------
def _padded(values, gpu):
    host = np.concatenate([np.full(D.PAD, D.SENTINEL), np.asarray(values, np.float32), np.full(D.PAD, D.SENTINEL)])
    buf = _up(host, gpu)
    view = buf[D.PAD:D.PAD + values.size]
    assert view.data_ptr() % 16 == 0
    return buf, view, host


def _pads_intact(buf):
    h = buf.cpu().numpy()
    return bool(np.all(h[:D.PAD] == D.SENTINEL) and np.all(h[-D.PAD:] == D.SENTINEL))


def _run_step_rows(row, gpu, inp):
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    e, n = row['entry'], row['n']
    gbuf, g, ghost = _padded(inp['g'], gpu)
    tbuf, theta, _ = _padded(inp['theta'], gpu)
    mbuf, m, _ = _padded(inp['m'], gpu)
    step = torch.tensor([row['step0']], dtype=torch.int32, device=gpu)
    if e == 'rmsprop_step':
        lr, decay, eps = row['hyper']
        lo, hi = (float('-inf'), float('inf')) if row['clip'] is None else row['clip']

        def run():
            rc = L.ggan_rmsprop_step(_p(theta), _p(g), _p(m), n, lr, decay, eps, row['gscale'], lo, hi, F._stream())
            assert rc == 0, (rc, L.ggan_last_error())
        _, recs = _profiled(run)
        _check_launches(row, recs)
        fr, not_edge, near, moved = D.rms_fractions(inp['g'], inp['theta'], inp['m'], theta.cpu().numpy(), m.cpu().numpy(), row['hyper'],
                                                    row['gscale'], row['clip'])
        print('OPTIM %s worst fraction of the bound: ms %.4f theta %.4f (%.2f %% of the elements within their bound of a clip edge)'
              % (row_id(row), fr['ms'], fr['theta'], 100 * near))
        assert D.within(fr) and not_edge == 0 and moved == 0 and near <= 0.01, (fr, not_edge, moved, near)
        assert int(step.item()) == row['step0']
        bufs = (gbuf, tbuf, mbuf)
    else:
        vbuf, v, _ = _padded(inp['v'], gpu)
        lr, b1, b2, eps = row['hyper']
        counted = e == 'adam_step_counted'

        def run():
            fn = L.ggan_adam_step_counted if counted else L.ggan_adam_step
            rc = fn(_p(theta), _p(g), _p(m), _p(v), n, _p(step), lr, b1, b2, eps, row['gscale'], F._stream())
            assert rc == 0, (rc, L.ggan_last_error())
            if not counted:
                assert L.ggan_adam_advance(_p(step), F._stream()) == 0
        _, recs = _profiled(run)
        _check_launches(row, recs)
        assert int(step.item()) == row['step0'] + (0 if counted else 1)
        th1, m1, v1 = theta.cpu().numpy(), m.cpu().numpy(), v.cpu().numpy()
        fr = D.adam_fractions(inp['g'], inp['theta'], inp['m'], inp['v'], th1, m1, v1, D.ordinal(row), row['hyper'], row['gscale'])
        print('OPTIM %s worst fraction of the bound: m %.4f v %.4f theta %.4f (at zero weights %.4f)'
              % (row_id(row), fr['m'], fr['v'], fr['theta'], fr['theta_at_0']))
        assert D.within(fr), fr
        still = (inp['g'] == 0) & (inp['m'] == 0) & (inp['v'] == 0)
        assert _same_bits(inp['theta'][still], th1[still]), 'g = m = v = 0 moved a weight'
        bufs = (gbuf, tbuf, mbuf, vbuf)
    assert all(_pads_intact(b) for b in bufs), 'a store outside a buffer'
    assert _same_bits(gbuf.cpu().numpy(), ghost), 'the gradient is only read'


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_takes_its_path_and_matches_float64(gpu, idx):
    from graphical_gan_amd import functional as F
    row = ROWS[idx]
    F.workspace(gpu)                     # (allocated and zeroed outside the profiled region)
    inp = D.inputs(row, 9000 + idx)
    (_run_pack_rows if row['entry'] in ('pack', 'pack_adam') else _run_step_rows)(row, gpu, inp)
