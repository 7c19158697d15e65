"""-m gpu: every path of the pointwise, reduction and staging kernels (csrc/pointwise.hip), row by row of tests/_pointwise_dispatch.py.
The row's entry point runs through the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the row's
launches, each with the work-item count of the row's grid and block; every operand sits between sentinels at the row's base offset and
every output starts as NaN; the sentinels and the inputs must be bit-unchanged afterwards; the device's outputs (and, for the two-stage
sums, its partials read back from the workspace) go to _pointwise_dispatch.check().  Each row prints the worst observed fraction of its
bounds; a figure above 1 fails."""
import ctypes as C

import numpy as np
import pytest

import _pointwise_dispatch as D
from _pointwise_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled

pytestmark = pytest.mark.gpu
RES_FLOATS = D.WS_RESERVED // 4


def _check_launches(row, recs):
    """exactly the row's labels; every (label, work-items per launch) as often as the row says"""
    want = {(l[0], D.threads(l)): l[1] for l in row['launches']}
    assert len(want) == len(row['launches'])
    got = {}
    for r in recs:
        got[(r['name'], r['grid'])] = got.get((r['name'], r['grid']), 0) + r['launches']
    print('launches %s' % sorted(got.items()))
    assert got == want, (sorted(got.items()), sorted(want.items()))


class _Bufs:
    """the row's device buffers: PAD sentinels, the row's offset, the data (inputs, or NaN for outputs), PAD sentinels"""

    def __init__(self, row, inp, gpu):
        import torch
        self.b = {}
        for name, kind, dt, n in D.buffers(row):
            off = row['off'].get(name, 0)
            lo = D.PAD + off
            host = np.full(lo + n + D.PAD, D.SENTINEL if dt is np.float32 else D.INT_SENTINEL, dtype=dt)
            host[lo:lo + n] = inp[name] if kind == 'in' else np.nan
            dev = torch.from_numpy(host).to(gpu)
            assert dev.data_ptr() % 16 == 0 and (dev.data_ptr() + 4 * lo) % 16 == (4 * off) % 16
            self.b[name] = (dev, host, lo, n, kind)

    def addr(self, name, elems=0):
        dev, _, lo, _, _ = self.b[name]
        return dev.data_ptr() + 4 * (lo + elems)

    def p(self, name, elems=0):
        return C.c_void_p(self.addr(name, elems)) if name in self.b else C.c_void_p(None)

    def read(self, written=()):
        """-> {output name: values}; asserts the sentinels of every buffer and the bits of every input (but those named in `written`)"""
        out = {}
        for name, (dev, host, lo, n, kind) in self.b.items():
            now = dev.cpu().numpy()
            assert np.array_equal(now[:lo], host[:lo]) and np.array_equal(now[lo + n:], host[lo + n:]), 'a store outside %s' % name
            if kind == 'out' or name in written:
                out[name] = now[lo:lo + n].copy()
            else:
                assert np.array_equal(now.view(np.uint32), host.view(np.uint32)), '%s is only read' % name
        return out


def _workspace(row, gpu):
    """-> (device buffer or None, ws_bytes, floats of scratch): zeroed reserved bytes, NaN scratch, PAD sentinels"""
    import torch
    have = D.ws_floats(row)
    if have is None:
        return None, D.WS_RESERVED + (1 << 20), 0
    host = np.concatenate([np.zeros(RES_FLOATS, np.float32), np.full(have, np.nan, np.float32), np.full(D.PAD, D.SENTINEL)])
    return torch.from_numpy(host).to(gpu), D.WS_RESERVED + 4 * have, have


def _run(row, inp, gpu):
    """-> (outputs for check(), profiler records)"""
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    e, p = row['entry'], row['p']
    B = _Bufs(row, inp, gpu)
    st = F._stream()
    extra, written = {}, ()
    ws = ws_bytes = have = None
    if e in ('colsum_tall', 'chansum'):
        ws, ws_bytes, have = _workspace(row, gpu)
    if e == 'stage':
        ws = F.workspace(gpu)
    wsp = C.c_void_p(ws.data_ptr()) if ws is not None else C.c_void_p(None)
    n_parts = C.c_int(-7)

    def run():
        if e == 'act_fwd':
            rc = L.ggan_act_fwd(B.p('x'), B.p('y'), p['n'], p['act'], D.ALPHA, st)
        elif e == 'act_bwd':
            rc = L.ggan_act_bwd(B.p('gy'), B.p('ref'), B.p('gx'), p['n'], p['act'], D.ALPHA, st)
        elif e == 'act_bwd_chansum':
            rc = L.ggan_act_bwd_chansum(B.p('gy'), B.p('ref'), B.p('gx'), B.p('parts'), p['cap'], C.byref(n_parts), p['N'], p['C'], p['HW'],
                                        p['act'], D.ALPHA, st)
            rc = rc or L.ggan_act_bwd(B.p('gy'), B.p('ref'), B.p('gx2'), p['N'] * p['C'] * p['HW'], p['act'], D.ALPHA, st)
        elif e == 'bias_add':
            rc = L.ggan_bias_add(B.p('x'), B.p('bias'), B.p('y'), p['N'], p['C'], p['HW'], st)
        elif e == 'cast_scale':
            rc = L.ggan_cast_scale_i32(B.p('x'), B.p('noise'), B.p('y'), p['n'], p['div'], p['mul'], st)
        elif e == 'cast_ring':
            ca = B.p('ctr', 0) if p['ctr_a'] is not None else C.c_void_p(None)
            cb = B.p('ctr', 1) if p['ctr_b'] is not None else C.c_void_p(None)
            rc = L.ggan_cast_scale_ring_i32(B.p('ring'), p['nslots'], ca, cb, p['offset'], B.p('noise'), B.p('y'), p['n'], p['div'], p['mul'], st)
            rc = rc or L.ggan_cast_scale_i32(B.p('ring', D.ring_slot(p) * p['n']), B.p('noise'), B.p('y2'), p['n'], p['div'], p['mul'], st)
        elif e == 'axpby':
            a, b, c = p['abc']
            rc = L.ggan_axpby(B.p('x'), B.p('y'), B.p('x' if p['inplace'] else 'out'), p['n'], a, b, c, st)
        elif e == 'row_lerp':
            rc = L.ggan_row_lerp(B.p('x'), B.p('y'), B.p('alpha'), B.p('out'), p['rows'], p['cols'], st)
        elif e == 'colsum':
            rc = L.ggan_colsum(B.p('x'), B.p('out'), p['rows'], p['cols'], st)
        elif e == 'colsum_tall':
            rc = L.ggan_colsum_tall(B.p('x'), B.p('out'), p['rows'], p['cols'], wsp, ws_bytes, st)
        elif e == 'chansum':
            rc = L.ggan_chansum(B.p('x'), B.p('out'), p['N'], p['C'], p['HW'], wsp, ws_bytes, st)
        elif e == 'reparam_fwd':
            rc = L.ggan_reparam_fwd(B.p('mean'), B.p('log_std'), B.p('eps'), B.p('z'), B.p('sd'), p['n'], st)
        elif e == 'reparam_bwd':
            rc = L.ggan_reparam_bwd(B.p('gz'), B.p('gsd'), B.p('eps'), B.p('sd'), B.p('gmean'), B.p('glog'), p['n'], st)
        elif e == 'stage':
            if p['join']:
                rc = L.ggan_gemm_split(p['ta'], 0, p['M'], p['Nn'], p['K'], B.p('A'), B.p('A2'), p['split'], B.p('B'), None, B.p('C'), None, 0, None,
                                       D.ACT_NONE, 0.0, wsp, ws.numel(), st)
            else:
                rc = L.ggan_gemm_split(0, 0, p['M'], p['Nn'], p['K'], B.p('A'), None, 0, B.p('B'), None, B.p('C'), B.p('C2'), p['split'], None,
                                       D.ACT_NONE, 0.0, wsp, ws.numel(), st)
        else:
            raise KeyError(e)
        assert rc == 0, (rc, L.ggan_last_error())
    _, recs = _profiled(run)
    torch.cuda.synchronize()
    if e == 'axpby' and p['inplace']:
        written = ('x',)
    if e == 'cast_ring':
        written = ('ctr',)                   # (read back and held bitwise by check())
    out = B.read(written)
    if e == 'axpby' and p['inplace']:
        out['out'] = out.pop('x')
    if e == 'act_bwd_chansum':
        out['n_parts'] = n_parts.value
    if e in ('colsum_tall', 'chansum') and ws is not None:
        h = ws.cpu().numpy()
        assert not h[:RES_FLOATS].any(), 'the reserved bytes of the workspace are left zero'
        assert np.all(h[RES_FLOATS + have:] == D.SENTINEL), 'a store behind the workspace'
        two = D.tall_plan(row) is not None if e == 'colsum_tall' else D.chan_plan(row)[0] > 1
        if two:
            out['part'] = h[RES_FLOATS:RES_FLOATS + have].copy()
        else:
            assert np.all(np.isnan(h[RES_FLOATS:RES_FLOATS + have])), 'a fallback wrote to the workspace'
    return out, recs


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_takes_its_path_and_matches_float64(gpu, idx, monkeypatch):
    from graphical_gan_amd import functional as F
    monkeypatch.delenv('GGAN_GEMM_SK', raising=False)
    row = ROWS[idx]
    F.workspace(gpu)                     # (allocated and zeroed outside the profiled region)
    inp = D.inputs(row, 7000 + idx)
    out, recs = _run(row, inp, gpu)
    _check_launches(row, recs)
    fr = D.check(row, inp, out)
    print('POINTWISE %s fractions of the bounds: %s' % (row_id(row), '  '.join('%s %.4f' % kv for kv in sorted(fr.items()))))
    assert D.within(fr), (row_id(row), row['note'], fr)


def test_rejected_and_empty_calls_launch_nothing_and_leave_their_outputs_alone(gpu):
    import torch
    from graphical_gan_amd import _lib
    L = _lib.load()
    bufs = [torch.full((4096,), float('nan'), dtype=torch.float32, device=gpu) for _ in range(7)]
    pointer = lambda k: bufs[k].data_ptr()

    def run():
        for case in D.REJECTED:
            rc, msg, n_parts = D.call(L, case, pointer)
            assert rc != 0 and case[0] in msg and case[2] in msg and n_parts == -7, (case, rc, msg)
        for case in D.EMPTY:
            rc, _, _ = D.call(L, case, pointer)
            assert rc == 0, case
    _, recs = _profiled(run)
    assert recs == [], recs
    assert all(bool(torch.isnan(b).all()) for b in bufs)
