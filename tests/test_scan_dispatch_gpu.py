"""-m gpu: the transition-operator scan (csrc/dynscan.hip), row by row of tests/_scan_dispatch.py.  ggan_dyn_scan_fwd, then
ggan_dyn_scan_bwd on the forward's own zs, h1, h2, through the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler must have
seen exactly the row's launches; every operand sits between sentinels at the offset _scan_dispatch.offset() gives it and every output
starts as NaN; sentinels and inputs must be bit-unchanged; the device's outputs go to _scan_dispatch.check(), which measures every
stage of every step against float64 from the device's own previous stage.  Each row prints the worst fraction per stage; above 1 fails."""
import ctypes as C

import numpy as np
import pytest

import _scan_dispatch as D
from _scan_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled
from test_pointwise_dispatch_gpu import _check_launches

pytestmark = pytest.mark.gpu


class _Bufs:
    def __init__(self, gpu):
        self.gpu, self.b = gpu, {}

    def add(self, name, values=None, shape=None):
        import torch
        n = int(np.prod(shape if values is None else values.shape))
        lo = D.PAD + D.offset(name)
        host = np.full(lo + n + D.PAD, D.SENTINEL, np.float32)
        host[lo:lo + n] = np.nan if values is None else values.ravel()
        dev = torch.from_numpy(host).to(self.gpu)
        assert dev.data_ptr() % 16 == 0 and (dev.data_ptr() + 4 * lo) % 16 == 4 * D.offset(name)
        self.b[name] = (dev, host, lo, n, values is None, shape if values is None else values.shape)

    def p(self, name):
        if name not in self.b:
            return C.c_void_p(None)
        dev, _, lo, _, _, _ = self.b[name]
        return C.c_void_p(dev.data_ptr() + 4 * lo)

    def read(self, keep=()):
        out = {}
        for name, (dev, host, lo, n, is_out, shape) in self.b.items():
            now = dev.cpu().numpy()
            assert np.array_equal(now[:lo], host[:lo]) and np.array_equal(now[lo + n:], host[lo + n:]), 'a store outside %s' % name
            if is_out:
                out[name] = now[lo:lo + n].reshape(shape).copy()
            else:
                assert np.array_equal(now.view(np.uint32), host.view(np.uint32)), '%s is only read' % name
        return out


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_runs_both_scans_and_every_stage_matches_float64(gpu, idx):
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    row = ROWS[idx]
    d = D.inputs(row, 8000 + idx)
    sh = D.shapes(row)
    B = _Bufs(gpu)
    for k in D.INPUTS:
        if d[k] is not None:
            B.add(k, d[k])
    for k in D.FWD_OUT:
        if row['bwd_only']:
            B.add(k, d[k])
        else:
            B.add(k, shape=sh[k])
    for k in D.BWD_OUT:
        if not (row['null'] and k in ('d_z0', 'd_eps')):
            B.add(k, shape=sh[k])
    st = F._stream()
    dims = (row['B'], row['T'], row['dl'], row['dt'], D.H)

    def run():
        if not row['bwd_only']:
            rc = L.ggan_dyn_scan_fwd(*dims, B.p('z0'), B.p('eps'), B.p('w_in'), B.p('b_in'), B.p('w_1'), B.p('b_1'), B.p('w_out'), B.p('b_out'),
                                     B.p('zw'), B.p('b_zw'), D.ALPHA, B.p('zs'), B.p('h1'), B.p('h2'), st)
            assert rc == 0, (rc, L.ggan_last_error())
        rc = L.ggan_dyn_scan_bwd(*dims, B.p('g_zs'), B.p('zs'), B.p('eps'), B.p('h1'), B.p('h2'), B.p('w_in'), B.p('w_1'), B.p('w_out'), B.p('zw'),
                                 D.ALPHA, B.p('G1'), B.p('G2'), B.p('Go'), B.p('Xin'), B.p('d_z0'), B.p('d_eps'), st)
        assert rc == 0, (rc, L.ggan_last_error())
    _, recs = _profiled(run)
    torch.cuda.synchronize()
    _check_launches(row, recs)
    out = B.read()
    fr = D.check(row, d, out)
    print('SCAN %s fractions of the bounds: %s' % (row_id(row), '  '.join('%s %.4f' % kv for kv in sorted(fr.items()))))
    assert D.within(fr), (row_id(row), row['note'], fr)


def test_rejected_calls_launch_nothing_and_leave_their_outputs_alone(gpu):
    import torch
    from graphical_gan_amd import _lib
    L = _lib.load()
    bufs = [torch.full((1 << 17,), float('nan'), dtype=torch.float32, device=gpu) for _ in range(12)]
    pointer = lambda k: bufs[k].data_ptr()

    def run():
        for case in D.REJECTED:
            rc, msg = D.call(L, case, pointer)
            assert rc != 0 and case[0] in msg and case[2] in msg, (case, rc, msg)
    _, recs = _profiled(run)
    assert recs == [], recs
    assert all(bool(torch.isnan(b).all()) for b in bufs)
