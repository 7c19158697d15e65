"""-m gpu: every path of the latent-space and noise kernels (csrc/latent.hip), row by row of tests/_latent_dispatch.py.  A row's calls run
through the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the row's launches, each with the
work-item count of the row's grid and block.  Every buffer sits between sentinel pads, outputs start as NaN (integers as -1, colbest as
the caller's zeros); afterwards the inputs and the pads must keep their bits.  The outputs are checked in the stages of
_latent_dispatch's docstring -- each stage against float64 from the float32 values the stage itself read, the exact stages bit for bit.
Each check prints the worst observed fraction of its bound; a figure above 1 fails.  The calls of REJECTED must come back non-zero with
a message, no launch and untouched outputs."""
import ctypes as C

import numpy as np
import pytest

import _latent_dispatch as D
from _latent_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled
from test_cost_dispatch_gpu import DeviceAlloc

pytestmark = pytest.mark.gpu

_SENT = {np.dtype(np.float32): D.SENTINEL, np.dtype(np.int32): -12345, np.dtype(np.int64): -12345}


class Buf:
    """a device buffer of float32 / int32 / int64 between PAD sentinels on either side; out: filled with `fill`, else it holds `values` and
    is read-only"""
    def __init__(self, gpu, values=None, n=0, fill=np.nan, dtype=np.float32):
        import torch
        self.out = values is None
        body = np.full(n, fill, dtype) if self.out else np.ascontiguousarray(np.ravel(values), dtype)
        pad = np.full(D.PAD, _SENT[np.dtype(dtype)], dtype)
        self.host = np.concatenate([pad, body, pad])
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        self.n, self.size = body.size, body.itemsize

    def p(self):
        return C.c_void_p(self.dev.data_ptr() + self.size * D.PAD)

    def get(self, shape=None, tail=False):
        a = self.dev.cpu().numpy()[D.PAD:D.PAD + self.n + (D.PAD if tail else 0)]
        return a.reshape(shape) if shape is not None else a

    def intact(self):
        now = self.dev.cpu().numpy()
        same = lambda a, b: a.tobytes() == b.tobytes()
        return same(now[:D.PAD], self.host[:D.PAD]) and same(now[-D.PAD:], self.host[-D.PAD:]) and (self.out or same(now, self.host))


class Bufs:
    def __init__(self, gpu):
        self.gpu, self.all = gpu, []

    def inp(self, values, dtype=np.float32):
        self.all.append(Buf(self.gpu, values, dtype=dtype))
        return self.all[-1]

    def out(self, n, fill=np.nan, dtype=np.float32):
        self.all.append(Buf(self.gpu, None, n, fill, dtype))
        return self.all[-1]

    def intact(self):
        return all(b.intact() for b in self.all)


def _check_launches(row, recs):
    """exactly the row's labels; every (label, work-items per launch) as often as the row says"""
    want = {}
    for l in row['launches']:
        want[(l[0], D.threads(l))] = want.get((l[0], D.threads(l)), 0) + l[1]
    got = {}
    for r in recs:
        got[(r['name'], r['grid'])] = got.get((r['name'], r['grid']), 0) + r['launches']
    print('launches %s' % sorted(got.items()))
    assert got == want, (sorted(got.items()), sorted(want.items()))


def _ok(L, rc):
    assert rc == 0, (rc, L.ggan_last_error())


def _p(b):
    return b.p() if b is not None else None


def _run_noise(row, inp, B, L, S):
    import torch
    specs = row['specs']
    n = len(specs)
    assert n <= D.NOISE_MAX and all(0 < s[1] <= D.BIG_N for s in specs)                   # (bounds, before anything runs)
    state = B.out(3, 0, np.int64)
    calls = [[B.out(s[1]) for s in specs] for _ in row['draws']]
    sizes = (C.c_size_t * n)(*[s[1] for s in specs])
    kinds, a, b, widths = D._ints([s[0] for s in specs]), D._floats([s[2] for s in specs]), D._floats([s[3] for s in specs]), D._ints([s[4] for s in specs])
    states = []

    def run():
        state.dev[D.PAD] = row['seed']
        for d, bufs in zip(row['draws'], calls):
            if d is not None:
                state.dev[D.PAD + 1] = d
            _ok(L, L.ggan_noise_fill(D._ptrs([x.p() for x in bufs]), sizes, kinds, a, b, widths, n, state.p(), S))
            torch.cuda.synchronize()
            states.append(tuple(int(x) for x in state.get()))
    return run, lambda: dict(vals=[[x.get(tail=True) for x in bufs] for bufs in calls], states=states)


def _run_latent(row, inp, B, L, S):
    Bn, K, Dn, temp, lp = row['B'], row['K'], row['D'], row['temp'], float(inp['log_pi'])
    assert K <= D.GMM_MAX_K and (Bn <= D.GMM_MAX_K or not row['bwd'])
    z, mu, u, gl, gk = B.inp(inp['z']), B.inp(inp['mu']), B.inp(inp['u']), B.inp(inp['gl']), B.inp(inp['gk'])
    o = {k: B.out(Bn * K) for k in ('lg', 'k', 'k_nolog', 'lg_stc', 'soft', 'k_stc', 'lg_st', 'k_st')}
    calls = D.bwd_calls(row)
    g = {}
    for name, _, _, _, _, dz, dmu in calls:
        g['dz' + name], g['dmu' + name] = B.out(Bn * Dn) if dz else None, B.out(K * Dn) if dmu else None

    def run():
        _ok(L, L.ggan_gmm_latent_fwd(z.p(), mu.p(), u.p(), o['lg'].p(), o['k'].p(), Bn, K, Dn, lp, temp, S))
        _ok(L, L.ggan_gmm_latent_fwd(z.p(), mu.p(), u.p(), None, o['k_nolog'].p(), Bn, K, Dn, lp, temp, S))
        _ok(L, L.ggan_gmm_latent_st_fwd(z.p(), mu.p(), u.p(), o['lg_stc'].p(), o['k_stc'].p(), o['soft'].p(), Bn, K, Dn, lp, temp, D.MODE_STC, S))
        _ok(L, L.ggan_gmm_latent_st_fwd(z.p(), mu.p(), None, o['lg_st'].p(), o['k_st'].p(), None, Bn, K, Dn, lp, temp, D.MODE_ST, S))
        for name, st, mode, wgl, wgk, dz, dmu in calls:
            pgl, pgk, pdz, pdmu = gl.p() if wgl else None, gk.p() if wgk else None, _p(g['dz' + name]), _p(g['dmu' + name])
            if st:                                                       # STC reads the soft the forward kept; ST reads none
                _ok(L, L.ggan_gmm_latent_st_bwd(z.p(), mu.p(), o['soft'].p() if mode == D.MODE_STC else None, pgl, pgk, pdz, pdmu, Bn, K, Dn, temp, mode, S))
            else:
                _ok(L, L.ggan_gmm_latent_bwd(z.p(), mu.p(), o['k'].p(), pgl, pgk, pdz, pdmu, Bn, K, Dn, temp, S))

    def collect():
        out = {k: v.get((Bn, K)) for k, v in o.items()}
        for k, v in g.items():
            out[k] = None if v is None else v.get((Bn, Dn) if k.startswith('dz') else (K, Dn))
        return out
    return run, collect


def _run_mix(row, inp, B, L, S):
    Bn, K, Dn = row['B'], row['K'], row['D']
    k, mu, noise, out = B.inp(inp['k']), B.inp(inp['mu']), B.inp(inp['noise']), B.out(Bn * Dn)
    assert Dn % 4 == 0 and all(x.p().value % 16 == 0 for x in (mu, noise, out))

    def run():
        _ok(L, L.ggan_mix_mean(k.p(), mu.p(), noise.p(), out.p(), Bn, K, Dn, S))
    return run, lambda: dict(out=out.get((Bn, Dn)))


def _run_post(row, inp, B, L, S):
    K, Dn, lp = row['K'], row['D'], float(inp['log_pi'])
    N = inp['labels'].size
    assert K <= D.POSTERIOR_MAX_K and all(0 <= r0 and r0 + b <= N for r0, b in row['batches'])
    mu, labels = B.inp(inp['mu']), B.inp(inp['labels'], np.int32)
    zs = [B.inp(z) for z in inp['zs']]
    probs = [B.out(b * K) for _, b in row['batches']]
    assign, assign2 = B.out(N, -1, np.int32), B.out(N, -1, np.int32)
    col, col2 = B.out(K, 0, np.int64), B.out(K, 0, np.int64)
    correct = B.out(1, -7, np.int32)

    def run():
        for (r0, b), z, p in zip(row['batches'], zs, probs):
            _ok(L, L.ggan_gmm_posterior_assign(z.p(), mu.p(), lp, b, K, Dn, r0, p.p(), assign.p(), col.p(), S))
            _ok(L, L.ggan_gmm_posterior_assign(z.p(), mu.p(), lp, b, K, Dn, r0, None, assign2.p(), col2.p(), S))
        _ok(L, L.ggan_cluster_accuracy(assign.p(), labels.p(), col.p(), N, K, correct.p(), S))
    return run, lambda: dict(probs=[p.get((b, K)) for p, (_, b) in zip(probs, row['batches'])], assign=assign.get(), assign2=assign2.get(),
                             colbest=col.get().view(np.uint64), colbest2=col2.get().view(np.uint64), correct=int(correct.get()[0]))


def _run_acc(row, inp, B, L, S):
    N, K = row['N'], row['K']
    assign, labels, col = B.inp(inp['assign'], np.int32), B.inp(inp['labels'], np.int32), B.inp(inp['colbest'].view(np.int64), np.int64)
    correct = B.out(1, -7, np.int32)

    def run():
        _ok(L, L.ggan_cluster_accuracy(assign.p(), labels.p(), col.p(), N, K, correct.p(), S))
    return run, lambda: dict(correct=int(correct.get()[0]))


_RUN = dict(noise=_run_noise, latent=_run_latent, mix=_run_mix, post=_run_post, acc=_run_acc)


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_takes_its_path_and_matches_float64(gpu, idx):
    from graphical_gan_amd import functional as F, _lib, evaluate as E
    L = _lib.load()
    row = ROWS[idx]
    inp = D.inputs(row, 9000 + idx)
    B = Bufs(gpu)
    run, collect = _RUN[row['entry']](row, inp, B, L, F._stream())
    _, recs = _profiled(run)
    _check_launches(row, recs)
    out = collect()
    assert B.intact(), 'an input or a sentinel pad changed'
    fr, broken = D.check(row, inp, out)
    kernels = D.kernels_of(row)
    for key in sorted(fr):
        print('LATENTFRAC %s %s %s %.4f' % (row_id(row), kernels[key], key, fr[key]))
    assert not broken and D.within(fr), (fr, broken)
    if row['entry'] == 'post':
        assert out['correct'] == E.decode_cluster_accuracy(out['assign'], inp['labels'], out['colbest'])
    if row['entry'] == 'acc':
        assert out['correct'] == E.decode_cluster_accuracy(inp['assign'], inp['labels'], inp['colbest'])


@pytest.mark.parametrize('item', D.REJECTED, ids=[r['id'] for r in D.REJECTED])
def test_rejected_call_returns_an_error_and_launches_nothing(gpu, item):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    A = DeviceAlloc(gpu)
    rc, recs = _profiled(lambda: item['call'](L, A, F._stream()))
    msg = (L.ggan_last_error() or b'').decode()
    assert rc != 0 and item['fn'] in msg, (rc, msg)
    assert recs == [], recs
    assert A.outs and A.outputs_untouched(), 'a rejected call wrote to an output'
