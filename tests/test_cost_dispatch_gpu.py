"""-m gpu: every path of the cost kernels (csrc/losses.hip, cost_head.h), row by row of tests/_cost_dispatch.py.  A row's calls run through
the C ABI between ggan_prof_reset / ggan_prof_enable; the profiler must have seen exactly the row's launches, each with the work-item
count of the row's grid and block (a record holds that product, not the grid's shape).  Every buffer sits between sentinel pads, outputs
start as NaN; afterwards the inputs and the pads must keep their bits and every output must be finite.  The outputs are checked in the
stages of _cost_dispatch's docstring -- each stage against float64 from the float32 values the stage itself read, the exact stages bit
for bit.  Each check prints the worst observed fraction of its bound; a figure above 1 fails.  The calls of REJECTED must come back
non-zero with a message, no launch and untouched outputs."""
import ctypes as C

import numpy as np
import pytest

import _cost_dispatch as D
from _cost_dispatch import ROWS, row_id
from test_conv_dispatch_gpu import _profiled

pytestmark = pytest.mark.gpu


class Buf:
    """a device buffer of float32 between PAD sentinels on either side; out: NaN-filled (or `fill`), else it holds `values` and is read-only"""
    def __init__(self, gpu, values=None, n=0, fill=np.nan, dtype=np.float32):
        import torch
        self.out = values is None
        body = np.full(n, fill, dtype) if self.out else np.ascontiguousarray(np.ravel(values), dtype)
        pad = np.full(D.PAD, D.SENTINEL if dtype == np.float32 else -12345, dtype)
        self.host = np.concatenate([pad, body, pad])
        self.dev = torch.from_numpy(self.host.copy()).to(gpu)
        self.n = body.size

    def p(self, off=0):
        assert 0 <= off < max(self.n, 1)
        return C.c_void_p(self.dev.data_ptr() + 4 * (D.PAD + off))

    def get(self, shape=None):
        a = self.dev.cpu().numpy()[D.PAD:D.PAD + self.n]
        return a.reshape(shape) if shape is not None else a

    def intact(self):
        now = self.dev.cpu().numpy()
        same = lambda a, b: np.array_equal(a.view(np.uint32), b.view(np.uint32))
        return same(now[:D.PAD], self.host[:D.PAD]) and same(now[-D.PAD:], self.host[-D.PAD:]) and (self.out or same(now, self.host))


class Bufs:
    def __init__(self, gpu):
        self.gpu, self.all = gpu, []

    def inp(self, values, dtype=np.float32):
        self.all.append(Buf(self.gpu, values, dtype=dtype))
        return self.all[-1]

    def out(self, n, fill=np.nan):
        self.all.append(Buf(self.gpu, None, n, fill))
        return self.all[-1]

    def intact(self):
        return all(b.intact() for b in self.all)


def _check_launches(row, recs):
    """exactly the row's labels; every (label, work-items per launch) as often as the row says"""
    want = {(l[0], D.threads(l)): l[1] for l in row['launches']}
    assert len(want) == len(row['launches'])
    got = {}
    for r in recs:
        got[(r['name'], r['grid'])] = got.get((r['name'], r['grid']), 0) + r['launches']
    print('launches %s' % sorted(got.items()))
    assert got == want, (sorted(got.items()), sorted(want.items()))


def _ok(L, rc):
    assert rc == 0, (rc, L.ggan_last_error())


def _f1(b):
    return np.float32(b.get()[0])


def _offsets(ns):
    return [int(o) for o in np.concatenate([[0], np.cumsum(ns)[:-1]])]


def _table(B, terms, xs):
    """-> (the logits buffer, ctypes tables xs / labels / weights / ns, count, term offsets)"""
    ns = [t[0] for t in terms]
    X = B.inp(np.concatenate(xs))
    offs = _offsets(ns)
    return X, D._ptrs([X.p(o) for o in offs]), D._floats([t[1] for t in terms]), D._floats([t[2] for t in terms]), D._ints(ns), len(ns), offs


def _run_single(row, inp, B, L, S):
    n, mean = row['n'], row['kind'] == 'mean'
    x, gl = B.inp(inp['x']), B.inp([row['gloss']])
    loss, gx = B.out(1, row['prior'] if row['acc'] else np.nan), B.out(n)

    def run():
        if mean:
            _ok(L, L.ggan_mean_fwd(x.p(), row['w'], loss.p(), n, row['acc'], S))
            _ok(L, L.ggan_mean_bwd(gl.p(), row['w'], gx.p(), n, S))
        else:
            _ok(L, L.ggan_bce_logits_fwd(x.p(), row['z'], row['w'], loss.p(), n, row['acc'], S))
            _ok(L, L.ggan_bce_logits_bwd(x.p(), row['z'], row['w'], gl.p(), gx.p(), n, S))
    return run, lambda: dict(loss=_f1(loss), gx=gx.get())


def _run_table(row, inp, B, L, S):
    terms, mean = row['terms'], row['kind'] == 'mean'
    X, xs, lab, wts, ns, c, offs = _table(B, terms, inp['xs'])
    N = X.n
    G, G3, gl = B.out(N), B.out(N), B.inp([3.0])
    la, lb, lc = B.out(1), B.out(1), B.out(1)
    gp = lambda g: D._ptrs([g.p(o) for o in offs])

    def run():
        if mean:
            _ok(L, L.ggan_mean_multi_fwd_grad(xs, wts, ns, c, lb.p(), gp(G), S))
            _ok(L, L.ggan_mean_multi_fwd_grad(xs, wts, ns, c, la.p(), None, S))
        else:
            _ok(L, L.ggan_bce_logits_multi_fwd(xs, lab, wts, ns, c, la.p(), S))
            _ok(L, L.ggan_bce_logits_multi_fwd_grad(xs, lab, wts, ns, c, lb.p(), gp(G), S))
            _ok(L, L.ggan_bce_logits_multi_bwd(xs, lab, wts, ns, c, gl.p(), gp(G3), S))
        for k, ((n, z, w), o) in enumerate(zip(terms, offs)):           # one accumulating launch per term, the first onto NaN
            if mean:
                _ok(L, L.ggan_mean_fwd(X.p(o), w, lc.p(), n, int(k > 0), S))
            else:
                _ok(L, L.ggan_bce_logits_fwd(X.p(o), z, w, lc.p(), n, int(k > 0), S))

    def collect():
        if mean:
            return dict(loss_fg=_f1(lb), loss_null=_f1(la), loss_terms=_f1(lc), gxs=G.get())
        return dict(loss_fwd=_f1(la), loss_fg=_f1(lb), loss_terms=_f1(lc), gxs=G.get(), gxs3=G3.get())
    return run, collect


def _run_heads(row, inp, B, L, S):
    terms = D.all_terms(row)
    X, xs, lab, wts, ns, c, offs = _table(B, terms, inp['xs'])
    G, G2, loss, loss2 = B.out(X.n), B.out(X.n), B.out(1), B.out(1)
    gp = lambda g: D._ptrs([g.p(o) for o in offs])
    heads = row['heads']
    assert all(sum(t) == M <= D.HEAD_MAX_ROWS for M, _, t in heads) and len(heads) <= D.BCE_HEADS          # (bounds, before anything runs)
    hs, ws = [B.inp(h) for h in inp['h']], [B.inp(w) for w in inp['w_out']]
    ghs, dws, dbs = [B.out(M * H) for M, H, _ in heads], [B.out(H) for _, H, _ in heads], [B.out(1) for _ in heads]
    tab = lambda bs: D._ptrs([b.p() for b in bs])

    def run():
        _ok(L, L.ggan_bce_heads_bwd(xs, lab, wts, ns, c, loss.p(), gp(G), len(heads), D._ints([len(t) for _, _, t in heads]),
                                    D._ints([M for M, _, _ in heads]), D._ints([H for _, H, _ in heads]), tab(hs), tab(ws),
                                    D._floats([row['alpha']] * len(heads)), tab(ghs), tab(dws) if row['dw'] else None,
                                    tab(dbs) if row['db'] else None, S))
        _ok(L, L.ggan_bce_logits_multi_fwd_grad(xs, lab, wts, ns, c, loss2.p(), gp(G2), S))

    def collect():
        untouched = lambda bs: all(np.all(np.isnan(b.get())) for b in bs)
        assert row['dw'] or untouched(dws), 'd_wouts was NULL'
        assert row['db'] or untouched(dbs), 'd_bouts was NULL'
        return dict(loss=_f1(loss), loss_fg=_f1(loss2), gxs=G.get(), gxs_fg=G2.get(), gh=[g.get((M, H)) for g, (M, H, _) in zip(ghs, heads)],
                    dw=[b.get() if row['dw'] else None for b in dws], db=[_f1(b) if row['db'] else None for b in dbs])
    return run, collect


def _run_dist(row, inp, B, L, S):
    n = row['n']
    x, y, go = B.inp(inp['x']), B.inp(inp['y']), B.inp([row['gout']])
    out = B.out(1, row['prior'] if row['acc'] else np.nan)
    gx, gy = B.out(n) if row['gx'] else None, B.out(n) if row['gy'] else None

    def run():
        _ok(L, L.ggan_dist_fwd(x.p(), y.p(), out.p(), n, row['p'], row['w'], row['acc'], S))
        _ok(L, L.ggan_dist_bwd(x.p(), y.p(), go.p(), gx.p() if gx else None, gy.p() if gy else None, n, row['p'], row['w'], S))
    return run, lambda: dict(out=_f1(out), gx=gx.get() if gx else None, gy=gy.get() if gy else None)


def _run_gp(row, inp, B, L, S):
    Bn, Dn, lam = row['B'], row['D'], row['lam']
    g, one, gpen = B.inp(inp['g']), B.inp([1.0]), B.inp([row['gpen']])
    arrive = B.inp([0], dtype=np.int32)
    sl, pen = B.out(Bn), B.out(1)
    twice = [(B.out(Bn), B.out(1), B.out(Bn * Dn)) for _ in range(2)]
    gg1, gg = B.out(Bn * Dn), B.out(Bn * Dn)
    counter = []

    def run():
        import torch
        _ok(L, L.ggan_gp_penalty_fwd(g.p(), sl.p(), pen.p(), Bn, Dn, lam, S))
        for s2, p2, u2 in twice:
            _ok(L, L.ggan_gp_penalty_fwd_grad(g.p(), s2.p(), p2.p(), u2.p(), arrive.p(), Bn, Dn, lam, S))
            torch.cuda.synchronize()
            counter.append(int(arrive.get()[0]))
        _ok(L, L.ggan_gp_penalty_bwd(g.p(), sl.p(), one.p(), gg1.p(), Bn, Dn, lam, S))
        _ok(L, L.ggan_gp_penalty_bwd(g.p(), sl.p(), gpen.p(), gg.p(), Bn, Dn, lam, S))
    sh = (Bn, Dn)
    return run, lambda: dict(slopes=sl.get(), pen=_f1(pen), slopes2=twice[0][0].get(), pen2=_f1(twice[0][1]), gg_unit=twice[0][2].get(sh),
                             slopes3=twice[1][0].get(), pen3=_f1(twice[1][1]), gg_unit3=twice[1][2].get(sh), gg1=gg1.get(sh), gg=gg.get(sh),
                             arrive=counter)


def _run_mmd(row, inp, B, L, S):
    m, n, d, ns = row['m'], row['n'], row['d'], row['ns']
    assert m + n <= D.MMD_MAX_ROWS and ns <= D.MMD_MAX_SIGMAS
    X, Y, go = B.inp(inp['X']), B.inp(inp['Y']), B.inp([row['gout']])
    sig, wts = D._floats(list(inp['sigmas'])), D._floats(list(inp['wts'])) if inp['wts'] is not None else None      # host arrays
    out, rows = B.out(1), B.out(m + n)
    dX, dY = B.out(m * d) if row['dX'] else None, B.out(n * d) if row['dY'] else None
    u = '_unbiased' if row['unbiased'] else ''

    def run():
        _ok(L, getattr(L, 'ggan_mix_rbf_mmd2%s_fwd' % u)(X.p(), Y.p(), m, n, d, sig, wts, ns, out.p(), rows.p(), S))
        _ok(L, getattr(L, 'ggan_mix_rbf_mmd2%s_bwd' % u)(X.p(), Y.p(), m, n, d, sig, wts, ns, go.p(), dX.p() if dX else None, dY.p() if dY else None, S))
    return run, lambda: dict(rows=rows.get(), out=_f1(out), dX=dX.get((m, d)) if dX else None, dY=dY.get((n, d)) if dY else None)


def _run_agg(row, inp, B, L, S):
    kind, nx, nz, d, nc = row['kind'], row['nx'], row['nz'], row['d'], row['n_coms']
    assert nx <= D.AGG_MAX and d <= D.AGG_MAX
    ns = 2 * nz if kind == 2 else nz
    mu, sd, go = B.inp(inp['mu']), B.inp(inp['sd']), B.inp([1.0])
    k, eps = (B.inp(inp['k']), B.inp(inp['eps'])) if kind != 1 else (None, None)          # (what a kind does not read is NULL)
    zp = B.inp(inp['zp']) if kind != 0 else None
    p = lambda b: b.p() if b else None
    out, Z, A, Bv, T = B.out(1), B.out(ns * d), B.out(ns * nx), B.out(ns), B.out(ns)
    W, GZ, gmu, gsd = B.out(ns * nx), B.out(ns * d), B.out(nx * d), B.out(nx * d)

    def run():
        _ok(L, L.ggan_agg_div_fwd(kind, mu.p(), sd.p(), p(k), p(eps), p(zp), nx, nz, d, nc, out.p(), Z.p(), A.p(), Bv.p(), T.p(), S))
        _ok(L, L.ggan_agg_div_bwd(kind, mu.p(), sd.p(), p(k), p(eps), nx, nz, d, nc, Z.p(), A.p(), Bv.p(), go.p(), W.p(), GZ.p(), gmu.p(), gsd.p(), S))
    return run, lambda: dict(out=_f1(out), Z=Z.get((ns, d)), A=A.get((ns, nx)), Bv=Bv.get(), T=T.get(), W=W.get((ns, nx)), GZ=GZ.get((ns, d)),
                             gmu=gmu.get((nx, d)), gsd=gsd.get((nx, d)))


_RUN = dict(single=_run_single, table=_run_table, heads=_run_heads, dist=_run_dist, gp=_run_gp, mmd=_run_mmd, agg=_run_agg)


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_takes_its_path_and_matches_float64(gpu, idx):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    row = ROWS[idx]
    inp = D.inputs(row, 7000 + idx)
    B = Bufs(gpu)
    run, collect = _RUN[row['entry']](row, inp, B, L, F._stream())
    _, recs = _profiled(run)
    _check_launches(row, recs)
    out = collect()
    assert B.intact(), 'an input or a sentinel pad changed'
    fr, broken = D.check(row, inp, out)
    kernels = D.kernels_of(row)
    for key in sorted(fr):
        print('COSTFRAC %s %s %s %.4f' % (row_id(row), kernels[key], key, fr[key]))
    assert not broken and D.within(fr), (fr, broken)


class DeviceAlloc(D.Alloc):
    def __init__(self, gpu):
        D.Alloc.__init__(self)
        self.gpu = gpu

    def make(self, n):
        import torch
        t = torch.full((n,), float('nan'), dtype=torch.float32, device=self.gpu)
        return t, t.data_ptr()

    def read(self, handle):
        return handle.cpu().numpy()


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
