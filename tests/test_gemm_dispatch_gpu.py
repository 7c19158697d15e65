"""-m gpu: every kernel instance of the GEMM family (csrc/gemm.hip), by name and by the variant the name hides.  For each row of
tests/_gemm_dispatch.py the C entry point runs under the row's environment between ggan_prof_reset / ggan_prof_enable; the profiler
must have seen exactly the row's kernel (and the helpers the row lists), once, with the row's grid; the GGAN_TRACE_GEMM line of the
launch -- waves, operand path, loads in flight, split count, k per split, grid -- must equal the row's recorded plan; and every output
must match a float64 numpy reference within TOL of its largest entry, the figure test_ops_gpu.py holds for these products.  Operands
sit in NaN-filled buffers (at the row's base offset) and outputs start as NaN, so a read outside an operand or an element no workgroup
stores shows.

BIG_ROWS reach the generic loader, which only an operand of 0x7FFFFFF0 bytes or more selects.  An fp32 sum over 10^7 terms holds no
tolerance, so those rows carry exactly representable data (entries -1, 0, 1; see _gemm_dispatch.py) and the device result must EQUAL
the reference.  The large operand is built on the device from a small block and per-copy multipliers and never leaves it."""
import ctypes as C
import re

import numpy as np
import pytest

import _gemm_dispatch as D
from _gemm_dispatch import ROWS, BIG_ROWS, row_id
from test_conv_dispatch_gpu import _profiled
from test_ops_gpu import TOL, _rel, _t

pytestmark = pytest.mark.gpu

ALPHA = 0.2
HEADS = ('critic_head_fwd', 'critic_head_fwd_bce', 'critic_head_bwd', 'critic_head_bwd_tail')
_LINE = re.compile(r'\[ggan\] gemm (?!tail )(.+?) waves=(-?\d+) fast=(-?\d+) ns=(\d+) SK=(\d+) kps=(\d+) vecA=(\d) vecA2=(\d) vecB=(\d) a2=(\d) c2=(\d) '
                   r'colsum=(\d) grid=\((\d+),(\d+),(\d+)\)(?: wgs=\[(\d+),(\d+)\))?')
_TAIL = re.compile(r'\[ggan\] gemm tail (\S+) wgs=\[(\d+),(\d+)\)')


def _lines(err):
    out = []
    for m in _LINE.findall(err):
        x = dict(name=m[0], waves=int(m[1]), fast=int(m[2]), ns=int(m[3]), SK=int(m[4]), kps=int(m[5]), vecA=int(m[6]), vecA2=int(m[7]),
                 vecB=int(m[8]), a2=int(m[9]), c2=int(m[10]), colsum=int(m[11]), grid=(int(m[12]), int(m[13]), int(m[14])))
        if m[15]:
            x['wgs'] = (int(m[15]), int(m[16]))
        out.append(x)
    return out, [(m[0], (int(m[1]), int(m[2]))) for m in _TAIL.findall(err)]


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else None)


def _host(values, ctype):
    arr = (ctype * len(values))(*values)
    return arr, C.cast(arr, C.c_void_p)


def _dev(a, gpu, off=0, band=0):
    """a float32 copy of `a` on the device, `off` floats into a NaN-filled buffer that ends 4 floats behind it; `band` (a multiple of
    4) more NaN floats on each side"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert band % 4 == 0
    buf = torch.full((band + off + a.size + 4 + band,), float('nan'), dtype=torch.float32, device=gpu)
    off += band
    view = buf[off:off + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view


def _out(shape, gpu):
    import torch
    return torch.full(shape, float('nan'), dtype=torch.float32, device=gpu)


def _slope(ref, mask):
    return np.where(ref > 0, 1.0, ALPHA if mask == 'lrelu' else 0.0)


def _act(v, act):
    return v if act == 'none' else np.maximum(ALPHA * v, v) if act == 'lrelu' else np.maximum(v, 0.0)


def _code(F, act):
    return {None: F.ACT_NONE, 'none': F.ACT_NONE, 'lrelu': F.ACT_LRELU, 'relu': F.ACT_RELU}[act]


def _continuous(rng, shape):
    """a mask's reference tensor: continuous, no exact zero, nothing within fp32 rounding of the kink"""
    r = rng.standard_normal(shape).astype(np.float32)
    r[np.abs(r) < 1e-3] = 0.5
    assert np.all(r != 0.0)
    return r


def _run_product(row, gpu, rng):
    """-> [(what, device result, float64 reference)] of a product row (gemm, gemm_split, gemm_colsum, the two masked gradients)"""
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    ta, tb, M, N, K = row['shape']
    oa, oa2, ob, oref = row['off']
    ws, st = F.workspace(gpu), F._stream()
    a_split, c_split, entry = row['a_split'], row['c_split'], row['entry']
    opA = rng.standard_normal((M, K)).astype(np.float32)
    opB = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32) if row['bias'] else None
    stA = opA.T if ta else opA                                   # as stored: [K, M] or [M, K]
    stB = opB.T if tb else opB
    A1, A2 = (stA[:, :a_split], stA[:, a_split:]) if a_split else (stA, None)
    tA, tA2, tB = _dev(A1, gpu, oa), (_dev(A2, gpu, oa2) if a_split else None), _dev(stB, gpu, ob)
    tbias = _dev(bias, gpu) if bias is not None else None
    a64, b64 = opA.astype(np.float64), opB.astype(np.float64)
    outs = []
    if entry == 'gemm':
        c = _out((M, N), gpu)
        rc = L.ggan_gemm(ta, tb, M, N, K, _p(tA), _p(tB), _p(tbias), _p(c), _code(F, row['act']), ALPHA, _p(ws), ws.numel(), st)
        outs = [('C', c, _act(a64 @ b64 + (bias if bias is not None else 0.0), row['act']))]
    elif entry == 'gemm_split':
        ref = _act(a64 @ b64 + (bias if bias is not None else 0.0), row['act'])
        c = _out((M, c_split or N), gpu)
        c2 = _out((M, N - c_split), gpu) if c_split else None
        cs = _out((N,), gpu) if row.get('colsum') else None
        rc = L.ggan_gemm_split(ta, tb, M, N, K, _p(tA), _p(tA2), a_split, _p(tB), _p(tbias), _p(c), _p(c2), c_split, _p(cs),
                               _code(F, row['act']), ALPHA, _p(ws), ws.numel(), st)
        outs = [('C', c, ref[:, :c_split] if c_split else ref)]
        if c_split:
            outs.append(('C2', c2, ref[:, c_split:]))
        if cs is not None:
            outs.append(('colsum', cs, b64.sum(0)))
    elif entry == 'gemm_colsum':
        c, cs = _out((M, N), gpu), _out((N,), gpu)
        rc = L.ggan_gemm_colsum(ta, M, N, K, _p(tA), _p(tB), _p(c), _p(cs), _p(ws), ws.numel(), st)
        outs = [('C', c, a64 @ b64), ('colsum', cs, b64.sum(0))]
    elif entry == 'linear_bwd_data_act':                         # dx[M, N] = (g * act'(y))[M, K] @ w[N, K]^T
        assert (ta, tb) == (0, 1)
        y = _continuous(rng, (M, K))
        dx = _out((M, N), gpu)
        rc = L.ggan_linear_bwd_data_act(M, K, N, _p(tA), _p(_dev(y, gpu, oref)), _code(F, row['mask']), ALPHA, _p(tB), _p(dx), _p(ws), ws.numel(), st)
        outs = [('dx', dx, (a64 * _slope(y, row['mask'])) @ b64)]
    else:                                                        # dw[M, N] = x[K, M]^T @ (g * act'(y))[K, N];  db = its column sums
        assert entry == 'linear_bwd_weight_act' and (ta, tb) == (1, 0)
        y = _continuous(rng, (K, N))
        dw, db = _out((M, N), gpu), _out((N,), gpu)
        rc = L.ggan_linear_bwd_weight_act(K, N, M, _p(tA), _p(tB), _p(_dev(y, gpu, oref)), _code(F, row['mask']), ALPHA, _p(dw), _p(db), _p(ws),
                                          ws.numel(), st)
        gm = b64 * _slope(y, row['mask'])
        outs = [('dw', dw, a64 @ gm), ('db', db, gm.sum(0))]
    assert rc == 0, rc
    return outs


def _bce_terms(terms, logits):
    cost, g, r0 = 0.0, np.zeros(len(logits)), 0
    for n, z, wt in terms:
        x = logits[r0:r0 + n]
        cost += wt * np.mean(np.maximum(x, 0) - x * z + np.log1p(np.exp(-np.abs(x))))
        g[r0:r0 + n] = wt / n * (1.0 / (1.0 + np.exp(-x)) - z)
        r0 += n
    return cost, g


def _run_head(row, gpu, rng):
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    M, K1, K2, H = row['shape']
    o1, o2, ow = row['off']
    ws, st = F.workspace(gpu), F._stream()
    entry = row['entry']
    a1 = rng.standard_normal((M, K1)).astype(np.float32)
    a2 = rng.standard_normal((M, K2)).astype(np.float32) if K2 else None
    w = (rng.standard_normal((K1 + K2, H)) / np.sqrt(K1 + K2)).astype(np.float32)
    b = (0.1 * rng.standard_normal(H)).astype(np.float32)
    wo = (rng.standard_normal(H) / np.sqrt(H) * 3).astype(np.float32)
    bo = rng.standard_normal(1).astype(np.float32)
    A = (np.concatenate([a1, a2], 1) if K2 else a1).astype(np.float64)
    w64, wo64 = w.astype(np.float64), wo.astype(np.float64)
    pre = A @ w64 + b
    assert np.abs(pre).min() > 1e-5                   # no pre-activation within fp32 rounding of the LeakyReLU kink
    h = np.maximum(ALPHA * pre, pre)
    logits = h @ wo64 + bo[0]
    ta1, ta2, tw = _dev(a1, gpu, o1), (_dev(a2, gpu, o2) if K2 else None), _dev(w, gpu, ow)
    tb_, two, tbo = _dev(b, gpu), _dev(wo, gpu), _dev(bo, gpu)
    terms = row.get('terms')
    if terms:
        rows_h, rows_p = _host([t[0] for t in terms], C.c_int)
        lab_h, lab_p = _host([t[1] for t in terms], C.c_float)
        wts_h, wts_p = _host([t[2] for t in terms], C.c_float)
    if entry == 'critic_head_fwd':
        th, tl = _out((M, H), gpu), _out((M,), gpu)
        rc = L.ggan_critic_head_fwd(M, K1, K2, H, _p(ta1), _p(ta2), _p(tw), _p(tb_), _p(two), _p(tbo), ALPHA, _p(th), _p(tl), _p(ws), ws.numel(), st)
        outs = [('h', th, h), ('logits', tl, logits)]
    elif entry == 'critic_head_fwd_bce':
        th, tl, tg, tgh = _out((M, H), gpu), _out((M,), gpu), _out((M,), gpu), _out((M, H), gpu)
        rc = L.ggan_critic_head_fwd_bce(M, K1, K2, H, _p(ta1), _p(ta2), _p(tw), _p(tb_), _p(two), _p(tbo), ALPHA, _p(th), _p(tl), 0, len(terms),
                                        rows_p, lab_p, wts_p, _p(tg), _p(tgh), _p(ws), ws.numel(), st)
        _, g = _bce_terms(terms, logits)
        outs = [('h', th, h), ('logits', tl, logits), ('g', tg, g), ('gh', tgh, g[:, None] * wo64[None, :] * np.where(pre > 0, 1.0, ALPHA))]
    else:
        all_ = row['need'] == 'all'
        h32 = h.astype(np.float32)
        g = (rng.standard_normal(M) + 1.0).astype(np.float32)            # (a sum well away from zero: d_bout is compared relatively)
        th, tg = _dev(h32, gpu), _dev(g, gpu)
        d_a1, d_a2 = _out((M, K1), gpu), (_out((M, K2), gpu) if K2 else None)
        d_w, d_b = (_out((K1 + K2, H), gpu), _out((H,), gpu)) if all_ else (None, None)
        d_wo, d_bo = (_out((H,), gpu), _out((1,), gpu)) if all_ else (None, None)
        if entry == 'critic_head_bwd':
            tgh = _out((M, H), gpu)
            rc = L.ggan_critic_head_bwd(M, K1, K2, H, _p(tg), _p(ta1), _p(ta2), _p(tw), _p(th), _p(two), ALPHA, _p(tgh), _p(d_a1), _p(d_a2), _p(d_w),
                                        _p(d_b), _p(d_wo), _p(d_bo), _p(ws), ws.numel(), st)
            gh = g.astype(np.float64)[:, None] * wo64[None, :] * np.where(h32 > 0, 1.0, ALPHA)
            outs = [('gh', tgh, gh)]
        else:
            gh32 = rng.standard_normal((M, H)).astype(np.float32)
            lg32 = rng.standard_normal(M).astype(np.float32)
            tgh, tlg, loss = _dev(gh32, gpu), _dev(lg32, gpu), _out((1,), gpu)
            rc = L.ggan_critic_head_bwd_tail(M, K1, K2, H, _p(ta1), _p(ta2), _p(tw), _p(th), _p(two), ALPHA, _p(tgh), _p(d_a1), _p(d_a2), _p(d_w),
                                             _p(d_b), _p(d_wo), _p(d_bo), _p(tlg), _p(tg), 0, len(terms), rows_p, lab_p, wts_p, C.c_void_p(None),
                                             _p(loss), _p(ws), ws.numel(), st)
            gh = gh32.astype(np.float64)
            outs = [('cost', loss, np.array([_bce_terms(terms, lg32.astype(np.float64))[0]]))]
        d_a = gh @ w64.T
        outs.append(('d_a1', d_a1, d_a[:, :K1]))
        if K2:
            outs.append(('d_a2', d_a2, d_a[:, K1:]))
        if all_:
            g64 = g.astype(np.float64)
            outs += [('d_w', d_w, A.T @ gh), ('d_b', d_b, gh.sum(0)), ('d_wout', d_wo, h32.astype(np.float64).T @ g64),
                     ('d_bout', d_bo, np.array([g64.sum()]))]
    assert rc == 0, rc
    return outs


def _check_dispatch(row, recs, err):
    names = sorted(set(r['name'] for r in recs))
    assert names == sorted(set((row['kernel'],) + tuple(row['also']))), (names, row)
    main = [r for r in recs if r['name'] == row['kernel']]
    assert len(main) == 1 and main[0]['launches'] == 1, main
    lines, tails = _lines(err)
    mine = [x for x in lines if x['name'] == row['kernel']]
    print('%s grid %d trace %r tails %r' % (row['kernel'], main[0]['grid'], mine, tails))
    assert len(mine) == len(row['expect']), (lines, row['expect'])
    for got, want in zip(mine, row['expect']):
        assert {k: got.get(k) for k in want} == want, (got, want)
    want_tails = ([(row['kernel'], row['tail'])] if row.get('tail') else []) + \
        ([('head_tail_k', (0, 2 + (row['shape'][3] - 1) // 16))] if 'head_tail_k' in row['also'] else [])
    assert tails == want_tails, (tails, want_tails)
    x = row['expect'][-1]
    wgs = row['tail'][1] if row.get('tail') else x['wgs'][1] if 'wgs' in x else x['grid'][0] * x['grid'][1] * x['grid'][2]
    assert main[0]['grid'] == wgs * 64 * x['waves'], (main[0]['grid'], wgs, x['waves'])
    # every line of the call names a kernel the row knows
    assert {x['name'] for x in lines} <= set((row['kernel'],) + tuple(row['also'])), lines


def _prepare(row, gpu, monkeypatch, capfd):
    from graphical_gan_amd import functional as F
    monkeypatch.delenv('GGAN_GEMM_SK', raising=False)
    for k, v in row['env'].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv('GGAN_TRACE_GEMM', '1')
    F.workspace(gpu)                     # (allocated and zeroed outside the profiled region)
    capfd.readouterr()


@pytest.mark.parametrize('idx', range(len(ROWS)), ids=[row_id(r) for r in ROWS])
def test_row_runs_its_kernel_and_matches_float64(gpu, idx, monkeypatch, capfd):
    row = ROWS[idx]
    _prepare(row, gpu, monkeypatch, capfd)
    rng = np.random.default_rng(2000 + idx)
    results, recs = _profiled(lambda: (_run_head if row['entry'] in HEADS else _run_product)(row, gpu, rng))
    err = capfd.readouterr().err
    _check_dispatch(row, recs, err)                                                    # (a)
    for what, got, ref in results:                                                     # (b)
        got = got.cpu().numpy()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        assert np.all(np.isfinite(got)), (what, 'elements nobody stored: %d' % int(np.isnan(got).sum()))
        e = _rel(got, ref)
        print('%s %s rel %.3e (tol %.0e)' % (row['kernel'], what, e, TOL))
        assert e < TOL, (what, e, TOL)


# ---- the generic loader --------------------------------------------------------------------------------------------------------------------
def _copies(gpu, mult, block, axis, out=None):
    """mult[r] * block for every copy r, side by side along `axis` of the stored matrix, written on the device into `out`"""
    import torch
    reps, (rows, cols) = len(mult), block.shape
    tb, tm = _t(block, gpu), _t(mult, gpu)
    if axis == 0:
        out = torch.empty((reps * rows, cols), dtype=torch.float32, device=gpu) if out is None else out
        torch.mul(tb.unsqueeze(0), tm.view(-1, 1, 1), out=out.view(reps, rows, cols))
    else:
        out = torch.empty((rows, reps * cols), dtype=torch.float32, device=gpu) if out is None else out
        torch.mul(tb.unsqueeze(1), tm.view(1, -1, 1), out=out.view(rows, reps, cols))
    return out


def _run_big(row, gpu, d):
    import torch
    from graphical_gan_amd import functional as F, _lib
    L = _lib.load()
    ta, tb, M, N, K = row['shape']
    ws, st = F.workspace(gpu), F._stream()
    code = _code(F, row['mask'])
    c, cs, tA2, tR = _out((M, N), gpu), None, None, None
    if row['along'] == 'M':
        ka = row['a_split'] or K
        buf = torch.empty(M * K, dtype=torch.float32, device=gpu)            # [A | second source]: the second starts M * ka floats on
        tA = _copies(gpu, d['mult'], d['blockA'], 0, out=buf[:M * ka].view(M, ka))
        if row['a_split']:
            tA2 = _copies(gpu, d['mult2'], d['block2'], 0, out=buf[M * ka:].view(M, K - ka))
            assert tA2.data_ptr() - tA.data_ptr() > 2 ** 31
        tB = _t(d['B'], gpu)
        if row['mask']:
            tR = _copies(gpu, d['multR'], d['blockR'], 0)
    elif row['along'] == 'K':
        tA = _copies(gpu, d['mult'], d['blockA'], 0)
        tB = _copies(gpu, d['multB'], d['blockB'], 1 if tb else 0)
        if row['mask']:
            tR = _copies(gpu, d['multR'], d['blockR'], 0)
    else:
        tA, tB = _t(d['A'], gpu), _copies(gpu, d['mult'], d['blockB'], 0)
    big = tA if row['big'] == 'A' else tB
    assert big.numel() * 4 >= 0x7FFFFFF0
    if row['entry'] == 'gemm':
        rc = L.ggan_gemm(ta, tb, M, N, K, _p(tA), _p(tB), _p(None), _p(c), F.ACT_NONE, 0.0, _p(ws), ws.numel(), st)
    elif row['entry'] == 'gemm_split':
        rc = L.ggan_gemm_split(ta, tb, M, N, K, _p(tA), _p(tA2), row['a_split'], _p(tB), _p(None), _p(c), _p(None), 0, _p(None), F.ACT_NONE, 0.0,
                               _p(ws), ws.numel(), st)
    elif row['entry'] == 'linear_bwd_data_act':
        rc = L.ggan_linear_bwd_data_act(M, K, N, _p(tA), _p(tR), code, D.BIG_ALPHA, _p(tB), _p(c), _p(ws), ws.numel(), st)
    else:
        cs = _out((N,), gpu)
        rc = L.ggan_linear_bwd_weight_act(K, N, M, _p(tA), _p(tB), _p(tR), code, D.BIG_ALPHA, _p(c), _p(cs), _p(ws), ws.numel(), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dict(C=c.cpu().numpy(), **({'colsum': cs.cpu().numpy()} if cs is not None else {}))


@pytest.mark.parametrize('idx', range(len(BIG_ROWS)), ids=[row_id(r) for r in BIG_ROWS])
def test_big_row_runs_the_generic_loader_and_is_exact(gpu, idx, monkeypatch, capfd):
    import torch
    row = BIG_ROWS[idx]
    free, _ = torch.cuda.mem_get_info(gpu)
    if free < 16 << 30:
        pytest.skip('needs 16 GiB of free device memory, %.1f free' % (free / 2.0 ** 30))
    _prepare(row, gpu, monkeypatch, capfd)
    d = D.big_operands(row, np.random.default_rng(3000 + idx))
    ref = D.big_reference(row, d)
    assert D.big_bound(row, d) < 2 ** 23 and all(np.abs(v).max() > 0 for v in ref.values())
    try:
        got, recs = _profiled(lambda: _run_big(row, gpu, d))
    finally:
        torch.cuda.empty_cache()
    # (the operand builders run inside the profiled region but are torch's own kernels: the profiler records the library's launches only)
    _check_dispatch(row, recs, capfd.readouterr().err)
    assert set(got) == set(ref)
    for what in ref:
        assert got[what].shape == ref[what].shape, (what, got[what].shape, ref[what].shape)
        bad = int((got[what].astype(np.float64) != ref[what]).sum())
        print('%s %s: %d of %d elements differ' % (row['kernel'], what, bad, ref[what].size))
        _rel(got[what], ref[what])                                                      # (0 in the report)
        assert bad == 0, (what, bad)
