"""What each dispatch test of the transition-operator scan (csrc/dynscan.hip: dyn_scan_fwd_k, dyn_scan_bwd_k) runs: one row per shape
and edge (plain data), the rows' inputs, `planned()`, `run32` -- both kernels restated in float32 numpy in their own order -- and
`check()`, the float64 restatement of every stage of every step with its derived bound.

tests/test_scan_dispatch_gpu.py runs every row through the C ABI between ggan_prof_reset / ggan_prof_enable: ggan_dyn_scan_fwd, then
ggan_dyn_scan_bwd on the forward's own zs, h1, h2; the profiler must have seen exactly the row's launches; every operand sits between
sentinels (w_in and w_1, which the backward reads as float4, on 16-byte boundaries, everything else one float off) and every output
starts as NaN.  tests/test_scan_dispatch_cpu.py holds labels and constants against the source, hands run32's outputs to check() and
requires every wrong kernel of MUTANTS to miss on the row MUTANT_ROW names.

A row: B, T, dl, dt, mode ('res' | 'res_w'), null (d_z0 and d_eps are NULL), bwd_only (no forward launch: zs, h1, h2 are inputs, and a
tenth of h1 / h2 is exactly +0 or -0 -- the backward's mask `h > 0 ? 1 : alpha` must take alpha there), launches, note.

A norm over a whole sequence hides one wrong element and an error a later step damps, so every stage of every step is measured on
its own, element by element, against float64 from the float32 values that stage itself read -- the DEVICE's previous stage -- and no
element is left out: lrelu is 1-Lipschitz, so an error in front of a kink is no larger behind it, and the backward's masks come from
the device's own h1 / h2, which the forward stored.  u = 2^-24; a bound is (roundings on the longest chain) u sum|terms| + TINY:
  h1[t]     from zs[:, t] and eps: din fmaf onto b_in, then fl(alpha v): din u (|b_in| + sum|in w_in|) + u |h1|
  h2[t]     from h1[t]: 8 chains of 32 fmaf, a tree of 3, + b_1: 36 u (sum|h1 w_1| + |b_1|) + u |h2|
  zs[t+1]   from h2[t] and zs[:, t]: the products, wave_sum's 6, the 4-way combine's 2, + b_out: 10 u (sum|h2 w_out| + |b_out|);
            'res': + z, one more rounding; 'res_w': dl fmaf onto b_zw and the final sum: dl u (|b_zw| + sum|z zw|) + u |z'|
  zs[:, 0]  bitwise z0.   Go[T-1] bitwise g_zs[:, T].   Xin[t] bitwise [zs_t | eps].
  G2[t]     from Go[t] and the sign of h2: dl fmaf and the mask: (dl + 1) u |mask| sum|go w_out|
  G1[t]     from G2[t] and h1: 4 products / fmaf per lane, wave_sum's 6, the mask: 11 u |mask| sum|G2 w_1|
  Go[t-1]   from G1[t] and Go[t]: the input path (10 roundings), 'res' + go + g_zs (2 more), 'res_w' dl fmaf of go zw onto it and
            + g_zs (dl + 1 more), on the magnitudes of all parts.   d_z0: the same rule at t = 0.
  d_eps     the sum over t of the eps part of the input gradients, each recomputed from the device's G1[t]: (10 + T) u sum|G1 w_in|.

Worst observed fraction of the bound per stage, MI355X, 2026-10-21 (test_scan_dispatch_gpu.py prints every row's; above 1 fails):
  dyn_scan_fwd_k   h1 0.43   h2 0.03   zs 0.09
  dyn_scan_bwd_k   G2 0.76   G1 0.07   Go 0.06   d_z0 0.05   d_eps 0.03      (zs[0], Go[T-1], Xin: bitwise)"""
import numpy as np

H = 256
MAXD = 16
K_THREADS = 256
U = 2.0 ** -24
TINY = 2.0 ** -126
ALPHA = 0.2
PAD = 8
SENTINEL = np.float32(-12345.678)
f32 = np.float32
SCALES = dict(w_in=0.3, b_in=0.1, w_1=0.08, b_1=0.1, w_out=0.08, b_out=0.1, zw=0.3, b_zw=0.1)          # test_dyn_scan's


def planned(row):
    fwd = () if row['bwd_only'] else (('dyn_scan_fwd_k', 1, (row['B'],), (K_THREADS,)),)
    return fwd + (('dyn_scan_bwd_k', 1, (row['B'],), (K_THREADS,)),)


def threads(launch):
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


ROWS = []


def _row(B, T, dl, dt, mode, note, null=False, bwd_only=False):
    r = dict(B=B, T=T, dl=dl, dt=dt, mode=mode, null=null, bwd_only=bwd_only, note=note)
    r['launches'] = planned(r)
    ROWS.append(r)


_row(1, 1, 1, 1, 'res', 'width 1, T = 1, one sequence')
_row(3, 2, 16, 16, 'res', 'dl = dt = MAXD: in_s, red, wout, go_s, gin_s filled exactly')
_row(3, 2, 16, 16, 'res_w', 'dl = dt = MAXD with the zw chain')
_row(2, 3, 16, 1, 'res', 'dl = 16, dt = 1', null=True)
_row(2, 3, 1, 16, 'res_w', 'dl = 1, dt = 16: zw is 1 x 1')
_row(5, 4, 8, 8, 'res_w', 'the scripts\' widths', null=True)
_row(3, 30, 8, 8, 'res', 'a 30-step recurrence, every step measured on its own')
_row(33, 2, 4, 6, 'res_w', 'B = 33, din = 10: a ragged last trip of the w_in rows over the four waves')
_row(4, 3, 6, 4, 'res', 'backward alone on given h1 / h2, a tenth of them exactly +-0', bwd_only=True)
_row(4, 3, 6, 4, 'res_w', 'backward alone on given h1 / h2, a tenth of them exactly +-0', bwd_only=True)


def row_id(row):
    return 'B%d-T%d-dl%d-dt%d-%s%s%s' % (row['B'], row['T'], row['dl'], row['dt'], row['mode'], '-null' if row['null'] else '',
                                          '-bwd' if row['bwd_only'] else '')


def by_id(rid):
    hits = [r for r in ROWS if row_id(r) == rid]
    assert len(hits) == 1, rid
    return hits[0]


def shapes(row):
    """-> {name: shape} of every array of a row"""
    B, T, dl, dt = row['B'], row['T'], row['dl'], row['dt']
    return dict(z0=(B, dl), eps=(B, dt), w_in=(dl + dt, H), b_in=(H,), w_1=(H, H), b_1=(H,), w_out=(H, dl), b_out=(dl,), zw=(dl, dl), b_zw=(dl,),
                g_zs=(B, T + 1, dl), zs=(B, T + 1, dl), h1=(T, B, H), h2=(T, B, H), G1=(T, B, H), G2=(T, B, H), Go=(T, B, dl),
                Xin=(T, B, dl + dt), d_z0=(B, dl), d_eps=(B, dt))


INPUTS = ('z0', 'eps', 'w_in', 'b_in', 'w_1', 'b_1', 'w_out', 'b_out', 'zw', 'b_zw', 'g_zs')
FWD_OUT = ('zs', 'h1', 'h2')
BWD_OUT = ('G1', 'G2', 'Go', 'Xin', 'd_z0', 'd_eps')
ALIGNED = ('w_in', 'w_1')               # read as float4 by the backward: 16-byte boundaries; everything else sits one float off


def offset(name):
    return 0 if name in ALIGNED else 1


def inputs(row, seed):
    rng = np.random.default_rng(seed)
    sh = shapes(row)
    mk = lambda name, sc=1.0: (sc * rng.standard_normal(sh[name])).astype(np.float32)
    d = dict(z0=mk('z0'), eps=mk('eps'), g_zs=mk('g_zs'))
    for k, sc in SCALES.items():
        d[k] = mk(k, sc)
    if row['mode'] == 'res':
        d['zw'] = d['b_zw'] = None
    if row['bwd_only']:
        d['zs'] = mk('zs')
        for k in ('h1', 'h2'):
            h = mk(k)
            z = rng.random(h.shape) < 0.1
            h[z] = np.where(rng.random(int(z.sum())) < 0.5, f32(0.0), f32(-0.0))
            d[k] = h
    return d


# ---- the two kernels in float32 numpy, in their own order -----------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf: the product is exact in float64; one rounding to float64 in front of the one to float32 (a stand-in, not held bitwise)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def lrelu32(v):
    return np.maximum(f32(ALPHA) * v, v)


def wave_sum32(v):
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def fwd32(row, d, mutant=None):
    B, T, dl, dt = row['B'], row['T'], row['dl'], row['dt']
    din = dl + dt
    zs = np.full((B, T + 1, dl), np.nan, np.float32)
    h1s, h2s = np.full((T, B, H), np.nan, np.float32), np.full((T, B, H), np.nan, np.float32)
    z = d['z0'].copy()
    zs[:, 0] = z
    wout = d['w_out'].copy()
    if mutant == 'width_16_truncated_to_15':
        wout[:, 15:] = 0
    zw = d['zw'].T if (mutant == 'zw_transposed_fwd' and d['zw'] is not None) else d['zw']
    for t in range(T):
        x = np.concatenate([z, d['eps']], 1)
        if mutant == 'eps_from_offset_0':
            x = np.concatenate([z, np.resize(z, (B, dt)) if dl >= dt else np.concatenate([z, np.zeros((B, dt - dl), np.float32)], 1)], 1)
        a = np.broadcast_to(d['b_in'], (B, H)).astype(np.float32)
        for i in range(din):
            a = fma32(x[:, i:i + 1], d['w_in'][i][None, :], a)
        h1 = lrelu32(a)
        h1s[t] = h1
        s = np.zeros((B, 8, H), np.float32)
        for k in range(0, H, 8):
            s = fma32(h1[:, k:k + 8, None], d['w_1'][None, k:k + 8, :], s)
        c = ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])) + ((s[:, 4] + s[:, 5]) + (s[:, 6] + s[:, 7])) + d['b_1']
        h2 = lrelu32(c)
        h2s[t] = h2
        prod = h2[:, :, None] * wout[None]                                  # [B, H, dl]
        w = wave_sum32(prod.transpose(0, 2, 1).reshape(B, dl, 4, 64))      # [B, dl, 4]
        o = ((w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])) + d['b_out']
        if zw is not None:
            r = np.broadcast_to(d['b_zw'], (B, dl)).astype(np.float32)
            for i in range(dl):
                r = fma32(z[:, i:i + 1], zw[i][None, :], r)
            zn = o + r
        else:
            zn = o if mutant == 'residual_dropped' else o + z
        zs[:, t + 1] = zn
        z = zn
    return dict(zs=zs, h1=h1s, h2=h2s)


def _rows_dot32(g, W):
    """sum_n g[b, n] W[k, n] as the backward forms it: lane l holds n = 4l .. 4l + 3, fmaf(x, fmaf(y, fmaf(z, w))) then the butterfly"""
    B = g.shape[0]
    gq = g.reshape(B, 1, 64, 4)
    wq = W.reshape(1, W.shape[0], 64, 4)
    v = fma32(gq[..., 0], wq[..., 0], fma32(gq[..., 1], wq[..., 1], fma32(gq[..., 2], wq[..., 2], gq[..., 3] * wq[..., 3])))
    return wave_sum32(v)                                                     # [B, rows of W]


def bwd32(row, d, f, mutant=None):
    """f: zs, h1, h2 (the forward's outputs, or the row's inputs)"""
    B, T, dl, dt = row['B'], row['T'], row['dl'], row['dt']
    din = dl + dt
    a = f32(ALPHA)
    G1, G2 = np.full((T, B, H), np.nan, np.float32), np.full((T, B, H), np.nan, np.float32)
    Go, Xin = np.full((T, B, dl), np.nan, np.float32), np.full((T, B, din), np.nan, np.float32)
    go = d['g_zs'][:, T].copy()
    deps = np.zeros((B, dt), np.float32)
    zw = d['zw'].T if (mutant == 'zw_transposed_bwd' and d['zw'] is not None) else d['zw']
    pos = (lambda h: h >= 0) if mutant == 'mask_ge' else (lambda h: h > 0)
    for t in range(T - 1, -1, -1):
        Go[t] = go
        Xin[t] = np.concatenate([f['zs'][:, t], d['eps']], 1)
        g2 = np.zeros((B, H), np.float32)
        for j in range(dl):
            g2 = fma32(go[:, j:j + 1], d['w_out'][None, :, j], g2)
        g2 = g2 * np.where(pos(f['h2'][t]), f32(1), a)
        G2[t] = g2
        g1 = _rows_dot32(g2, d['w_1']) * np.where(pos(f['h1'][t]), f32(1), a)
        G1[t] = g1
        gin = _rows_dot32(g1, d['w_in'])                                      # [B, din]
        gz = gin[:, :dl].copy()
        if zw is not None:
            for j in range(dl):
                gz = fma32(go[:, j:j + 1], zw[None, :, j], gz)
        else:
            gz = gz + go
        if mutant != 'g_zs_not_added':
            gz = gz + d['g_zs'][:, t]
        deps = gin[:, dl:].copy() if mutant == 'd_eps_last_step_only' else deps + gin[:, dl:]
        go = gz
    return dict(G1=G1, G2=G2, Go=Go, Xin=Xin, d_z0=go, d_eps=deps)


def run32(row, d, mutant=None):
    f = {k: d[k] for k in FWD_OUT} if row['bwd_only'] else fwd32(row, d, mutant)
    out = dict(f) if not row['bwd_only'] else {}
    out.update(bwd32(row, d, f, mutant))
    if row['null']:
        del out['d_z0'], out['d_eps']
    return out


# ---- float64 restatement, stage by stage -----------------------------------------------------------------------------------------------------
def d64(a):
    return np.asarray(a, np.float64)


def _frac(err, bound):
    err, bound = np.atleast_1d(d64(err)), np.atleast_1d(d64(bound))
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    f = np.where(np.isfinite(err) & np.isfinite(bound), f, np.inf)
    return float(np.max(f))


def _bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return 0.0 if got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)) else np.inf


def within(fr):
    return all(f <= 1.0 for f in fr.values())


def _lrelu64(v):
    return np.maximum(float(f32(ALPHA)) * v, v)


def check(row, d, out):
    """-> {stage: worst fraction of its bound over all steps and elements} (a broken bitwise stage: inf)"""
    B, T, dl, dt = row['B'], row['T'], row['dl'], row['dt']
    din = dl + dt
    a = float(f32(ALPHA))
    fr = {}
    up = lambda key, v: fr.__setitem__(key, max(fr.get(key, 0.0), v))
    W = {k: (d64(d[k]) if d[k] is not None else None) for k in SCALES}
    eps = d64(d['eps'])
    f = {k: (d[k] if row['bwd_only'] else out[k]) for k in FWD_OUT}
    zs, h1, h2 = (d64(f[k]) for k in FWD_OUT)
    if not row['bwd_only']:
        fr['zs[0]=z0'] = _bits(out['zs'][:, 0], d['z0'])
        for t in range(T):
            x = np.concatenate([zs[:, t], eps], 1)
            pre = x @ W['w_in'] + W['b_in']
            mag = np.abs(x) @ np.abs(W['w_in']) + np.abs(W['b_in'])
            ref = _lrelu64(pre)
            up('h1', _frac(np.abs(h1[t] - ref), din * U * mag + U * np.abs(ref) + TINY))
            pre = h1[t] @ W['w_1'] + W['b_1']
            mag = np.abs(h1[t]) @ np.abs(W['w_1']) + np.abs(W['b_1'])
            ref = _lrelu64(pre)
            up('h2', _frac(np.abs(h2[t] - ref), 36 * U * mag + U * np.abs(ref) + TINY))
            o = h2[t] @ W['w_out'] + W['b_out']
            bo = 10 * U * (np.abs(h2[t]) @ np.abs(W['w_out']) + np.abs(W['b_out']))
            if row['mode'] == 'res_w':
                r = zs[:, t] @ W['zw'] + W['b_zw']
                br = dl * U * (np.abs(zs[:, t]) @ np.abs(W['zw']) + np.abs(W['b_zw']))
                ref, bound = o + r, bo + br + U * np.abs(o + r)
            else:
                ref, bound = o + zs[:, t], bo + U * np.abs(o + zs[:, t])
            up('zs', _frac(np.abs(zs[:, t + 1] - ref), bound + TINY))
    G1, G2, Go = d64(out['G1']), d64(out['G2']), d64(out['Go'])
    g_zs = d64(d['g_zs'])
    fr['Go[T-1]=g_zs[T]'] = _bits(out['Go'][T - 1], d['g_zs'][:, T])
    deps, bdeps = np.zeros((B, dt)), np.zeros((B, dt))
    for t in range(T - 1, -1, -1):
        up('Xin', _bits(out['Xin'][t], np.concatenate([f['zs'][:, t], d['eps']], 1)))
        m2 = np.where(np.asarray(f['h2'][t]) > 0, 1.0, a)
        m1 = np.where(np.asarray(f['h1'][t]) > 0, 1.0, a)
        ref = m2 * (Go[t] @ W['w_out'].T)
        up('G2', _frac(np.abs(G2[t] - ref), (dl + 1) * U * m2 * (np.abs(Go[t]) @ np.abs(W['w_out']).T) + TINY))
        ref = m1 * (G2[t] @ W['w_1'].T)
        up('G1', _frac(np.abs(G1[t] - ref), 11 * U * m1 * (np.abs(G2[t]) @ np.abs(W['w_1']).T) + TINY))
        gin = G1[t] @ W['w_in'].T                                            # [B, din]
        mgin = np.abs(G1[t]) @ np.abs(W['w_in']).T
        if row['mode'] == 'res_w':
            ref = gin[:, :dl] + Go[t] @ W['zw'].T + g_zs[:, t]
            bound = (10 + dl + 1) * U * (mgin[:, :dl] + np.abs(Go[t]) @ np.abs(W['zw']).T + np.abs(g_zs[:, t]))
        else:
            ref = gin[:, :dl] + Go[t] + g_zs[:, t]
            bound = (10 + 2) * U * (mgin[:, :dl] + np.abs(Go[t]) + np.abs(g_zs[:, t]))
        if t > 0:
            up('Go', _frac(np.abs(Go[t - 1] - ref), bound + TINY))
        elif not row['null']:
            fr['d_z0'] = _frac(np.abs(d64(out['d_z0']) - ref), bound + TINY)
        deps += gin[:, dl:]
        bdeps += mgin[:, dl:]
    if not row['null']:
        fr['d_eps'] = _frac(np.abs(d64(out['d_eps']) - deps), (10 + T) * U * bdeps + TINY)
    else:
        fr['null'] = 0.0 if 'd_z0' not in out and 'd_eps' not in out else np.inf
    return fr


# ---- wrong kernels (test_scan_dispatch_cpu.py) ---------------------------------------------------------------------------------------------------
MUTANT_ROW = {
    'eps_from_offset_0': 'B5-T4-dl8-dt8-res_w-null',
    'residual_dropped': 'B3-T30-dl8-dt8-res',
    'zw_transposed_fwd': 'B5-T4-dl8-dt8-res_w-null',
    'zw_transposed_bwd': 'B33-T2-dl4-dt6-res_w',
    'mask_ge': 'B4-T3-dl6-dt4-res-bwd',
    'd_eps_last_step_only': 'B3-T30-dl8-dt8-res',
    'g_zs_not_added': 'B3-T2-dl16-dt16-res',
    'width_16_truncated_to_15': 'B3-T2-dl16-dt16-res',
}
MUTANTS = tuple(MUTANT_ROW)

# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
# ggan_dyn_scan_fwd(B, T, dl, dt, Hdim, z0, eps, w_in, b_in, w_1, b_1, w_out, b_out, zw, b_zw, alpha, zs, h1, h2, stream)
# ggan_dyn_scan_bwd(B, T, dl, dt, Hdim, g_zs, zs, eps, h1, h2, w_in, w_1, w_out, zw, alpha, G1, G2, Go, Xin, d_z0, d_eps, stream)
_FWD = [2, 3, 8, 8, H] + ['p%d' % k for k in range(8)] + [None, None, ALPHA, 'p8', 'p9', 'p10']
_BWD = [2, 3, 8, 8, H] + ['p%d' % k for k in range(8)] + [None, ALPHA, 'p8', 'p9', 'p10', 'p11', None, None]


def _with(base, **at):
    a = list(base)
    for k, v in at.items():
        a[int(k[1:])] = v
    return tuple(a)


REJECTED = ([('ggan_dyn_scan_fwd', _with(_FWD, **kw), word) for kw, word in (
                (dict(a2=17), 'unsupported shape'), (dict(a3=0), 'unsupported shape'), (dict(a4=128), 'unsupported shape'), (dict(a3=17), 'unsupported shape'),
                (dict(a2=0), 'unsupported shape'), (dict(a0=0), 'unsupported shape'), (dict(a1=0), 'unsupported shape'),
                (dict(a13='p11'), 'zw and b_zw go together'), (dict(a14='p11'), 'zw and b_zw go together'), (dict(a5=None), 'null pointer'),
                (dict(a16=None), 'null pointer'))] +
            [('ggan_dyn_scan_bwd', _with(_BWD, **kw), word) for kw, word in (
                (dict(a2=17), 'unsupported shape'), (dict(a3=0), 'unsupported shape'), (dict(a4=128), 'unsupported shape'),
                (dict(a11=('p6', 4)), '16-byte aligned'), (dict(a10=('p5', 4)), '16-byte aligned'), (dict(a11=('p6', 8)), '16-byte aligned'),
                (dict(a5=None), 'null pointer'), (dict(a18=None), 'null pointer'))])
ACCEPTED_SHAPES = ((1, 1), (16, 16), (16, 1), (1, 16))          # (dl, dt) the guards let through: the rows hold each


def call(L, case, pointer):
    import ctypes as C
    fn, args = case[0], case[1]
    real = []
    for a in args:
        if isinstance(a, str):
            real.append(C.c_void_p(pointer(int(a[1:]))))
        elif isinstance(a, tuple):
            real.append(C.c_void_p(pointer(int(a[0][1:])) + a[1]))
        else:
            real.append(a)
    rc = getattr(L, fn)(*real, None)
    return rc, (L.ggan_last_error() or b'').decode()
