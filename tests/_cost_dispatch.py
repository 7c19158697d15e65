"""Which path of the cost kernels (csrc/losses.hip, cost_head.h) each dispatch test runs: one row per scenario and edge (plain data), the
rows' inputs, a float32 restatement of every kernel in the kernel's summation order (run32: the CPU stand-in for the device), the float64
restatements and derived bounds every output is held to in stages (check), `planned()`, a transcription of each entry point's launch
list, and REJECTED, the calls that must be refused before any launch.

tests/test_cost_dispatch_gpu.py runs every row through the C ABI between sentinel pads, asserts that the profiler saw exactly the row's
launches (label, count, grid x block: all a record holds), and hands the outputs to check().  tests/test_cost_dispatch_cpu.py holds
labels, kernels and constants against the source text, recomputes every row's launches with planned(), asserts from the rows which edges
the table reaches, and proves that run32 passes every bound while each wrong kernel of MUTANTS misses one or breaks a bitwise stage.

A row: entry (below), its parameters, launches ((label, launches, grid, block, kernel), ...) and a note.  One row makes every call of
its scenario, so that the bitwise relations between entry points can be held:
  single  kind bce | mean; n, z, w, gloss, acc, prior: X_fwd (accumulate = acc: onto NaN when 0, onto `prior` when 1) and X_bwd
  table   kind bce | mean; terms ((n, z, w), ...): bce_logits_multi_fwd, _multi_fwd_grad, _multi_bwd (gloss 3) and one accumulating
          bce_logits_fwd per term; mean_multi_fwd_grad with gxs given and NULL and one accumulating mean_fwd per term.  The terms' logits
          and gradients lie back to back in one buffer, as BceSum lays them
  heads   heads ((M, H, (n, ...)), ...), dw, db (False: d_wouts / d_bouts NULL), alpha: bce_heads_bwd, and bce_logits_multi_fwd_grad on
          the same table
  dist    p, n, gx, gy (False: NULL), acc, prior, w, gout: dist_fwd, dist_bwd
  gp      B, D, lam, gpen: gp_penalty_fwd, gp_penalty_fwd_grad twice on one `arrive`, gp_penalty_bwd with gpen = 1 and with gpen
  mmd     m, n, d, ns, wts, dX, dY (False: NULL), unbiased, gout, variant normal | shared | far: mix_rbf_mmd2[_unbiased]_fwd, _bwd
  agg     kind, nx, nz, d, n_coms, wide: agg_div_fwd, agg_div_bwd

Inputs (inputs()), float32 on the host: BCE logits are a normal draw at scale 4 carrying +-0, +-1e-6, +-20, +-88, +-89, +-100, +-1e4;
a tenth of the head's h is exactly 0; a tenth of the distance pairs are bitwise equal; gp rows have norms from 1e-3 to 30 and one
one-hot row; the MMD sets are normal draws (shared: two rows of Y are two rows of X; far: Y is 200 away); agg as kl_aggregated.py
draws them (wide: std 50).

Stages and bounds (u = 2^-24; no stage carries another's error).  A float32 sum is held to k u sum|terms| with k the longest chain of
additions: chain(n, block) = ceil(n / block) of the thread loop + 6 of wave_sum + block / 64 of block_sum's serial loop.
  expf, log1pf, logf   P_EXP = 3, P_LOG1P = 2, P_LOG = 3 ulps (1 ulp = 2 u relative): the OpenCL conformance limits -- a condition, not
          a measurement, as P_POW in _optim_dispatch.  A value below 2^-126 may be flushed: TINY per such operation.
  bce value   max(v, 0) - v z + log1p(exp(-|v|)): u (|v z| + |a - b| + (2 P_EXP + 2 P_LOG1P) c + |value|); c inherits exp's relative error
          because e / (1 + e) <= log1p(e).
  cost    |w| / n (sum of the value bounds + chain u sum|values|) + 2 u |w mean| (the division and the product) [+ u |total| per
          accumulation or later term].
  bce grad    K_GRAD u |g|, g = gloss w / n in float64, K_GRAD = 2 P_EXP / 4 + 6 = 7.5: exp's error reaches the sigmoid scaled by
          s (1 - s) <= 1/4; 1 + e, the reciprocal, the subtraction of z, the product and the two roundings of g are one u each, all on
          values of size <= 1.  Absolute: the subtraction cancels for large |v|, which is the reference's own behaviour.
  mean grad   bitwise fl(fl(gloss w) / n).
  head    from the device's own gxs: gh 2 u |gh|; d_wout (ceil(M / 16) + 5) u sum|g h| (the fmaf chain of a row group, combine16's 4
          levels, one for an uncontracted product); d_bout (ceil(M / 16) + 4) u sum|g|.
  dist    value: 3 u d^2 (p = 2) or u |d| (p = 1) per element, chain(n, 1024), then as cost.  Gradient 4 u |v|; +-0 where x == y.
  gp      slopes from g: ((chain(D, 256) + 1) / 2 + 1) u slope.  pen from the device's slopes: lam / B (3 + chain(B, 256)) u sum (s - 1)^2
          + 2 u pen.  gg from the device's slopes: 6 u |gg|.
  mmd     row_scratch[r] from the inputs and the float32 gamma (formed on the host as 1.f / (2.f * s * s)): per pair
          |coef| sum_s wt_s e_s (|arg_s| (d + 4) + 2 P_EXP + ns + 4) u -- the distance chain of d fmaf's on differences of 2 u, the product
          with gamma, expf, the sum over sigmas, the coefficient -- plus chain(m + n, 256) u sum|coef k|.  Gradient rows: per j
          (the same for cf[j], + 2 for wt gamma and gout) on |cf_j (z_r - z_j)| plus (m + n + 2) u for the difference and the fmaf chain.
  agg     Z from the inputs: (nx + 1) u (sum|k mu| + sum|k sd| |eps|).  Bv from the device's Z: (chain(d, 128) + 2) / 2 u sum(z^2 + log 2pi).
          A from the device's Z: u / 2 sum_dd (5 r^2 + 4 P_LOG |log sd| + (d + 2)(r^2 + log 2pi + 2 |log sd|)).
          T and W from the device's A and Bv (the log-sum-exp stages).  Sq = sum_j exp(a_j - max) has the relative error
          rSq = u (sum_j e_j (|a_j - max| + 2 P_EXP) / Sq + chain(nx, 128)): the rounding of each argument moves its exponential by u |arg|.
          lq = max + logf(Sq) - logf(nx): rSq + u (2 P_LOG (|log Sq| + log nx) + |max + log Sq| + |lq|).  The mixture of jsd,
          M = Sq exp(mq - mm) + n_coms exp(b - mm): its two parts' relative errors weighted by their shares, + u; lm as lq.  T: the errors of
          what it subtracts (halved for jsd) + u |T|.  W: each responsibility e / S carries (|arg| + 2 P_EXP + 1) u + the sum's error, then
          3 u |W| for gout / nz, the product and the 0.5.
          GZ from the device's own W (the kernel reads back what it stored), A, Bv, Z: dL/db carries M's and pe's errors, then 4 u per
          term and a chain of nx + 1 subtractions on |v z| + sum|terms|.  gmu, gsd from the device's W, GZ, Z: (ns + nq + 5) u sum|terms|
          and (ns + nq + 9) u sum|terms| with the two parts of gsd's difference counted apart.
  TOL_LONG    no stage is held to it: every bound above is derived.
  products    where a bound is k roundings of one product (gh 2, the distance gradient 4, gg 6) it is Higham's gamma_k = k u / (1 - k u).
  bitwise mmd2_final and agg_div_final are the float32 sums in row order of the device's own partials; gp_penalty_fwd and _fwd_grad
          give the same slopes and pen, twice; gg_unit is gp_penalty_bwd with gpen = 1; the table's loss is the same from multi_fwd,
          multi_fwd_grad, heads_bwd and the accumulating launches, and so are the gxs.

Worst observed fraction of the bound per kernel, MI355X, 2026-10-20 (test_cost_dispatch_gpu.py prints every row's; above 1 fails):
  agg_div_bwd_comps_k      gmu 0.48   gsd 0.37
  agg_div_bwd_samples_k    GZ 0.34   W 0.51
  agg_div_fwd_k            A 0.49   Bv 0.15   T 0.30   Z 0.33
  bce_bwd_k                gx 0.24
  bce_fwd_k                loss 0.16
  bce_head_bwd_k           d_bout 0.08   d_wout 0.16   gh 0.87   gxs 0.22   loss 0.14
  bce_multi_bwd_k          gxs3 0.29
  bce_multi_fwd_k          gxs 0.30   loss 0.08
  dist_bwd_k               gx 0.55   gy 0.55
  dist_fwd_k               out 0.05
  gp_bwd_k                 gg 0.57   gg1 0.52
  gp_pen_k                 pen 0.07
  gp_slopes_k              slopes 0.22
  mean_bwd_k               gx 0.00
  mean_fwd_k               loss 0.03
  mean_multi_fwd_k         gxs 0.00   loss 0.01
  mmd2_bwd_k               dX 0.09   dY 0.08
  mmd2_rows_k              rows 0.06
  gp_fwd_grad_k, mmd2_final_k, agg_div_final_k: bitwise stages only (equal to gp_slopes_k / gp_pen_k / gp_bwd_k with gpen = 1; the float32 sums in row order)
mean_bwd_k and the mean table's gxs are bitwise too (0.00: equal); gh comes near its bound because it is two roundings held to gamma_2."""
import ctypes as C
import re

import numpy as np


# ---- constants the transcription copies (test_cost_dispatch_cpu.py holds them against the source text) --------------------------------
BCE_MAX = 16                   # GGAN_BCE_MAX
BCE_HEADS = 2                  # GGAN_BCE_HEADS
HEAD_MAX_ROWS = 2048           # GGAN_HEAD_BCE_MAX_ROWS
MMD_MAX_ROWS = 512
MMD_MAX_SIGMAS = 8             # kMmdMaxSigmas
AGG_MAX = 8192                 # d and nx of agg_div
K_BLOCK = 256
DIST_FWD_BLOCK = 1024
AGG_BLOCK = 128
FINAL_BLOCK = 64
GRID_CAP = 2048                # grid_for
HEAD_COLS = 16                 # columns per workgroup of head_columns

U = 2.0 ** -24
TINY = 2.0 ** -126
P_EXP, P_LOG1P, P_LOG = 3, 2, 3
K_GRAD = 2 * P_EXP / 4.0 + 6
LOG2PI32 = np.float32(1.8378770664093453)

PAD = 8
SENTINEL = np.float32(-12345.678)
EDGE_LOGITS = (0.0, -0.0, 1e-6, -1e-6, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0, 1e4, -1e4)
SIGMAS = {1: (2.0,), 6: (2.0, 5.0, 10.0, 20.0, 40.0, 80.0), 8: (1.0, 2.0, 5.0, 10.0, 20.0, 40.0, 80.0, 160.0)}
WTS = (1.0, 0.5, 2.0, 0.25, 1.5, 1.0, 0.75, 3.0)

f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def chain(n, block):
    return cdiv(n, block) + 6 + block // 64


def gam(k):
    """Higham's gamma_k: what k roundings in a row can do to a product, relative"""
    return k * U / (1.0 - k * U)


def grid_for(n):
    return min(max(cdiv(n, K_BLOCK * 4), 1), GRID_CAP)


# ---- rows ----------------------------------------------------------------------------------------------------------------------------------
def _row(entry, launches, note, **kw):
    return dict(entry=entry, launches=tuple(launches), note=note, **kw)


ROWS = []
# single terms: n at and around one trip of the 256-thread loop
for _i, (_n, _gx) in enumerate(((1, 1), (255, 1), (256, 1), (257, 2), (800, 4))):
    _kw = dict(n=_n, z=(1.0, 0.0, 0.9, 1.0, 0.0)[_i], w=(1.0, 0.5, 2.0, 1.0, 0.25)[_i], gloss=(1.0, 3.0, 0.5)[_i % 3], acc=_i % 2, prior=0.75)
    ROWS.append(_row('single', (('bce_logits_fwd', 1, (1,), (256,), 'bce_fwd_k'), ('bce_logits_bwd', 1, (_gx,), (256,), 'bce_bwd_k')),
                     'bce, one term of %d' % _n, kind='bce', **_kw))
    ROWS.append(_row('single', (('mean_fwd', 1, (1,), (256,), 'mean_fwd_k'), ('mean_bwd', 1, (_gx,), (256,), 'mean_bwd_k')),
                     'mean, one term of %d' % _n, kind='mean', **_kw))
# tables
_LENS, _LABELS, _WEIGHTS = (1, 7, 256, 257, 800), (1.0, 0.0, 0.9), (1.0, 0.5, 0.25)
_TABLES = [
    (((800, 1.0, 1.0),), 4, 'count 1'),
    (((1, 0.9, 0.5),), 1, 'count 1, one logit'),
    (((256, 1.0, 0.5), (257, 0.0, 0.5), (7, 0.9, 1.0)), 2, 'count 3'),
    (((7, 1.0, 1.0), (800, 0.0, 1.0), (1, 0.9, 2.0)), 4, 'count 3, the longest term in the middle: idle workgroups beside the short ones'),
    (tuple((_LENS[(3 * k) % 5], _LABELS[k % 3], _WEIGHTS[(k // 3) % 3]) for k in range(BCE_MAX)), 4, 'count 16 = GGAN_BCE_MAX, lengths mixed'),
]
for _terms, _gx, _note in _TABLES:
    _c = len(_terms)
    ROWS.append(_row('table', (('bce_logits_fwd', 1 + _c, (1,), (256,), 'bce_multi_fwd_k+bce_fwd_k'), ('bce_logits_fwd_grad', 1, (1,), (256,), 'bce_multi_fwd_k'),
                               ('bce_logits_bwd', 1, (_gx, _c), (256,), 'bce_multi_bwd_k')), 'bce table, ' + _note, kind='bce', terms=_terms))
    ROWS.append(_row('table', (('mean_multi_fwd', 2, (1,), (256,), 'mean_multi_fwd_k'), ('mean_fwd', _c, (1,), (256,), 'mean_fwd_k')),
                     'mean table, ' + _note, kind='mean', terms=_terms))
# the head backward
_HEADS = [
    (((2, 1, (1, 1)),), 2, True, True, 'M < 16: row groups stay empty; H = 1'),
    (((15, 16, (15,)),), 2, False, True, 'one term, H = 16, d_wouts NULL'),
    (((17, 17, (7, 10)),), 3, True, False, 'H % 16 = 1, d_bouts NULL'),
    (((128, 33, (1, 7, 60, 60)),), 4, True, True, 'four terms, three column workgroups'),
    (((2048, 5, (2047, 1)),), 2, True, True, 'M = GGAN_HEAD_BCE_MAX_ROWS fills gs_[]; a term of more than one trip'),
    (((17, 17, (7, 10)), (40, 33, (39, 1))), 6, True, True, 'two heads, terms 2 + 2, other M and H'),
    (((300, 3, (299, 1)), (2, 1, (1, 1))), 3, False, False, 'two heads, both optional tables NULL'),
]
for _heads, _wg, _dw, _db, _note in _HEADS:
    ROWS.append(_row('heads', (('bce_head_bwd', 1, (_wg,), (256,), 'bce_head_bwd_k'), ('bce_logits_fwd_grad', 1, (1,), (256,), 'bce_multi_fwd_k')),
                     _note, heads=_heads, dw=_dw, db=_db, alpha=0.2))
# distances
for _p in (1, 2):
    for _i, (_n, _gx) in enumerate(((1, 1), (1023, 1), (1024, 1), (1025, 2), (5000, 5))):
        ROWS.append(_row('dist', (('dist_fwd', 1, (1,), (1024,), 'dist_fwd_k'), ('dist_bwd', 1, (_gx,), (256,), 'dist_bwd_k')),
                         'p = %d, n = %d' % (_p, _n), p=_p, n=_n, gx=(_i + _p) % 3 != 1, gy=(_i + _p) % 3 != 2, acc=(_i + _p) % 2, prior=-0.5,
                         w=(1.0, 0.5, 2.0)[_i % 3], gout=(1.0, 3.0)[_i % 2]))
# the gradient penalty
for _B, _D in ((1, 1), (7, 255), (256, 256), (257, 257), (300, 5), (64, 3072)):
    ROWS.append(_row('gp', (('gp_slopes', 1, (_B,), (256,), 'gp_slopes_k'), ('gp_penalty', 1, (1,), (256,), 'gp_pen_k'),
                            ('gp_fwd_grad', 2, (_B,), (256,), 'gp_fwd_grad_k'), ('gp_penalty_bwd', 2, (_B,), (256,), 'gp_bwd_k')),
                     'B = %d, D = %d' % (_B, _D), B=_B, D=_D, lam=10.0, gpen=0.7))
# training MMD^2
_MMD = [
    (1, 1, 1, 1, False, True, True, 'normal', (0,)),
    (2, 2, 3, 6, True, True, True, 'shared', (0, 1)),
    (5, 9, 16, 8, False, False, True, 'normal', (0, 1)),
    (128, 129, 5, 1, True, True, False, 'normal', (0, 1)),
    (256, 256, 8, 6, False, True, True, 'shared', (0, 1)),
    (300, 212, 16, 8, True, True, True, 'normal', (0, 1)),
    (3, 4, 260, 6, True, True, True, 'normal', (0, 1)),
    (5, 9, 16, 6, False, True, True, 'far', (0, 1)),
]
for _m, _n, _d, _ns, _wts, _dX, _dY, _variant, _ests in _MMD:
    for _unb in _ests:
        _l = ('mmd2u_rows', 'mmd2u_bwd') if _unb else ('mmd2_rows', 'mmd2_bwd')
        ROWS.append(_row('mmd', ((_l[0], 1, (_m + _n,), (256,), 'mmd2_rows_k'), ('mmd2_final', 1, (1,), (64,), 'mmd2_final_k'),
                                 (_l[1], 1, (_m + _n,), (256,), 'mmd2_bwd_k')),
                         '%s, sets %s' % ('unbiased' if _unb else 'biased', _variant), m=_m, n=_n, d=_d, ns=_ns, wts=_wts, dX=_dX, dY=_dY,
                         unbiased=_unb, gout=3.0, variant=_variant))
# aggregated-posterior divergences
_AGG = [(1, 1, 1, 1, False), (5, 7, 3, 5, False), (129, 3, 2, 129, False), (4, 3, 129, 4, False), (2, 2, 8192, 2, False), (8192, 2, 2, 8192, False),
        (5, 7, 3, 11, False), (6, 9, 40, 6, True)]
for _nx, _nz, _d, _nc, _wide in _AGG:
    for _kind in ((0, 2) if _wide else (0, 1, 2)):
        _ns = 2 * _nz if _kind == 2 else _nz
        ROWS.append(_row('agg', (('agg_div_fwd', 1, (_ns,), (128,), 'agg_div_fwd_k'), ('agg_div_final', 1, (1,), (64,), 'agg_div_final_k'),
                                 ('agg_div_bwd_samples', 1, (_ns,), (128,), 'agg_div_bwd_samples_k'),
                                 ('agg_div_bwd_comps', 1, (_nx,), (128,), 'agg_div_bwd_comps_k')),
                         'kind %d%s%s' % (_kind, ', std 50' if _wide else '', ', n_coms != nx' if _nc != _nx else ''),
                         kind=_kind, nx=_nx, nz=_nz, d=_d, n_coms=_nc, wide=_wide))


def row_id(row):
    e = row['entry']
    if e == 'single':
        return 'single-%s-n%d-acc%d' % (row['kind'], row['n'], row['acc'])
    if e == 'table':
        return 'table-%s-c%d-%s' % (row['kind'], len(row['terms']), '_'.join(str(t[0]) for t in row['terms'][:4]))
    if e == 'heads':
        return 'heads-' + '+'.join('%dx%dt%d' % (M, H, len(t)) for M, H, t in row['heads']) + ('' if row['dw'] else '-nodw') + ('' if row['db'] else '-nodb')
    if e == 'dist':
        return 'dist-p%d-n%d%s%s-acc%d' % (row['p'], row['n'], '' if row['gx'] else '-nogx', '' if row['gy'] else '-nogy', row['acc'])
    if e == 'gp':
        return 'gp-%dx%d' % (row['B'], row['D'])
    if e == 'mmd':
        return 'mmd%s-%d-%d-%d-s%d%s%s%s-%s' % ('u' if row['unbiased'] else '', row['m'], row['n'], row['d'], row['ns'], '-wts' if row['wts'] else '',
                                                '' if row['dX'] else '-nodX', '' if row['dY'] else '-nodY', row['variant'])
    return 'agg-k%d-%d-%d-%d-c%d%s' % (row['kind'], row['nx'], row['nz'], row['d'], row['n_coms'], '-wide' if row['wide'] else '')


def threads(launch):
    """the profiler's grid figure of a launch: work-items"""
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


# ---- each entry point's launch list, transcribed -------------------------------------------------------------------------------------------
def _merge(launches):
    out = {}
    for label, grid, block, kernel in launches:
        k = (label, grid, block)
        out[k] = (out[k][0] + 1, out[k][1] + [kernel]) if k in out else (1, [kernel])
    return tuple((k[0], v[0], k[1], k[2], '+'.join(sorted(set(v[1]), key=v[1].index))) for k, v in out.items())


def planned(row):
    """-> the launches the transcription derives for a row, those of one (label, grid, block) counted together"""
    e, b = row['entry'], (K_BLOCK,)
    if e == 'single':
        n = row['n']
        if row['kind'] == 'bce':
            return _merge([('bce_logits_fwd', (1,), b, 'bce_fwd_k'), ('bce_logits_bwd', (cdiv(n, 256),), b, 'bce_bwd_k')])
        return _merge([('mean_fwd', (1,), b, 'mean_fwd_k'), ('mean_bwd', (cdiv(n, 256),), b, 'mean_bwd_k')])
    if e == 'table':
        ns = [t[0] for t in row['terms']]
        if row['kind'] == 'bce':
            return _merge([('bce_logits_fwd', (1,), b, 'bce_multi_fwd_k'), ('bce_logits_fwd_grad', (1,), b, 'bce_multi_fwd_k'),
                           ('bce_logits_bwd', (cdiv(max(ns), 256), len(ns)), b, 'bce_multi_bwd_k')] + [('bce_logits_fwd', (1,), b, 'bce_fwd_k')] * len(ns))
        return _merge([('mean_multi_fwd', (1,), b, 'mean_multi_fwd_k')] * 2 + [('mean_fwd', (1,), b, 'mean_fwd_k')] * len(ns))
    if e == 'heads':
        wg = 1 + sum(cdiv(H, HEAD_COLS) for _, H, _ in row['heads'])
        return _merge([('bce_head_bwd', (wg,), b, 'bce_head_bwd_k'), ('bce_logits_fwd_grad', (1,), b, 'bce_multi_fwd_k')])
    if e == 'dist':
        return _merge([('dist_fwd', (1,), (DIST_FWD_BLOCK,), 'dist_fwd_k'), ('dist_bwd', (grid_for(row['n']),), b, 'dist_bwd_k')])
    if e == 'gp':
        B = (row['B'],)
        return _merge([('gp_slopes', B, b, 'gp_slopes_k'), ('gp_penalty', (1,), b, 'gp_pen_k')] + [('gp_fwd_grad', B, b, 'gp_fwd_grad_k')] * 2 +
                      [('gp_penalty_bwd', B, b, 'gp_bwd_k')] * 2)
    if e == 'mmd':
        tot, u = (row['m'] + row['n'],), 'u' if row['unbiased'] else ''
        return _merge([('mmd2%s_rows' % u, tot, b, 'mmd2_rows_k'), ('mmd2_final', (1,), (FINAL_BLOCK,), 'mmd2_final_k'), ('mmd2%s_bwd' % u, tot, b, 'mmd2_bwd_k')])
    ns, a = ((2 if row['kind'] == 2 else 1) * row['nz'],), (AGG_BLOCK,)
    return _merge([('agg_div_fwd', ns, a, 'agg_div_fwd_k'), ('agg_div_final', (1,), (FINAL_BLOCK,), 'agg_div_final_k'),
                   ('agg_div_bwd_samples', ns, a, 'agg_div_bwd_samples_k'), ('agg_div_bwd_comps', (row['nx'],), a, 'agg_div_bwd_comps_k')])


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
_c32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


def logits(rng, n, turn=0):
    """a normal draw at scale 4 carrying EDGE_LOGITS (all of them from n = 28 on, else the first n of the list turned by `turn`)"""
    x = _c32(4.0 * rng.standard_normal(n))
    E = np.roll(np.asarray(EDGE_LOGITS, np.float32), -turn)
    k = min(n, len(E))
    x[(np.arange(k) * (n // k)) if n >= 2 * len(E) else np.arange(k)] = E[:k]
    return x


def all_terms(row):
    """(n, z, w) of every term of a table or heads row, in table order (a head's terms weigh 1 / terms, labels alternate with 0.9 last)"""
    if row['entry'] == 'table':
        return list(row['terms'])
    out = []
    for M, H, ns in row['heads']:
        out += [(n, (1.0, 0.0, 0.9)[(i + len(out)) % 3], 1.0 / len(ns)) for i, n in enumerate(ns)]
    return out


def inputs(row, seed):
    """-> dict of float32 host arrays"""
    rng = np.random.default_rng(seed)
    e = row['entry']
    if e == 'single':
        return dict(x=logits(rng, row['n'], seed) if row['kind'] == 'bce' else _c32(4.0 * rng.standard_normal(row['n'])))
    if e in ('table', 'heads'):
        bce = e == 'heads' or row['kind'] == 'bce'
        out = dict(xs=[logits(rng, n, seed + 3 * k) if bce else _c32(4.0 * rng.standard_normal(n)) for k, (n, _, _) in enumerate(all_terms(row))])
        if e == 'heads':
            out['h'], out['w_out'] = [], []
            for M, H, _ in row['heads']:
                h = _c32(rng.standard_normal((M, H)))
                zero = rng.random((M, H)) < 0.1
                h[zero] = np.where(rng.random(int(zero.sum())) < 0.5, 0.0, -0.0)
                h.flat[0] = 0.0                                  # (at least one, whatever the size)
                out['h'].append(h)
                out['w_out'].append(_c32(rng.standard_normal(H)))
        return out
    if e == 'dist':
        x, y = _c32(rng.standard_normal(row['n'])), _c32(rng.standard_normal(row['n']))
        same = rng.random(row['n']) < 0.1
        same[0] = row['n'] > 1 or seed % 2 == 0
        y[same] = x[same]
        return dict(x=x, y=y)
    if e == 'gp':
        B, D = row['B'], row['D']
        g = rng.standard_normal((B, D))
        g[np.abs(g) < 1e-3] = 1e-3                               # (no all-zero row, whatever D)
        norms = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), size=B))
        norms[:2] = (30.0, 1e-3)[:min(B, 2)]
        g = g / np.sqrt((g * g).sum(1, keepdims=True)) * norms[:, None]
        g[B // 2] = 0.0
        g[B // 2, seed % D] = 1.0                                # one-hot: the norm is exactly 1
        return dict(g=_c32(g))
    if e == 'mmd':
        m, n, d = row['m'], row['n'], row['d']
        X, Y = _c32(rng.standard_normal((m, d))), _c32(1.5 * rng.standard_normal((n, d)) + 0.5)
        if row['variant'] == 'shared':
            Y[:2] = X[:2]
        if row['variant'] == 'far':
            Y = _c32(Y + 200.0)
        return dict(X=X, Y=Y, sigmas=_c32(SIGMAS[row['ns']]), wts=_c32(WTS[:row['ns']]) if row['wts'] else None)
    nx, nz, d = row['nx'], row['nz'], row['d']
    if row['wide']:
        mu, sd, es = 0.01 * rng.standard_normal((nx, d)), np.full((nx, d), 50.0), 1e-3
    else:
        mu, sd, es = rng.standard_normal((nx, d)), np.exp(0.4 * rng.standard_normal((nx, d))), 1.0
    k = np.zeros((nz, nx))
    k[np.arange(nz), rng.integers(0, nx, nz)] = 1
    return dict(mu=_c32(mu), sd=_c32(sd), k=_c32(k), eps=_c32(es * rng.standard_normal((nz, d))), zp=_c32(rng.standard_normal((nz, d))))


# ---- the kernels in float32, in their summation order (no contraction: a device fmaf rounds once where this rounds twice) --------------------
MUTANTS = ('one_trip:cost', 'one_trip:heads_g', 'one_trip:dist', 'one_trip:gp_slopes', 'one_trip:gp_pen', 'one_trip:mmd_rows', 'one_trip:mmd_bwd_j',
           'one_trip:mmd_bwd_k', 'one_trip:agg_d', 'one_trip:agg_nx', 'accumulate_ignored', 'accumulate_always', 'term0_added_to_stale',
           'bce_no_abs', 'sigmoid_exp_ratio', 'label_weight_swapped', 'n_from_longest', 'head1_reads_head0_terms', 'dbout_every_wg',
           'alpha_on_ge', 'p1_plus_at_zero', 'gp_no_over_B', 'pen_stale_slope', 'unbiased_m2', 'diagonal_kept', 'cross_plus', 'wts_ignored',
           'gamma_no_half', 'jsd_shared_shift', 'ncoms_is_nx', 'lognx_dropped', 'gsd_no_inv_sg')
NAN32 = f32(np.nan)


def _lanes(a, blk, one_trip=False):
    """per-thread sums of a[..., i] over i = thread, thread + blk, ... -> (..., blk)"""
    n = a.shape[-1]
    trips = cdiv(n, blk)
    pad = np.zeros(a.shape[:-1] + (trips * blk,), np.float32)
    pad[..., :n] = a
    pad = pad.reshape(a.shape[:-1] + (trips, blk))
    s = np.zeros(a.shape[:-1] + (blk,), np.float32)
    for t in range(1 if one_trip else trips):
        s = s + pad[..., t, :]
    return s


def block_sum32(s):
    """wave_sum's xor butterfly per 64 lanes, then block_sum's serial loop over the waves (lane 0's view)"""
    blk = s.shape[-1]
    v = s.reshape(s.shape[:-1] + (blk // 64, 64))
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    t = np.zeros(s.shape[:-1], np.float32)
    for w in range(blk // 64):
        t = t + v[..., w, 0]
    return t


def seq_sum32(a):
    s = f32(0)
    for v in np.asarray(a, np.float32).ravel():
        s = f32(s + v)
    return s


def bce_value32(v, z, mut=None):
    e = np.exp(-v) if mut == 'bce_no_abs' else np.exp(-np.abs(v))
    return (np.maximum(v, f32(0)) - v * z) + np.log1p(e)


def bce_grad32(g, v, z, mut=None):
    if mut == 'sigmoid_exp_ratio':
        return g * (np.exp(v) / (f32(1) + np.exp(v)) - z)
    return g * (f32(1) / (f32(1) + np.exp(-v)) - z)


def _zw(z, w, mean, mut):
    return (f32(w), f32(z)) if (mut == 'label_weight_swapped' and not mean) else (f32(z), f32(w))


def _term32(x, z, w, mean, ndiv, mut):
    vals = x if mean else bce_value32(x, z, mut)
    s = block_sum32(_lanes(vals, K_BLOCK, mut == 'one_trip:cost'))
    return f32(w * (s / f32(ndiv)))


def _single32(row, inp, mut):
    mean, x, n = row['kind'] == 'mean', inp['x'], row['n']
    z, w = _zw(row['z'], row['w'], mean, mut)
    r = _term32(x, z, w, mean, n, mut)
    acc = {'accumulate_ignored': 0, 'accumulate_always': 1}.get(mut, row['acc'])
    prior = f32(row['prior']) if row['acc'] else NAN32
    g = f32(f32(row['gloss']) * w) / f32(n)
    return dict(loss=f32(prior + r) if acc else r, gx=np.full(n, g, np.float32) if mean else bce_grad32(g, x, z, mut))


def _table32(terms, xs, mean, mut):
    """-> (total, total of one accumulating launch per term, unit-seed gxs, gloss = 3 gxs)"""
    nmax = max(t[0] for t in terms)
    tot = chainv = None
    gxs, gxs3 = [], []
    for k, ((n, z, w), x) in enumerate(zip(terms, xs)):
        z, w = _zw(z, w, mean, mut)
        nd = nmax if mut == 'n_from_longest' else n
        r = _term32(x, z, w, mean, nd, mut)
        tot = (f32(NAN32 + r) if mut == 'term0_added_to_stale' else r) if k == 0 else f32(tot + r)
        acc = {'accumulate_ignored': 0, 'accumulate_always': 1}.get(mut, int(k > 0))
        chainv = f32((NAN32 if chainv is None else chainv) + r) if acc else r
        for out, gl in ((gxs, f32(1)), (gxs3, f32(3))):
            g = f32(gl * w) / f32(nd)
            out.append(np.full(n, g, np.float32) if mean else bce_grad32(g, x, z, mut))
    return tot, chainv, np.concatenate(gxs), np.concatenate(gxs3)


def _tab32(row, inp, mut):
    mean = row['kind'] == 'mean'
    tot, chainv, gxs, gxs3 = _table32(row['terms'], inp['xs'], mean, mut)
    if mean:
        return dict(loss_fg=tot, loss_null=tot, loss_terms=chainv, gxs=gxs)
    return dict(loss_fwd=tot, loss_fg=tot, loss_terms=chainv, gxs=gxs, gxs3=gxs3)


def _combine16(red):
    """red (16, ...) -> combine16's balanced tree"""
    while red.shape[0] > 1:
        red = red[0::2] + red[1::2]
    return red[0]


def head32(g, h, w_out, alpha, mut=None):
    """head_columns<true> from g -> (gh, d_wout, d_bout)"""
    M, H = h.shape
    sel = np.where((h >= 0) if mut == 'alpha_on_ge' else (h > 0), f32(1), f32(alpha))
    gh = (g[:, None] * w_out[None, :]) * sel
    trips = cdiv(M, 16)
    gp_, hp = np.zeros(trips * 16, np.float32), np.zeros((trips * 16, H), np.float32)
    gp_[:M], hp[:M] = g, h
    acc, gs = np.zeros((16, H), np.float32), np.zeros(16, np.float32)
    for t in range(trips):
        acc = acc + gp_[16 * t:16 * t + 16, None] * hp[16 * t:16 * t + 16]
        gs = gs + gp_[16 * t:16 * t + 16]
    db = _combine16(gs)
    return gh, _combine16(acc), f32(db * cdiv(H, HEAD_COLS)) if mut == 'dbout_every_wg' else db


def _heads32(row, inp, mut):
    terms = all_terms(row)
    tot, _, gxs, _ = _table32(terms, inp['xs'], False, mut)
    out = dict(loss=tot, loss_fg=tot, gxs=gxs, gxs_fg=gxs, gh=[], dw=[], db=[])
    k = r0 = 0
    for a, (M, H, ns) in enumerate(row['heads']):
        g = gxs[r0:r0 + M].copy()
        if mut == 'head1_reads_head0_terms' and a == 1:
            g = np.zeros(M, np.float32)
            M0 = min(M, row['heads'][0][0])
            g[:M0] = gxs[:M0]
        if mut == 'one_trip:heads_g':
            o = 0
            for n in ns:
                g[o + 256:o + n] = NAN32
                o += n
        gh, dw, db = head32(g, inp['h'][a], inp['w_out'][a], row['alpha'], mut)
        out['gh'].append(gh)
        out['dw'].append(dw if row['dw'] else None)
        out['db'].append(db if row['db'] else None)
        k, r0 = k + len(ns), r0 + M
    return out


def _dist32(row, inp, mut):
    x, y, n, p = inp['x'], inp['y'], row['n'], row['p']
    d = x - y
    s = block_sum32(_lanes(d * d if p == 2 else np.abs(d), DIST_FWD_BLOCK, mut == 'one_trip:dist'))
    r = f32(f32(row['w']) * (s / f32(n)))
    acc = {'accumulate_ignored': 0, 'accumulate_always': 1}.get(mut, row['acc'])
    prior = f32(row['prior']) if row['acc'] else NAN32
    g = f32(f32(row['gout']) * f32(row['w'])) / f32(n)
    sign = np.where(d > 0, f32(1), np.where(d < 0, f32(-1), f32(1 if mut == 'p1_plus_at_zero' else 0)))
    v = g * (f32(2) * d if p == 2 else sign)
    return dict(out=f32(prior + r) if acc else r, gx=v if row['gx'] else None, gy=-v if row['gy'] else None)


def _gp32(row, inp, mut):
    g, B, D, lam = inp['g'], row['B'], row['D'], f32(row['lam'])
    sl = np.sqrt(block_sum32(_lanes(g * g, K_BLOCK, mut == 'one_trip:gp_slopes')))

    def pen_of(s):
        dlt = s - f32(1)
        return f32(lam * (block_sum32(_lanes(dlt * dlt, K_BLOCK, mut == 'one_trip:gp_pen')) / f32(B)))

    def gg_of(gpen):
        den = sl if mut == 'gp_no_over_B' else f32(B) * sl
        return ((((f32(gpen) * lam) * f32(2)) * (sl - f32(1))) / den)[:, None] * g
    pen = pen_of(sl)
    stale = pen_of(np.full(B, NAN32)) if mut == 'pen_stale_slope' else pen
    return dict(slopes=sl, pen=pen, slopes2=sl, pen2=stale, slopes3=sl, pen3=pen, gg_unit=gg_of(1.0), gg_unit3=gg_of(1.0), gg1=gg_of(1.0),
                gg=gg_of(row['gpen']), arrive=[0, 0])


def gamma32(sigmas, mut=None):
    s = np.asarray(sigmas, np.float32)
    return f32(1) / ((s * s) if mut == 'gamma_no_half' else (f32(2) * s * s))


def _coef32(m, n, unbiased, mut):
    tot = m + n
    inx = np.arange(tot) < m
    same = inx[:, None] == inx[None, :]
    fm, fn = f32(m), f32(n)
    cx, cy = f32(1) / (fm * fm), f32(1) / (fn * fn)
    if unbiased and mut != 'unbiased_m2':
        cx, cy = f32(1) / (fm * f32(m - 1)), f32(1) / (fn * f32(n - 1))
    cross = f32(-1) / (fm * fn)
    Cm = np.where(same, np.where(inx[:, None], cx, cy), -cross if mut == 'cross_plus' else cross).astype(np.float32)
    if unbiased and mut != 'diagonal_kept':
        Cm[np.arange(tot), np.arange(tot)] = 0
    return Cm


def _mmd32(row, inp, mut):
    m, n, d, ns = row['m'], row['n'], row['d'], row['ns']
    Zs = np.concatenate([inp['X'], inp['Y']])
    tot = m + n
    gam = gamma32(inp['sigmas'], mut)
    wt = inp['wts'] if (inp['wts'] is not None and mut != 'wts_ignored') else np.ones(ns, np.float32)
    dist = np.zeros((tot, tot), np.float32)
    for k in range(d):
        t = Zs[:, None, k] - Zs[None, :, k]
        dist = dist + t * t
    kv, gv = np.zeros_like(dist), np.zeros_like(dist)
    for s in range(ns):
        e = np.exp(-gam[s] * dist)
        kv = kv + wt[s] * e
        gv = gv + (wt[s] * gam[s]) * e
    Cm = _coef32(m, n, row['unbiased'], mut)
    rows = block_sum32(_lanes(Cm * kv, K_BLOCK, mut == 'one_trip:mmd_rows'))
    cf = ((f32(-4) * Cm) * gv) * f32(row['gout'])
    if mut == 'one_trip:mmd_bwd_j':
        cf[:, 256:] = NAN32
    dZ = np.zeros((tot, d), np.float32)
    for j in range(tot):
        dZ = dZ + cf[:, j, None] * (Zs - Zs[j][None, :])
    if mut == 'one_trip:mmd_bwd_k':
        dZ[:, 256:] = NAN32
    return dict(rows=rows, out=seq_sum32(rows), dX=dZ[:m] if row['dX'] else None, dY=dZ[m:] if row['dY'] else None)


def _agg32(row, inp, mut):
    kind, nx, nz, d = row['kind'], row['nx'], row['nz'], row['d']
    nc = f32(nx if mut == 'ncoms_is_nx' else row['n_coms'])
    mu, sd = inp['mu'], inp['sd']
    nsamp = 2 * nz if kind == 2 else nz
    qs = np.zeros(nsamp, bool) if kind == 1 else (np.arange(nsamp) < nz)
    Z = np.empty((nsamp, d), np.float32)
    idx = np.argmax(inp['k'], 1)
    if kind != 1:
        Z[:nz] = sd[idx] * inp['eps'] + mu[idx]
    if kind != 0:
        Z[nsamp - nz:] = inp['zp']
    one_d, one_nx = mut == 'one_trip:agg_d', mut == 'one_trip:agg_nx'
    Bv = f32(-0.5) * block_sum32(_lanes(Z * Z + LOG2PI32, AGG_BLOCK, one_d))
    acc = np.zeros((nsamp, nx), np.float32)
    lsd = f32(2) * np.log(sd)
    for dd in range(d):
        r = (Z[:, dd, None] - mu[None, :, dd]) / sd[None, :, dd]
        acc = acc + ((r * r + LOG2PI32) + lsd[None, :, dd])
    A = f32(-0.5) * acc
    if one_nx:
        A[:, AGG_BLOCK:] = NAN32
    if one_d:
        Z[:, AGG_BLOCK:] = NAN32
    mq = A.max(1)
    mm = np.maximum(mq, Bv) if kind == 2 else mq
    shift = mm if mut == 'jsd_shared_shift' else mq
    Sq = block_sum32(_lanes(np.exp(A - shift[:, None]), AGG_BLOCK))
    lq = (mq + np.log(Sq)) if mut == 'lognx_dropped' else (mq + np.log(Sq)) - np.log(f32(nx))
    if mut == 'jsd_shared_shift':
        lq = (shift + np.log(Sq)) - np.log(f32(nx))
    pe = nc * np.exp(Bv - mm)
    Mx = Sq * np.exp(shift - mm) + pe
    if kind == 0:
        T = lq - Bv
    elif kind == 1:
        T = Bv - lq
    else:
        lm = (mm + np.log(Mx)) - np.log(f32(nx) + nc)
        T = np.where(qs, f32(0.5) * (lq - lm), f32(0.5) * (Bv - lm))
    out = f32(seq_sum32(T) / f32(nz))
    # backward
    gs = f32(1.0) / f32(nz)                                          # gout = 1
    rq = np.exp(A - shift[:, None]) / Sq[:, None]
    if kind == 0:
        W = rq
    elif kind == 1:
        W = -rq
    else:
        rm = np.exp(A - mm[:, None]) / Mx[:, None]
        W = np.where(qs[:, None], f32(0.5) * (rq - rm), f32(-0.5) * rm)
    W = (W * gs).astype(np.float32)
    v = np.full(nsamp, -gs, np.float32) if kind == 0 else gs * (f32(-0.5) * pe / Mx)
    GZ = np.full((nsamp, d), NAN32)
    nq = 0 if kind == 1 else nz
    if nq:
        zq = Z[:nq]
        accz = -v[:nq, None] * zq
        for j in range(nx):
            accz = accz - W[:nq, j, None] * (zq - mu[j][None, :]) / (sd[j] * sd[j])[None, :]
        GZ[:nq] = accz
    i2 = f32(1) / (sd * sd)
    gm, gsg = np.zeros((nx, d), np.float32), np.zeros((nx, d), np.float32)
    for i in range(nsamp):
        r = Z[i][None, :] - mu
        gm = gm + W[i][:, None] * (r * i2)
        gsg = gsg + W[i][:, None] * ((r * r * i2 / sd) if mut == 'gsd_no_inv_sg' else (r * r * i2 / sd - f32(1) / sd))
    for i in range(nq):
        j = idx[i]
        gz = inp['k'][i, j] * GZ[i]
        gm[j] = gm[j] + gz
        gsg[j] = gsg[j] + gz * inp['eps'][i]
    return dict(out=out, Z=Z, A=A, Bv=Bv, T=T.astype(np.float32), W=W, GZ=GZ, gmu=gm, gsd=gsg)


_RUN32 = dict(single=_single32, table=_tab32, heads=_heads32, dist=_dist32, gp=_gp32, mmd=_mmd32, agg=_agg32)


def run32(row, inp, mut=None):
    """every output of a row's calls from the float32 restatement; `mut` names one wrong kernel of MUTANTS"""
    with np.errstate(all='ignore'):
        return _RUN32[row['entry']](row, inp, mut)


# ---- float64 restatements and the staged checks ----------------------------------------------------------------------------------------------
def d64(x):
    return np.asarray(x, np.float64)


def r32(x):
    """a scalar as the kernel receives it: rounded to float32"""
    return float(np.float32(x))


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def _frac(err, bound):
    """worst err / bound; an error where the bound is 0 counts as infinite, and so does every element whose error or bound is not finite"""
    err, bound = np.atleast_1d(d64(err)), np.atleast_1d(d64(bound))
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    f = np.where(np.isfinite(err) & np.isfinite(bound), f, np.inf)
    return float(np.max(f))


def within(fractions):
    return all(f <= 1.0 for f in fractions.values())


def sigmoid64(v):
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def term64(x, z, w, mean):
    """-> (w mean(value), its bound) of one term in float64 from the float32 logits"""
    v, z, w, n = d64(x), r32(z), r32(w), x.size
    if mean:
        val, tb = v, np.zeros(n)
    else:
        a, b, c = np.maximum(v, 0.0), v * z, np.log1p(np.exp(-np.abs(v)))
        val = a - b + c
        tb = np.abs(b) + np.abs(a - b) + (2 * P_EXP + 2 * P_LOG1P) * c + np.abs(val) + 2 * TINY / U
    r = w * val.sum() / n
    return r, abs(w) / n * U * (tb.sum() + chain(n, K_BLOCK) * np.abs(val).sum()) + 2 * U * abs(r)


def table64(terms, xs, mean):
    rs, bs = zip(*[term64(x, z, w, mean) for (n, z, w), x in zip(terms, xs)])
    return sum(rs), sum(bs) + (len(rs) * U * sum(abs(r) for r in rs) if len(rs) > 1 else 0.0)


def grad_fraction(gx, x, z, w, gloss, n, mean):
    g = r32(gloss) * r32(w) / n
    if mean:
        return 0.0 if same_bits(gx, np.full(n, f32(f32(gloss) * f32(w)) / f32(n), np.float32)) else np.inf
    return _frac(np.abs(d64(gx) - g * (sigmoid64(d64(x)) - r32(z))), np.full(n, K_GRAD * U * abs(g)))


def _chk_single(row, inp, out, fr, broken):
    mean, n = row['kind'] == 'mean', row['n']
    r, b = term64(inp['x'], row['z'], row['w'], mean)
    if row['acc']:
        r = r32(row['prior']) + r
        b += U * abs(r)
    fr['loss'] = _frac(abs(float(out['loss']) - r), b)
    fr['gx'] = grad_fraction(out['gx'], inp['x'], row['z'], row['w'], row['gloss'], n, mean)


def _chk_grads(terms, xs, gxs, gloss, mean):
    worst, o = 0.0, 0
    for (n, z, w), x in zip(terms, xs):
        worst = max(worst, grad_fraction(gxs[o:o + n], x, z, w, gloss, n, mean))
        o += n
    return worst


def _chk_table(row, inp, out, fr, broken):
    mean = row['kind'] == 'mean'
    r, b = table64(row['terms'], inp['xs'], mean)
    fr['loss'] = _frac(abs(float(out['loss_fg']) - r), b)
    fr['gxs'] = _chk_grads(row['terms'], inp['xs'], out['gxs'], 1.0, mean)
    for other in ('loss_null',) if mean else ('loss_fwd',):
        if not same_bits(out[other], out['loss_fg']):
            broken.append('%s != loss of fwd_grad' % other)
    if not same_bits(out['loss_terms'], out['loss_fg']):
        broken.append('one accumulating launch per term gives another loss')
    if not mean:
        fr['gxs3'] = _chk_grads(row['terms'], inp['xs'], out['gxs3'], 3.0, False)


def head64(g, h, w_out, alpha):
    """from the float32 g: gh, d_wout, d_bout in float64 and their bounds"""
    g, h, w = d64(g), d64(h), d64(w_out)
    M = h.shape[0]
    gh = g[:, None] * w[None, :] * np.where(h > 0, 1.0, r32(alpha))
    k = cdiv(M, 16)
    return ((gh, gam(2) * np.abs(gh) + TINY), ((g[:, None] * h).sum(0), (k + 5) * U * np.abs(g[:, None] * h).sum(0) + TINY),
            (g.sum(), (k + 4) * U * np.abs(g).sum() + TINY))


def _chk_heads(row, inp, out, fr, broken):
    terms = all_terms(row)
    r, b = table64(terms, inp['xs'], False)
    fr['loss'] = _frac(abs(float(out['loss']) - r), b)
    fr['gxs'] = _chk_grads(terms, inp['xs'], out['gxs'], 1.0, False)
    if not same_bits(out['loss'], out['loss_fg']):
        broken.append('loss != bce_logits_multi_fwd_grad')
    if not same_bits(out['gxs'], out['gxs_fg']):
        broken.append('gxs != bce_logits_multi_fwd_grad')
    r0 = 0
    fr.update(gh=0.0, d_wout=0.0, d_bout=0.0)
    for a, (M, H, ns) in enumerate(row['heads']):
        (gh, bgh), (dw, bdw), (db, bdb) = head64(out['gxs'][r0:r0 + M], inp['h'][a], inp['w_out'][a], row['alpha'])
        fr['gh'] = max(fr['gh'], _frac(np.abs(d64(out['gh'][a]) - gh), bgh))
        if row['dw']:
            fr['d_wout'] = max(fr['d_wout'], _frac(np.abs(d64(out['dw'][a]) - dw), bdw))
        if row['db']:
            fr['d_bout'] = max(fr['d_bout'], _frac(abs(float(out['db'][a]) - db), bdb))
        r0 += M


def _chk_dist(row, inp, out, fr, broken):
    x, y, n, p = d64(inp['x']), d64(inp['y']), row['n'], row['p']
    w, d = r32(row['w']), d64(inp['x']) - d64(inp['y'])
    val = d * d if p == 2 else np.abs(d)
    r = w * val.sum() / n
    b = abs(w) / n * U * ((3 if p == 2 else 1) * val.sum() + chain(n, DIST_FWD_BLOCK) * val.sum()) + 2 * U * abs(r)
    if row['acc']:
        r = r32(row['prior']) + r
        b += U * abs(r)
    fr['out'] = _frac(abs(float(out['out']) - r), b)
    g = r32(row['gout']) * w / n
    v = g * (2.0 * d if p == 2 else np.sign(d))
    for key, ref in (('gx', v), ('gy', -v)):
        if row[key]:
            fr[key] = _frac(np.abs(d64(out[key]) - ref), gam(4) * np.abs(ref))
            if np.any(bits(out[key])[d == 0] & 0x7fffffff):
                broken.append('%s is not +-0 where x == y' % key)


def _chk_gp(row, inp, out, fr, broken):
    g, B, D, lam = d64(inp['g']), row['B'], row['D'], r32(row['lam'])
    sl = np.sqrt((g * g).sum(1))
    fr['slopes'] = _frac(np.abs(d64(out['slopes']) - sl), ((chain(D, K_BLOCK) + 1) / 2.0 + 1) * U * sl)
    s = d64(out['slopes'])
    pen = lam * ((s - 1.0) ** 2).sum() / B
    fr['pen'] = _frac(abs(float(out['pen']) - pen), lam / B * (3 + chain(B, K_BLOCK)) * U * ((s - 1.0) ** 2).sum() + 2 * U * abs(pen))
    for key, gpen in (('gg1', 1.0), ('gg', row['gpen'])):
        ref = (r32(gpen) * lam * 2.0 * (s - 1.0) / (B * s))[:, None] * g
        fr[key] = _frac(np.abs(d64(out[key]) - ref), gam(6) * np.abs(ref))
    for a, b_, what in (('slopes2', 'slopes', 'slopes of fwd_grad != fwd'), ('pen2', 'pen', 'pen of fwd_grad != fwd'), ('slopes3', 'slopes2', 'second launch: slopes'),
                        ('pen3', 'pen2', 'second launch: pen'), ('gg_unit3', 'gg_unit', 'second launch: gg_unit'), ('gg_unit', 'gg1', 'gg_unit != bwd with gpen = 1')):
        if not same_bits(out[a], out[b_]):
            broken.append(what)
    if list(out['arrive']) != [0, 0]:
        broken.append('arrive not left at zero: %s' % (list(out['arrive']),))


def mmd64(row, inp):
    """-> (row sums, their bounds, gradient rows of [X; Y], their bounds) in float64 from the float32 inputs and the float32 gamma"""
    m, n, d, ns = row['m'], row['n'], row['d'], row['ns']
    Zs = np.concatenate([d64(inp['X']), d64(inp['Y'])])
    tot = m + n
    gam = d64(gamma32(inp['sigmas']))
    wt = d64(inp['wts']) if inp['wts'] is not None else np.ones(ns)
    D2 = ((Zs[:, None, :] - Zs[None, :, :]) ** 2).sum(-1)
    arg = -gam[None, None, :] * D2[:, :, None]
    e = np.exp(arg)
    inx = np.arange(tot) < m
    same = inx[:, None] == inx[None, :]
    if row['unbiased']:
        Cm = np.where(same, np.where(inx[:, None], 1.0 / (m * max(m - 1, 1)), 1.0 / (n * max(n - 1, 1))), -1.0 / (m * n))
        Cm[np.arange(tot), np.arange(tot)] = 0.0
    else:
        Cm = np.where(same, np.where(inx[:, None], 1.0 / (m * m), 1.0 / (n * n)), -1.0 / (m * n))
    kv = (wt * e).sum(-1)
    rel = np.abs(arg) * (d + 4) + 2 * P_EXP + ns + 4
    rows = (Cm * kv).sum(1)
    brows = (np.abs(Cm) * ((wt * e * rel).sum(-1) * U + wt.sum() * TINY)).sum(1) + chain(tot, K_BLOCK) * U * (np.abs(Cm) * kv).sum(1)
    go = r32(row['gout'])
    cf = -4.0 * Cm * (wt * gam * e).sum(-1) * go
    cferr = np.abs(4.0 * Cm * go) * ((wt * gam * e * (rel + 2)).sum(-1) * U + (wt * gam).sum() * TINY)
    diff = Zs[:, None, :] - Zs[None, :, :]
    dZ = (cf[:, :, None] * diff).sum(1)
    bZ = ((cferr + np.abs(cf) * (tot + 2) * U)[:, :, None] * np.abs(diff)).sum(1) + TINY
    return rows, brows, dZ, bZ


def _chk_mmd(row, inp, out, fr, broken):
    m = row['m']
    rows, brows, dZ, bZ = mmd64(row, inp)
    fr['rows'] = _frac(np.abs(d64(out['rows']) - rows), brows)
    if not same_bits(out['out'], seq_sum32(out['rows'])):
        broken.append('mmd2_final is not the float32 sum of row_scratch in row order')
    for key, sl in (('dX', slice(0, m)), ('dY', slice(m, None))):
        if row[key]:
            fr[key] = _frac(np.abs(d64(out[key]) - dZ[sl]), bZ[sl])


def agg64(row, inp, out):
    """every stage of agg_div in float64, each from the inputs of its own stage as `out` holds them -> ({stage: (ref, bound)}, samples drawn from q)"""
    kind, nx, nz, d, nc = row['kind'], row['nx'], row['nz'], row['d'], float(row['n_coms'])
    mu, sd = d64(inp['mu']), d64(inp['sd'])
    nsamp = 2 * nz if kind == 2 else nz
    nq = 0 if kind == 1 else nz
    qs = np.arange(nsamp) < nq
    L = float(LOG2PI32)
    st = {}
    Zr, Zb = np.zeros((nsamp, d)), np.zeros((nsamp, d))
    if nq:
        k, eps = d64(inp['k']), d64(inp['eps'])
        Zr[:nq] = k @ mu + (k @ sd) * eps
        Zb[:nq] = (nx + 1) * U * (np.abs(k) @ np.abs(mu) + (np.abs(k) @ sd) * np.abs(eps)) + TINY
    if kind != 0:
        Zr[nsamp - nz:] = d64(inp['zp'])
    st['Z'] = (Zr, Zb)
    Z = d64(out['Z'])
    st['Bv'] = (-0.5 * (Z * Z + L).sum(1), (chain(d, AGG_BLOCK) + 2) / 2.0 * U * (Z * Z + L).sum(1))
    r = (Z[:, None, :] - mu[None]) / sd[None]
    lsd = np.log(sd)[None]
    st['A'] = (-0.5 * (r * r + L + 2 * lsd).sum(2),
               0.5 * U * (5 * r * r + 4 * P_LOG * np.abs(lsd) + (d + 2) * (r * r + L + 2 * np.abs(lsd))).sum(2))
    A, b = d64(out['A']), d64(out['Bv'])
    mq = A.max(1)
    arg = A - mq[:, None]
    e = np.exp(arg)
    Sq = e.sum(1)
    rSq = U * ((e * (np.abs(arg) + 2 * P_EXP)).sum(1) / Sq + chain(nx, AGG_BLOCK))           # relative error of the device's Sq
    lq = mq + np.log(Sq) - np.log(nx)
    elq = rSq + U * (2 * P_LOG * (np.abs(np.log(Sq)) + np.log(nx)) + np.abs(mq + np.log(Sq)) + np.abs(lq)) + TINY
    mm = np.maximum(mq, b) if kind == 2 else mq
    a1, a2 = mq - mm, b - mm
    pe = nc * np.exp(a2)
    Mx = Sq * np.exp(a1) + pe
    rpe = U * (np.abs(a2) + 2 * P_EXP + 2)
    rM = (Sq * np.exp(a1) / Mx) * (rSq + U * (np.abs(a1) + 2 * P_EXP + 1)) + (pe / Mx) * rpe + U
    lm = mm + np.log(Mx) - np.log(nx + nc)
    elm = rM + U * (2 * P_LOG * (np.abs(np.log(Mx)) + np.log(nx + nc)) + np.abs(mm + np.log(Mx)) + np.abs(lm)) + TINY
    T = {0: lq - b, 1: b - lq, 2: np.where(qs, 0.5 * (lq - lm), 0.5 * (b - lm))}[kind]
    st['T'] = (T, (elq if kind != 2 else 0.5 * (np.where(qs, elq, 0.0) + elm)) + U * np.abs(T))
    gs = 1.0 / nz
    rq, rm = e / Sq[:, None], np.exp(A - mm[:, None]) / Mx[:, None]
    erq = rq * ((np.abs(arg) + 2 * P_EXP + 1) * U + rSq[:, None])
    erm = rm * ((np.abs(A - mm[:, None]) + 2 * P_EXP + 1) * U + rM[:, None])
    W = gs * {0: rq, 1: -rq, 2: np.where(qs[:, None], 0.5 * (rq - rm), -0.5 * rm)}[kind]
    st['W'] = (W, gs * (erq if kind != 2 else 0.5 * (np.where(qs[:, None], erq, 0.0) + erm)) + 3 * U * np.abs(W) + TINY)
    # GZ from the device's own W (the kernel reads the values it stored) and, for dL/db, its A and Bv
    v = gs * (-np.ones(nsamp) if kind == 0 else -0.5 * pe / Mx)
    rv = 2 * U if kind == 0 else rM + rpe + 3 * U
    i2 = 1.0 / (sd * sd)
    Wq = d64(out['W'])[:nq]
    tz = Wq[:, :, None] * (Z[:nq, None, :] - mu[None]) * i2[None]
    st['GZ'] = (-v[:nq, None] * Z[:nq] - tz.sum(1),
                (np.atleast_1d(rv)[:nq if kind else 1, None] + 2 * U) * np.abs(v[:nq, None] * Z[:nq]) + 4 * U * np.abs(tz).sum(1) +
                (nx + 1) * U * (np.abs(v[:nq, None] * Z[:nq]) + np.abs(tz).sum(1)) + TINY)
    Wd, GZd = d64(out['W']), d64(out['GZ'])[:nq]
    rr = Z[:, None, :] - mu[None]                                   # (sample, component, dd)
    gm_t = Wd[:, :, None] * rr * i2[None]
    gs_a, gs_b = Wd[:, :, None] * rr * rr * (i2 / sd)[None], Wd[:, :, None] / sd[None]
    gm, gsg = gm_t.sum(0), (gs_a - gs_b).sum(0)
    am, asg = np.abs(gm_t).sum(0), (np.abs(gs_a) + np.abs(gs_b)).sum(0)
    if nq:
        k, eps = d64(inp['k']), d64(inp['eps'])
        gz = k[:, :, None] * GZd[:, None, :]                        # (sample, component, dd)
        gm, gsg = gm + gz.sum(0), gsg + (gz * eps[:, None, :]).sum(0)
        am, asg = am + np.abs(gz).sum(0), asg + np.abs(gz * eps[:, None, :]).sum(0)
    st['gmu'] = (gm, (nsamp + nq + 5) * U * am + TINY)
    st['gsd'] = (gsg, (nsamp + nq + 9) * U * asg + TINY)
    return st, nq


def _chk_agg(row, inp, out, fr, broken):
    st, nq = agg64(row, inp, out)
    for key, (ref, bound) in st.items():
        got = d64(out[key])[:nq] if key == 'GZ' else d64(out[key])
        fr[key] = _frac(np.abs(got - ref), bound)
    if not np.all(np.isnan(np.asarray(out['GZ'])[nq:])):
        broken.append('GZ written for a sample that was not drawn from q')
    if not same_bits(out['out'], f32(seq_sum32(out['T']) / f32(row['nz']))):
        broken.append('agg_div_final is not the float32 sum of T in sample order, / nz')


_CHECK = dict(single=_chk_single, table=_chk_table, heads=_chk_heads, dist=_chk_dist, gp=_chk_gp, mmd=_chk_mmd, agg=_chk_agg)


def _all_finite(out, skip=('GZ', 'arrive')):
    for k, v in out.items():
        for a in (v if isinstance(v, list) else [v]):
            if a is not None and k not in skip and not np.all(np.isfinite(np.asarray(a, np.float64))):
                return k
    return None


def check(row, inp, out):
    """-> ({check: worst fraction of its bound}, [bitwise stages that do not hold]) for the outputs `out` of a row's calls"""
    fr, broken = {}, []
    with np.errstate(all='ignore'):
        _CHECK[row['entry']](row, inp, out, fr, broken)
    bad = _all_finite(out)
    if bad:
        broken.append('%s is not finite' % bad)
    return fr, broken


def kernels_of(row):
    """{check name: the kernel it measures} -- for the per-kernel worst figures"""
    e = row['entry']
    if e == 'single':
        return dict(loss='%s_fwd_k' % row['kind'], gx='%s_bwd_k' % row['kind'])
    if e == 'table':
        return dict(loss='%s_multi_fwd_k' % row['kind'], gxs='%s_multi_fwd_k' % row['kind'], gxs3='bce_multi_bwd_k')
    if e == 'heads':
        return dict(loss='bce_head_bwd_k', gxs='bce_head_bwd_k', gh='bce_head_bwd_k', d_wout='bce_head_bwd_k', d_bout='bce_head_bwd_k')
    if e == 'dist':
        return dict(out='dist_fwd_k', gx='dist_bwd_k', gy='dist_bwd_k')
    if e == 'gp':
        return dict(slopes='gp_slopes_k', pen='gp_pen_k', gg1='gp_bwd_k', gg='gp_bwd_k')
    if e == 'mmd':
        return dict(rows='mmd2_rows_k', dX='mmd2_bwd_k', dY='mmd2_bwd_k')
    return dict(Z='agg_div_fwd_k', Bv='agg_div_fwd_k', A='agg_div_fwd_k', T='agg_div_fwd_k', W='agg_div_bwd_samples_k', GZ='agg_div_bwd_samples_k',
                gmu='agg_div_bwd_comps_k', gsd='agg_div_bwd_comps_k')


# ---- calls that must be refused before any launch ------------------------------------------------------------------------------------------
class Alloc:
    """hands out float buffers for a rejected call: host memory here (the CPU module), device memory in the GPU module's subclass.
    Outputs are NaN-filled and remembered, so that their bits can be held afterwards."""
    def __init__(self):
        self.outs, self.keep = [], []

    def make(self, n):
        a = np.full(n, np.nan, np.float32)
        return a, a.ctypes.data

    def read(self, handle):
        return handle

    def buf(self, n, out=False):
        handle, ptr = self.make(max(int(n), 1))
        self.keep.append(handle)
        if out:
            self.outs.append(handle)
        return C.c_void_p(ptr)

    def outputs_untouched(self):
        return all(bool(np.all(bits(self.read(h)) == bits(NAN32))) for h in self.outs)


def _ptrs(ps):
    return (C.c_void_p * len(ps))(*[p.value for p in ps])


def _floats(vs):
    return (C.c_float * len(vs))(*vs)


def _ints(vs):
    return (C.c_int * len(vs))(*vs)


def _table_args(A, ns, count, gxs=True):
    k = max(len(ns), 1)
    ns = list(ns) or [4]
    x = [A.buf(n) for n in ns]
    g = [A.buf(n, out=True) for n in ns]
    return (_ptrs(x), _floats([1.0] * k), _floats([1.0] * k), _ints(ns), count), (_ptrs(g) if gxs else None)


def _rej_table(fn, count):
    def call(L, A, stream):
        (xs, lab, wts, ns, c), gxs = _table_args(A, [4] * max(count, 1), count)
        loss, gl = A.buf(1, out=True), A.buf(1)
        if fn == 'ggan_bce_logits_multi_fwd':
            return L.ggan_bce_logits_multi_fwd(xs, lab, wts, ns, c, loss, stream)
        if fn == 'ggan_bce_logits_multi_fwd_grad':
            return L.ggan_bce_logits_multi_fwd_grad(xs, lab, wts, ns, c, loss, gxs, stream)
        if fn == 'ggan_bce_logits_multi_bwd':
            return L.ggan_bce_logits_multi_bwd(xs, lab, wts, ns, c, gl, gxs, stream)
        if fn == 'ggan_mean_multi_fwd_grad':
            return L.ggan_mean_multi_fwd_grad(xs, wts, ns, c, loss, gxs, stream)
        return _heads_call(L, A, stream, [4] * max(count, 1), c, 1, [max(count, 1)], [4 * max(count, 1)], [3])
    return call


def _heads_call(L, A, stream, ns, count, nheads, head_terms, Ms, Hs):
    """one logits vector per head, its terms consecutive row ranges of it"""
    x = A.buf(sum(ns) + 8)
    g = A.buf(sum(ns) + 8, out=True)
    offs = np.concatenate([[0], np.cumsum(ns)[:-1]]) if ns else []
    xs, gxs = _ptrs([C.c_void_p(x.value + 4 * int(o)) for o in offs]), _ptrs([C.c_void_p(g.value + 4 * int(o)) for o in offs])
    k = len(ns)
    hs = [A.buf(M * H) for M, H in zip(Ms, Hs)]
    ws = [A.buf(H) for H in Hs]
    ghs = [A.buf(M * H, out=True) for M, H in zip(Ms, Hs)]
    dws = [A.buf(H, out=True) for H in Hs]
    dbs = [A.buf(1, out=True) for _ in Hs]
    return L.ggan_bce_heads_bwd(xs, _floats([1.0] * k), _floats([1.0] * k), _ints(ns), count, A.buf(1, out=True), gxs, nheads, _ints(head_terms),
                                _ints(Ms), _ints(Hs), _ptrs(hs), _ptrs(ws), _floats([0.2] * len(Hs)), _ptrs(ghs), _ptrs(dws), _ptrs(dbs), stream)


def _rej_heads(ns, nheads, head_terms, Ms, Hs):
    return lambda L, A, stream: _heads_call(L, A, stream, ns, len(ns), nheads, head_terms, Ms, Hs)


def _rej_dist(bwd):
    def call(L, A, stream):
        if bwd:
            return L.ggan_dist_bwd(A.buf(8), A.buf(8), A.buf(1), A.buf(8, out=True), A.buf(8, out=True), 8, 3, 1.0, stream)
        return L.ggan_dist_fwd(A.buf(8), A.buf(8), A.buf(1, out=True), 8, 3, 1.0, 0, stream)
    return call


def _rej_mmd(bwd, unbiased, m, n, ns):
    def call(L, A, stream):
        d = 2
        sig = _floats([2.0 + i for i in range(ns)])
        X, Y = A.buf(m * d), A.buf(n * d)
        u = '_unbiased' if unbiased else ''
        if bwd:
            return getattr(L, 'ggan_mix_rbf_mmd2%s_bwd' % u)(X, Y, m, n, d, sig, None, ns, A.buf(1), A.buf(m * d, out=True), A.buf(n * d, out=True), stream)
        return getattr(L, 'ggan_mix_rbf_mmd2%s_fwd' % u)(X, Y, m, n, d, sig, None, ns, A.buf(1, out=True), A.buf(m + n, out=True), stream)
    return call


def _rej_agg(bwd, kind, nx, nz, d):
    def call(L, A, stream):
        ns = 2 * nz
        mu, sd, k, eps, zp = A.buf(nx * d), A.buf(nx * d), A.buf(ns * nx), A.buf(ns * d), A.buf(ns * d)
        if bwd:
            return L.ggan_agg_div_bwd(kind, mu, sd, k, eps, nx, nz, d, nx, A.buf(ns * d), A.buf(ns * nx), A.buf(ns), A.buf(1), A.buf(ns * nx, out=True),
                                      A.buf(ns * d, out=True), A.buf(nx * d, out=True), A.buf(nx * d, out=True), stream)
        return L.ggan_agg_div_fwd(kind, mu, sd, k, eps, zp, nx, nz, d, nx, A.buf(1, out=True), A.buf(ns * d, out=True), A.buf(ns * nx, out=True),
                                  A.buf(ns, out=True), A.buf(ns, out=True), stream)
    return call


_TABLE_FNS = ('ggan_bce_logits_multi_fwd', 'ggan_bce_logits_multi_fwd_grad', 'ggan_bce_logits_multi_bwd', 'ggan_mean_multi_fwd_grad', 'ggan_bce_heads_bwd')
REJECTED = [dict(id='%s-count%d' % (fn[5:], c), fn=fn, call=_rej_table(fn, c)) for fn in _TABLE_FNS for c in (0, BCE_MAX + 1)]
REJECTED += [
    dict(id='heads-nheads3', fn='ggan_bce_heads_bwd', call=_rej_heads([4, 4, 4], BCE_HEADS + 1, [1, 1, 1], [4, 4, 4], [3, 3, 3])),
    dict(id='heads-M2049', fn='ggan_bce_heads_bwd', call=_rej_heads([HEAD_MAX_ROWS + 1], 1, [1], [HEAD_MAX_ROWS + 1], [1])),
    dict(id='heads-terms-do-not-cover-rows', fn='ggan_bce_heads_bwd', call=_rej_heads([4, 5], 1, [2], [10], [3])),
    dict(id='dist_fwd-p3', fn='ggan_dist_fwd', call=_rej_dist(False)),
    dict(id='dist_bwd-p3', fn='ggan_dist_bwd', call=_rej_dist(True)),
]
for _bwd in (False, True):
    _s = 'bwd' if _bwd else 'fwd'
    REJECTED += [
        dict(id='mmd2_%s-rows513' % _s, fn='ggan_mix_rbf_mmd2_' + _s, call=_rej_mmd(_bwd, 0, 256, MMD_MAX_ROWS - 256 + 1, 6)),
        dict(id='mmd2_%s-ns9' % _s, fn='ggan_mix_rbf_mmd2_' + _s, call=_rej_mmd(_bwd, 0, 4, 4, MMD_MAX_SIGMAS + 1)),
        dict(id='mmd2u_%s-m1' % _s, fn='ggan_mix_rbf_mmd2_unbiased_' + _s, call=_rej_mmd(_bwd, 1, 1, 4, 6)),
        dict(id='agg_%s-d8193' % _s, fn='ggan_agg_div_' + _s, call=_rej_agg(_bwd, 0, 2, 2, AGG_MAX + 1)),
        dict(id='agg_%s-nx8193' % _s, fn='ggan_agg_div_' + _s, call=_rej_agg(_bwd, 0, AGG_MAX + 1, 2, 2)),
        dict(id='agg_%s-kind3' % _s, fn='ggan_agg_div_' + _s, call=_rej_agg(_bwd, 3, 2, 2, 2)),
    ]


def source_kernels(text):
    """names of the __global__ kernels of a source text"""
    return sorted(set(re.findall(r'__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\(', text)))
