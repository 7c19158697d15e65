"""Which path of the pointwise, reduction and staging kernels (csrc/pointwise.hip: 16 kernels, 19 launch sites) each dispatch test runs:
one row per entry point and edge (plain data), the rows' inputs, `planned()` -- a transcription of the host dispatch --, `run32` -- every
kernel restated in float32 numpy in the kernel's own order -- and `check()`, the float64 restatements with their derived bounds and the
bitwise stages.

tests/test_pointwise_dispatch_gpu.py runs every row through the C ABI between ggan_prof_reset / ggan_prof_enable, asserts that the
profiler saw exactly the row's launches (label, count, work-items), that the sentinels around every buffer are intact, and hands the
device's outputs to check().  tests/test_pointwise_dispatch_cpu.py holds labels and constants against the source text, planned() against
every row, the enumerated edges against the rows, hands run32's outputs to check() (so every bound is shown reachable without a GPU)
and requires every wrong kernel of MUTANTS to miss on the row MUTANT_ROW names.

A row:
  entry     act_fwd | act_bwd | act_bwd_chansum | bias_add | cast_scale | cast_ring | axpby | row_lerp | colsum | colsum_tall | chansum |
            reparam_fwd | reparam_bwd | stage
  p         the entry point's parameters (shapes, act code, scalars, which optional pointers are NULL, the workspace case `ws`:
            full | null | short -- one float less than the partials need -- | reserved -- ws_bytes not above GGAN_WS_RESERVED)
  off       base offset in floats of every operand from a 16-byte boundary: 1 for the operands only scalar loops read, 0 (any multiple
            of 4) for whatever a float4 load or an aligned16 guard touches
  launches  ((label, launches, grid, block), ...): every launch the row causes, in order; planned(row) must give the same
  note      which edge the row is there for

Buffers (buffers(row)): every operand sits between PAD sentinel floats, outputs start as NaN.

Stages and bounds (u = 2^-24; every stage is measured against float64 from the float32 values that stage itself read -- the device's
own intermediate outputs where there are any --, so no stage carries another's error; a reference result below 2^-126 adds TINY = 2^-126
absolute: flushing is the build's choice):
  bitwise   identity, relu and lrelu forward (fl(alpha v) and fmaxf; relu at v = +-0 may give either zero: C leaves the sign of
            fmaxf(-0, +0) open); relu and lrelu backward (`r > 0 ? g : alpha g` -- a reference of +-0 takes alpha g / +0); bias_add
            fl(x + bias[c]); cast_scale without noise fl(mul fl(fl(x / div) - 0.5)), with noise that plus the noise by a separate add or by
            one fma -- one of the two for ALL elements of the row; cast_ring = cast_scale on the expected slot; gx of act_bwd_chansum =
            act_bwd; gmean = gz or +0; chansum_final = the float32 lane-strided sum plus butterfly of the device's own partials; the
            staged products (entries -1, 0, 1: exact); axpby (0, 0, c) = c and alpha = 0 of row_lerp = x.
  tanh      P_TANH = 5 ulps, sigmoid's and reparam's expf P_EXP = 3 ulps: the OpenCL conformance limits, a condition as in
            _cost_dispatch; an ulp is at most 2 u |value|.  sigmoid r = 1 / (1 + e): expf's 6 u e moves r by 6 u e r^2 = 6 u r (1 - r), the
            sum and the quotient (correctly rounded) add u r each: u r (2 + 6 (1 - r)).
  act_bwd   tanh g (1 - r r): r r, the difference, the product: u |g| (r^2 + 2 |1 - r^2|) (uncontracted; fma(-r, r, 1) only removes
            one).  sigmoid (g r) (1 - r): three roundings on the result, 3 u |g r (1 - r)|.
  axpby     a x, b y, their sum, + c: u (3 |a x| + 3 |b y| + |c|).     row_lerp  x + a (y - x): u (2 |a (y - x)| + |out|).
  sums      (longest addition chain) u sum|terms|, the chain counted per kernel by chain_*() below: the thread's trips (+ 2 for the
            (x+y)+(z+w) grouping of a float4), wave_sum's 6, block_sum's serial loop over the waves or the 2 levels of (a+b)+(c+d).
  reparam   sd: 2 P_EXP u sd.  z = fmaf(eps, sd, mean) from the device's own sd: one rounding, u |z|.  glog = (a eps + b) sd:
            u sd (|a eps| + 2 |a eps + b|).
(1 + 2^-20 on every counted bound covers the second-order terms.)

Found unreachable: the `if (S < 1) S = 1` clamp of ggan_act_bwd_chansum -- cdiv(512, C), N and parts_cap / C are all at least 1 once the
guard `parts_cap >= C` has passed.

Worst observed fraction of the bound per kernel, MI355X, 2026-10-21 (test_pointwise_dispatch_gpu.py prints every row's figure; one above
1 fails):
  act_fwd_k          tanh 0.25   sigmoid 0.69             act_bwd_k          tanh' 0.65   sigmoid' 0.95
  act_bwd_chansum_k  parts 0.29                           axpby_k            out 0.92
  row_lerp32_k / row_lerp_k   out 0.99                    colsum_k           out 0.49
  colsum_part_k      part 0.07                            chansum_part_k     part 0.16   (single-stage out 0.00)
  reparam_fwd_k      sd 0.23   z 0.9995                   reparam_bwd_k      glog 0.95
  bias_add_k, cast_scale_k, cast_scale_ring_k, chansum_final_k, stage_cols_k<JOIN>: bitwise stages only
z is one rounding held to u |z|: half an ulp is the bound itself just above a power of two; row_lerp likewise where alpha is 0."""
import re

import numpy as np

# ---- constants the transcription copies (test_pointwise_dispatch_cpu.py holds them against the source text) ----------------------------
K_BLOCK = 256
GRID_CAP = 2048
ACT_PER_THREAD = 16            # grid_for(n, 16) of act_fwd_k / act_bwd_k
PER_THREAD = 4                 # grid_for's default
ABC_THREADS = 256              # act_bwd_chansum_k
ABC_SPREAD = 512               # S = cdiv(512, C)
ABC_MAX_S = 64
SLAB_ROWS = 64                 # colsum_tall: at least 64 rows per slab
TALL_WGS = 1024
CHAN_WGS = 1024
ONE_BIG = 16384                # chansum<one>: 1024 threads from N * HW >= 16384
HW_256, HW_128 = 1024, 256     # chansum<part>: 256 threads from HW >= 1024, 128 from HW >= 256, else 64
LERP_LIMIT = 4.0e9
WS_RESERVED = 16384
ACT_NONE, ACT_LRELU, ACT_RELU, ACT_TANH, ACT_SIGMOID = 0, 1, 2, 3, 4

U = 2.0 ** -24
TINY = 2.0 ** -126
P_EXP, P_TANH = 3, 5
SECOND = 1.0 + 2.0 ** -20
ALPHA = 0.2
PAD = 8
SENTINEL = np.float32(-12345.678)
INT_SENTINEL = np.int32(-123456789)
ACT_BIG = GRID_CAP * K_BLOCK * ACT_PER_THREAD + 4099           # 2048 * 4096 + 4099
BIG = GRID_CAP * K_BLOCK * PER_THREAD + 1027                    # 2048 * 1024 + 1027
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
f32 = np.float32


def cdiv(a, b):
    return -(-a // b)


def grid_for(n, per_thread=PER_THREAD):
    return min(max(cdiv(n, K_BLOCK * per_thread), 1), GRID_CAP)


# ---- the host dispatch, transcribed ----------------------------------------------------------------------------------------------------
def abc_plan(N, C, cap):
    """ggan_act_bwd_chansum -> (first S, which clamp bound it, ipb, final S)"""
    S, by = cdiv(ABC_SPREAD, C), 'spread'
    if S > N:
        S, by = N, 'N'
    if S > cap // C:
        S, by = cap // C, 'cap'
    if S > ABC_MAX_S:
        S, by = ABC_MAX_S, '64'
    if S < 1:
        S, by = 1, 'one'
    ipb = cdiv(N, S)
    return S, by, ipb, cdiv(N, ipb)


def ws_floats(row):
    """floats of scratch behind the reserved bytes that the row's workspace holds (None: the pointer is NULL)"""
    p = row['p']
    if row['entry'] == 'colsum_tall':
        need = p['cols'] * min(cdiv(TALL_WGS, cdiv(p['cols'], 64)), p['rows'] // SLAB_ROWS)
    else:
        need = p['C'] * min(CHAN_WGS // p['C'], p['N'])
    return {'full': need, 'null': None, 'short': need - 1, 'reserved': 0}[p['ws']]


def tall_plan(row):
    """ggan_colsum_tall -> (P, rows per slab) or None for the fallback to ggan_colsum"""
    p = row['p']
    tiles = cdiv(p['cols'], 64)
    P = min(cdiv(TALL_WGS, tiles), p['rows'] // SLAB_ROWS)
    have = ws_floats(row)
    if P < 2 or have is None or have == 0 or p['cols'] * P > have:
        return None
    return P, cdiv(p['rows'], P)


def chan_plan(row):
    """ggan_chansum -> (P, threads)"""
    p = row['p']
    P = min(CHAN_WGS // p['C'], p['N'])
    have = ws_floats(row)
    if have is None or have == 0 or p['C'] * P > have:
        P = 1
    if P <= 1:
        return 1, (1024 if p['N'] * p['HW'] >= ONE_BIG else 256)
    return P, (256 if p['HW'] >= HW_256 else (128 if p['HW'] >= HW_128 else 64))


def lerp_is_32(rows, cols):
    return float(rows * cols) * cols < LERP_LIMIT


def planned(row):
    """-> the launches the transcription derives for a row"""
    e, p = row['entry'], row['p']
    one = lambda label, n, per=PER_THREAD: ((label, 1, (grid_for(n, per),), (K_BLOCK,)),)
    if e == 'act_fwd':
        return one('act_fwd', p['n'], ACT_PER_THREAD)
    if e == 'act_bwd':
        return one('act_bwd', p['n'], ACT_PER_THREAD)
    if e == 'act_bwd_chansum':
        S = abc_plan(p['N'], p['C'], p['cap'])[3]
        return (('act_bwd_chansum', 1, (p['C'], S), (ABC_THREADS,)),) + one('act_bwd', p['N'] * p['C'] * p['HW'], ACT_PER_THREAD)
    if e == 'bias_add':
        return one('bias_add', p['N'] * p['C'] * p['HW'])
    if e == 'cast_scale':
        return one('cast_scale_i32', p['n'])
    if e == 'cast_ring':
        return one('cast_scale_ring_i32', p['n']) + one('cast_scale_i32', p['n'])
    if e in ('axpby', 'reparam_fwd', 'reparam_bwd'):
        return one(e, p['n'])
    if e == 'row_lerp':
        return one('row_lerp<32>' if lerp_is_32(p['rows'], p['cols']) else 'row_lerp<64>', p['rows'] * p['cols'])
    if e == 'colsum' or (e == 'colsum_tall' and tall_plan(row) is None):
        return (('colsum', 1, (cdiv(p['cols'], 64),), (64,)),)
    if e == 'colsum_tall':
        P, _ = tall_plan(row)
        return (('colsum_tall', 1, (cdiv(p['cols'], 64), P), (256,)), ('chansum_final', 1, (cdiv(p['cols'], 4),), (256,)))
    if e == 'chansum':
        P, threads = chan_plan(row)
        if P <= 1:
            return (('chansum<one>', 1, (p['C'], 1), (threads,)),)
        return (('chansum<part>', 1, (p['C'], P), (threads,)), ('chansum_final', 1, (cdiv(p['C'], 4),), (256,)))
    if e == 'stage':
        R, Ct = stage_shape(p)
        st = ('stage_cols<join>' if p['join'] else 'stage_cols<deal>', 1, (cdiv(R * Ct, K_BLOCK),), (K_BLOCK,))
        # the product: K < 2 * BK, so gemm_plan never splits K; one 64 x 64 tile per workgroup of 256
        pr = ('gemm_kernel<%s, false>' % ('true' if p['ta'] else 'false'), 1, (cdiv(p['Nn'], 64), cdiv(p['M'], 64), 1), (256,))
        return (st, pr) if p['join'] else (pr, st)
    raise KeyError(e)


def stage_shape(p):
    """(R, C) of the matrix ggan_gemm_split stages: [A | A2] (rows of op(A) storage) or the [M, N] product"""
    if p['join']:
        return (p['K'], p['M']) if p['ta'] else (p['M'], p['K'])
    return p['M'], p['Nn']


def threads(launch):
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


# ---- rows ------------------------------------------------------------------------------------------------------------------------------
ROWS = []


def _row(entry, note='', off=None, **p):
    r = dict(entry=entry, p=p, off=off or {}, note=note)
    r['launches'] = planned(r)
    ROWS.append(r)
    return r


_NS = (1, 3, 4, 5, 1023, 1024, 1027, 4099)
_ACTS = (0, 1, 2, 3, 4, 5)
for _i, _n in enumerate(_NS):
    for _a in _ACTS:
        # every act at n = 1, 5 and 4099; the other lengths take one act each in turn
        if _n in (1, 5, 4099) or _a == _i % 6:
            _row('act_fwd', 'n %% 4 = %d, act %d' % (_n % 4, _a), n=_n, act=_a)
            _row('act_bwd', 'n %% 4 = %d, act %d, a tenth of ref +-0' % (_n % 4, _a), n=_n, act=_a)
_row('act_fwd', 'the capped grid: several trips of the float4 loop and a tail', n=ACT_BIG, act=ACT_TANH)
_row('act_bwd', 'the capped grid: several trips of the float4 loop and a tail', n=ACT_BIG, act=ACT_SIGMOID)

for _N, _C, _HW, _cap, _a, _note in (
        (3, 600, 4, 1800, ACT_LRELU, 'S bound by cdiv(512, C) = 1; C = 600; HW = 4'),
        (5, 1, 255, 64, ACT_RELU, 'S bound by N; C = 1; HW = 255: one trip of the scalar loop'),
        (40, 8, 1, 24, ACT_TANH, 'S bound by parts_cap / C = 3; ipb 14, short last slab of 12; HW = 1'),
        (200, 1, 259, 1000, ACT_SIGMOID, 'S bound by 64, ipb 4, recomputed S = 50; HW = 259: a second trip of the scalar loop'),
        (9, 100, 1028, 600, ACT_LRELU, 'first S 6, ipb 2, recomputed S = 5, last slab one image; HW = 1028: a second float4 trip'),
        (2, 3, 1024, 3, ACT_NONE, 'parts_cap == C: one slab; HW = 1024: exactly one float4 trip'),
        (7, 5, 4, 36, ACT_LRELU, 'parts_cap / C = 7 = N: every slab one image, one unused float behind the slabs')):
    _row('act_bwd_chansum', _note, N=_N, C=_C, HW=_HW, cap=_cap, act=_a)

for _s in ((1, 1, 1), (3, 5, 1), (2, 1, 7), (3, 5, 7), (1, 7, (BIG) // 7 + 1)):
    _row('bias_add', 'N C HW = %d' % (_s[0] * _s[1] * _s[2]), off=dict(x=1, bias=1, y=1), N=_s[0], C=_s[1], HW=_s[2])
_row('bias_add', 'N C HW = 2048 * 1024 + 1027 exactly: the capped grid with a ragged last trip', off=dict(x=1, bias=1, y=1), N=1, C=1, HW=BIG)

for _n, _div, _mul, _noise in ((1, 255.0, 2.0, False), (1, 256.0, 1.0, True), (257, 255.0, 2.0, False), (257, 255.0, 2.0, True),
                               (257, 256.0, 1.0, False), (257, 255.0, 3.0, False), (300, 256.0, 2.0, True), (BIG, 255.0, 2.0, True), (BIG, 256.0, 1.0, False)):
    _row('cast_scale', 'div %g mul %g noise %s' % (_div, _mul, _noise), off=dict(x=1, noise=1, y=1), n=_n, div=_div, mul=_mul, noise=_noise)

for _ns, _a, _b, _o, _noise, _note in (
        (1, 5, 7, 3, False, 'one slot'),
        (3, None, 4, 0, True, 'ctr_a NULL'),
        (3, 5, None, 0, False, 'ctr_b NULL'),
        (7, None, None, 9, True, 'both NULL: the offset alone'),
        (7, 5, -6, 0, False, 'a sum of -1: slot nslots - 1'),
        (3, 5, -6, 0, True, 'a sum of -1: slot nslots - 1'),
        (7, -10, -11, 0, False, 'a negative multiple of nslots: slot 0'),
        (7, I32_MAX, I32_MAX, 3, True, 'the sum needs 64 bits: 2^32 + 1'),
        (3, I32_MAX, I32_MAX, 3, False, 'the sum needs 64 bits: 2^32 + 1'),
        (7, I32_MIN, I32_MIN, -5, False, 'a very negative sum: -2^32 - 5')):
    _row('cast_ring', _note, off=dict(ring=1, noise=1, y=1, y2=1), n=257, nslots=_ns, ctr_a=_a, ctr_b=_b, offset=_o, noise=_noise, div=255.0, mul=2.0)

for _n in (1, 5, 1027, BIG):
    for _j, _abc in enumerate(((1.0, 1.0, 0.0), (0.5, -2.0, 0.25), (0.0, 0.0, 3.0))):
        if _n == BIG and _j != 1:
            continue
        _row('axpby', 'a b c = %s' % (_abc,), off=dict(x=1, y=1, out=1), n=_n, abc=_abc, y=True, inplace=False)
_row('axpby', 'y NULL', off=dict(x=1, out=1), n=1027, abc=(0.5, -2.0, 0.25), y=False, inplace=False)
_row('axpby', 'y NULL, out == x, n = 1: the call functional/_core.py makes', n=1, abc=(0.5, 0.0, 0.25), y=False, inplace=True)
_row('axpby', 'out == x with y given', off=dict(x=1, y=1), n=5, abc=(0.5, -2.0, 0.25), y=True, inplace=True)

for _r, _c, _note in ((64, 300, ''), (5, 1, 'cols 1: fdiv is the identity'), (3, 2, ''), (7, 3, ''), (3999, 1000, 'rows cols^2 = 3.999e9'),
                      (1, 63245, 'the top of the FastDiv range: one row, cols^2 = 3 999 930 025'),
                      (1, 63246, 'cols^2 = 4 000 056 516: the 64-bit kernel'), (2, 50000, 'rows cols^2 = 5e9: the 64-bit kernel')):
    _row('row_lerp', _note, off=dict(x=1, y=1, alpha=1, out=1), rows=_r, cols=_c)

for _r in (1, 2, 257):
    for _c in (1, 63, 64, 65, 130):
        _row('colsum', '', off=dict(x=1, out=1), rows=_r, cols=_c)

for _r, _c, _ws, _note in ((127, 65, 'full', 'rows / 64 < 2: colsum'), (128, 65, 'null', 'ws NULL: colsum'),
                           (128, 65, 'short', 'ws one float short: colsum'), (128, 65, 'reserved', 'ws_bytes not above the reserved bytes: colsum'),
                           (6401, 130, 'full', 'P = 100 > 64, slab 98 short (31 rows), slab 99 empty'),
                           (65600, 3, 'full', 'P = 1024: the last slabs empty'), (128, 65, 'full', 'P = 2, a ragged second tile'),
                           (128, 64, 'full', 'P = 2, one full tile'), (200, 64, 'full', 'P = 3, slabs of 67 rows: rows % 4 != 0')):
    _row('colsum_tall', _note, off=dict(x=1, out=1), rows=_r, cols=_c, ws=_ws)

for _N, _C, _HW, _ws, _note in (
        (1, 3, 16383, 'full', 'N = 1: P = 1; 256 threads'), (1, 3, 16384, 'full', 'N = 1: P = 1; 1024 threads'),
        (1, 1100, 16383, 'full', '1024 / C = 0; 256 threads'), (1, 1100, 16384, 'full', '1024 / C = 0; 1024 threads'),
        (3, 2, 5461, 'null', 'ws NULL; N HW = 16383: 256 threads'), (4, 2, 4096, 'null', 'ws NULL; N HW = 16384: 1024 threads'),
        (3, 2, 5461, 'short', 'ws one float short; 256 threads'), (4, 2, 4096, 'short', 'ws one float short; 1024 threads'),
        (4, 2, 4096, 'reserved', 'ws_bytes not above the reserved bytes'),
        (5, 6, 1, 'full', 'P = 5; 64 threads; C % 4 = 2'), (5, 6, 255, 'full', '64 threads, scalar loop with 4 trips'),
        (5, 6, 256, 'full', '128 threads, float4'), (5, 6, 1023, 'full', '128 threads, scalar, 8 trips'),
        (5, 6, 1024, 'full', '256 threads, float4, one trip'), (5, 8, 1028, 'full', '256 threads, float4, a second trip; C % 4 = 0'),
        (400, 3, 1, 'full', 'P = 341: chansum_final_k walks six partials per lane'),
        (70, 5, 4, 'full', 'P = 70 > 64: lanes 0..5 add two partials')):
    _row('chansum', _note, N=_N, C=_C, HW=_HW, ws=_ws)

for _n in (1, 5, 1027, BIG):
    _row('reparam_fwd', '', off=dict(mean=1, log_std=1, eps=1, z=1, sd=1), n=_n)
    for _gz, _gsd in ((True, True), (False, True), (True, False)):
        if _n == BIG and not (_gz and _gsd):
            continue
        _row('reparam_bwd', 'gz %s gsd %s' % (_gz, _gsd), off=dict(gz=1, gsd=1, eps=1, sd=1, gmean=1, glog=1), n=_n, gz=_gz, gsd=_gsd)

for _join, _ta, _M, _N, _K, _split, _note in (
        (True, 0, 15, 4, 17, 1, 'R C = 255, split 1'), (True, 0, 16, 3, 16, 15, 'R C = 256, split C - 1'),
        (True, 1, 257, 3, 1, 1, 'R C = 257 (ta: the sources split the output rows), split 1'),
        (True, 0, 15, 4, 17, 16, 'R C = 255, split C - 1'),
        (False, 0, 15, 17, 5, 16, 'R C = 255, split C - 1'), (False, 0, 16, 16, 5, 1, 'R C = 256, split 1'),
        (False, 0, 1, 257, 5, 1, 'R C = 257, split 1')):
    _row('stage', _note, join=_join, ta=_ta, M=_M, Nn=_N, K=_K, split=_split)


def row_id(row):
    p = row['p']
    parts = []
    for k in sorted(p):
        v = p[k]
        if isinstance(v, (tuple, list)):
            v = 'x'.join('%g' % x for x in v)
        elif isinstance(v, float):
            v = '%g' % v
        parts.append('%s%s' % (k, v))
    return re.sub(r'[^0-9A-Za-z_.+-]+', '_', row['entry'] + '-' + '-'.join(parts))


def by_id(rid):
    hits = [r for r in ROWS if row_id(r) == rid]
    assert len(hits) == 1, rid
    return hits[0]


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
def buffers(row):
    """-> [(name, 'in' | 'out', dtype, elements)] of the row's device buffers (offsets: row['off'])"""
    e, p = row['entry'], row['p']
    F, I = np.float32, np.int32
    if e == 'act_fwd':
        return [('x', 'in', F, p['n']), ('y', 'out', F, p['n'])]
    if e == 'act_bwd':
        return [('gy', 'in', F, p['n']), ('ref', 'in', F, p['n']), ('gx', 'out', F, p['n'])]
    if e == 'act_bwd_chansum':
        n = p['N'] * p['C'] * p['HW']
        return [('gy', 'in', F, n), ('ref', 'in', F, n), ('gx', 'out', F, n), ('gx2', 'out', F, n), ('parts', 'out', F, p['cap'])]
    if e == 'bias_add':
        n = p['N'] * p['C'] * p['HW']
        return [('x', 'in', F, n), ('bias', 'in', F, p['C']), ('y', 'out', F, n)]
    if e == 'cast_scale':
        return [('x', 'in', I, p['n'])] + ([('noise', 'in', F, p['n'])] if p['noise'] else []) + [('y', 'out', F, p['n'])]
    if e == 'cast_ring':
        return ([('ring', 'in', I, p['n'] * p['nslots'])] + ([('noise', 'in', F, p['n'])] if p['noise'] else []) +
                [('ctr', 'in', I, 2), ('y', 'out', F, p['n']), ('y2', 'out', F, p['n'])])
    if e == 'axpby':
        return ([('x', 'in', F, p['n'])] + ([('y', 'in', F, p['n'])] if p['y'] else []) + ([] if p['inplace'] else [('out', 'out', F, p['n'])]))
    if e == 'row_lerp':
        n = p['rows'] * p['cols']
        return [('x', 'in', F, n), ('y', 'in', F, n), ('alpha', 'in', F, p['rows']), ('out', 'out', F, n)]
    if e in ('colsum', 'colsum_tall'):
        return [('x', 'in', F, p['rows'] * p['cols']), ('out', 'out', F, p['cols'])]
    if e == 'chansum':
        return [('x', 'in', F, p['N'] * p['C'] * p['HW']), ('out', 'out', F, p['C'])]
    if e == 'reparam_fwd':
        return [(k, 'in', F, p['n']) for k in ('mean', 'log_std', 'eps')] + [('z', 'out', F, p['n']), ('sd', 'out', F, p['n'])]
    if e == 'reparam_bwd':
        return ([(k, 'in', F, p['n']) for k, on in (('gz', p['gz']), ('gsd', p['gsd']), ('eps', True), ('sd', True)) if on] +
                [('gmean', 'out', F, p['n']), ('glog', 'out', F, p['n'])])
    if e == 'stage':
        M, N, K, sp = p['M'], p['Nn'], p['K'], p['split']
        if p['join']:
            R, Ct = stage_shape(p)
            return [('A', 'in', F, R * sp), ('A2', 'in', F, R * (Ct - sp)), ('B', 'in', F, K * N), ('C', 'out', F, M * N)]
        return [('A', 'in', F, M * K), ('B', 'in', F, K * N), ('C', 'out', F, M * sp), ('C2', 'out', F, M * (N - sp))]
    raise KeyError(e)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
PLANTED = np.asarray([0.0, -0.0, 1e-6, -1e-6, 20.0, -20.0, 80.0, -80.0, 100.0, -100.0, 1e4, -1e4], np.float32)
CAST_EDGES = np.asarray(list(range(256)) + [-1, -255, -256, -1000, 2 ** 24 + 1, -(2 ** 24) - 1, I32_MIN, I32_MAX, I32_MAX - 1], np.int32)


def _plant(rng, a, values, n_first=True):
    """values at random positions (the first elements too when the array is short, so that n = 1, 3, 4, 5 see some of them)"""
    n = a.size
    if n >= 4 * values.size:
        pos = rng.choice(n, size=values.size, replace=False)
        a[pos] = values
    else:
        k = rng.integers(0, values.size)
        a[:] = np.resize(np.roll(values, -k), n) if n_first else a
    return a


def _normal3(rng, n):
    return (3.0 * rng.standard_normal(n)).astype(np.float32)


def _zero_tenth(rng, a):
    z = rng.random(a.size) < 0.1
    a[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    return a


def fwd_stand_in(x, act):
    """a forward output in float32 (correctly rounded from float64): what act_bwd's `ref` is for tanh and sigmoid"""
    x64 = x.astype(np.float64)
    if act == ACT_TANH:
        return np.tanh(x64).astype(np.float32)
    if act == ACT_SIGMOID:
        return (1.0 / (1.0 + np.exp(-np.maximum(x64, -80.0)))).astype(np.float32)
    return x


def _ints(rng, n):
    """every int of 0..255 first, then the edge values (as many as fit: n = 257 holds one of them, chosen by the seed), then pixels"""
    a = rng.integers(0, 256, size=n).astype(np.int32)
    k = int(rng.integers(0, 9))
    edges = np.roll(CAST_EDGES[256:], -k)
    if n >= 256:
        a[:256] = CAST_EDGES[:256]
        m = min(n - 256, edges.size)
        a[256:256 + m] = edges[:m]
    else:
        a[:] = np.resize(edges, n)
    return a


def inputs(row, seed):
    """-> {buffer name: host array} of the row's 'in' buffers (and 'alpha', the slope, where the entry takes one)"""
    rng = np.random.default_rng(seed)
    e, p = row['entry'], row['p']
    if e == 'act_fwd':
        return dict(x=_plant(rng, _normal3(rng, p['n']), PLANTED))
    if e in ('act_bwd', 'act_bwd_chansum'):
        n = p['n'] if e == 'act_bwd' else p['N'] * p['C'] * p['HW']
        ref = fwd_stand_in(_plant(rng, _normal3(rng, n), PLANTED), p['act'])
        gy = _plant(rng, _normal3(rng, n), np.asarray([0.0, -0.0, 20.0, -20.0, 1e4, -1e4], np.float32), n_first=False)
        return dict(gy=gy, ref=_zero_tenth(rng, ref))
    if e == 'bias_add':
        return dict(x=_normal3(rng, p['N'] * p['C'] * p['HW']), bias=_normal3(rng, p['C']))
    if e == 'cast_scale':
        d = dict(x=_ints(rng, p['n']))
        if p['noise']:
            d['noise'] = rng.uniform(0.0, 1.0 / 128, p['n']).astype(np.float32)
        return d
    if e == 'cast_ring':
        ring = np.concatenate([np.roll(_ints(rng, p['n']), 37 * s) + np.int32(0) for s in range(p['nslots'])])
        ring[p['n'] - 1::p['n']] = np.arange(p['nslots'], dtype=np.int32) + 1000         # (no two slots alike, whatever the roll)
        d = dict(ring=ring, ctr=np.asarray([p['ctr_a'] or 0, p['ctr_b'] or 0], np.int64).astype(np.int32))
        if p['noise']:
            d['noise'] = rng.uniform(0.0, 1.0 / 128, p['n']).astype(np.float32)
        return d
    if e == 'axpby':
        d = dict(x=_normal3(rng, p['n']))
        if p['y']:
            d['y'] = _normal3(rng, p['n'])
        return d
    if e == 'row_lerp':
        n = p['rows'] * p['cols']
        alpha = rng.uniform(0, 1, p['rows']).astype(np.float32)
        alpha[::3] = 0.0
        if p['rows'] > 1:
            alpha[1::3] = 1.0
        return dict(x=rng.standard_normal(n).astype(np.float32), y=rng.standard_normal(n).astype(np.float32), alpha=alpha)
    if e in ('colsum', 'colsum_tall'):
        return dict(x=rng.standard_normal(p['rows'] * p['cols']).astype(np.float32))
    if e == 'chansum':
        return dict(x=rng.standard_normal(p['N'] * p['C'] * p['HW']).astype(np.float32))
    if e in ('reparam_fwd', 'reparam_bwd'):
        n = p['n']
        ls = rng.uniform(-20.0, 80.0, n).astype(np.float32)
        _plant(rng, ls, np.asarray([0.0, -0.0, -20.0, 80.0, 1e-6, -1e-6], np.float32))
        eps = rng.standard_normal(n).astype(np.float32)
        if e == 'reparam_fwd':
            return dict(mean=rng.standard_normal(n).astype(np.float32), log_std=ls, eps=eps)
        d = dict(eps=eps, sd=np.exp(ls.astype(np.float64)).astype(np.float32))
        if p['gz']:
            d['gz'] = _plant(rng, rng.standard_normal(n).astype(np.float32), np.asarray([0.0, -0.0], np.float32), n_first=False)
        if p['gsd']:
            d['gsd'] = rng.standard_normal(n).astype(np.float32)
        return d
    if e == 'stage':
        M, N, K, sp = p['M'], p['Nn'], p['K'], p['split']
        tern = lambda shape: rng.integers(-1, 2, size=shape).astype(np.float32)
        B = tern((K, N))
        if p['join']:
            R, Ct = stage_shape(p)
            whole = tern((R, Ct))
            return dict(A=np.ascontiguousarray(whole[:, :sp]).ravel(), A2=np.ascontiguousarray(whole[:, sp:]).ravel(), B=B.ravel(), whole=whole)
        return dict(A=tern((M, K)).ravel(), B=B.ravel())
    raise KeyError(e)


# ---- the kernels in float32 numpy, in their own order (mutant: one of MUTANTS) --------------------------------------------------------------
def _nan(n):
    return np.full(n, np.nan, np.float32)


def _stride_cover(n, grid, block, mutant, which):
    """elements a grid-stride loop of `grid` x `block` threads reaches; the one-trip mutants stop after the first trip"""
    reach = np.ones(n, bool)
    if mutant == which:
        reach[grid * block:] = False
    return reach


def act_apply32(x, act, alpha=ALPHA, mutant=None):
    a = f32(alpha)
    if act == ACT_LRELU:
        return a * x if mutant == 'lrelu_always_alpha' else np.maximum(a * x, x)
    if act == ACT_RELU:
        return np.where(x > 0, x, f32(0))
    if act == ACT_TANH:
        return np.tanh(x.astype(np.float64)).astype(np.float32)
    if act == ACT_SIGMOID:
        with np.errstate(over='ignore'):
            e = np.exp(-x.astype(np.float64)).astype(np.float32)
            return f32(1) / (f32(1) + e)
    return x.copy()


def act_grad32(g, r, act, alpha=ALPHA, mutant=None):
    a = f32(alpha)
    pos = (r >= 0) if mutant == 'act_grad_ge' else (r > 0)
    if act == ACT_LRELU:
        return np.where(pos, g, a * g)
    if act == ACT_RELU:
        return np.where(pos, g, f32(0))
    if act == ACT_TANH:
        return g * (f32(1) - r * r)
    if act == ACT_SIGMOID:
        return g * r if mutant == 'sigmoid_grad_without_1_minus_r' else g * r * (f32(1) - r)
    return g.copy()


def _act_cover(n, mutant):
    """act_fwd_k / act_bwd_k: the float4 loop over n >> 2 groups, then the tail from (n4 << 2) + i (at most 3 elements: one trip)"""
    grid = grid_for(n, ACT_PER_THREAD)
    reach = np.ones(n, bool)
    if mutant == 'float4_one_trip':
        reach[4 * grid * K_BLOCK:4 * (n >> 2)] = False
    return reach


def wave_sum32(v):
    """the xor butterfly over the last axis (64 lanes) -> lane 0's value"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _thread_sums(planes, nthreads):
    """planes [..., images, HW] -> [..., nthreads]: thread t adds, image after image, elements t, t + nthreads, ... of each plane (as
    (x+y)+(z+w) groups of four when HW % 4 == 0); a missing trip adds +0, which changes no float32 sum"""
    HW = planes.shape[-1]
    if HW % 4 == 0:
        q = planes.reshape(planes.shape[:-1] + (HW // 4, 4))
        planes = (q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3])
    L = planes.shape[-1]
    trips = cdiv(L, nthreads)
    padded = np.zeros(planes.shape[:-1] + (trips * nthreads,), np.float32)
    padded[..., :L] = planes
    padded = padded.reshape(planes.shape[:-1] + (trips, nthreads))
    acc = np.zeros(planes.shape[:-2] + (nthreads,), np.float32)
    for i in range(planes.shape[-2]):
        for t in range(trips):
            acc = acc + padded[..., i, t, :]
    return acc


def block_sum32(acc):
    """wave_sum per 64 lanes, then block_sum's serial loop over the waves"""
    w = wave_sum32(acc.reshape(acc.shape[:-1] + (acc.shape[-1] // 64, 64)))
    t = np.zeros(w.shape[:-1], np.float32)
    for i in range(w.shape[-1]):
        t = t + w[..., i]
    return t


def chansum_part32(x, N, C, HW, P, nthreads, mutant=None):
    """chansum_part_k -> part[C, P]: block (c, p) sums the planes p, p + P, ... of channel c"""
    x = x.reshape(N, C, HW)
    k = cdiv(N, P)
    planes = np.zeros((C, P, k, HW), np.float32)
    for p in range(P):
        imgs = x[p::P]                                   # [images of p, C, HW]
        planes[:, p, :imgs.shape[0], :] = imgs.transpose(1, 0, 2)
    return block_sum32(_thread_sums(planes, nthreads))


def final32(part, mutant=None):
    """chansum_final_k: part[C, P] -> out[C]; lane l adds partials l, l + 64, ...; the butterfly"""
    C, P = part.shape
    if mutant == 'final_transposed':
        part = part.ravel()[:C * P].reshape(P, C).T          # reads part[p * C + c]
    if mutant == 'final_stops_at_64':
        part = part[:, :64]
        P = part.shape[1]
    k = cdiv(P, 64)
    padded = np.zeros((C, k * 64), np.float32)
    padded[:, :P] = part
    padded = padded.reshape(C, k, 64)
    s = np.zeros((C, 64), np.float32)
    for i in range(k):
        s = s + padded[:, i]
    return wave_sum32(s)


def colsum32(x, rows, cols):
    x = x.reshape(rows, cols)
    s = np.zeros(cols, np.float32)
    for r in range(rows):
        s = s + x[r]
    return s


def colsum_part32(x, rows, cols, rps, P, mutant=None):
    """colsum_part_k -> part[cols, P]: four row lanes, (sm0 + sm1) + (sm2 + sm3)"""
    x = x.reshape(rows, cols)
    k = cdiv(rps, 4)
    padded = np.zeros((P, k * 4, cols), np.float32)
    for p in range(P):
        r0, r1 = p * rps, min(rows, p * rps + rps)
        if r1 > r0:
            padded[p, :r1 - r0] = x[r0:r1]
    padded = padded.reshape(P, k, 4, cols)
    s = np.zeros((P, 4, cols), np.float32)
    for i in range(k):
        s = s + padded[:, i]
    part = ((s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])).T.copy()
    if mutant == 'empty_slab_stale':
        for p in range(P):
            if p * rps >= rows:
                part[:, p] = np.nan                      # the scratch's previous content
    return part


def cast_scale32(x, noise, div, mul, mutant=None, fused=False):
    xf = x.astype(np.float32)
    if mutant == 'cast_scale_reordered':
        v = f32(mul) * xf / f32(div) - f32(0.5) * f32(mul)
    else:
        t = xf / f32(div) - f32(0.5)
        if noise is not None and fused:
            return (f32(mul).astype(np.float64) * t.astype(np.float64) + noise.astype(np.float64)).astype(np.float32)
        v = f32(mul) * t
    return v + noise if noise is not None else v


def ring_slot(p, mutant=None):
    a = (1 if mutant == 'null_counter_is_1' else 0) if p['ctr_a'] is None else p['ctr_a']
    b = (1 if mutant == 'null_counter_is_1' else 0) if p['ctr_b'] is None else p['ctr_b']
    c = p['offset'] + a + b
    if mutant == 'counter_sum_32bit':
        c = (c + 2 ** 31) % 2 ** 32 - 2 ** 31
    if mutant == 'ring_without_plus_nslots':
        return int(np.fmod(c, p['nslots']))              # C's %: the sign of the dividend
    return c % p['nslots']


def make_fastdiv(d):
    return (0 if d <= 1 else (2 ** 32 // d + 1) & 0xFFFFFFFF), d


def fdiv(n, fd, mutant=None):
    """n: uint64 array of 32-bit values"""
    mul, d = fd
    if d <= 1:
        return n
    if mutant == 'fdiv_multiplier_minus_1':
        mul -= 1
    return (n * np.uint64(mul)) >> np.uint64(32)


def run32(row, inp, mutant=None):
    """-> {output name: float32 array}: what the row's kernels compute, restated in float32 numpy"""
    e, p = row['entry'], row['p']
    if e == 'act_fwd':
        reach = _act_cover(p['n'], mutant)
        return dict(y=np.where(reach, act_apply32(inp['x'], p['act'], mutant=mutant), f32('nan')))
    if e == 'act_bwd':
        reach = _act_cover(p['n'], mutant)
        return dict(gx=np.where(reach, act_grad32(inp['gy'], inp['ref'], p['act'], mutant=mutant), f32('nan')))
    if e == 'act_bwd_chansum':
        N, C, HW, cap = p['N'], p['C'], p['HW'], p['cap']
        S0, _, ipb, S = abc_plan(N, C, cap)
        if mutant == 'ipb_from_first_S':
            ipb = cdiv(N, cdiv(ABC_SPREAD, C))                          # the S before its clamps
        full = act_grad32(inp['gy'], inp['ref'], p['act'], mutant=mutant).reshape(N, C, HW)
        g3 = np.full((N, C, HW), np.nan, np.float32)
        reach = np.ones(HW, bool)
        if mutant == 'abc_float4_one_trip' and HW % 4 == 0:
            reach[4 * ABC_THREADS:] = False
        if mutant == 'abc_scalar_one_trip' and HW % 4 != 0:
            reach[ABC_THREADS:] = False
        parts = _nan(cap)
        for s in range(S):
            n0, n1 = s * ipb, min(s * ipb + ipb, N)
            g3[n0:n1] = np.where(reach, full[n0:n1], f32('nan'))
            planes = np.where(reach, full[n0:n1], f32(0)).transpose(1, 0, 2)                       # [C, images, HW]
            w = wave_sum32(_thread_sums(planes, ABC_THREADS).reshape(C, 4, 64))
            v = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
            if mutant == 'parts_indexed_c_S':
                parts[np.arange(C) * S + s] = v
            else:
                parts[s * C:(s + 1) * C] = v
        gx = g3.ravel()
        return dict(gx=gx, gx2=act_grad32(inp['gy'], inp['ref'], p['act']), parts=parts, n_parts=S)
    if e == 'bias_add':
        n = p['N'] * p['C'] * p['HW']
        j = np.arange(n)
        c = (j % p['C']) if mutant == 'bias_index_j_mod_C' else (j // p['HW']) % p['C']
        y = inp['x'] + inp['bias'][c]
        reach = _stride_cover(n, grid_for(n), K_BLOCK, mutant, 'scalar_one_trip')
        return dict(y=np.where(reach, y, f32('nan')))
    if e == 'cast_scale':
        return dict(y=cast_scale32(inp['x'], inp.get('noise'), p['div'], p['mul'], mutant))
    if e == 'cast_ring':
        slot = ring_slot(p, mutant)
        y2 = cast_scale32(inp['ring'][ring_slot(p) * p['n']:][:p['n']], inp.get('noise'), p['div'], p['mul'])
        if slot < 0:
            return dict(y=_nan(p['n']), y2=y2, ctr=inp['ctr'].copy())         # (reads in front of the ring)
        return dict(y=cast_scale32(inp['ring'][slot * p['n']:][:p['n']], inp.get('noise'), p['div'], p['mul']), y2=y2, ctr=inp['ctr'].copy())
    if e == 'axpby':
        a, b, c = (f32(v) for v in p['abc'])
        x = inp['x']
        y = inp.get('y', x if mutant == 'axpby_null_y_is_x' else None)
        out = a * x + (b * y if y is not None else f32(0)) + (f32(0) if mutant == 'axpby_ignores_c' else c)
        return dict(out=out.astype(np.float32))
    if e == 'row_lerp':
        rows, cols = p['rows'], p['cols']
        j = np.arange(rows * cols, dtype=np.uint64)
        if mutant == 'lerp_row_by_rows':
            r = j // np.uint64(rows)
        elif lerp_is_32(rows, cols):
            r = fdiv(j, make_fastdiv(cols), mutant)
        else:
            r = j // np.uint64(cols)
        a = inp['alpha'][np.minimum(r, np.uint64(rows - 1)).astype(np.int64)]
        out = inp['x'] + a * (inp['y'] - inp['x'])
        return dict(out=np.where(r < rows, out, f32('nan')))
    if e == 'colsum' or (e == 'colsum_tall' and tall_plan(row) is None):
        return dict(out=colsum32(inp['x'], p['rows'], p['cols']))
    if e == 'colsum_tall':
        P, rps = tall_plan(row)
        part = colsum_part32(inp['x'], p['rows'], p['cols'], rps, P, mutant)
        return dict(part=part.ravel(), out=final32(part, mutant))
    if e == 'chansum':
        N, C, HW = p['N'], p['C'], p['HW']
        P, nthreads = chan_plan(row)
        if mutant == 'P_without_clamp_to_N':
            P = CHAN_WGS // C
            if C * P > (ws_floats(row) or 0):                # (the workspace holds the clamped P's partials: the single-stage launch)
                P = 1
        if P <= 1:
            return dict(out=chansum_part32(inp['x'], N, C, HW, 1, nthreads)[:, 0])
        part = chansum_part32(inp['x'], N, C, HW, P, nthreads)
        return dict(part=part.ravel(), out=final32(part, mutant))
    if e == 'reparam_fwd':
        sd = np.exp(inp['log_std'].astype(np.float64)).astype(np.float32)
        z = (inp['eps'].astype(np.float64) * sd.astype(np.float64) + inp['mean'].astype(np.float64)).astype(np.float32)       # fmaf: one rounding
        reach = _stride_cover(p['n'], grid_for(p['n']), K_BLOCK, mutant, 'scalar_one_trip')
        return dict(sd=np.where(reach, sd, f32('nan')), z=np.where(reach, z, f32('nan')))
    if e == 'reparam_bwd':
        zero = np.zeros(p['n'], np.float32)
        a, b = inp.get('gz', zero), inp.get('gsd', zero)
        glog = (a * inp['eps'] + b) * inp['sd']
        if mutant == 'reparam_gsd_without_sd':
            glog = a * inp['eps'] * inp['sd'] + b
        return dict(gmean=a.copy(), glog=glog)
    if e == 'stage':
        M, N, K, sp = p['M'], p['Nn'], p['K'], p['split']
        B = inp['B'].reshape(K, N)
        if p['join']:
            opA = inp['whole'].T if p['ta'] else inp['whole']
            return dict(C=(opA @ B).astype(np.float32).ravel())
        prod = inp['A'].reshape(M, K) @ B
        return dict(C=np.ascontiguousarray(prod[:, :sp]).ravel(), C2=np.ascontiguousarray(prod[:, sp:]).ravel())
    raise KeyError(e)


# ---- float64 restatements, bounds and bitwise stages ------------------------------------------------------------------------------------
def d64(a):
    return np.asarray(a, np.float64)


def _frac(err, bound):
    """worst err / bound; an error where the bound is 0 counts as infinite, and so does every element whose error or bound is not finite"""
    err, bound = np.atleast_1d(d64(err)), np.atleast_1d(d64(bound))
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    f = np.where(np.isfinite(err) & np.isfinite(bound), f, np.inf)
    return float(np.max(f))


def _bits(got, want):
    """0.0 where the two float32 (or int32) arrays are bit-identical, else inf"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return np.inf
    return 0.0 if np.array_equal(got.view(np.uint32), want.view(np.uint32)) else np.inf


def _floor(ref):
    return np.where(np.abs(ref) < TINY, TINY, 0.0)


def within(fr):
    return all(f <= 1.0 for f in fr.values())


def chain_threads(images, L, nthreads, float4):
    """additions one thread of a plane-summing kernel chains: images x trips (+ 2 inside a float4 group)"""
    return images * cdiv(L // 4 if float4 else L, nthreads) + (2 if float4 else 0)


def act_fwd_frac(x, y, act):
    x64, y64 = d64(x), d64(y)
    if act == ACT_LRELU:
        return _bits(y, np.maximum(f32(ALPHA) * x, x))
    if act == ACT_RELU:
        want = np.where(x > 0, x, f32(0))
        ok = (y.view(np.uint32) == want.view(np.uint32)) | ((x == 0) & (y == 0))
        return 0.0 if bool(np.all(ok)) else np.inf
    if act == ACT_TANH:
        ref = np.tanh(x64)
        return _frac(np.abs(y64 - ref), 2 * P_TANH * U * np.abs(ref) + _floor(ref))
    if act == ACT_SIGMOID:
        with np.errstate(over='ignore'):
            ref = 1.0 / (1.0 + np.exp(-x64))
        return _frac(np.abs(y64 - ref), SECOND * U * ref * (2 + 2 * P_EXP * (1 - ref)) + _floor(ref))
    return _bits(y, x)


def act_bwd_frac(g, r, gx, act):
    g64, r64, o64 = d64(g), d64(r), d64(gx)
    if act == ACT_LRELU:
        return _bits(gx, np.where(r > 0, g, f32(ALPHA) * g))
    if act == ACT_RELU:
        return _bits(gx, np.where(r > 0, g, f32(0)))
    if act == ACT_TANH:
        ref = g64 * (1 - r64 * r64)
        return _frac(np.abs(o64 - ref), SECOND * U * np.abs(g64) * (r64 * r64 + 2 * np.abs(1 - r64 * r64)) + _floor(ref))
    if act == ACT_SIGMOID:
        ref = g64 * r64 * (1 - r64)
        return _frac(np.abs(o64 - ref), SECOND * 3 * U * np.abs(ref) + TINY)
    return _bits(gx, g)


def check(row, inp, out):
    """-> {stage: worst fraction of its bound (a broken bitwise stage: inf)} for a row's outputs `out` (the device's, or run32's)"""
    e, p = row['entry'], row['p']
    fr = {}
    if e == 'act_fwd':
        fr['y'] = act_fwd_frac(inp['x'], out['y'], p['act'])
    elif e == 'act_bwd':
        fr['gx'] = act_bwd_frac(inp['gy'], inp['ref'], out['gx'], p['act'])
    elif e == 'act_bwd_chansum':
        N, C, HW, cap = p['N'], p['C'], p['HW'], p['cap']
        _, _, ipb, S = abc_plan(N, C, cap)
        fr['gx=act_bwd'] = _bits(out['gx'], out['gx2'])
        fr['gx2'] = act_bwd_frac(inp['gy'], inp['ref'], out['gx2'], p['act'])
        fr['n_parts'] = 0.0 if int(out['n_parts']) == S else np.inf
        g = d64(out['gx']).reshape(N, C, HW)
        parts = d64(out['parts'])
        worst = 0.0
        for s in range(S):
            sl = g[s * ipb:min(N, s * ipb + ipb)]
            k = chain_threads(sl.shape[0], HW, ABC_THREADS, HW % 4 == 0) + 6 + 2
            worst = max(worst, _frac(np.abs(parts[s * C:(s + 1) * C] - sl.sum((0, 2))), k * U * np.abs(sl).sum((0, 2)) + TINY))
        fr['parts'] = worst
        fr['unused slabs'] = 0.0 if bool(np.all(np.isnan(out['parts'][S * C:]))) else np.inf
    elif e == 'bias_add':
        c = (np.arange(inp['x'].size) // p['HW']) % p['C']
        fr['y'] = _bits(out['y'], inp['x'] + inp['bias'][c])
    elif e == 'cast_scale':
        noise = inp.get('noise')
        fr['y'] = min(_bits(out['y'], cast_scale32(inp['x'], noise, p['div'], p['mul'])),
                      _bits(out['y'], cast_scale32(inp['x'], noise, p['div'], p['mul'], fused=True)) if noise is not None else np.inf)
    elif e == 'cast_ring':
        slot = ring_slot(p)
        x = inp['ring'][slot * p['n']:][:p['n']]
        fr['y=cast_scale(slot)'] = _bits(out['y'], out['y2'])
        noise = inp.get('noise')
        fr['y2'] = min(_bits(out['y2'], cast_scale32(x, noise, p['div'], p['mul'])),
                       _bits(out['y2'], cast_scale32(x, noise, p['div'], p['mul'], fused=True)) if noise is not None else np.inf)
        fr['ctr'] = _bits(out['ctr'], inp['ctr'])
    elif e == 'axpby':
        a, b, c = (float(f32(v)) for v in p['abc'])
        x, y = d64(inp['x']), d64(inp['y']) if p['y'] else 0.0
        ref = a * x + b * y + c
        fr['out'] = _frac(np.abs(d64(out['out']) - ref), SECOND * U * (3 * np.abs(a * x) + 3 * np.abs(b * y) + abs(c)) + _floor(ref))
        if a == 0 and b == 0:
            fr['out=c'] = _bits(out['out'], np.full(p['n'], f32(c)))
    elif e == 'row_lerp':
        rows, cols = p['rows'], p['cols']
        a = np.repeat(inp['alpha'], cols)
        x, y, a64 = d64(inp['x']), d64(inp['y']), d64(a)
        ref = x + a64 * (y - x)
        fr['out'] = _frac(np.abs(d64(out['out']) - ref), SECOND * U * (2 * np.abs(a64 * (y - x)) + np.abs(ref)) + _floor(ref))
        fr['alpha=0'] = _bits(out['out'][a == 0], inp['x'][a == 0])
    elif e == 'colsum' or (e == 'colsum_tall' and tall_plan(row) is None):
        x = d64(inp['x']).reshape(p['rows'], p['cols'])
        fr['out'] = _frac(np.abs(d64(out['out']) - x.sum(0)), p['rows'] * U * np.abs(x).sum(0) + TINY)
        if e == 'colsum_tall':
            fr['fallback'] = 0.0 if 'part' not in out else np.inf
    elif e == 'colsum_tall':
        rows, cols = p['rows'], p['cols']
        P, rps = tall_plan(row)
        x = d64(inp['x']).reshape(rows, cols)
        part = np.asarray(out['part'], np.float32)[:cols * P].reshape(cols, P)
        k = cdiv(rps, 4) + 2
        worst, empty_ok = 0.0, True
        for q in range(P):
            sl = x[q * rps:min(rows, q * rps + rps)]
            if sl.shape[0] == 0:
                empty_ok = empty_ok and _bits(part[:, q], np.zeros(cols, np.float32)) == 0.0
                continue
            worst = max(worst, _frac(np.abs(d64(part[:, q]) - sl.sum(0)), k * U * np.abs(sl).sum(0) + TINY))
        fr['part'] = worst
        fr['empty slab +0'] = 0.0 if empty_ok else np.inf
        fr['out=final(part)'] = _bits(out['out'], final32(part))
    elif e == 'chansum':
        N, C, HW = p['N'], p['C'], p['HW']
        P, nthreads = chan_plan(row)
        x = d64(inp['x']).reshape(N, C, HW)
        f4 = HW % 4 == 0
        if P <= 1:
            k = chain_threads(N, HW, nthreads, f4) + 6 + nthreads // 64
            fr['out'] = _frac(np.abs(d64(out['out']) - x.sum((0, 2))), k * U * np.abs(x).sum((0, 2)) + TINY)
            fr['one stage'] = 0.0 if 'part' not in out else np.inf
        else:
            if 'part' not in out:
                return {'two stages': np.inf}
            part = np.asarray(out['part'], np.float32)[:C * P].reshape(C, P)
            k = chain_threads(cdiv(N, P), HW, nthreads, f4) + 6 + nthreads // 64
            ref = np.stack([x[q::P].sum((0, 2)) for q in range(P)], 1)
            mag = np.stack([np.abs(x[q::P]).sum((0, 2)) for q in range(P)], 1)
            fr['part'] = _frac(np.abs(d64(part) - ref), k * U * mag + TINY)
            fr['out=final(part)'] = _bits(out['out'], final32(part))
    elif e == 'reparam_fwd':
        ls, sd = d64(inp['log_std']), d64(out['sd'])
        ref = np.exp(ls)
        fr['sd'] = _frac(np.abs(sd - ref), 2 * P_EXP * U * ref + _floor(ref))
        z = d64(inp['eps']) * sd + d64(inp['mean'])
        fr['z'] = _frac(np.abs(d64(out['z']) - z), SECOND * U * np.abs(z) + TINY)
    elif e == 'reparam_bwd':
        zero = np.zeros(p['n'], np.float32)
        a, b = inp.get('gz', zero), inp.get('gsd', zero)
        fr['gmean'] = _bits(out['gmean'], a)
        ae = d64(a) * d64(inp['eps'])
        ref = (ae + d64(b)) * d64(inp['sd'])
        fr['glog'] = _frac(np.abs(d64(out['glog']) - ref), SECOND * U * d64(inp['sd']) * (np.abs(ae) + 2 * np.abs(ae + d64(b))) + _floor(ref))
    elif e == 'stage':
        want = run32(row, inp)
        for key in want:
            fr[key] = _bits(out[key], want[key])
    else:
        raise KeyError(e)
    return fr


# ---- wrong kernels the rows must tell from the right one (test_pointwise_dispatch_cpu.py) -----------------------------------------------
def _rid(entry, **match):
    hits = [r for r in ROWS if r['entry'] == entry and all(r['p'].get(k) == v for k, v in match.items())]
    assert hits, (entry, match)
    return row_id(hits[0])


MUTANT_ROW = {
    'float4_one_trip': _rid('act_fwd', n=ACT_BIG),
    'scalar_one_trip': _rid('bias_add', HW=BIG),
    'abc_float4_one_trip': _rid('act_bwd_chansum', HW=1028),
    'abc_scalar_one_trip': _rid('act_bwd_chansum', HW=259),
    'act_grad_ge': _rid('act_bwd', n=4099, act=ACT_LRELU),
    'lrelu_always_alpha': _rid('act_fwd', n=4099, act=ACT_LRELU),
    'sigmoid_grad_without_1_minus_r': _rid('act_bwd', n=4099, act=ACT_SIGMOID),
    'bias_index_j_mod_C': _rid('bias_add', N=3, C=5, HW=7),
    'ring_without_plus_nslots': _rid('cast_ring', nslots=7, ctr_a=5, ctr_b=-6),
    'null_counter_is_1': _rid('cast_ring', nslots=3, ctr_a=None),
    'counter_sum_32bit': _rid('cast_ring', nslots=7, ctr_a=I32_MAX),
    # (mul = 2 and 1 are powers of two: the reordered product is the same float there; a row with mul = 3 tells it apart)
    'cast_scale_reordered': _rid('cast_scale', n=257, noise=False, mul=3.0),
    'axpby_ignores_c': _rid('axpby', n=5, abc=(0.5, -2.0, 0.25), inplace=False),
    'axpby_null_y_is_x': _rid('axpby', n=1027, y=False),
    'lerp_row_by_rows': _rid('row_lerp', rows=7, cols=3),
    'fdiv_multiplier_minus_1': _rid('row_lerp', rows=64, cols=300),
    'ipb_from_first_S': _rid('act_bwd_chansum', N=200),
    'parts_indexed_c_S': _rid('act_bwd_chansum', N=40),
    'empty_slab_stale': _rid('colsum_tall', rows=6401),
    'final_transposed': _rid('chansum', N=5, HW=255),
    'final_stops_at_64': _rid('chansum', N=400),
    'P_without_clamp_to_N': _rid('chansum', N=5, HW=1),
    'reparam_gsd_without_sd': _rid('reparam_bwd', n=1027, gz=True, gsd=True),
}
MUTANTS = tuple(MUTANT_ROW)
# Two wrong kernels the issue of this table asked for compute the same outputs as the right one, so no row can tell them apart
# (test_pointwise_dispatch_cpu.py asserts the reasons): the tail of act_fwd_k / act_bwd_k holds at most 3 elements and the smallest grid
# 256 threads, so a tail loop that stops after one trip is the same kernel ('tail_one_trip'); and a tail that starts at n4 + i instead
# of (n4 << 2) + i strides on to n all the same -- it recomputes elements the float4 loop already stored, with the same values, and still
# reaches the last three ('tail_from_n4').  The loops that can stop early are the float4 body, the scalar kernels, and the two loops of
# act_bwd_chansum_k: each has its mutant above.
EQUIVALENT_MUTANTS = ('tail_one_trip', 'tail_from_n4')


# ---- argument errors and empty calls (both modules make them: the answer comes before anything touches a device) -----------------------
# An argument is a number, None (NULL), 'pK' (buffer K of the caller's), ('pK', bytes) (that pointer moved off its boundary) or 'np'
# (an int the entry point may write *n_parts to).  GOOD: a call every check accepts; REQUIRED: the positions of its required pointers.
GOOD = {
    'ggan_act_fwd': ['p0', 'p1', 64, 1, ALPHA],
    'ggan_act_bwd': ['p0', 'p1', 'p2', 64, 1, ALPHA],
    'ggan_act_bwd_chansum': ['p0', 'p1', 'p2', 'p3', 8, 'np', 2, 4, 8, 1, ALPHA],
    'ggan_bias_add': ['p0', 'p1', 'p2', 2, 4, 8],
    'ggan_cast_scale_i32': ['p0', None, 'p1', 64, 255.0, 2.0],
    'ggan_cast_scale_ring_i32': ['p0', 3, None, None, 0, None, 'p1', 16, 255.0, 2.0],
    'ggan_axpby': ['p0', None, 'p1', 64, 1.0, 1.0, 0.0],
    'ggan_row_lerp': ['p0', 'p1', 'p2', 'p3', 4, 16],
    'ggan_colsum': ['p0', 'p1', 4, 16],
    'ggan_colsum_tall': ['p0', 'p1', 4, 16, None, 0],
    'ggan_chansum': ['p0', 'p1', 2, 4, 8, None, 0],
    'ggan_reparam_fwd': ['p0', 'p1', 'p2', 'p3', 'p4', 64],
    'ggan_reparam_bwd': ['p0', 'p1', 'p2', 'p3', 'p4', 'p5', 64],
}
REQUIRED = {
    'ggan_act_fwd': (0, 1), 'ggan_act_bwd': (0, 1, 2), 'ggan_act_bwd_chansum': (0, 1, 2, 3, 5), 'ggan_bias_add': (0, 1, 2),
    'ggan_cast_scale_i32': (0, 2), 'ggan_cast_scale_ring_i32': (0, 6), 'ggan_axpby': (0, 2), 'ggan_row_lerp': (0, 1, 2, 3),
    'ggan_colsum': (0, 1), 'ggan_colsum_tall': (0, 1), 'ggan_chansum': (0, 1), 'ggan_reparam_fwd': (0, 1, 2, 3, 4),
    'ggan_reparam_bwd': (2, 3, 4, 5),
}


def _with(fn, **at):
    a = list(GOOD[fn])
    for k, v in at.items():
        a[int(k[1:])] = v
    return fn, tuple(a)


_BAD_ARGUMENT = ('ggan_bias_add', 'ggan_cast_scale_ring_i32', 'ggan_row_lerp', 'ggan_colsum', 'ggan_colsum_tall', 'ggan_chansum')      # one message for all
REJECTED = [_with(fn, **{'a%d' % i: None}) + ('bad argument' if fn in _BAD_ARGUMENT else 'null pointer',) for fn in GOOD for i in REQUIRED[fn]]
REJECTED += [_with('ggan_act_fwd', **{'a%d' % i: ('p%d' % i, 4)}) + ('aligned',) for i in (0, 1)]
REJECTED += [_with('ggan_act_bwd', **{'a%d' % i: ('p%d' % i, 4)}) + ('aligned',) for i in (0, 1, 2)]
REJECTED += [_with('ggan_act_bwd_chansum', **{'a%d' % i: ('p%d' % i, 4)}) + ('aligned',) for i in (0, 1, 2)]
REJECTED += [_with('ggan_act_bwd_chansum', a4=3) + ('shape',)]                      # parts_cap < C
REJECTED += [_with('ggan_act_bwd_chansum', **{'a%d' % i: v}) + ('shape',) for i in (6, 7, 8) for v in (0, -1)]
REJECTED += [_with('ggan_bias_add', **{'a%d' % i: 0}) + ('bad',) for i in (3, 4, 5)]
REJECTED += [_with('ggan_cast_scale_ring_i32', a1=v) + ('bad',) for v in (0, -1)]
REJECTED += [_with(fn, **{'a%d' % i: v}) + ('bad',) for fn, ii in (('ggan_row_lerp', (4, 5)), ('ggan_colsum', (2, 3)), ('ggan_colsum_tall', (2, 3)),
                                                                  ('ggan_chansum', (2, 3, 4))) for i in ii for v in (0, -1)]
REJECTED += [_with('ggan_reparam_bwd', a0=None, a1=None) + ('null',)]
EMPTY = [_with(fn, **{'a%d' % i: 0}) for fn, i in (('ggan_act_fwd', 2), ('ggan_act_bwd', 3), ('ggan_cast_scale_i32', 3),
                                                   ('ggan_cast_scale_ring_i32', 7), ('ggan_axpby', 3), ('ggan_reparam_fwd', 5), ('ggan_reparam_bwd', 6))]
# (ggan_reparam_bwd with ONE gradient NULL is a valid call: positions 0 and 1 are not in REQUIRED)


def call(L, case, pointer):
    """make one REJECTED / EMPTY call -> (return code, message, the int behind 'np'); pointer(K) -> address of the caller's buffer K"""
    import ctypes as C
    fn, args = case[0], case[1]
    n_parts = C.c_int(-7)
    real = []
    for a in args:
        if a == 'np':
            real.append(C.pointer(n_parts))
        elif isinstance(a, str):
            real.append(C.c_void_p(pointer(int(a[1:]))))
        elif isinstance(a, tuple):
            real.append(C.c_void_p(pointer(int(a[0][1:])) + a[1]))
        elif a is None and fn == 'ggan_act_bwd_chansum' and len(real) == 5:
            real.append(C.POINTER(C.c_int)())
        else:
            real.append(a)
    rc = getattr(L, fn)(*real, None)
    return rc, (L.ggan_last_error() or b'').decode(), n_parts.value
