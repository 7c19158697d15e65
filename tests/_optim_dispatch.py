"""Which path of the optimizer tail (csrc/optim.hip: pack_k, pack_adam_k, adam_k<PRE>, rmsprop_k) each dispatch test runs: one row
per entry point and edge (plain data), the rows' inputs, the float64 restatements they are measured against, the derived bounds, and
`planned()`, a transcription of the host dispatch and of the in-kernel path predicate.

tests/test_optim_dispatch_gpu.py runs every row through the C ABI, asserts that the profiler saw exactly the row's launches with their
work-item counts (grid x block: all a profiler record holds), that the pointers it built have the alignment the row states, and checks every output in stages (below) inside sentinel-filled
buffers.  tests/test_optim_dispatch_cpu.py checks labels and constants against the source text, recomputes every row's launches with
planned(), asserts which (path, chunk, tail) combinations and arrival-group counts the table reaches, and proves on the CPU that the
rows' inputs tell sixteen wrong kernels from the right one.

A row:
  entry     pack_adam (ggan_pack_adam) | pack (ggan_pack_parts2) | adam_step (ggan_adam_step + ggan_adam_advance) |
            adam_step_counted (ggan_adam_step_counted) | rmsprop_step (ggan_rmsprop_step)
  tensors   pack / pack_adam: the tensor table, one T() per tensor --
              size            floats
              parts, stride   slabs summed into it and the floats between them (stride 0 where parts == 1)
              soff            source offset in floats from a 16-byte boundary
              src             False: the source pointer is NULL
              parts2, stride2, soff2   the second contribution (parts2 == 0: none)
              slot            offset of the tensor in flat / theta / m / v, modulo 4
  n         adam_step*, rmsprop_step: floats
  step0     the device counter before the first launch (the update's ordinal is step0 + 1; adam_step_counted: step0 itself)
  hyper     Adam: (lr, beta1, beta2, eps);  RMSProp: (lr, decay, eps)
  gscale    grad_scale
  clip      rmsprop_step: None or (lo, hi)
  repeat    launches in a row (pack_adam arrival rows: 3; pack rows with a counter: 2)
  split     pack_adam: k > 0 -- tensors [0:k] are launched with arrive == NULL, then tensors [k:] with the counters
  bump      pack: the counter is given (False: NULL)
  launches  ((label, launches, grid, block), ...): every launch the row causes (the profiler records the product of grid and block, so
            the GPU module can hold that product, not the shape; the shape is held against planned() on the CPU)
  note      which edge the row is there for

Inputs (inputs()): gradients at per-element scales 0 (exactly), 1e-6, 1e-3 and 1 -- at 1e-6 and a first step sqrt(v) is 3e-8, of eps's
size; weights at exactly 0, +-1e-3, +-1 -- at 0 the whole update is resolved to a few ulps; moments zero (step0 == 0) or warm (v >= 0,
m at the gradient's scale); nothing below 1e-15, so no denormal appears anywhere.

Stages and bounds (u = 2^-24, half an ulp relative; no stage carries another's error):
  flat    bitwise the float32 sum in slab order, src slabs then src2 slabs (0 for a missing source).
  m       against float64 from the float32 inputs: M_ROUNDINGS * u * (|b1 m| + |(1 - b1) gg|).  adam1 (csrc/optim.hip) under -ffp-contract=on rounds
          1 - b1, b1 * m, (1 - b1) * gg and the sum: 4 (a contraction removes one).  First order the error is at most
          u (2 |b1 m| + 3 |(1 - b1) gg|): what the count leaves over covers the second-order terms.
  v       likewise, V_ROUNDINGS = 5: 1 - b2, b2 * v, (1 - b2) * gg, (..) * gg, the sum; u (2 |b2 v| + 4 |(1 - b2) gg^2|) first order.
  gscale  gg = g * grad_scale adds one rounding to each count when grad_scale != 1 (v sees it twice, gg enters squared:
          u (2 |b2 v| + 6 |..|) <= 6 u (|b2 v| + |..|) still holds).
  theta   against float64 from the DEVICE's own new m and v and the float64 lr_t:
          (r_lr(t) + TH_ROUNDINGS * u) |delta| + u |theta_new|,  delta = lr_t m / (sqrt(v) + eps).
          TH_ROUNDINGS = 9: lr_t = lr * sqrtf(1 - powf(b2, t)) / (1 - powf(b1, t)) rounds the two differences, the root, the product and
          the quotient (5, beside powf), the update rounds lr_t * m, sqrtf(v), + eps and the quotient (4); u |theta_new| is the final
          subtraction.  sqrtf and / are correctly rounded (the compiler's default for HIP, no fast-math flag in build.py).
          r_lr(t) = P u (b2^t / (1 - b2^t) / 2 + b1^t / (1 - b1^t)): what P ulps of powf do to lr_t.  P = 16, the OpenCL conformance
          limit for pow -- a condition, not a measurement; the ROCm installation ships no documented figure for powf.
  rmsprop ms as v (decay for b2).  theta against float64 from the device's own ms: (RMS_ROUNDINGS [+ 1 with grad_scale]) u |delta| +
          u |theta - delta|, delta = lr gg / sqrt(ms + eps), RMS_ROUNDINGS = 4 (lr * gg, ms + eps, the root, the quotient), then the clip
          (exact, and it contracts errors).  Where the float64 unclipped value lies within its bound of a clip edge either side is
          accepted (the value must still lie within the bound of the clipped reference); everywhere else an element past an edge must
          be the edge, bit for bit.  test_optim_dispatch_cpu.py asserts that at most 1 % of a row's elements are that close.
  g = 0 on m = v = 0 (ms = 0): the weight is bit-unchanged.

Worst observed fraction of the bound per family, MI355X, 2026-10-20 (test_optim_dispatch_gpu.py prints the figure of every row; one
above 1 fails):
  pack_adam          m 0.31   v 0.54   theta 0.9997 (over the zero weights alone 0.28)
  adam_step          m 0.25   v 0.44   theta 0.9997 (0.20)
  adam_step_counted  m 0.30   v 0.30   theta 0.9999 (0.21)
  rmsprop_step       ms 0.47  theta 1.0000 to four places, and below 1 (the float32 restatement of the CPU module: 0.99996)
theta's figure comes from weights of size 1 that an update carries just past 1: there half an ulp is 2^-24 of the value, which is the
bound's last term itself.  Where that term vanishes (zero weights) the update alone uses under a third of its bound."""
import re

import numpy as np

# ---- constants the transcription copies (test_optim_dispatch_cpu.py holds them against the source text) --------------------------------
K_BLOCK = 256
PACK_CHUNK = 4096              # kPackChunk
PACK_CHUNK_MANY = 1024         # pack_chunk(slabs > PACK_SLABS_MANY)
PACK_SLABS_MANY = 4
PACK_GRID_CAP = 512            # ggan_pack_parts2: gx
GRID_CAP = 2048                # grid_for
STEP_PER_THREAD = 8            # grid_for(n, 8) of adam_k / rmsprop_k
PACK_MAX = 64
ARRIVE_STRIDE = 1024
ARRIVE_INTS = 33 * ARRIVE_STRIDE
ARRIVE_GROUPS = 32

U = 2.0 ** -24
P_POW = 16
M_ROUNDINGS, V_ROUNDINGS, TH_ROUNDINGS, RMS_ROUNDINGS = 4, 5, 9, 4

PAD = 8                        # sentinel floats in front of and behind every buffer (a multiple of 4)
SENTINEL = np.float32(-12345.678)
HP = (2e-4, 0.5, 0.999, 1e-8)              # the scripts' own Adam settings
HP99 = (1e-3, 0.9, 0.9, 1e-8)
RMS_HP = (5e-5, 0.9, 1e-10)
CLIP = (-0.01, 0.01)
BIG = GRID_CAP * K_BLOCK * STEP_PER_THREAD + 1027          # past one trip of the capped grid of grid_for(n, 8)
PACK_BIG = PACK_GRID_CAP * PACK_CHUNK + 4099
SIZES = (1, 3, 4, 5, 1023, 1024, 1027, 4095, 4096, 4097, 4099, 8194)
SLAB_SIZES = (5, 1027, 4099)
ADAM_KEYS = ('pack_adam', 'adam_step', 'adam_step_counted')


def cdiv(a, b):
    return -(-a // b)


def T(size, parts=1, smod=0, soff=0, src=True, parts2=0, smod2=0, soff2=0, slot=0):
    """one tensor of a table; a slab stride is the size rounded up to 4, plus 4, plus smod (so stride % 4 == smod)"""
    st = lambda p, mod: (cdiv(size, 4) * 4 + 4 + mod) if p > 1 else 0
    return dict(size=size, parts=parts, stride=st(parts, smod), soff=soff, src=src, parts2=parts2, stride2=st(parts2, smod2), soff2=soff2,
                slot=slot)


def _row(entry, launches, tensors=(), n=0, step0=0, hyper=None, gscale=1.0, clip=None, repeat=1, split=0, bump=True, note=''):
    hyper = hyper if hyper is not None else (RMS_HP if entry == 'rmsprop_step' else HP)
    return dict(entry=entry, tensors=tuple(tensors), n=n, step0=step0, hyper=tuple(hyper), gscale=gscale, clip=clip, repeat=repeat, split=split,
                bump=bump, launches=tuple(launches), note=note)


def _pa(tensors, nb, note='', **kw):
    return _row('pack_adam', (('pack_adam', kw.get('repeat', 1), (nb,), (K_BLOCK,)),), tensors, note=note, **kw)


def _pk(tensors, gx, note='', **kw):
    return _row('pack', (('pack', kw.get('repeat', 1), (gx, len(tensors)), (K_BLOCK,)),), tensors, note=note, **kw)


_TABLES = [
    # (tensors, workgroups of pack_adam, grid.x of pack, note)
    ([T(n) for n in SIZES], 16, 3, 'float4 path, every size class; 4097: the second workgroup holds only the tail'),
    ([T(n, soff=1) for n in SIZES], 16, 3, 'scalar path: src one float past a 16-byte boundary'),
    ([T(n, slot=1) for n in SIZES], 16, 3, 'scalar path: slot offset 1 mod 4'),
    ([T(n, slot=3) for n in SIZES], 16, 3, 'scalar path: slot offset 3 mod 4'),
    ([T(n, soff=i % 2) for i, n in enumerate(reversed(SIZES))], 16, 3, 'both paths side by side, the sizes at other positions of first[]'),
    ([T(n, parts=2) for n in SLAB_SIZES], 4, 2, '2 slabs, stride % 4 == 0: float4'),
    ([T(n, parts=3, smod=1) for n in SLAB_SIZES], 4, 2, '3 slabs, stride % 4 == 1: scalar'),
    ([T(n, parts=4) for n in SLAB_SIZES], 4, 2, '4 slabs, no src2: the chunk stays 4096'),
    ([T(n, parts=4, parts2=1) for n in SLAB_SIZES], 8, 2, '4 + 1 slabs: chunk 1024'),
    ([T(n, parts=5) for n in (1023, 1024, 1025, 1027, 2049, 4100)], 14, 2, '5 slabs: chunk 1024 at its size classes'),
    ([T(n, parts2=4) for n in SLAB_SIZES], 8, 2, 'src2 of 4 slabs, stride2 % 4 == 0: float4, chunk 1024'),
    ([T(n, parts2=2, smod2=1) for n in SLAB_SIZES], 4, 2, 'src2 of 2 slabs, stride2 % 4 == 1: scalar'),
    ([T(n, parts2=1, soff2=1) for n in SLAB_SIZES], 4, 2, 'src2 one float past a boundary: scalar'),
    ([T(1027), T(4099, src=False), T(5)], 4, 2, 'src == NULL: flat is 0, Adam runs with g = 0 on warm moments'),
    ([T(1027), T(4099, src=False, parts2=1), T(7, src=False, parts2=2)], 4, 2, 'src == NULL with src2 given'),
    ([T(1027), T(0), T(4099)], 4, 2, 'a size-0 tensor between two others: one idle workgroup'),
    ([T(1 + i % 7, soff=(i // 7) % 2) for i in range(PACK_MAX)], 64, 1, 'count == GGAN_PACK_MAX: the whole walk over first[]'),
    ([T(n, parts=5, soff=1) for n in (1023, 1024, 1025, 1027, 2049, 4100)], 14, 2, '5 slabs on the scalar path: chunk 1024'),
]
_WARM = {13: 9, 14: 9}                    # (the no-gradient tables run on warm moments)

ROWS = [_pa(t, nb, note, step0=_WARM.get(i, (0, 1, 9, 999, 99999)[i % 5]), gscale=(1.0, 0.5, 1.0 / 3)[i % 3])
        for i, (t, nb, _, note) in enumerate(_TABLES)]
# ---- arrival counters: fewer than 32, exactly 32, more than 32 workgroups; three launches in a row ------------------------------------------
ROWS += [_pa([T((nb - 1) * PACK_CHUNK + 5)], nb, '%d workgroups, three launches: the two-level arrival counter' % nb, repeat=3,
             step0=(0, 1, 9)[i % 3]) for i, nb in enumerate((1, 31, 32, 33, 64, 65))]
# ---- a partial update (arrive == NULL), then the launch that completes it -------------------------------------------------------------------
ROWS += [_row('pack_adam', (('pack_adam', 1, (2,), (K_BLOCK,)), ('pack_adam', 1, (4,), (K_BLOCK,))),
              [T(1027), T(5, soff=1), T(4099), T(3), T(1024)], step0=9, split=2, note='tensors [0:2] with arrive == NULL, then [2:5]')]
# ---- ordinals and the second pair of betas ------------------------------------------------------------------------------------------------
ROWS += [_pa([T(1027), T(5, soff=1)], 2, 'ordinal %d' % (s + 1), step0=s) for s in (0, 1, 9, 999, 99999)]
ROWS += [_pa([T(1027), T(5, soff=1)], 2, 'beta1 = beta2 = 0.9', step0=1, hyper=HP99, gscale=0.5)]
# ---- ggan_pack_parts2 on the same tables ----------------------------------------------------------------------------------------------------
ROWS += [_pk(t, gx, note, repeat=2 if i % 2 == 0 else 1, bump=i % 2 == 0) for i, (t, _, gx, note) in enumerate(_TABLES)]
ROWS += [_pk([T(5), T(PACK_BIG)], PACK_GRID_CAP, 'the capped grid: a second trip of the grid-stride loop, with a tail', repeat=2),
         _pk([T(5), T(PACK_BIG, soff=1)], PACK_GRID_CAP, 'the capped grid on the scalar path', bump=False)]
# ---- adam_k<false>, adam_k<true> ----------------------------------------------------------------------------------------------------------
_NS = (1, 3, 4, 5, 255, 1025, BIG)


def _grid_for(n):
    return min(max(cdiv(n, K_BLOCK * STEP_PER_THREAD), 1), GRID_CAP)


_GRIDS = {1: 1, 3: 1, 4: 1, 5: 1, 255: 1, 1025: 1, BIG: 2048}          # written out: planned() computes them from grid_for's transcription
for _i, _n in enumerate(_NS):
    ROWS.append(_row('adam_step', (('adam_step', 1, (_GRIDS[_n],), (K_BLOCK,)), ('adam_advance', 1, (1,), (1,))), n=_n,
                     step0=(0, 1, 9, 999, 99999)[_i % 5], gscale=(1.0, 0.5, 1.0 / 3)[_i % 3], hyper=HP99 if _n == 255 else HP,
                     note='adam_k<false>: the ordinal is step + 1, ggan_adam_advance moves the counter'))
    ROWS.append(_row('adam_step_counted', (('adam_step', 1, (_GRIDS[_n],), (K_BLOCK,)),), n=_n, step0=(100000, 1000, 10, 2, 1)[_i % 5],
                     gscale=(1.0 / 3, 1.0, 0.5)[_i % 3], hyper=HP99 if _n == 5 else HP,
                     note='adam_k<true>: the counter already holds the ordinal and stays'))
# ---- rmsprop_k ------------------------------------------------------------------------------------------------------------------------------
for _i, _n in enumerate((1, 5, 1025, BIG)):
    for _j, _clip in enumerate((None, CLIP)):
        ROWS.append(_row('rmsprop_step', (('rmsprop_step', 1, (_GRIDS[_n],), (K_BLOCK,)),), n=_n, clip=_clip,
                         gscale=(1.0, 1.0 / 3)[(_i + _j) % 2], note='clip %s' % (_clip,)))


def row_id(row):
    if row['entry'] in ('pack', 'pack_adam'):
        t = row['tensors']
        what = '%dx%s' % (len(t), '-'.join(sorted({('f4' if p['path'] == 'float4' else 'sc') + str(p['chunk']) for p in tensor_plans(row)})))
        return '%s-%s-max%d-t%d-gs%.2f%s%s%s-%s' % (row['entry'], what, max(x['size'] for x in t), row['step0'], row['gscale'],
                                                  '-x%d' % row['repeat'] if row['repeat'] > 1 else '', '-split%d' % row['split'] if row['split'] else '',
                                                  '' if row['bump'] else '-nobump', re.sub(r'[^0-9A-Za-z]+', '_', row['note'])[:48])
    return '%s-n%d-t%d-gs%.2f-b%g%s' % (row['entry'], row['n'], row['step0'], row['gscale'], row['hyper'][1], '-clip' if row['clip'] else '')


def threads(launch):
    """the profiler's grid figure of a launch: work-items"""
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


# ---- the host dispatch and the in-kernel path predicate, transcribed -----------------------------------------------------------------------
def slabs_of(t):
    return t['parts'] + t['parts2']          # (parts2 == 0: no second source)


def chunk_of(t):
    return PACK_CHUNK_MANY if slabs_of(t) > PACK_SLABS_MANY else PACK_CHUNK


def path_of(t):
    """the predicate of pack_k and pack_adam_k: float4 when src is there, src, flat + off and src2 sit on 16-byte boundaries, and the slab
    strides of a source with more than one slab are multiples of 4 (flat, theta, m, v themselves are 16-byte aligned: the entry refuses
    others)"""
    ok = (t['src'] and t['soff'] % 4 == 0 and t['slot'] % 4 == 0 and (t['parts2'] == 0 or t['soff2'] % 4 == 0)
          and (t['parts'] == 1 or t['stride'] % 4 == 0) and (t['parts2'] <= 1 or t['stride2'] % 4 == 0))
    return 'float4' if ok else 'scalar'


def tensor_plans(row, lo=0, hi=None):
    """per tensor of tensors[lo:hi] in one pack_adam launch: path, chunk, workgroup range [first, last], the workgroup that owns the
    1..3-element tail (None: no tail) and whether that workgroup has no float4 work at all"""
    out, nb = [], 0
    for t in row['tensors'][lo:hi]:
        n, chunk = t['size'], chunk_of(t)
        wgs = cdiv(max(n, 1), chunk)
        path = path_of(t)
        tail = nb + wgs - 1 if (path == 'float4' and n % 4) else None
        out.append(dict(path=path, chunk=chunk, first=nb, last=nb + wgs - 1, tail=tail,
                        tail_only=tail is not None and (wgs - 1) * chunk >= (n // 4) * 4))
        nb += wgs
    return out


def segments(row):
    """-> [(lo, hi, with arrival counters)] of a pack_adam row's launches, in order"""
    k = len(row['tensors'])
    if row['split']:
        return [(0, row['split'], False), (row['split'], k, True)]
    return [(0, k, True)] * row['repeat']


def planned(row):
    """-> the launches the transcription derives for a row"""
    e = row['entry']
    if e == 'pack_adam':
        nbs = [tensor_plans(row, lo, hi)[-1]['last'] + 1 for lo, hi, _ in segments(row)]
        return tuple(('pack_adam', nbs.count(nb), (nb,), (K_BLOCK,)) for nb in sorted(set(nbs), key=nbs.index))
    if e == 'pack':
        mx = max(t['size'] for t in row['tensors'])
        return (('pack', row['repeat'], (min(max(cdiv(mx, K_BLOCK * 16), 1), PACK_GRID_CAP), len(row['tensors'])), (K_BLOCK,)),)
    step = (e if e == 'rmsprop_step' else 'adam_step', 1, (_grid_for(row['n']),), (K_BLOCK,))
    return (step, ('adam_advance', 1, (1,), (1,))) if e == 'adam_step' else (step,)


def arrival_groups(nb):
    """-> (groups, members of every group) of the two-level arrival counter of a pack_adam launch of nb workgroups"""
    groups = min(nb, ARRIVE_GROUPS)
    return groups, [(nb - g + ARRIVE_GROUPS - 1) // ARRIVE_GROUPS for g in range(groups)]


# ---- layout --------------------------------------------------------------------------------------------------------------------------------
def layout(tensors):
    """-> (offset of every tensor in flat / theta / m / v, floats of those buffers): PAD sentinels at both ends, at least 4 between two
    slots, every offset = slot (mod 4)"""
    offs, cur = [], PAD
    for t in tensors:
        off = cdiv(cur, 4) * 4 + 4 + t['slot']
        offs.append(off)
        cur = off + t['size']
    return offs, cdiv(cur, 4) * 4 + PAD


def src_host(size, parts, stride, soff, slabs):
    """the source buffer of a tensor as the device holds it: `soff` floats, then the slabs `stride` apart, NaN everywhere else (a read
    outside a slab poisons the sum) -> (buffer, index of the first slab's first float)"""
    body = (parts - 1) * stride + size
    buf = np.full(soff + body + 4, np.nan, dtype=np.float32)
    for p in range(parts):
        buf[soff + p * stride: soff + p * stride + size] = slabs[p]
    return buf, soff


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
_f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
G_SCALES = np.asarray([0.0, 1e-6, 1e-3, 1.0])
W_VALUES = np.asarray([0.0, 1e-3, -1e-3, 1.0, -1.0])


def _grad(rng, n, parts, scale=None):
    """-> (float32 slabs [parts, n], per-element scale): magnitudes in [0.5, 1.5) * scale, either sign, exact zeros where the scale is 0"""
    if scale is None:
        scale = G_SCALES[rng.integers(0, 4, size=n)]
    slabs = scale * rng.uniform(0.5, 1.5, size=(parts, n)) * rng.choice([-1.0, 1.0], size=(parts, n)) + 0.0
    return _f32(slabs), scale


def _state(rng, n, scale, warm):
    """-> float32 theta, m, v of n elements; warm moments sit at the gradient's scale (1e-3 where the gradient is exactly 0)"""
    theta = _f32(W_VALUES[rng.integers(0, len(W_VALUES), size=n)])
    if not warm:
        return theta, np.zeros(n, np.float32), np.zeros(n, np.float32)
    s = np.where(scale > 0, scale, 1e-3)
    return theta, _f32(s * rng.uniform(0.1, 1.0, size=n) * rng.choice([-1.0, 1.0], size=n)), _f32(s * s * rng.uniform(0.25, 1.0, size=n))


def is_warm(row):
    return row['step0'] > (1 if row['entry'] == 'adam_step_counted' else 0)


def inputs(row, seed):
    """-> dict of float32 host arrays.  pack / pack_adam: src[k], src2[k] (slab arrays [parts, size] or None) and theta, m, v in the
    layout() of the whole table, sentinels everywhere else;  adam_step*, rmsprop_step: g, theta, m, v (ms) of n floats."""
    rng = np.random.default_rng(seed)
    e = row['entry']
    if e in ('pack', 'pack_adam'):
        offs, total = layout(row['tensors'])
        out = dict(src=[], src2=[], theta=np.full(total, SENTINEL), m=np.full(total, SENTINEL), v=np.full(total, SENTINEL))
        for t, off in zip(row['tensors'], offs):
            n = t['size']
            s1, sc1 = _grad(rng, n, t['parts'])
            s2, sc2 = _grad(rng, n, max(t['parts2'], 1), sc1 if t['src'] else None)       # (both contributions at one scale per element)
            out['src'].append(s1 if t['src'] else None)
            out['src2'].append(s2 if t['parts2'] else None)
            scale = sc1 if t['src'] else (sc2 if t['parts2'] else np.zeros(n))
            th, m, v = _state(rng, n, scale, is_warm(row))
            out['theta'][off:off + n], out['m'][off:off + n], out['v'][off:off + n] = th, m, v
        return out
    n = row['n']
    g, scale = _grad(rng, n, 1)
    if e != 'rmsprop_step':
        th, m, v = _state(rng, n, scale, is_warm(row))
        return dict(g=g[0], theta=th, m=m, v=v)
    # RMSProp: classes by position (a row of n elements holds the first n classes of its phase): weights exactly at the clip edges, one
    # float inside them, outside them, in the interior, at 0; ms at TF's initial 1.0, warm at the gradient's scale, or 0 -- and 0 with g = 0
    lo, hi = (np.float32(c) for c in CLIP)
    inside = lambda x: np.nextafter(x, np.float32(0), dtype=np.float32)
    edge = [hi, lo, inside(hi), inside(lo), np.float32(0.02), np.float32(-0.02), np.float32(1.0), np.float32(-1.0), np.float32(1e-3),
            np.float32(-1e-3), np.float32(0.0), np.float32(0.005)]
    cls = (np.arange(n) + seed) % 16
    theta = _f32(np.asarray(edge + [0.0, 1e-3, -0.5, 0.009])[cls])
    g = g[0]
    at_edge = cls < 2                                                 # (a weight ON an edge moves off it by far more than its bound)
    scale = np.where(at_edge & (scale < 1e-3), 1e-3, scale)
    g[at_edge] = _grad(rng, n, 1, scale)[0][0][at_edge]
    s = np.where(scale > 0, scale, 1e-3)
    ms = _f32(np.where(cls % 3 == 0, 1.0, s * s * rng.uniform(0.25, 1.0, size=n)))
    zero = (cls == 8) | (cls == 12) | (cls == 5)                      # ms = 0 with g = 0: an interior weight, a zero one, one outside the clip
    ms[zero], g[zero] = 0.0, 0.0
    first = (cls == 13) & (scale > 0)                                 # ms = 0 on a first gradient: eps decides at the 1e-6 scale
    ms[first] = 0.0
    return dict(g=g, theta=theta, m=ms, v=None)


def flat_sum(src, src2, n):
    """the float32 sum in slab order: src slabs, then src2 slabs; 0 for no source at all"""
    a = np.zeros(n, np.float32)
    if src is not None:
        a = src[0].copy()
        for p in range(1, src.shape[0]):
            a = a + src[p]
    if src2 is not None:
        for p in range(src2.shape[0]):
            a = a + src2[p]
    return a


# ---- float64 restatements and the staged checks ----------------------------------------------------------------------------------------------
def f64(x):
    """a hyper-parameter as the kernel receives it: rounded to float32"""
    return float(np.float32(x))


def lr_at(t, hyper):
    """lr_t = lr sqrt(1 - b2^t) / (1 - b1^t) in float64, from the float32-rounded hyper-parameters"""
    lr, b1, b2 = f64(hyper[0]), f64(hyper[1]), f64(hyper[2])
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def r_lr(t, hyper):
    """relative error of lr_t when each powf is P_POW ulps off"""
    b1, b2 = f64(hyper[1]), f64(hyper[2])
    return P_POW * U * (b2 ** t / (1.0 - b2 ** t) / 2.0 + b1 ** t / (1.0 - b1 ** t))


def adam64(g32, th0, m0, v0, t, hyper, gscale, mutant=None):
    """TensorFlow's Adam in float64 from float32 values -> (m, v, theta); `mutant` names one of the wrong kernels of MUTANTS"""
    lr, b1, b2, eps = (f64(h) for h in hyper)
    gs = f64(gscale)
    g, th0, m0, v0 = (np.asarray(a, np.float64) for a in (g32, th0, m0, v0))
    gg = g * gs
    m = b1 * m0 + (1.0 - b1) * gg
    v = b2 * v0 + (1.0 - b2) * gg * gg
    if mutant == 'gscale_missing_from_v':
        v = b2 * v0 + (1.0 - b2) * g * g
    if mutant == 'one_minus_beta1_for_v':
        v = b2 * v0 + (1.0 - b1) * gg * gg
    tt = {'ordinal_minus_1': t - 1, 'ordinal_plus_1': t + 1}.get(mutant, t)
    lr_t = lr * np.sqrt(1.0 - b2 ** tt) / (1.0 - b1 ** tt) if tt > 0 else np.inf
    if mutant == 'betas_swapped_in_correction':
        lr_t = lr * np.sqrt(1.0 - b1 ** t) / (1.0 - b2 ** t)
    if mutant == 'no_bias_correction':
        lr_t = lr
    num = m0 if mutant == 'update_from_old_m' else m
    if mutant == 'eps_inside_root':
        theta = th0 - lr_t * num / np.sqrt(v + eps)
    elif mutant == 'eps_dropped':
        with np.errstate(divide='ignore', invalid='ignore'):
            theta = th0 - lr_t * np.where(num == 0, 0.0, num / np.sqrt(v))
    elif mutant == 'pytorch_eps':
        theta = th0 - lr / (1.0 - b1 ** t) * num / (np.sqrt(v / (1.0 - b2 ** t)) + eps)
    else:
        theta = th0 - lr_t * num / (np.sqrt(v) + eps)
    return m, v, theta


def _frac(err, bound, bad=None):
    """worst err / bound; an error where the bound is 0 counts as infinite, and so does every element whose error or bound is not
    finite (a NaN or an infinity in an output, or in what the bound is formed from) or that `bad` marks: the figure is never NaN"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        f = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    f = np.where(np.isfinite(err) & np.isfinite(bound), f, np.inf)
    if bad is not None:
        f = np.where(bad, np.inf, f)
    return float(np.max(f))


def within(fractions):
    """every figure of a fractions dict is at most 1 (written so that a NaN, should one ever get here, fails)"""
    return all(f <= 1.0 for f in fractions.values())


def adam_fractions(g32, th0, m0, v0, th1, m1, v1, t, hyper, gscale):
    """(th1, m1, v1): what a kernel made of (th0, m0, v0) and the float32 gradient g32 at ordinal t -> worst error as a fraction of its
    bound for m, v (against float64 from the inputs) and theta (against float64 from m1, v1 themselves; theta_at_0: over the zero weights
    alone)"""
    lr, b1, b2, eps = (f64(h) for h in hyper)
    gs = f64(gscale)
    extra = 0 if gs == 1.0 else 1
    g, th0, m0, v0, th1, m1, v1 = (np.asarray(a, np.float64) for a in (g32, th0, m0, v0, th1, m1, v1))
    gg = g * gs
    m, v, _ = adam64(g32, th0, m0, v0, t, hyper, gscale)
    bm = (M_ROUNDINGS + extra) * U * (np.abs(b1 * m0) + np.abs((1.0 - b1) * gg))
    bv = (V_ROUNDINGS + extra) * U * (np.abs(b2 * v0) + np.abs((1.0 - b2) * gg * gg))
    with np.errstate(invalid='ignore'):
        delta = lr_at(t, hyper) * m1 / (np.sqrt(v1) + eps)          # (a negative v1: NaN here, an infinite figure for theta below)
    theta = th0 - delta
    bt = (r_lr(t, hyper) + TH_ROUNDINGS * U) * np.abs(delta) + U * np.abs(theta)
    zero = th0 == 0                               # (there the final subtraction is exact: the figure is the update's own)
    return dict(m=_frac(np.abs(m1 - m), bm), v=_frac(np.abs(v1 - v), bv, bad=~(v1 >= 0)), theta=_frac(np.abs(th1 - theta), bt),
                theta_at_0=_frac(np.abs(th1 - theta)[zero], bt[zero]))


def rms64(g32, th0, ms0, hyper, gscale, clip, mutant=None):
    """tf.train.RMSPropOptimizer (momentum 0) and the clip in float64 -> (ms, theta)"""
    lr, decay, eps = (f64(h) for h in hyper)
    gg = np.asarray(g32, np.float64) * f64(gscale)
    th0, ms0 = np.asarray(th0, np.float64), np.asarray(ms0, np.float64)
    ms = decay * ms0 + (1.0 - decay) * gg * gg
    lo, hi = (-np.inf, np.inf) if clip is None else (f64(clip[0]), f64(clip[1]))
    if mutant == 'rms_eps_outside_root':
        return ms, np.clip(th0 - lr * gg / (np.sqrt(ms) + eps), lo, hi)
    if mutant == 'rms_clip_before_update':
        return ms, np.clip(th0, lo, hi) - lr * gg / np.sqrt(ms + eps)
    return ms, np.clip(th0 - lr * gg / np.sqrt(ms + eps), lo, hi)


def rms_fractions(g32, th0, ms0, th1, ms1, hyper, gscale, clip):
    """-> (worst fractions for ms and theta, elements past a clip edge that are not the edge bit for bit, share of the elements whose
    float64 unclipped value lies within its bound of an edge, elements with ms = g = 0 whose weight changed)"""
    lr, decay, eps = (f64(h) for h in hyper)
    gs = f64(gscale)
    extra = 0 if gs == 1.0 else 1
    gg = np.asarray(g32, np.float64) * gs
    th0d, ms0d, th1d, ms1d = (np.asarray(a, np.float64) for a in (th0, ms0, th1, ms1))
    ms, _ = rms64(g32, th0, ms0, hyper, gscale, clip)
    bms = (V_ROUNDINGS + extra) * U * (np.abs(decay * ms0d) + np.abs((1.0 - decay) * gg * gg))
    with np.errstate(invalid='ignore', divide='ignore'):
        delta = lr * gg / np.sqrt(ms1d + eps)
    raw = th0d - delta
    bt = (RMS_ROUNDINGS + extra) * U * np.abs(delta) + U * np.abs(raw)
    lo, hi = (-np.inf, np.inf) if clip is None else (f64(clip[0]), f64(clip[1]))
    near = (np.abs(raw - lo) <= bt) | (np.abs(raw - hi) <= bt)
    past_lo, past_hi = (raw < lo) & ~near, (raw > hi) & ~near
    th1f = np.asarray(th1, np.float32)
    not_edge = int(np.sum(th1f[past_lo] != np.float32(lo))) + int(np.sum(th1f[past_hi] != np.float32(hi)))
    still = (np.asarray(ms0) == 0) & (np.asarray(g32) == 0) & (th0d >= lo) & (th0d <= hi)
    moved = int(np.sum(np.asarray(th1, np.float32)[still].view(np.uint32) != np.asarray(th0, np.float32)[still].view(np.uint32)))
    return (dict(ms=_frac(np.abs(ms1d - ms), bms, bad=~(ms1d >= 0)), theta=_frac(np.abs(th1d - np.clip(raw, lo, hi)), bt)), not_edge,
            float(np.mean(near)) if near.size else 0.0, moved)


def rms_near_share(g32, th0, ms0, hyper, gscale, clip):
    """share of the elements whose float64 unclipped reference lies within its bound of a clip edge -- from the reference alone (rms64's
    own ms, no kernel's)"""
    if clip is None:
        return 0.0
    lr, decay, eps = (f64(h) for h in hyper)
    gs = f64(gscale)
    gg = np.asarray(g32, np.float64) * gs
    ms, _ = rms64(g32, th0, ms0, hyper, gscale, clip)
    delta = lr * gg / np.sqrt(ms + eps)
    raw = np.asarray(th0, np.float64) - delta
    bt = (RMS_ROUNDINGS + (0 if gs == 1.0 else 1)) * U * np.abs(delta) + U * np.abs(raw)
    near = (np.abs(raw - f64(clip[0])) <= bt) | (np.abs(raw - f64(clip[1])) <= bt)
    return float(np.mean(near)) if near.size else 0.0


def ordinal(row, launch=0):
    """the update's ordinal of a row's launch"""
    if row['entry'] == 'adam_step_counted':
        return row['step0']
    return row['step0'] + 1 + (launch if not row['split'] else 0)


# ---- wrong kernels the rows must tell from the right one (test_optim_dispatch_cpu.py) ------------------------------------------------------
ADAM_MUTANTS = ('eps_inside_root', 'eps_dropped', 'pytorch_eps', 'betas_swapped_in_correction', 'ordinal_minus_1', 'ordinal_plus_1',
                'no_bias_correction', 'gscale_missing_from_v', 'one_minus_beta1_for_v', 'update_from_old_m')
PACK_MUTANTS = ('tail_untouched', 'one_float4_group_untouched', 'slabs_in_reverse_order', 'src2_dropped')
RMS_MUTANTS = ('rms_eps_outside_root', 'rms_clip_before_update')
MUTANTS = ADAM_MUTANTS + PACK_MUTANTS + RMS_MUTANTS


def f32_kernel(g32, th0, m0, v0, t, hyper, gscale):
    """adam1 as written, in float32 numpy without contraction (numpy's float32 power for powf) -> (theta, m, v): the CPU stand-in for the
    right kernel"""
    f = np.float32
    lr, b1, b2, eps = (f(h) for h in hyper)
    one = f(1)
    lr_t = lr * np.sqrt(one - np.power(b2, f(t), dtype=np.float32)) / (one - np.power(b1, f(t), dtype=np.float32))
    gg = np.asarray(g32, np.float32) * f(gscale)
    m = b1 * np.asarray(m0, np.float32) + (one - b1) * gg
    v = b2 * np.asarray(v0, np.float32) + (one - b2) * gg * gg
    th = np.asarray(th0, np.float32) - lr_t * m / (np.sqrt(v) + eps)
    assert th.dtype == np.float32 and m.dtype == np.float32 and v.dtype == np.float32
    return th, m, v


def f32_rms_kernel(g32, th0, ms0, hyper, gscale, clip):
    f = np.float32
    lr, decay, eps = (f(h) for h in hyper)
    gg = np.asarray(g32, np.float32) * f(gscale)
    ms = decay * np.asarray(ms0, np.float32) + (f(1) - decay) * gg * gg
    th = np.asarray(th0, np.float32) - lr * gg / np.sqrt(ms + eps)
    lo, hi = (f('-inf'), f('inf')) if clip is None else (f(clip[0]), f(clip[1]))
    th = np.minimum(np.maximum(th, lo), hi)
    assert th.dtype == np.float32 and ms.dtype == np.float32
    return th, ms
