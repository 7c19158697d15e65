"""Which kernel instance of the normalisation family (csrc/bn.hip, csrc/linear_bn.hip) each dispatch test runs: one row per instance,
threshold side and fused activation (plain data), and the host side of those tests: the rows' inputs and their float64 references.

tests/test_norm_dispatch_gpu.py runs every row, asserts that the profiler saw exactly the row's launches -- every name with its count
and its grid -- and that every output matches the float64 reference.  tests/test_norm_dispatch_cpu.py parses the GGAN_LAUNCH sites of
the two sources and fails when a (label, kernel, template argument) has no row, a row names no launch or two kernels share a label; it
recomputes every row's launches from a Python transcription of the dispatch predicates, and it builds the masked rows' inputs and
asserts their margin from the activation's kink.

A row:
  entry     bn_fwd (ggan_bn_fwd_train) | bn_bwd (ggan_bn_bwd_act) | sync (the four ggan_bn_sync_* entry points, the batch cut into `world`
            replicas and the statistics rows gathered by hand) | bwd_bwd (ggan_bn_bwd_bwd through autograd: BatchNormTrain, its first
            backward recorded, then the second) | split (ggan_bn_split_fwd_train / _bwd_act through BatchNormGroupedTrain) |
            lin_fwd (ggan_linear_bn_rows_fwd) | lin_bwd (ggan_linear_bn_rows_bwd)
  shape     (N, C, HW) -- HW == 1 is the [N, C] rows layout; sync: N is the whole batch, world * n; lin_*: (M, K, N)
  act       fused activation: none | lrelu (alpha 0.2) | relu | tanh | sigmoid -- the forward's epilogue, the backward's mask
  chansum   bn_bwd: gx_chansum is requested
  off       bn_bwd: base offset in floats of x, gy, gx and the mask's reference y (0: 16-byte aligned; 1: one float past a boundary)
  const     a channel whose values are all exactly 0.5: its sums and mean are exact in float32, y equals offset exactly, gx is finite
  world, groups   sync: replicas;  split: statistic groups
  launches  ((label, launches, grid, block), ...): every launch of the family the row causes, in launch order
  note      which edge the row is there for

To add a row: pick the smallest shape on the side of the threshold you want (C small and odd, so a wrong channel stride shows), write
the launches the dispatch in bn.hip / linear_bn.hip makes for it (`planned()` in test_norm_dispatch_cpu.py computes them without a
GPU), and run the two dispatch modules.  A masked row (lrelu / relu) needs no care: inputs() moves every x whose pre-activation lies
within MARGIN of the kink.
"""
import numpy as np

EPS = 1e-5
ALPHA = 0.2
MARGIN = 1e-4          # float64 |pre-activation| every element of a masked row keeps: a float32 evaluation cannot take the other branch
ACTS = ('none', 'lrelu', 'relu', 'tanh', 'sigmoid')          # position = GGAN_ACT_* code
MASKS = ('lrelu', 'relu')

REG, STREAM, ROWSF = 'bn_fwd_nchw_reg_k', 'bn_fwd_nchw_k', 'bn_fwd_rows_k'
R4S, R4L, BREG, BSTREAM, BROWS = 'bn_bwd_nchw_reg4_k<256>', 'bn_bwd_nchw_reg4_k<1024>', 'bn_bwd_nchw_reg_k', 'bn_bwd_nchw_k', 'bn_bwd_rows_k'


def _row(entry, shape, launches, act='none', chansum=False, off=(0, 0, 0, 0), const=None, world=1, groups=1, note=''):
    return dict(entry=entry, shape=tuple(shape), act=act, alpha=ALPHA if act == 'lrelu' else 0.0, chansum=chansum, off=tuple(off),
                const=const, world=world, groups=groups, launches=tuple(launches), note=note)


def _one(entry, shape, kernel, grid, block, **kw):
    return _row(entry, shape, ((kernel, 1, grid, block),), **kw)


def _sync(shape, world, act, bwd):
    C = shape[1]
    names = ('bn_sync_stats', 'bn_sync_apply') + (('bn_sync_bwd_stats', 'bn_sync_bwd_apply') if bwd else ())
    return _row('sync', shape, tuple((n, world, (C,), (256,)) for n in names), act=act, world=world)


def _bb(shape, act):
    C = shape[1]
    return _row('bwd_bwd', shape, ((REG, 1, (C,), (1024,)), (BREG, 1, (C,), (1024,)), ('bn_bwd_bwd', 1, (C,), (256,))), act=act)


def _split_row(shape, act):
    """two groups of one image / one row each: one slab per group, one workgroup per elementwise pass"""
    C, nchw = shape[1], len(shape) == 3
    lay, grid, block = ('nchw', (C, 1, 2), (256,)) if nchw else ('rows', (1, 1, 2), (64, 4))
    return _row('split', shape, (('bn_split_stats_' + lay, 1, grid, block), ('bn_split_merge', 1, (1, 2), (64, 16)),
                                 ('bn_split_apply', 1, (1,), (256,)), ('bn_split_bwd_stats_' + lay, 1, grid, block),
                                 ('bn_split_bwd_merge', 1, (1,), (64, 16)), ('bn_split_bwd_apply', 1, (1,), (256,))), act=act, groups=2)


ROWS = [
    # ---- ggan_bn_fwd_train: every kernel with every epilogue ---------------------------------------------------------------------------
    _one('bn_fwd', (1820, 5, 9), REG, (5,), (1024,), note='16380 elements per channel: the last size below kRegE * kThreads with HW = 9'),
    _one('bn_fwd', (4096, 3, 4), REG, (3,), (1024,), act='tanh', note='16384 = kRegE * kThreads exactly: every register slot of every thread'),
    _one('bn_fwd', (334, 3, 49), REG, (3,), (1024,), act='lrelu', note='HW = 49, 16366 elements: the largest numerators of the mulhi division'),
    _one('bn_fwd', (1024, 3, 4), REG, (3,), (1024,), act='relu'),
    _one('bn_fwd', (6, 5, 16), REG, (5,), (1024,), act='sigmoid', note='96 elements: most threads hold nothing'),
    _one('bn_fwd', (64, 3, 2), REG, (3,), (1024,), const=1, note='channel 1 is 0.5 everywhere, 128 = 2^7 elements: sum, mean exact, variance 0'),
    _one('bn_fwd', (1821, 5, 9), STREAM, (5,), (1024,), note='16389 elements: the first size past the register kernel with HW = 9'),
    _one('bn_fwd', (4097, 3, 4), STREAM, (3,), (1024,), act='lrelu', note='16388 elements: one image past the register kernel'),
    _one('bn_fwd', (1821, 3, 9), STREAM, (3,), (1024,), act='relu'),
    _one('bn_fwd', (4097, 5, 4), STREAM, (5,), (1024,), act='tanh'),
    _one('bn_fwd', (1821, 3, 9), STREAM, (3,), (1024,), act='sigmoid'),
    _one('bn_fwd', (1, 5), ROWSF, (1,), (32, 16), note='one row: every variance is 0, y = offset'),
    _one('bn_fwd', (17, 33), ROWSF, (2,), (32, 16), act='lrelu', note='ragged 32-column tile, ragged 16-slice walk'),
    _one('bn_fwd', (40, 64), ROWSF, (2,), (32, 16), act='relu'),
    _one('bn_fwd', (17, 33), ROWSF, (2,), (32, 16), act='tanh'),
    _one('bn_fwd', (40, 64), ROWSF, (2,), (32, 16), act='sigmoid'),
    # ---- ggan_bn_bwd_act: every kernel with every mask, every threshold from both sides ---------------------------------------------------
    _one('bn_bwd', (1024, 3, 4), R4S, (3,), (256,), act='lrelu', chansum=True, note='4096 elements = 16 * 256: the last size of the 256-thread kernel'),
    _one('bn_bwd', (1024, 5, 4), R4S, (5,), (256,), act='relu'),
    _one('bn_bwd', (1024, 3, 4), R4S, (3,), (256,)),
    _one('bn_bwd', (6, 5, 16), R4S, (5,), (256,), act='lrelu', chansum=True, note='the aligned twin of the four offset rows'),
    _one('bn_bwd', (1025, 3, 4), R4L, (3,), (1024,), note='4100 elements: one image past the 256-thread kernel'),
    _one('bn_bwd', (1025, 5, 4), R4L, (5,), (1024,), act='lrelu'),
    _one('bn_bwd', (4096, 3, 4), R4L, (3,), (1024,), act='relu', chansum=True, note='16384 = 16 * 1024: the last size held in registers'),
    _one('bn_bwd', (1820, 5, 9), BREG, (5,), (1024,), act='lrelu', chansum=True, note='16380 elements, HW % 4 != 0: the scalar register kernel'),
    _one('bn_bwd', (334, 3, 49), BREG, (3,), (1024,), note='HW = 49, 16366 elements: the largest numerators of the mulhi division'),
    _one('bn_bwd', (334, 3, 49), BREG, (3,), (1024,), act='relu', chansum=True),
    _one('bn_bwd', (64, 3, 2), BREG, (3,), (1024,), act='lrelu', const=1, note='channel 1 constant: xhat = 0, gx = scale * invstd * (g - mean g)'),
    _one('bn_bwd', (6, 5, 16), BREG, (5,), (1024,), act='lrelu', chansum=True, off=(1, 0, 0, 0), note='x one float past a 16-byte boundary'),
    _one('bn_bwd', (6, 5, 16), BREG, (5,), (1024,), act='lrelu', off=(0, 1, 0, 0), note='gy one float past a 16-byte boundary'),
    _one('bn_bwd', (6, 5, 16), BREG, (5,), (1024,), act='lrelu', off=(0, 0, 1, 0), note='gx one float past a 16-byte boundary'),
    _one('bn_bwd', (6, 5, 16), BREG, (5,), (1024,), act='lrelu', off=(0, 0, 0, 1), note='the mask reference one float past a 16-byte boundary'),
    _one('bn_bwd', (4097, 3, 4), BSTREAM, (3,), (1024,), act='lrelu', chansum=True, note='16388 elements, v4 eligible: past every register kernel'),
    _one('bn_bwd', (1821, 5, 9), BSTREAM, (5,), (1024,), act='relu', note='16389 elements: the first size past the scalar register kernel'),
    _one('bn_bwd', (1821, 3, 9), BSTREAM, (3,), (1024,), chansum=True),
    _one('bn_bwd', (1, 5), BROWS, (1,), (32, 16), note='one row: xhat = 0 and g - mean g = 0, gx is exactly 0'),
    _one('bn_bwd', (17, 33), BROWS, (2,), (32, 16), act='lrelu', note='ragged 32-column tile, ragged 16-slice walk'),
    _one('bn_bwd', (40, 64), BROWS, (2,), (32, 16), act='relu'),
    # ---- cross-replica: 315 (n = 5, HW = 63) and 1030 (n = 10, HW = 103) elements per replica and channel -- a second (fifth) trip of the
    #      256-stride walk and a ragged tail; tanh / sigmoid epilogues run the forward pair only ---------------------------------------------
    _sync((10, 3, 63), 2, 'none', True),
    _sync((15, 5, 63), 3, 'lrelu', True),
    _sync((20, 3, 103), 2, 'relu', True),
    _sync((30, 3, 103), 3, 'tanh', False),
    _sync((10, 5, 63), 2, 'sigmoid', False),
    # ---- second derivative, through autograd: forward, first backward (recorded), second backward -------------------------------------------
    _bb((5, 3, 63), 'none'),
    _bb((5, 3, 63), 'lrelu'),
    _bb((10, 3, 103), 'none'),
    _bb((10, 3, 103), 'lrelu'),
    # ---- Linear + BatchNorm rows in one launch: M = 16 R ------------------------------------------------------------------------------------
    _one('lin_fwd', (16, 20, 32), 'linear_bn_rows_k<1>', (1,), (512,), act='relu'),
    _one('lin_fwd', (32, 20, 32), 'linear_bn_rows_k<2>', (1,), (512,), act='lrelu'),
    _one('lin_fwd', (48, 20, 32), 'linear_bn_rows_k<3>', (1,), (512,), act='tanh'),
    _one('lin_fwd', (64, 20, 32), 'linear_bn_rows_k<4>', (1,), (512,), act='sigmoid'),
    _one('lin_fwd', (80, 20, 32), 'linear_bn_rows_k<5>', (1,), (512,)),
    _one('lin_fwd', (96, 20, 32), 'linear_bn_rows_k<6>', (1,), (512,), act='relu'),
    _one('lin_fwd', (112, 20, 32), 'linear_bn_rows_k<7>', (1,), (512,), act='lrelu'),
    _one('lin_fwd', (128, 20, 32), 'linear_bn_rows_k<8>', (1,), (512,), act='tanh'),
    _one('lin_fwd', (80, 128, 96), 'linear_bn_rows_k<5>', (3,), (512,), act='relu'),
    _one('lin_fwd', (80, 128, 96), 'linear_bn_rows_k<5>', (3,), (512,)),
    _one('lin_fwd', (96, 128, 96), 'linear_bn_rows_k<6>', (3,), (512,), act='relu'),
    _one('lin_fwd', (96, 128, 96), 'linear_bn_rows_k<6>', (3,), (512,)),
    _one('lin_fwd', (112, 128, 96), 'linear_bn_rows_k<7>', (3,), (512,), act='relu'),
    _one('lin_fwd', (112, 128, 96), 'linear_bn_rows_k<7>', (3,), (512,)),
    _one('lin_bwd', (80, 64, 96), 'linear_bn_rows_bwd_k<4>', (3,), (512,), act='relu', note='K = 64: 4 k values per thread'),
    _one('lin_bwd', (112, 128, 96), 'linear_bn_rows_bwd_k<8>', (3,), (512,)),
    _one('lin_bwd', (96, 256, 96), 'linear_bn_rows_bwd_k<16>', (3,), (512,), act='relu'),
    # ---- the row-grouped chip-wide pair (tests/test_ssgan_bn_gpu.py covers its numbers): the labels of its launches, with every mask ----------
] + [_split_row(shape, act) for shape in ((2, 5, 9), (2, 37)) for act in ('none', 'lrelu', 'relu')]


def dims(row):
    """-> (N, C, HW) of a batch-norm row"""
    s = row['shape']
    return (s[0], s[1], s[2] if len(s) == 3 else 1)


def row_id(row):
    return '%s-%s-%s-%s%s%s%s%s' % (row['entry'], row['launches'][-1][0], 'x'.join(str(v) for v in row['shape']), row['act'],
                                   '-cs' if row['chansum'] else '', '-off%s' % ''.join(str(v) for v in row['off']) if any(row['off']) else '',
                                   '-const' if row['const'] is not None else '', '-w%d' % row['world'] if row['world'] > 1 else '')


def threads(launch):
    """the profiler's grid figure of a launch: work-items"""
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


# ---- inputs and float64 references ------------------------------------------------------------------------------------------------------
def apply_act(tp, v, act):
    return {'none': lambda t: t, 'lrelu': lambda t: tp.leaky_relu(t, ALPHA), 'relu': tp.relu, 'tanh': tp.tanh, 'sigmoid': tp.sigmoid}[act](v)


def _bn(tp, x, sc, of, act, gy, want_second=None):
    """float64 BatchNorm (+ activation) of float32-rounded inputs on the oracle tape -> dict of references"""
    axes = [0, 2] if x.ndim == 3 else [0]
    red = tuple(axes)
    X, S_, O = tp.T(x.astype(np.float64)), tp.T(sc.astype(np.float64)), tp.T(of.astype(np.float64))
    v = tp.batchnorm_train(X, S_, O, axes, EPS)
    y = apply_act(tp, v, act)
    mean = X.v.mean(axis=red)
    var = ((X.v - X.v.mean(axis=red, keepdims=True)) ** 2).mean(axis=red)
    out = dict(v=v.v, y=y.v, save_mean=mean, save_invstd=1.0 / np.sqrt(var + EPS))
    if gy is not None:
        G = tp.T(gy.astype(np.float64))
        gx, gs, go = tp.grad(tp.reduce_sum(tp.mul(y, G)), [X, S_, O])
        out.update(gx=gx.v, gscale=gs.v.reshape(-1), goffset=go.v.reshape(-1))
        if want_second is not None:
            rx, rg, rs = tp.grad(tp.reduce_sum(tp.mul(gx, tp.T(want_second.astype(np.float64)))), [X, G, S_])
            out.update(gx2=rx.v, ggy=rg.v, gscale2=rs.v.reshape(-1))
    return out


def inputs(row, seed):
    """-> (float32 inputs, float64 references) of a row, the inputs moved off the activation's kink where the row is masked (split rows:
    split_inputs)."""
    from oracle import tape as tp
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    masked = row['act'] in MASKS
    if row['entry'] in ('lin_fwd', 'lin_bwd'):
        M, K, N = row['shape']
        x = f32(rng.standard_normal((M, K)))
        w = f32(rng.standard_normal((K, N)) / np.sqrt(K))
        b = f32(0.1 * rng.standard_normal(N))
        sc, of = f32(1 + 0.2 * rng.standard_normal(N)), f32(0.2 * rng.standard_normal(N))
        gy = f32(rng.standard_normal((M, N)))
        h64 = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
        if row['entry'] == 'lin_fwd':
            for _ in range(8):                   # (the device forms h itself: a column with an element on the kink gets another offset)
                ref = _bn(tp, h64, sc, of, row['act'], None)
                bad = np.abs(ref['v']) < MARGIN
                if not masked or not bad.any():
                    break
                of[bad.any(axis=0)] += np.float32(1e-2)
            ref = _bn(tp, h64, sc, of, row['act'], None)
            ref['h'] = h64
            return dict(x=x, w=w, b=b, scale=sc, offset=of), ref
        h = f32(h64)
        for _ in range(4):
            ref = _bn(tp, h, sc, of, row['act'], None)
            bad = np.abs(ref['v']) < MARGIN
            if not masked or not bad.any():
                break
            h[bad] += np.where(ref['v'][bad] >= 0, 1, -1).astype(np.float32) * np.float32(1e-2)      # (scale > 0: v grows with h)
        ref = _bn(tp, h, sc, of, row['act'], gy)
        x64 = x.astype(np.float64)
        ref.update(dw=x64.T @ ref['gx'], db=ref['gx'].sum(0), dscale=ref['gscale'], doffset=ref['goffset'])
        return dict(x=x, gy=gy, h=h, y=f32(ref['y']), scale=sc, save_mean=f32(ref['save_mean']), save_invstd=f32(ref['save_invstd'])), ref
    N, C, HW = dims(row)
    shape = (N, C, HW) if len(row['shape']) == 3 else (N, C)
    x = f32(rng.standard_normal(shape) * 2 + 0.5)
    sc, of = f32(1 + 0.2 * rng.standard_normal(C)), f32(0.3 * rng.standard_normal(C))
    gy = f32(rng.standard_normal(shape))
    hh = f32(rng.standard_normal(shape)) if row['entry'] == 'bwd_bwd' else None
    if row['const'] is not None:
        x[:, row['const']] = 0.5
        of[row['const']] = 0.25              # (y of that channel: well away from the kink)
    assert np.all(sc > 0.1)
    for _ in range(4):
        ref = _bn(tp, x, sc, of, row['act'], None)
        bad = np.abs(ref['v']) < MARGIN
        if not masked or not bad.any():
            break
        x[bad] += np.where(ref['v'][bad] >= 0, 1, -1).astype(np.float32) * np.float32(1e-2)          # (scale > 0: v grows with x)
    ref = _bn(tp, x, sc, of, row['act'], gy, hh)
    inp = dict(x=x, scale=sc, offset=of, gy=gy, y=f32(ref['y']), save_mean=f32(ref['save_mean']), save_invstd=f32(ref['save_invstd']))
    if hh is not None:
        inp['h'] = hh
    return inp, ref


def margin(row, ref):
    """the smallest float64 |pre-activation| of a row: what decides a mask"""
    return float(np.abs(ref['v']).min())


def split_preact(x, sc, of, groups):
    """float64 affine output of the grouped BatchNorm: each of `groups` leading parts with its own biased batch statistics"""
    N, C = x.shape[0], x.shape[1]
    xg = x.astype(np.float64).reshape(groups, N // groups, C, -1)
    mean = xg.mean(axis=(1, 3), keepdims=True)
    var = ((xg - mean) ** 2).mean(axis=(1, 3), keepdims=True)
    v = (xg - mean) / np.sqrt(var + EPS) * sc.astype(np.float64).reshape(1, 1, C, 1) + of.astype(np.float64).reshape(1, 1, C, 1)
    return v.reshape(x.shape)


def split_inputs(row, seed):
    """-> float32 x, scale, offset, gy of a split row, drawn as tests/test_ssgan_bn_gpu.py draws them and, where the row is masked, moved
    off the kink: an x within MARGIN of it by 1e-2, the offset of a channel whose group holds one value (variance 0: y is the offset)"""
    import torch
    N, C, HW = dims(row)
    shape = (N, C) if HW == 1 else (N, C, 3, HW // 3)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64).float().numpy()
    sc = (1.0 + 0.3 * torch.randn(C, generator=g, dtype=torch.float64)).float().numpy()
    of = (0.2 * torch.randn(C, generator=g, dtype=torch.float64)).float().numpy()
    gy = torch.randn(shape, generator=g, dtype=torch.float64).float().numpy()
    for _ in range(4):
        v = split_preact(x, sc, of, row['groups'])
        bad = np.abs(v) < MARGIN
        if row['act'] not in MASKS or not bad.any():
            break
        if (N // row['groups']) * HW == 1:
            of[bad.any(axis=0)] += np.float32(1e-2)
        else:
            x[bad] += (np.where(v >= 0, 1, -1) * np.sign(sc).reshape((1, C) + (1,) * (x.ndim - 2)))[bad].astype(np.float32) * np.float32(1e-2)
    return x, sc, of, gy
