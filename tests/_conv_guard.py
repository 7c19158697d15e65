"""What a conv2d row runs INSIDE: the rows of tests/_conv_dispatch.py (and the rows below) once more, with every operand in its own
NaN-filled buffer, outputs that start as NaN inside NaN bands, a workspace that is NaN behind its zero head, mask references with
exact +0 / -0 entries, and a second data set whose every sum is exact in float32 (plain data and numpy, no fixtures).

tests/test_conv_guard_gpu.py runs ROWS + EXTRA_ROWS + MISALIGNED through the C entry points and hands the whole buffers, bands included,
to check().  tests/test_conv_guard_cpu.py proves check() on the CPU: it accepts a float32 numpy evaluation of every op (simulate()) and
rejects every entry of MUTANTS on the row MUTANT_ROW names.

Data sets (inputs(row, data, mask)):
  'gauss'  the distributions of test_conv_dispatch_gpu.py: standard normal x, gy, biases, the filter scaled by 1 / sqrt(25 Ci);
           slope 0.2; compared by max|got - ref| / max|ref| < TOL (forward, data gradient) or TOL_LONG (filter gradient)
  'exact'  x, gy in {-2 .. 2}, w in {-1, 0, 1}, biases in {-3 .. 3}, slope 1/2: every product, partial sum and split-K slab is a multiple
           of 1/2 below 2^23 (exact_bound), so the result is the same in any summation order and is compared by equality.  The fwd_cast
           row (its input is a scaled int32 ring: thirds of 255) stays on 'gauss'; no row has a tanh or sigmoid epilogue.
Masked ops (fwd_masked, dgrad_masked, wgrad_act, wgrad_parts) run with mask 'lrelu' and with 'relu'; a tenth of the mask reference is
exactly +0 or -0 (half each), where the derivative is alpha (LeakyReLU) or 0 (ReLU), as act_grad of csrc/common.h takes it.

Rows are in the schema of _conv_dispatch.ROWS.  Two more keys: `off` (MISALIGNED: the operand that sits one float off a 16-byte boundary)
and `nobias` (a wgrad_act row that passes no bias-gradient pointer: the only masked call the plain filter-gradient kernel takes).
"""
import zlib

import numpy as np

from _conv_dispatch import ROWS, row_id

TOL, TOL_LONG = 5e-6, 1e-5              # the figures of test_ops_gpu.py (asserted equal there by test_conv_guard_cpu.py)
WS_RESERVED = 16384                     # GGAN_WS_RESERVED of include/ggan.h, bytes
WS_FLOATS = 1 << 20                     # floats of workspace behind the head: the widened filter gradient wants 1 MiB behind its two copies
NAN_BITS = 0x7FC00000                   # the quiet NaN every band, output and workspace float starts as
RING_BAND = 1 << 30                     # what the int32 ring of fwd_cast is banded with
ALPHA = {'gauss': 0.2, 'exact': 0.5}
MASKED_OPS = ('fwd_masked', 'dgrad_masked', 'wgrad_act', 'wgrad_parts')
GAUSS_ONLY_OPS = ('fwd_cast',)
PARTS_CAP = 64                          # slabs the partial buffer of wgrad_parts has room for

# ---------------------------------------------------------------------------------------------------------------------------------
# rows
# ---------------------------------------------------------------------------------------------------------------------------------
_DG0 = {'GGAN_DG16': '0'}

EXTRA_ROWS = [
    # H != W on corr_kernel: forward, class pairs (MODE 1) and all classes (MODE 2); (8, 16) and (16, 8)
    dict(kernel='corr_kernel<0, 1, 1, 8, 1, true>', op='fwd', geom=(4, 12, 8, 16, 40, 'SAME'), target=8, env={},
         tiles=8, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=4)),
    dict(kernel='corr_kernel<0, 1, 1, 8, 1, true>', op='fwd', geom=(4, 12, 16, 8, 40, 'SAME'), target=8, env={},
         tiles=8, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=4)),
    dict(kernel='corr_kernel<0, 1, 1, 8, 1, true>', op='fwd_masked', geom=(4, 12, 8, 16, 40, 'SAME'), target=8, env={},
         tiles=8, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=4)),
    dict(kernel='corr_kernel<0, 1, 1, 8, 1, true>', op='fwd_masked', geom=(4, 12, 16, 8, 40, 'SAME'), target=8, env={},
         tiles=8, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=4)),
    dict(kernel='corr_kernel<1, 1, 1, 8, 1, true>', op='dgrad', geom=(2, 20, 8, 16, 24, 'SAME'), target=16, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<1, 1, 1, 8, 1, true>', op='dgrad', geom=(2, 20, 16, 8, 24, 'SAME'), target=16, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<1, 1, 1, 8, 1, true>', op='dgrad_masked', geom=(2, 20, 8, 16, 24, 'SAME'), target=16, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<1, 1, 1, 8, 1, true>', op='dgrad_masked', geom=(2, 20, 16, 8, 24, 'SAME'), target=16, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<2, 1, 1, 8, 1, true>', op='dgrad', geom=(4, 20, 8, 16, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<2, 1, 1, 8, 1, true>', op='dgrad', geom=(4, 20, 16, 8, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<2, 1, 1, 8, 1, true>', op='dgrad_masked', geom=(4, 20, 8, 16, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 4, 8), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<2, 1, 1, 8, 1, true>', op='dgrad_masked', geom=(4, 20, 16, 8, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(1, 8, 4), xq=4, xcd_p=0)),
    # pad_t != pad_l: (7, 8) has SAME pads (2, 1), (8, 28) has (1, 1) over 4 x 14 outputs
    dict(kernel='corr_kernel<0, 1, 1, 8, 1, true>', op='fwd', geom=(2, 12, 7, 8, 40, 'SAME'), target=4, env={},
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=5, tile=(2, 4, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<0, 2, 1, 4, 1, true>', op='fwd', geom=(2, 12, 8, 28, 40, 'SAME'), target=4, env={},
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=4, tile=(1, 4, 14), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<1, 2, 1, 4, 2, true>', op='dgrad', geom=(2, 20, 7, 8, 24, 'SAME'), target=2, env=_DG0,
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=4, tile=(2, 4, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<1, 2, 1, 4, 2, true>', op='dgrad_masked', geom=(2, 20, 7, 8, 24, 'SAME'), target=2, env=_DG0,
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=4, tile=(2, 4, 4), xq=4, xcd_p=0)),
    dict(kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad', geom=(2, 20, 8, 28, 24, 'SAME'), target=2, env=_DG0,
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 4, 14), xq=1, xcd_p=0)),
    dict(kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad_masked', geom=(2, 20, 8, 28, 24, 'SAME'), target=2, env=_DG0,
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 4, 14), xq=1, xcd_p=0)),
    dict(kernel='wgrad_kernel<0>', op='wgrad', geom=(3, 20, 7, 8, 24, 'SAME'), target=6, env={},
         tiles=4, sk=1, block=512, also=()),
    dict(kernel='wgrad_kernel<0>', op='wgrad_act', geom=(3, 20, 7, 8, 24, 'SAME'), target=6, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k', 'chansum<part>', 'chansum_final'),
         note='a 48-pixel chunk has no in-kernel bias sum: the widened path, channel sums of the masked copy'),
    dict(kernel='wgrad_kernel<2>', op='wgrad', geom=(2, 20, 8, 28, 24, 'SAME'), target=6, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k',)),
    dict(kernel='wgrad_kernel<2>', op='wgrad_act', geom=(2, 20, 8, 28, 24, 'SAME'), target=6, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k',)),
    # the three thin kernels (image side of <= 4 channels) at (16, 32) and (32, 16)
    dict(kernel='thin_fwd_kernel', op='fwd', geom=(2, 3, 16, 32, 64, 'SAME'), target=1, env={}, tiles=4, sk=1, block=512, also=()),
    dict(kernel='thin_fwd_kernel', op='fwd', geom=(2, 3, 32, 16, 64, 'SAME'), target=1, env={}, tiles=4, sk=1, block=512, also=()),
    dict(kernel='thin_fwd_kernel', op='fwd_masked', geom=(2, 3, 16, 32, 64, 'SAME'), target=1, env={}, tiles=4, sk=1, block=512, also=()),
    dict(kernel='thin_fwd_kernel', op='fwd_masked', geom=(2, 3, 32, 16, 64, 'SAME'), target=1, env={}, tiles=4, sk=1, block=512, also=()),
    dict(kernel='thin_dgrad_kernel', op='dgrad', geom=(2, 3, 16, 32, 32, 'SAME'), target=1, env={}, tiles=8, sk=1, block=512, also=()),
    dict(kernel='thin_dgrad_kernel', op='dgrad', geom=(2, 3, 32, 16, 32, 'SAME'), target=1, env={}, tiles=16, sk=1, block=512, also=()),
    dict(kernel='thin_dgrad_kernel', op='dgrad_masked', geom=(2, 3, 16, 32, 32, 'SAME'), target=1, env={}, tiles=8, sk=1, block=512, also=()),
    dict(kernel='thin_dgrad_kernel', op='dgrad_masked', geom=(2, 3, 32, 16, 32, 'SAME'), target=1, env={}, tiles=16, sk=1, block=512, also=()),
    dict(kernel='thin_wgrad_kernel', op='wgrad', geom=(6, 3, 16, 32, 32, 'SAME'), target=6, env={},
         tiles=2, sk=12, block=1024, also=('splitk_reduce_small_k',)),
    dict(kernel='thin_wgrad_kernel', op='wgrad', geom=(6, 3, 32, 16, 32, 'SAME'), target=6, env={},
         tiles=2, sk=24, block=1024, also=('splitk_reduce_small_k',)),
    dict(kernel='thin_wgrad_kernel', op='wgrad_act', geom=(6, 3, 16, 32, 32, 'SAME'), target=6, env={},
         tiles=2, sk=12, block=1024, also=('splitk_reduce_small_k',)),
    dict(kernel='thin_wgrad_kernel', op='wgrad_act', geom=(6, 3, 32, 16, 32, 'SAME'), target=6, env={},
         tiles=2, sk=24, block=1024, also=('splitk_reduce_small_k',)),
    # wgrad_kernel<..> at (8, 16) and (16, 8): its host predicate looks at W, Wo and pad_l only
    dict(kernel='wgrad_kernel<0>', op='wgrad', geom=(3, 20, 8, 16, 40, 'SAME'), target=6, env={}, tiles=6, sk=1, block=512, also=()),
    dict(kernel='wgrad_kernel<1>', op='wgrad_act', geom=(3, 20, 8, 16, 40, 'SAME'), target=6, env={}, tiles=6, sk=1, block=512, also=()),
    dict(kernel='wgrad_kernel<0>', op='wgrad', geom=(3, 20, 16, 8, 40, 'SAME'), target=6, env={}, tiles=6, sk=1, block=512, also=()),
    dict(kernel='wgrad_kernel<1>', op='wgrad_act', geom=(3, 20, 16, 8, 40, 'SAME'), target=6, env={}, tiles=6, sk=1, block=512, also=()),
    # masked rows for the select sites the dispatch table reaches with plain operands only
    dict(kernel='wgrad4_kernel<16>', op='wgrad_act', geom=(4, 20, 16, 16, 40, 'SAME'), target=4, env={'GGAN_WGRAD_SPLIT': '0'},
         tiles=4, sk=1, block=256, also=()),
    dict(kernel='conv_dgrad_naive', op='dgrad_masked', geom=(2, 5, 16, 16, 6, 'SAME'), target=1, env={}, tiles=10, sk=1, block=256, also=()),
    dict(kernel='conv_wgrad_naive', op='wgrad_act', geom=(1, 5, 4, 132, 6, 'SAME'), target=1, env={}, tiles=3, sk=1, block=256, also=(),
         nobias=True),
]

# One operand one float off a 16-byte boundary: the kernel that must run instead of the one the aligned call gets.  Outputs stay aligned.
MISALIGNED = [
    # forward (conv_corr.hip): x drops to the X4 = false instance, w to the plain kernel
    dict(off='x', kernel='corr_kernel<0, 2, 1, 4, 1, false>', op='fwd', geom=(4, 12, 12, 12, 40, 'SAME'), target=8, env={},
         tiles=8, sk=1, block=512, also=(), plan=dict(cfg=4, tile=(1, 6, 6), xq=1, xcd_p=4)),
    dict(off='w', kernel='conv_fwd_naive', op='fwd', geom=(4, 12, 12, 12, 40, 'SAME'), target=8, env={},
         tiles=23, sk=1, block=256, also=()),
    # thin forward (conv_thin.hip): x and w hand the layer to conv_corr.hip / the plain kernel
    dict(off='x', kernel='corr_kernel<0, 2, 2, 2, 1, false>', op='fwd', geom=(2, 3, 16, 16, 64, 'SAME'), target=1, env={},
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=6, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='w', kernel='conv_fwd_naive', op='fwd', geom=(2, 3, 16, 16, 64, 'SAME'), target=1, env={},
         tiles=32, sk=1, block=256, also=()),
    # data gradient (conv_corr.hip): gy and the mask reference drop to X4 = false, w to the plain kernel
    dict(off='gy', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad', geom=(4, 20, 16, 16, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='yref', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad_masked', geom=(4, 20, 16, 16, 24, 'SAME'), target=4, env=_DG0,
         tiles=4, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='w', kernel='conv_dgrad_naive', op='dgrad_masked', geom=(4, 20, 16, 16, 24, 'SAME'), target=4, env=_DG0,
         tiles=80, sk=1, block=256, also=()),
    # dg16 (conv_dg16.hip): every operand hands the call to the class kernels of conv_corr.hip
    dict(off='gy', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad', geom=(3, 32, 16, 16, 48, 'SAME'), target=2,
         env={'GGAN_DG16': '1', 'GGAN_DG16_FORCE': '1'}, tiles=3, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='yref', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad_masked', geom=(3, 32, 16, 16, 48, 'SAME'), target=2,
         env={'GGAN_DG16': '1', 'GGAN_DG16_FORCE': '1'}, tiles=3, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='w', kernel='conv_dgrad_naive', op='dgrad', geom=(3, 32, 16, 16, 48, 'SAME'), target=2,
         env={'GGAN_DG16': '1', 'GGAN_DG16_FORCE': '1'}, tiles=96, sk=1, block=256, also=()),
    # thin data gradient
    dict(off='gy', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad', geom=(2, 3, 16, 16, 32, 'SAME'), target=1, env={},
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='yref', kernel='corr_kernel<2, 2, 1, 4, 2, false>', op='dgrad_masked', geom=(2, 3, 16, 16, 32, 'SAME'), target=1, env={},
         tiles=2, sk=1, block=512, also=(), plan=dict(cfg=7, tile=(1, 8, 8), xq=1, xcd_p=0)),
    dict(off='w', kernel='conv_dgrad_naive', op='dgrad', geom=(2, 3, 16, 16, 32, 'SAME'), target=1, env={},
         tiles=6, sk=1, block=256, also=()),
    # filter gradient (conv_wgrad.hip): the widened path copies the operand (and applies the mask) into the workspace, 16-byte aligned
    dict(off='x', kernel='wgrad4_kernel<16, true>', op='wgrad', geom=(4, 20, 16, 16, 40, 'SAME'), target=4, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k',)),
    dict(off='gy', kernel='wgrad4_kernel<16, true>', op='wgrad', geom=(4, 20, 16, 16, 40, 'SAME'), target=4, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k',)),
    dict(off='yref', kernel='wgrad4_kernel<16, true>', op='wgrad_act', geom=(4, 20, 16, 16, 40, 'SAME'), target=4, env={},
         tiles=4, sk=1, block=512, also=('pad_width_k',)),
    # thin filter gradient: conv_wgrad.hip refuses the operand too, the widened path takes it
    dict(off='x', kernel='wgrad4_kernel<16, true>', op='wgrad', geom=(6, 3, 16, 16, 32, 'SAME'), target=6, env={},
         tiles=1, sk=1, block=512, also=('pad_width_k',)),
    dict(off='gy', kernel='wgrad4_kernel<16, true>', op='wgrad', geom=(6, 3, 16, 16, 32, 'SAME'), target=6, env={},
         tiles=1, sk=1, block=512, also=('pad_width_k',)),
    dict(off='yref', kernel='wgrad4_kernel<16, true>', op='wgrad_act', geom=(6, 3, 16, 16, 32, 'SAME'), target=6, env={},
         tiles=1, sk=1, block=512, also=('pad_width_k',)),
]

ALL_ROWS = ROWS + EXTRA_ROWS + MISALIGNED


def guard_id(row):
    return ('off_%s-' % row['off'] if 'off' in row else '') + row_id(row) + ('-nobias' if row.get('nobias') else '')


def data_sets(row):
    return ('gauss',) if row['op'] in GAUSS_ONLY_OPS else ('gauss', 'exact')


def masks(row):
    return ('lrelu', 'relu') if row['op'] in MASKED_OPS else (None,)


def find_row(op, geom5):
    """the first row of ROWS + EXTRA_ROWS with this op and (N, Ci, H, W, Co)"""
    for r in ROWS + EXTRA_ROWS:
        if r['op'] == op and tuple(r['geom'][:5]) == tuple(geom5):
            return r
    raise KeyError((op, geom5))


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def same_pads(size, k=5, stride=2):
    """-> (outputs, pad in front) of TF's SAME padding"""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2


def out_hw(row):
    return same_pads(row['geom'][2])[0], same_pads(row['geom'][3])[0]


def band(row):
    """floats of NaN on each side of every operand and output: at least one image plane and no less than 1024, a multiple of 4"""
    N, Ci, H, W, Co, _ = row['geom']
    return (max(H * W, 1024) + 3) & ~3


def exact_bound(row):
    """the largest |value| any partial sum of the 'exact' data set can reach (|x|, |gy| <= 2, |w| <= 1, |bias| <= 3)"""
    N, Ci, H, W, Co, _ = row['geom']
    Ho, Wo = out_hw(row)
    op = row['op']
    if op.startswith('fwd'):
        return 2 * 25 * Ci + 3
    if op.startswith('dgrad'):
        return 2 * 25 * Co + 3
    return 4 * N * Ho * Wo               # filter gradient; the bias sum is half of it


# ---------------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------------
def mask_reference(rng, shape):
    """continuous, except a tenth of the entries: exactly +0 and -0, half each"""
    r = rng.standard_normal(shape).astype(np.float32)
    r[r == 0.0] = 0.5
    flat = r.reshape(-1)
    idx = rng.permutation(flat.size)[:max(2, flat.size // 10)]
    flat[idx[0::2]] = 0.0
    flat[idx[1::2]] = -0.0
    assert np.signbit(flat[idx[1::2]]).all() and not np.signbit(flat[idx[0::2]]).any()
    return r


def inputs(row, data, mask=None):
    """-> dict of float32 arrays x, w, gy, yref, b_o, b_i (and ring for fwd_cast), plus alpha and mask"""
    assert data in data_sets(row) and mask in masks(row), (row, data, mask)
    N, Ci, H, W, Co, pad = row['geom']
    Ho, Wo = out_hw(row)
    rng = np.random.default_rng(zlib.crc32(('%s %s' % (guard_id(row), data)).encode()))
    if data == 'gauss':
        x = rng.standard_normal((N, Ci, H, W)).astype(np.float32)
        w = (rng.standard_normal((5, 5, Ci, Co)) / np.sqrt(25 * Ci)).astype(np.float32)
        gy = rng.standard_normal((N, Co, Ho, Wo)).astype(np.float32)
        b_o, b_i = rng.standard_normal(Co).astype(np.float32), rng.standard_normal(Ci).astype(np.float32)
    else:
        assert exact_bound(row) < 2 ** 23
        x = rng.integers(-2, 3, size=(N, Ci, H, W)).astype(np.float32)
        w = rng.integers(-1, 2, size=(5, 5, Ci, Co)).astype(np.float32)
        gy = rng.integers(-2, 3, size=(N, Co, Ho, Wo)).astype(np.float32)
        b_o, b_i = rng.integers(-3, 4, size=Co).astype(np.float32), rng.integers(-3, 4, size=Ci).astype(np.float32)
    inp = dict(x=x, w=w, gy=gy, b_o=b_o, b_i=b_i, alpha=ALPHA[data], mask=mask, yref=mask_reference(rng, (N, Co, Ho, Wo)))
    if row['op'] == 'fwd_cast':
        inp['ring'] = rng.integers(0, 256, size=(2, N, Ci * H * W)).astype(np.int32)
    return inp


def slope(inp, yref=None, ge=False):
    """the activation derivative at the mask reference: 1 where it is > 0 (`ge`: >= 0, the mutant), else alpha (lrelu) or 0 (relu)"""
    r = inp['yref'] if yref is None else yref
    return np.where((r >= 0) if ge else (r > 0), 1.0, inp['alpha'] if inp['mask'] == 'lrelu' else 0.0)


def reference(row, inp, sl=None):
    """float64, through oracle.ops -> {output name: array}.  `sl` replaces the mask's slope (mutants)."""
    from oracle import ops as O
    op = row['op']
    N, Ci, H, W, Co, pad = row['geom']
    x, w, gy = inp['x'].astype(np.float64), inp['w'].astype(np.float64), inp['gy'].astype(np.float64)
    b_o, b_i = inp['b_o'].astype(np.float64).reshape(1, -1, 1, 1), inp['b_i'].astype(np.float64).reshape(1, -1, 1, 1)
    if op in MASKED_OPS and sl is None:
        sl = slope(inp)
    if op == 'fwd':
        return dict(y=O.conv2d(x, w, 2, pad) + b_o)
    if op == 'fwd_masked':
        return dict(y=O.conv2d(x, w, 2, pad) * sl)
    if op == 'fwd_cast':
        xs = 2.0 * (inp['ring'][1].astype(np.float64) / 255.0 - 0.5).reshape(N, Ci, H, W)
        return dict(x=xs, y=O.conv2d(xs, w, 2, pad) + b_o)
    if op == 'dgrad':
        return dict(gx=O.conv2d_bwd_data(gy, w, (H, W), 2, pad))
    if op == 'dgrad_bias_act':
        return dict(gx=np.maximum(O.conv2d_bwd_data(gy, w, (H, W), 2, pad) + b_i, 0.0))
    if op == 'dgrad_masked':
        return dict(gx=O.conv2d_bwd_data(gy * sl, w, (H, W), 2, pad))
    if op == 'wgrad':
        return dict(gw=O.conv2d_bwd_filter(x, gy, 5, 2, pad))
    assert op in ('wgrad_act', 'wgrad_parts'), op
    out = dict(gw=O.conv2d_bwd_filter(x, gy * sl, 5, 2, pad))
    if not row.get('nobias'):
        out['gb'] = (gy * sl).sum((0, 2, 3))
    return out


def tolerance(row):
    return TOL_LONG if row['op'].startswith('wgrad') else TOL


# ---------------------------------------------------------------------------------------------------------------------------------
# workspace layout
# ---------------------------------------------------------------------------------------------------------------------------------
def out_elems(row):
    """floats of the output the split-K slabs are slabs of"""
    N, Ci, H, W, Co, _ = row['geom']
    Ho, Wo = out_hw(row)
    op = row['op']
    if op.startswith('fwd'):
        return N * Co * Ho * Wo
    if op.startswith('dgrad'):
        return N * Ci * H * W
    return 25 * Ci * Co


def slab_stride(row):
    """floats between split-K slabs: the filter-gradient kernels append the Co bias partials when they sum the bias themselves"""
    in_kernel_bias = row['op'] == 'wgrad_act' and not row.get('nobias') and 'chansum_final' not in row['also']
    return out_elems(row) + (row['geom'][4] if in_kernel_bias or row['op'] == 'wgrad_parts' else 0)


def ws_segments(row):
    """[(first float behind the head, floats)]: what of the workspace a correct run leaves finite.  sk > 1: sk slabs in a row.  The
    widened filter gradient (pad_width_k) first keeps its zero-extended copies of x and gy there, each rounded up to 256 bytes; the
    launches behind them skip a reserved head of their own, and the channel sums keep min(1024 // Co, N) partials per channel."""
    if row['op'] == 'wgrad_parts':
        return []
    N, Ci, H, W, Co, _ = row['geom']
    Ho, Wo = out_hw(row)
    segs, base = [], 0
    if 'pad_width_k' in row['also']:
        shift = same_pads(W)[1] - 1
        wop = (Wo + 3) & ~3
        while 2 * wop < W + shift:
            wop += 4
        xf, gf = N * Ci * H * 2 * wop, N * Co * Ho * wop
        segs += [(0, xf), ((xf + 63) & ~63, gf)]
        base = ((xf + 63) & ~63) + ((gf + 63) & ~63) + WS_RESERVED // 4
    if row['sk'] > 1:
        segs.append((base, row['sk'] * slab_stride(row)))
    if 'chansum<part>' in row['also']:
        segs.append((base, Co * min(1024 // Co, N)))
    return segs


# ---------------------------------------------------------------------------------------------------------------------------------
# check
# ---------------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max() / (np.abs(ref).max() + 1e-30))


def check(row, data, bufs, recs):
    """Pure numpy over whole buffers, bands included; raises AssertionError, returns {output: relative error}.
    bufs: {'out': {name: (whole float32 buffer, floats in front of the output, output shape)}, 'ws': whole workspace or None,
           'part': (whole buffer, floats in front, floats of capacity) for wgrad_parts}
    recs: {'ref': {name: float64 reference}, 'n_parts', 'stride' (wgrad_parts: what the entry point returned)}"""
    ref = recs['ref']
    exact = data == 'exact'
    # 1. bands
    outs = dict(bufs['out'])
    views = {}
    for name, (whole, off, shape) in outs.items():
        n = int(np.prod(shape))
        b = _bits(whole)
        assert off >= 4 and whole.size - off - n >= 4, (name, off, n, whole.size)
        assert np.all(b[:off] == NAN_BITS), '%s: a store in front of the output (%d floats)' % (name, int((b[:off] != NAN_BITS).sum()))
        assert np.all(b[off + n:] == NAN_BITS), '%s: a store behind the output (%d floats)' % (name, int((b[off + n:] != NAN_BITS).sum()))
        views[name] = whole[off:off + n].reshape(shape)
    if 'part' in bufs:
        whole, off, cap = bufs['part']
        b = _bits(whole)
        assert np.all(b[:off] == NAN_BITS) and np.all(b[off + cap:] == NAN_BITS), 'part: a store outside the partial buffer'
    # 2. every element finite
    for name, v in views.items():
        assert np.all(np.isfinite(v)), '%s: %d elements nobody stored, or not finite' % (name, int((~np.isfinite(v)).sum()))
    # 3. / 4. workspace
    ws = bufs.get('ws')
    if ws is not None:
        head = WS_RESERVED // 4
        assert np.all(_bits(ws[:head]) == 0), 'the reserved head of the workspace was written'
        want = np.zeros(ws.size - head, dtype=bool)
        for first, count in ws_segments(row):
            assert first + count <= want.size, (first, count)
            want[first:first + count] = True
        fin = np.isfinite(ws[head:])
        assert np.all(fin[want]), 'workspace: %d floats of the row\'s %d slabs were never written' % (int((~fin[want]).sum()), row['sk'])
        assert np.all(_bits(ws[head:])[~want] == NAN_BITS), 'workspace: %d floats written outside the row\'s slabs' % int(fin[~want].sum())
    else:
        assert not ws_segments(row), row
    # 7. wgrad_parts: the slabs, bias tails included, then what pack made of them
    errs = {}
    if row['op'] == 'wgrad_parts':
        whole, off, cap = bufs['part']
        n, stride = recs['n_parts'], recs['stride']
        elems = out_elems(row)
        assert n == row['sk'] and stride == elems + row['geom'][4] and n * stride <= cap, (n, stride, cap)
        slabs = whole[off:off + n * stride].reshape(n, stride)
        assert np.all(np.isfinite(slabs)), 'part: %d floats of the %d slabs never written' % (int((~np.isfinite(slabs)).sum()), n)
        assert np.all(_bits(whole[off + n * stride:off + cap]) == NAN_BITS), 'part: floats written behind the last slab'
        total = slabs.astype(np.float64).sum(0)
        views = dict(views, slabs_gw=total[:elems].reshape(ref['gw'].shape), slabs_gb=total[elems:])
        ref = dict(slabs_gw=ref['gw'], slabs_gb=ref['gb'], flat=np.concatenate([ref['gw'].reshape(-1), ref['gb']]))
    # 5. / 6. values: no element excused
    assert sorted(views) == sorted(ref), (sorted(views), sorted(ref))
    tol = tolerance(row)
    for name in sorted(views):
        got, want = views[name], ref[name]
        assert got.shape == want.shape, (name, got.shape, want.shape)
        if exact:
            assert np.array_equal(got.astype(np.float64), want), '%s: %d of %d elements differ' % (name, int((got != want).sum()), got.size)
            errs[name] = 0.0
        else:
            errs[name] = rel(got, want)
            assert errs[name] < tol, (name, errs[name], tol)
    return errs


def present_check(row, got, ref):
    """what test_conv_dispatch_gpu.py asks of a result: the shape and the relative error, nothing else"""
    return all(got[k].shape == ref[k].shape and rel(got[k], ref[k]) < tolerance(row) for k in ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# a correct run, in numpy
# ---------------------------------------------------------------------------------------------------------------------------------
def _banded(a, width):
    a = np.ascontiguousarray(a, dtype=np.float32)
    whole = np.full(width + a.size + width, np.nan, dtype=np.float32)
    assert np.all(_bits(whole) == NAN_BITS)
    whole[width:width + a.size] = a.reshape(-1)
    return whole, width, a.shape


def simulate(row, data, mask=None, got=None):
    """-> (bufs, recs) as a correct kernel leaves them: `got` (default: the float64 reference rounded to float32) inside NaN bands, the
    workspace with a zero head and the row's slabs (two halves of the result and zeros), NaN elsewhere"""
    inp = inputs(row, data, mask)
    ref = reference(row, inp)
    if got is None:
        got = {k: v.astype(np.float32) for k, v in ref.items()}
    bw = band(row)
    head = WS_RESERVED // 4
    ws = np.full(head + WS_FLOATS, np.nan, dtype=np.float32)
    ws[:head] = 0.0
    for first, count in ws_segments(row):
        ws[head + first:head + first + count] = 0.0
    bufs, recs = dict(out={}, ws=ws), dict(ref=ref)
    main = [k for k in ('y', 'gx', 'gw') if k in got][0]
    if row['op'] == 'wgrad_parts':
        elems, stride, n = out_elems(row), slab_stride(row), row['sk']
        flat = np.concatenate([got['gw'].reshape(-1), got['gb']])
        part = np.full(PARTS_CAP * stride, np.nan, dtype=np.float32)
        part[:n * stride] = 0.0
        part[:stride] = flat
        if n > 1:
            part[:stride] = flat / 2
            part[stride:2 * stride] = flat / 2
        whole, off, _ = _banded(part, bw)
        bufs['part'] = (whole, off, part.size)
        bufs['out']['flat'] = _banded(flat, bw)
        bufs['ws'] = None
        recs.update(n_parts=n, stride=stride)
        return bufs, recs
    if row['sk'] > 1:
        first, stride = ws_segments(row)[-1 if 'chansum<part>' not in row['also'] else -2][0], slab_stride(row)
        half = got[main].reshape(-1) / 2
        for s in (0, 1):
            ws[head + first + s * stride:head + first + s * stride + half.size] = half
    for k, v in got.items():
        bufs['out'][k] = _banded(v, bw)
    return bufs, recs


# ---------------------------------------------------------------------------------------------------------------------------------
# mutants: what a subtly wrong kernel leaves behind, built from a correct run
# ---------------------------------------------------------------------------------------------------------------------------------
def conv_explicit(x, w, pt, pl, Ho, Wo, top=None):
    """forward with explicit pads in float64.  `top`: [N * Ci, pt, W] rows that stand where the zero rows above each plane should"""
    N, Ci, H, W = x.shape
    P = 4
    xp = np.zeros((N, Ci, H + 2 * P, W + 2 * P))
    xp[:, :, P:P + H, P:P + W] = x
    if top is not None and pt:
        xp[:, :, P - pt:P, P:P + W] = top.reshape(N, Ci, pt, W)
    y = np.zeros((N, Ho, Wo, w.shape[3]))
    for i in range(5):
        for j in range(5):
            patch = xp[:, :, P - pt + i:P - pt + i + 2 * Ho:2, P - pl + j:P - pl + j + 2 * Wo:2]
            y += np.tensordot(patch, w[i, j].astype(np.float64), axes=([1], [0]))
    return np.ascontiguousarray(y.transpose(0, 3, 1, 2))


def _m_store_behind(row, data, mask):
    bufs, recs = simulate(row, data, mask)
    whole, off, shape = bufs['out']['y']
    whole[off + int(np.prod(shape))] = 1.0
    return bufs, recs


def _never_stored_result(row, data, mask):
    """the last image's first pixel quad of channel 0 is never stored: the buffer keeps what it held"""
    bufs, recs = simulate(row, data, mask)
    whole, off, shape = bufs['out']['y']
    n_img = int(np.prod(shape[1:]))
    return bufs, recs, slice(off + (shape[0] - 1) * n_img, off + (shape[0] - 1) * n_img + 4)


def _m_quad_never_stored(row, data, mask):
    bufs, recs, quad = _never_stored_result(row, data, mask)
    bufs['out']['y'][0][quad] = np.nan                     # the output started as NaN
    return bufs, recs


def _m_nan_top_halo(row, data, mask):
    """the rows above image 0 are read from in front of the tensor, where the band is NaN: one product reaches one output"""
    bufs, recs = simulate(row, data, mask)
    whole, off, shape = bufs['out']['y']
    whole[off] = np.nan
    return bufs, recs


def _m_unwritten_slab_added(row, data, mask):
    """the reduction adds sk + 1 slabs: the last one was never written and is NaN in this workspace, zeros in a zeroed one"""
    bufs, recs = simulate(row, data, mask)
    whole, off, shape = bufs['out']['y']
    whole[off:off + int(np.prod(shape))] = np.nan
    return bufs, recs


def _m_slab_twice(row, data, mask):
    bufs, recs = simulate(row, data, mask)
    whole, off, shape = bufs['out']['y']
    n = int(np.prod(shape))
    first = ws_segments(row)[-1][0]
    whole[off:off + n] += bufs['ws'][WS_RESERVED // 4 + first:WS_RESERVED // 4 + first + n]
    return bufs, recs


def ge_result(row, data, mask, yref=None):
    """the op with the mask written as >= (float32), and the reference of the same inputs; `yref` replaces the mask reference"""
    inp = inputs(row, data, mask)
    if yref is not None:
        inp = dict(inp, yref=yref)
    return ({k: v.astype(np.float32) for k, v in reference(row, inp, sl=slope(inp, ge=True)).items()}, reference(row, inp))


def _m_mask_ge(row, data, mask):
    return simulate(row, data, mask, got=ge_result(row, data, mask)[0])


def _m_pads_swapped(row, data, mask):
    inp = inputs(row, data, mask)
    N, Ci, H, W, Co, _ = row['geom']
    (Ho, pt), (Wo, pl) = same_pads(H), same_pads(W)
    assert pt != pl
    y = conv_explicit(inp['x'].astype(np.float64), inp['w'], pl, pt, Ho, Wo) + inp['b_o'].astype(np.float64).reshape(1, -1, 1, 1)
    return simulate(row, data, mask, got=dict(y=y.astype(np.float32)))


def _m_halo_from_previous_image(row, data, mask):
    """the pad rows above a plane hold the last rows of the plane in front of it in memory (zeros above the very first)"""
    inp = inputs(row, data, mask)
    N, Ci, H, W, Co, _ = row['geom']
    (Ho, pt), (Wo, pl) = same_pads(H), same_pads(W)
    planes = inp['x'].astype(np.float64).reshape(N * Ci, H, W)
    top = np.zeros((N * Ci, pt, W))
    top[1:] = planes[:-1, H - pt:, :]
    y = conv_explicit(inp['x'].astype(np.float64), inp['w'], pt, pl, Ho, Wo, top=top) + inp['b_o'].astype(np.float64).reshape(1, -1, 1, 1)
    return simulate(row, data, mask, got=dict(y=y.astype(np.float32)))


# name -> (builder, data set, mask)
MUTANTS = {
    'store_behind_output': (_m_store_behind, 'gauss', None),
    'quad_never_stored': (_m_quad_never_stored, 'gauss', None),
    'nan_through_top_halo': (_m_nan_top_halo, 'gauss', None),
    'unwritten_slab_added': (_m_unwritten_slab_added, 'gauss', None),
    'slab_counted_twice': (_m_slab_twice, 'exact', None),
    'mask_ge_lrelu': (_m_mask_ge, 'gauss', 'lrelu'),
    'mask_ge_relu': (_m_mask_ge, 'gauss', 'relu'),
    'pads_swapped': (_m_pads_swapped, 'gauss', None),
    'halo_from_previous_image': (_m_halo_from_previous_image, 'gauss', None),
}

# name -> (op, (N, Ci, H, W, Co)) of the row the mutant is caught on
MUTANT_ROW = {
    'store_behind_output': ('fwd', (3, 6, 16, 16, 20)),
    'quad_never_stored': ('fwd', (3, 12, 14, 14, 20)),          # ragged image group: 3 images, 2 per tile
    'nan_through_top_halo': ('fwd', (3, 6, 16, 16, 20)),
    'unwritten_slab_added': ('fwd', (2, 64, 8, 8, 32)),         # SK = 2
    'slab_counted_twice': ('fwd', (2, 64, 8, 8, 32)),
    'mask_ge_lrelu': ('fwd_masked', (4, 12, 12, 12, 40)),
    'mask_ge_relu': ('dgrad_masked', (4, 20, 16, 16, 24)),
    'pads_swapped': ('fwd', (2, 12, 7, 8, 40)),
    'halo_from_previous_image': ('fwd', (3, 6, 16, 16, 20)),
}


def mutant(name):
    """-> (row, data, bufs, recs) of the mutant on its row"""
    fn, data, mask = MUTANTS[name]
    row = find_row(*MUTANT_ROW[name])
    bufs, recs = fn(row, data, mask)
    return row, data, bufs, recs
