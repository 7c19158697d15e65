"""Which kernel instance of the 3-D convolution family (csrc/conv3d.hip) each dispatch test runs: one row per instance, step count,
split and edge geometry (plain data), and the host side of those tests: the rows' inputs and their float64 references.

tests/test_conv3d_dispatch_gpu.py runs every row's C entry point, asserts that the profiler saw exactly the row's launches -- every
label with its count and its grid -- and that every output matches the float64 oracle (oracle.ops.conv3d, conv3d_bwd_data,
conv3d_bwd_filter) evaluated on the float32-rounded inputs.  tests/test_conv3d_dispatch_cpu.py parses the GGAN_LAUNCH sites of
conv3d.hip and fails when a label or a template instance has no row, a row names no launch or two kernels share a label; it
recomputes every row's launches and plan from a Python transcription of fill / ig_ok / ig_split / the three entry points /
launch_splitk_reduce, and it checks the kernels' FastDiv divisions by brute force over every numerator a row forms.

A row:
  entry     fwd (ggan_conv3d_fwd) | wgrad (ggan_conv3d_wgrad) | dgrad (ggan_conv3d_dgrad) | im2col (ggan_im2col3d) | col2im (ggan_col2im3d)
  dims      (N, L, H, W, Ci, Co, fl, fs, stride_len, stride): x [N, L, H, W, Ci], filter [fl, fs, fs, Ci, Co], SAME padding
  bias, act, alpha    fwd: a bias is passed; the fused epilogue none | lrelu (alpha 0.2)
  ws        fwd / wgrad: the workspace handed in -- None, or the float count AFTER the kWsReserved bytes every workspace starts with
  off       the operands whose base lies one float past a 16-byte boundary (names as in include/ggan.h: x, w, y, gy, gw, gx, col)
  refused   the entry point must return non-zero, launch nothing and leave its NaN output NaN (launches (), plan None)
  run       None, or the reason the GPU module does not run the row (the two size_t instances of the layout kernels only)
  exact     the data are -1, 0, 1 and the comparison is equality (FASTDIV_ROWS)
  launches  ((label, launches, (grid x, y, z), block), ...) in launch order
  plan      fwd / wgrad: dict(SK, kps, steps, last) -- splits of the reduction, its length per split, k-steps of 32 a full split walks,
            length of the last split;  dgrad: dict(nc, classes ((M, K), ...)) -- the residue classes that have rows
  note      which edge the row is there for

To add a row: pick the smallest geometry that reaches the path, ragged against the tile (128x32 up to 32 result columns, else
64x64; filter gradient 64x64) unless the edge is the tile itself, let `planned()` of test_conv3d_dispatch_cpu.py compute launches and
plan, write them into the row, and run the two dispatch modules.
"""
import zlib

import numpy as np

ALPHA = 0.2
ACTS = ('none', 'lrelu')                   # position = GGAN_ACT_* code
WS_RESERVED = 16384                        # GGAN_WS_RESERVED of include/ggan.h, bytes
BIG = 4194304                              # a generous workspace: 16 MB of floats
ENTRY = dict(fwd='ggan_conv3d_fwd', wgrad='ggan_conv3d_wgrad', dgrad='ggan_conv3d_dgrad', im2col='ggan_im2col3d', col2im='ggan_col2im3d')
KIND = dict(fwd=0, wgrad=1, dgrad=2)
RS, RK = 'splitk_reduce_small_k', 'splitk_reduce_k'
SIZE_T_LABELS = ('im2col3d_k<size_t, 4>', 'im2col3d_k<size_t, 1>', 'col2im3d_k<size_t, 4>', 'col2im3d_k<size_t, 1>')
NOT_RUN = 'needs at least 0xF0000000 elements (15 GB of float32) before the 64-bit index instance is chosen'


def ig(kind, wm, wn, av4):
    return 'conv3d_igemm_k<%d, %d, %d, %s>' % (kind, wm, wn, 'true' if av4 else 'false')


def _row(entry, dims, launches, plan, bias=False, act='none', ws=None, off=(), refused=False, run=None, exact=False, note=''):
    return dict(entry=entry, dims=tuple(dims), bias=bias, act=act, alpha=ALPHA if act == 'lrelu' else 0.0, ws=ws, off=tuple(off),
                refused=refused, run=run, exact=exact, launches=tuple(launches), plan=plan, note=note)


ROWS = [
    # ---- ggan_conv3d_fwd: steps per split 1..5 at SK = 1 (Ci = 4: K = 20, 36, 72, 128, 144), both tiles, the direct epilogue
    _row('fwd', (2, 3, 5, 7, 4, 12, 5, 1, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 20}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 12, 1, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 96, 'steps': 3, 'last': 72}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 12, 2, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 12, 4, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 160, 'steps': 5, 'last': 144}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 36, 1, 3, 1, 1), (('conv3d_igemm_k<0, 2, 2, true>', 1, (4, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 4, 36, 4, 3, 1, 1), (('conv3d_igemm_k<0, 2, 2, true>', 1, (4, 1, 1), 256),), {'SK': 1, 'kps': 160, 'steps': 5, 'last': 144}, ws=BIG, bias=True, act='lrelu', note='direct launch with the bias + LeakyReLU epilogue'),
    # ---- forward, AV4 = false: four dword gathers per unit, at every thin channel count
    _row('fwd', (2, 3, 5, 7, 1, 12, 2, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 18}, ws=BIG, note='Ci = 1: the unit k = 8..11 straddles a tw wrap and a th wrap'),
    _row('fwd', (2, 3, 5, 7, 1, 36, 3, 3, 1, 1), (('conv3d_igemm_k<0, 2, 2, false>', 1, (4, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 27}, ws=BIG, bias=True),
    _row('fwd', (2, 3, 5, 7, 2, 12, 2, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 3, 36, 3, 3, 1, 1), (('conv3d_igemm_k<0, 2, 2, false>', 1, (4, 1, 1), 256),), {'SK': 1, 'kps': 96, 'steps': 3, 'last': 81}, ws=BIG, note='K = 81, K % 4 != 0'),
    _row('fwd', (2, 3, 5, 7, 3, 12, 3, 3, 2, 2), (('conv3d_igemm_k<0, 4, 1, false>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 96, 'steps': 3, 'last': 81}, ws=BIG, bias=True, act='lrelu'),
    _row('fwd', (2, 3, 5, 7, 5, 12, 2, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 96, 'steps': 3, 'last': 90}, ws=BIG),
    _row('fwd', (2, 3, 5, 7, 6, 36, 2, 2, 1, 1), (('conv3d_igemm_k<0, 2, 2, false>', 1, (4, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 48}, ws=BIG),
    # ---- forward, split reductions: one geometry under four workspaces, both reduce kernels, the epilogue in the reduce, a short last split
    _row('fwd', (1, 2, 5, 7, 16, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 8), 256), ('splitk_reduce_small_k', 1, (14, 1, 1), 256)), {'SK': 8, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, note='workspace cap 1/4: generous'),
    _row('fwd', (1, 2, 5, 7, 16, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 3), 256), ('splitk_reduce_k', 1, (4, 1, 1), 256)), {'SK': 3, 'kps': 352, 'steps': 11, 'last': 320}, ws=2620, note='workspace cap 2/4: the --sk loop stops at 3'),
    _row('fwd', (1, 2, 5, 7, 16, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 1024, 'steps': 32, 'last': 1024}, ws=1679, note='workspace cap 3/4: the --sk loop ends at 1'),
    _row('fwd', (1, 2, 5, 7, 16, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 1024, 'steps': 32, 'last': 1024}, ws=None, note='workspace cap 4/4: no workspace'),
    _row('fwd', (1, 2, 5, 7, 16, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 8), 256), ('splitk_reduce_small_k', 1, (14, 1, 1), 256)), {'SK': 8, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, bias=True, act='lrelu', note='split: bias + LeakyReLU move to the reduce'),
    _row('fwd', (1, 6, 25, 28, 16, 16, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (33, 1, 8), 256), ('splitk_reduce_k', 1, (263, 1, 1), 256)), {'SK': 8, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, bias=True, note='more than 65536 result elements: splitk_reduce_k at SK = 8'),
    _row('fwd', (1, 2, 5, 7, 12, 12, 3, 3, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 2), 256), ('splitk_reduce_k', 1, (4, 1, 1), 256)), {'SK': 2, 'kps': 192, 'steps': 6, 'last': 132}, ws=BIG, note='K = 324 in two splits of 192: the last split is 132, its last step 4 wide'),
    _row('fwd', (1, 2, 5, 7, 16, 36, 4, 4, 2, 2), (('conv3d_igemm_k<0, 2, 2, true>', 1, (1, 1, 8), 256), ('splitk_reduce_small_k', 1, (7, 1, 1), 256)), {'SK': 8, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, bias=True, act='lrelu', note='64x64 tiles, split, stride 2'),
    _row('fwd', (1, 2, 5, 7, 6, 12, 4, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, false>', 1, (1, 1, 3), 256), ('splitk_reduce_k', 1, (4, 1, 1), 256)), {'SK': 3, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, note='AV4 = false, split'),
    # ---- forward, SAME-padding asymmetry along each axis in turn
    _row('fwd', (2, 5, 4, 4, 4, 12, 4, 1, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 16}, ws=BIG, note='even filter at stride 1 along l: pad (1, 2)'),
    _row('fwd', (2, 4, 5, 4, 4, 12, 1, 4, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 64}, ws=BIG, note='even filter at stride 1 along h and w: pad (1, 2)'),
    _row('fwd', (2, 3, 5, 4, 4, 12, 1, 2, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 16}, ws=BIG, note='fs = 2: pad (0, 1)'),
    _row('fwd', (2, 3, 4, 6, 4, 12, 1, 3, 1, 2), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG, note='fs = 3 at stride 2 on even extents: pad (0, 1)'),
    _row('fwd', (2, 4, 3, 5, 4, 12, 3, 1, 2, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 12}, ws=BIG, note='fl = 3 at stride_len 2 on an even length: pad (0, 1)'),
    _row('fwd', (3, 1, 5, 4, 4, 12, 4, 1, 1, 1), (('conv3d_igemm_k<0, 4, 1, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 16}, ws=BIG, note='fl = 4 over L = 1: three of four taps in the padding'),
    # ---- ggan_conv3d_wgrad: steps per split 1..5 over the rows M = 20, 36, 72, 126, 147, then AV4 = false
    _row('wgrad', (1, 1, 4, 5, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 20}, ws=BIG),
    _row('wgrad', (1, 1, 6, 6, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG),
    _row('wgrad', (1, 2, 6, 6, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 96, 'steps': 3, 'last': 72}, ws=BIG),
    _row('wgrad', (1, 3, 6, 7, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG),
    _row('wgrad', (1, 3, 7, 7, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 160, 'steps': 5, 'last': 147}, ws=BIG),
    _row('wgrad', (1, 3, 6, 7, 1, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG, note='Ci = 1: the unit k = 8..11 straddles a tw wrap and a th wrap'),
    _row('wgrad', (1, 3, 6, 7, 2, 68, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (1, 2, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG, note='two column tiles'),
    _row('wgrad', (1, 3, 6, 7, 3, 12, 3, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG, note='K = 81: two row tiles, K % 4 != 0'),
    _row('wgrad', (1, 3, 6, 7, 3, 12, 3, 3, 2, 2), (('conv3d_igemm_k<1, 2, 2, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 32, 'steps': 1, 'last': 24}, ws=BIG),
    _row('wgrad', (1, 3, 6, 7, 5, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG),
    _row('wgrad', (1, 3, 6, 7, 6, 36, 2, 2, 1, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 126}, ws=BIG),
    # ---- filter gradient, split over the rows: one geometry under four workspaces, both reduce kernels
    _row('wgrad', (2, 3, 10, 10, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 4), 256), ('splitk_reduce_k', 1, (4, 1, 1), 256)), {'SK': 4, 'kps': 160, 'steps': 5, 'last': 120}, ws=BIG, note='workspace cap 1/4: generous; M = 600 in four splits of 160, the last 120'),
    _row('wgrad', (2, 3, 10, 10, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 2), 256), ('splitk_reduce_k', 1, (4, 1, 1), 256)), {'SK': 2, 'kps': 320, 'steps': 10, 'last': 280}, ws=1828, note='workspace cap 2/4: the --sk loop stops at 2'),
    _row('wgrad', (2, 3, 10, 10, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 608, 'steps': 19, 'last': 600}, ws=1727, note='workspace cap 3/4: the --sk loop ends at 1'),
    _row('wgrad', (2, 3, 10, 10, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 1), 256),), {'SK': 1, 'kps': 608, 'steps': 19, 'last': 600}, ws=None, note='workspace cap 4/4: no workspace'),
    _row('wgrad', (2, 4, 12, 12, 4, 12, 2, 3, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (2, 1, 9), 256), ('splitk_reduce_small_k', 1, (14, 1, 1), 256)), {'SK': 9, 'kps': 128, 'steps': 4, 'last': 128}, ws=BIG, note='M = 1152: nine splits, splitk_reduce_small_k'),
    _row('wgrad', (2, 4, 12, 12, 3, 12, 2, 3, 2, 1), (('conv3d_igemm_k<1, 2, 2, false>', 1, (1, 1, 4), 256), ('splitk_reduce_k', 1, (3, 1, 1), 256)), {'SK': 4, 'kps': 160, 'steps': 5, 'last': 96}, ws=BIG, note='AV4 = false, split'),
    # ---- filter gradient, SAME-padding asymmetry
    _row('wgrad', (2, 5, 4, 4, 4, 12, 4, 1, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 160, 'steps': 5, 'last': 160}, ws=BIG, note='even filter at stride 1 along l: pad (1, 2)'),
    _row('wgrad', (2, 4, 5, 4, 4, 12, 1, 4, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 160, 'steps': 5, 'last': 160}, ws=BIG, note='even filter at stride 1 along h and w: pad (1, 2)'),
    _row('wgrad', (2, 3, 5, 4, 4, 12, 1, 2, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 128, 'steps': 4, 'last': 120}, ws=BIG, note='fs = 2: pad (0, 1)'),
    _row('wgrad', (2, 3, 4, 6, 4, 12, 1, 3, 1, 2), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 36}, ws=BIG, note='fs = 3 at stride 2 on even extents: pad (0, 1)'),
    _row('wgrad', (2, 4, 3, 5, 4, 12, 3, 1, 2, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 60}, ws=BIG, note='fl = 3 at stride_len 2 on an even length: pad (0, 1)'),
    _row('wgrad', (3, 1, 5, 4, 4, 12, 4, 1, 1, 1), (('conv3d_igemm_k<1, 2, 2, true>', 1, (1, 1, 1), 256),), {'SK': 1, 'kps': 64, 'steps': 2, 'last': 60}, ws=BIG, note='fl = 4 over L = 1: three of four taps in the padding'),
    # ---- ggan_conv3d_dgrad: steps 1..5 of the only class (Co = 4, stride 1), both tiles, classes without rows and without taps
    _row('dgrad', (2, 3, 5, 7, 16, 4, 5, 1, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((210, 20),)}),
    _row('dgrad', (2, 3, 5, 7, 16, 4, 1, 3, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((210, 36),)}),
    _row('dgrad', (2, 3, 5, 7, 16, 4, 2, 3, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((210, 72),)}),
    _row('dgrad', (2, 3, 5, 7, 16, 4, 2, 4, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((210, 128),)}),
    _row('dgrad', (2, 3, 5, 7, 16, 4, 4, 3, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((210, 144),)}),
    _row('dgrad', (2, 3, 5, 7, 36, 4, 2, 3, 1, 1), (('conv3d_igemm_k<2, 2, 2, true>', 1, (4, 1, 1), 256),), {'nc': 1, 'classes': ((210, 72),)}, note='Ci = 36: 64x64 tiles, ragged'),
    _row('dgrad', (2, 3, 5, 7, 36, 12, 4, 3, 2, 2), (('conv3d_igemm_k<2, 2, 2, true>', 1, (1, 1, 8), 256),), {'nc': 8, 'classes': ((48, 24), (36, 48), (32, 48), (24, 96), (24, 24), (18, 48), (16, 48), (12, 96))}, note='64x64 tiles, eight classes'),
    _row('dgrad', (2, 3, 5, 7, 20, 12, 3, 3, 2, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 8), 256),), {'nc': 8, 'classes': ((48, 12), (36, 24), (32, 24), (24, 48), (24, 24), (18, 48), (16, 48), (12, 96))}, note='Ci = 20, ragged against 32; fl = 3 over stride_len 2: unequal taps per class'),
    _row('dgrad', (2, 1, 5, 7, 16, 8, 3, 3, 2, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 4), 256),), {'nc': 4, 'classes': ((24, 8), (18, 16), (16, 16), (12, 32))}, note='L = 1 at stride_len 2: no rows in the classes cl = 1, nc = 4'),
    _row('dgrad', (2, 3, 5, 1, 16, 8, 3, 3, 1, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 2), 256),), {'nc': 2, 'classes': ((18, 24), (12, 48))}, note='W = 1 at stride 2: no rows in the class cw = 1, nc = 2'),
    _row('dgrad', (3, 2, 5, 5, 32, 12, 1, 1, 2, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 8), 256),), {'nc': 8, 'classes': ((27, 12), (18, 0), (18, 0), (12, 0), (27, 0), (18, 0), (18, 0), (12, 0))}, note='1x1x1 filter over stride 2: seven classes without a tap, exact zeros'),
    _row('dgrad', (2, 3, 5, 7, 16, 4, 2, 2, 2, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 8), 256),), {'nc': 8, 'classes': ((48, 4), (36, 4), (32, 4), (24, 4), (24, 4), (18, 4), (16, 4), (12, 4))}, note='Co = 4, one tap per class: K = 4, below one step'),
    # ---- data gradient, SAME-padding asymmetry
    _row('dgrad', (2, 5, 4, 4, 16, 12, 4, 1, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((160, 48),)}, note='even filter at stride 1 along l: pad (1, 2)'),
    _row('dgrad', (2, 4, 5, 4, 16, 12, 1, 4, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (2, 1, 1), 256),), {'nc': 1, 'classes': ((160, 192),)}, note='even filter at stride 1 along h and w: pad (1, 2)'),
    _row('dgrad', (2, 3, 5, 4, 16, 12, 1, 2, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 1), 256),), {'nc': 1, 'classes': ((120, 48),)}, note='fs = 2: pad (0, 1)'),
    _row('dgrad', (2, 3, 4, 6, 16, 12, 1, 3, 1, 2), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 4), 256),), {'nc': 4, 'classes': ((36, 48), (36, 24), (36, 24), (36, 12))}, note='fs = 3 at stride 2 on even extents: pad (0, 1)'),
    _row('dgrad', (2, 4, 3, 5, 16, 12, 3, 1, 2, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 2), 256),), {'nc': 2, 'classes': ((60, 24), (60, 12))}, note='fl = 3 at stride_len 2 on an even length: pad (0, 1)'),
    _row('dgrad', (3, 1, 5, 4, 16, 12, 4, 1, 1, 1), (('conv3d_igemm_k<2, 4, 1, true>', 1, (1, 1, 1), 256),), {'nc': 1, 'classes': ((60, 48),)}, note='fl = 4 over L = 1: three of four taps in the padding'),
    # ---- the patch-matrix operators: V = 4, V = 1 by the channel count and by either base; exact against numpy
    _row('im2col', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('im2col3d_k<uint32_t, 4>', 1, (10, 1, 1), 256),), None),
    _row('im2col', (2, 3, 5, 7, 3, 1, 2, 3, 2, 1), (('im2col3d_k<uint32_t, 1>', 1, (30, 1, 1), 256),), None, note='V = 1 by Ci % 4 != 0'),
    _row('im2col', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('im2col3d_k<uint32_t, 1>', 1, (40, 1, 1), 256),), None, off=('x',), note='V = 1 by x one float past a 16-byte boundary'),
    _row('im2col', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('im2col3d_k<uint32_t, 1>', 1, (40, 1, 1), 256),), None, off=('col',), note='V = 1 by col one float past a 16-byte boundary'),
    _row('col2im', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('col2im3d_k<uint32_t, 4>', 1, (1, 1, 1), 256),), None),
    _row('col2im', (2, 3, 5, 7, 3, 1, 2, 3, 2, 1), (('col2im3d_k<uint32_t, 1>', 1, (3, 1, 1), 256),), None, note='V = 1 by Ci % 4 != 0'),
    _row('col2im', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('col2im3d_k<uint32_t, 1>', 1, (4, 1, 1), 256),), None, off=('gx',), note='V = 1 by gx one float past a 16-byte boundary'),
    _row('col2im', (2, 3, 5, 7, 4, 1, 2, 3, 2, 1), (('col2im3d_k<uint32_t, 1>', 1, (4, 1, 1), 256),), None, off=('col',), note='V = 1 by col one float past a 16-byte boundary'),
    # ---- argument checks: non-zero return, no launch, the NaN output stays NaN
    _row('fwd', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('x',), refused=True, note='x one float past a 16-byte boundary'),
    _row('fwd', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('w',), refused=True, note='w one float past a 16-byte boundary'),
    _row('fwd', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('y',), refused=True, note='y one float past a 16-byte boundary'),
    _row('fwd', (2, 3, 5, 7, 4, 6, 2, 3, 1, 1), (), None, ws=BIG, refused=True, note='a geometry ggan_conv3d_igemm_ok rejects'),
    _row('wgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('x',), refused=True, note='x one float past a 16-byte boundary'),
    _row('wgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('gy',), refused=True, note='gy one float past a 16-byte boundary'),
    _row('wgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, ws=BIG, off=('gw',), refused=True, note='gw one float past a 16-byte boundary'),
    _row('wgrad', (2, 3, 5, 7, 4, 6, 2, 3, 1, 1), (), None, ws=BIG, refused=True, note='a geometry ggan_conv3d_igemm_ok rejects'),
    _row('dgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, off=('gy',), refused=True, note='gy one float past a 16-byte boundary'),
    _row('dgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, off=('w',), refused=True, note='w one float past a 16-byte boundary'),
    _row('dgrad', (2, 3, 5, 7, 16, 12, 2, 3, 1, 1), (), None, off=('gx',), refused=True, note='gx one float past a 16-byte boundary'),
    _row('dgrad', (2, 3, 5, 7, 8, 12, 2, 3, 1, 1), (), None, refused=True, note='a geometry ggan_conv3d_igemm_ok rejects'),
    # ---- the 64-bit index instances of the layout kernels: not run
    _row('im2col', (1, 1, 1024, 1024, 4, 1, 4, 31, 1, 1), (('im2col3d_k<size_t, 4>', 1, (32768, 1, 1), 256),), None, run=NOT_RUN),
    _row('im2col', (1, 1, 1024, 1024, 3, 1, 4, 31, 1, 1), (('im2col3d_k<size_t, 1>', 1, (32768, 1, 1), 256),), None, run=NOT_RUN),
    _row('col2im', (16, 64, 1024, 1024, 4, 1, 1, 1, 1, 1), (('col2im3d_k<size_t, 4>', 1, (32768, 1, 1), 256),), None, run=NOT_RUN),
    _row('col2im', (16, 64, 1024, 1024, 5, 1, 1, 1, 1, 1), (('col2im3d_k<size_t, 1>', 1, (32768, 1, 1), 256),), None, run=NOT_RUN),
]

# The wide-volume rows: Wo = 4096 and 258 output rows of that width, 1 056 768 voxels.  FastDiv's n / 4096 is wrong from n = 1 052 671 on
# (conv.h: exact for n * d < 2^32), so ggan_conv3d_igemm_ok must not admit the geometry: functional.conv3d takes the patch route.
FASTDIV_ROWS = [
    _row('fwd', (1, 1, 258, 4096, 4, 4, 1, 1, 1, 1), (('im2col3d_k<uint32_t, 4>', 1, (4128, 1, 1), 256),), None, bias=True, exact=True),
    _row('wgrad', (1, 1, 258, 4096, 4, 4, 1, 1, 1, 1), (('im2col3d_k<uint32_t, 4>', 1, (4128, 1, 1), 256),), None, exact=True),
    _row('dgrad', (1, 1, 258, 4096, 16, 4, 1, 1, 1, 1), (('im2col3d_k<uint32_t, 4>', 1, (16512, 1, 1), 256), ('col2im3d_k<uint32_t, 4>', 1, (16512, 1, 1), 256)),
         None, exact=True),
]


def row_id(row):
    return '%s-%s-%s%s%s%s%s%s' % (row['entry'], row['launches'][0][0].replace(' ', '') if row['launches'] else 'refused',
                                   'x'.join(str(v) for v in row['dims']), '-b' if row['bias'] else '', '-' + row['act'] if row['act'] != 'none' else '',
                                   '-ws%s' % row['ws'] if row['entry'] in ('fwd', 'wgrad') and row['ws'] != BIG else '',
                                   '-off_' + '_'.join(row['off']) if row['off'] else '', '-notrun' if row['run'] else '')


def threads(launch):
    """the profiler's grid figure of a launch: work-items"""
    return int(np.prod(launch[2])) * launch[3]


def geometry(dims):
    """SAME padding as tf.nn.conv3d (fill() of conv3d.hip) -> ((Lo, Ho, Wo), (pl, ph, pw))"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    out = lambda n, st: -(-n // st)
    pad = lambda n, o, k, st: max((o - 1) * st + k - n, 0) // 2
    Lo, Ho, Wo = out(L, sl), out(H, s), out(W, s)
    return (Lo, Ho, Wo), (pad(L, Lo, fl, sl), pad(H, Ho, fs, s), pad(W, Wo, fs, s))


# ---- inputs and references ----------------------------------------------------------------------------------------------------------------
def im2col_ref(x, dims):
    """col[(n, ol, oh, ow), (dl, dh, dw, ci)] as a numpy gather (dtype of x)"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    (Lo, Ho, Wo), (pl, ph, pw) = geometry(dims)
    xp = np.zeros((N, max((Lo - 1) * sl + fl, pl + L), max((Ho - 1) * s + fs, ph + H), max((Wo - 1) * s + fs, pw + W), Ci), dtype=x.dtype)
    xp[:, pl:pl + L, ph:ph + H, pw:pw + W] = x
    col = np.zeros((N, Lo, Ho, Wo, fl, fs, fs, Ci), dtype=x.dtype)
    for dl in range(fl):
        for dh in range(fs):
            for dw in range(fs):
                col[:, :, :, :, dl, dh, dw] = xp[:, dl:dl + (Lo - 1) * sl + 1:sl, dh:dh + (Ho - 1) * s + 1:s, dw:dw + (Wo - 1) * s + 1:s]
    return col.reshape(N * Lo * Ho * Wo, fl * fs * fs * Ci)


def col2im_ref(col, dims):
    """the adjoint as a numpy scatter-add, taps ascending (dtype of col)"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = dims
    (Lo, Ho, Wo), (pl, ph, pw) = geometry(dims)
    c = col.reshape(N, Lo, Ho, Wo, fl, fs, fs, Ci)
    gp = np.zeros((N, max((Lo - 1) * sl + fl, pl + L), max((Ho - 1) * s + fs, ph + H), max((Wo - 1) * s + fs, pw + W), Ci), dtype=col.dtype)
    for dl in range(fl):
        for dh in range(fs):
            for dw in range(fs):
                gp[:, dl:dl + (Lo - 1) * sl + 1:sl, dh:dh + (Ho - 1) * s + 1:s, dw:dw + (Wo - 1) * s + 1:s] += c[:, :, :, :, dl, dh, dw]
    return np.ascontiguousarray(gp[:, pl:pl + L, ph:ph + H, pw:pw + W])


def inputs(row):
    """-> dict of the row's operands: float64 values that float32 holds exactly, from a seed derived from the row"""
    N, L, H, W, Ci, Co, fl, fs, sl, s = row['dims']
    (Lo, Ho, Wo), _ = geometry(row['dims'])
    rng = np.random.default_rng(zlib.crc32(row_id(row).encode()))
    if row['exact'] or row['entry'] in ('im2col', 'col2im'):
        # small integers: every sum is exact in float32 whatever its order (FASTDIV_ROWS: -1, 0, 1, at most 1 056 768 terms < 2^24)
        lim = 1 if row['exact'] else 64
        draw = lambda shape: rng.integers(-lim, lim + 1, size=shape).astype(np.float64)
    else:
        draw = lambda shape: rng.standard_normal(shape).astype(np.float32).astype(np.float64)
    K = fl * fs * fs * Ci
    inp = dict(x=draw((N, L, H, W, Ci)), gy=draw((N, Lo, Ho, Wo, Co)), b=draw((Co,)))
    inp['w'] = draw((fl, fs, fs, Ci, Co)) if row['exact'] else (draw((fl, fs, fs, Ci, Co)) / np.sqrt(K)).astype(np.float32).astype(np.float64)
    inp['col'] = draw((N * Lo * Ho * Wo, K))
    return inp


def reference(row, inp):
    """-> {output name: float64 reference} of the row's entry point on the inputs"""
    from oracle import ops as O
    N, L, H, W, Ci, Co, fl, fs, sl, s = row['dims']
    e = row['entry']
    if e == 'fwd':
        v = O.conv3d(inp['x'], inp['w'], sl, s) + (inp['b'] if row['bias'] else 0.0)
        return dict(y=np.where(v > 0, v, ALPHA * v) if row['act'] == 'lrelu' else v)
    if e == 'wgrad':
        return dict(gw=O.conv3d_bwd_filter(inp['x'], inp['gy'], fl, fs, sl, s))
    if e == 'dgrad':
        return dict(gx=O.conv3d_bwd_data(inp['gy'], inp['w'], inp['x'].shape, sl, s))
    if e == 'im2col':
        return dict(col=im2col_ref(inp['x'], row['dims']))
    return dict(gx=col2im_ref(inp['col'], row['dims']))
