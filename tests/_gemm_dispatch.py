"""Which kernel instance of the GEMM family (csrc/gemm.hip) each dispatch test runs: one row per instance and launch site (plain data).

tests/test_gemm_dispatch_gpu.py runs every row through the C entry point it names, asserts that the profiler saw exactly the row's
kernel (plus the helpers in `also`), once, with the row's grid, that the GGAN_TRACE_GEMM line of that launch equals `expect`, and that
every output matches a float64 numpy reference.  tests/test_gemm_dispatch_cpu.py derives every (name, FAST) and (name, NS) pair the
launch macros of gemm.hip can produce and fails when a pair has no row or a row names a pair the source no longer produces; it also
recomputes every `expect` from a Python transcription of gemm_plan and of the skinny predicate.

A row:
  kernel   the name GGAN_LAUNCH passes and _lib.prof_report() returns.  The variant the name hides is expect['fast'] / expect['ns'].
  entry    gemm | gemm_split | gemm_colsum | linear_bwd_data_act | linear_bwd_weight_act | critic_head_fwd | critic_head_fwd_bce |
           critic_head_bwd | critic_head_bwd_tail
  shape    (ta, tb, M, N, K) of the product C[M,N] = op(A) op(B) itself (linear_bwd_data_act(M, N, K) is the product
           (0, 1, M, K, N), linear_bwd_weight_act(M, N, K) is (1, 0, K, N, M)); the heads: (M, K1, K2, H)
  a_split  two-source operand: columns (k, or m when ta) >= a_split of op(A) come from a second buffer;  c_split: output columns
           >= c_split go to a second buffer (0: none)
  bias, act    epilogue: bias[N] and 'none' | 'lrelu' | 'relu';   mask: activation whose derivative masks the gradient operand (the
           reference tensor is continuous, without exact zeros)
  off      base offset in floats of A, the second source, B and the mask's reference tensor: 0, or 1..3 for a base that is not 16-byte
           aligned (the operand is a view into a larger buffer); the heads: of a1, a2, w
  need     heads: 'all' | 'data' (frozen weights: the data gradient alone);  terms: (rows, label, weight) of the cost the head knows
  env      GGAN_GEMM_SK if the row needs it (the test clears it first)
  expect   one dict per GGAN_TRACE_GEMM line that carries the row's kernel name, in launch order: waves, fast (-1: no such choice), ns
           (0: not the skinny kernel), SK, kps, grid (x, y, z); a member of a grouped launch adds wgs (first, end) and the row `tail`,
           the workgroup range of the cost tail
  also     the other kernels the call launches (split-K reduce helpers, head kernels, the other product of a head's backward)
  note     which edge the row is there for

To add a row: pick the smallest shape that reaches the instance with a ragged M and N tile (GGAN_TRACE_GEMM=1 prints the choice; the
transcription in test_gemm_dispatch_cpu.py computes it without a GPU), fill in `expect`, and run the two dispatch test modules.
K <= 4608 and M * N <= 2**20 for ROWS.  BIG_ROWS reach the generic loader (FAST == 0), which only an operand of at least 0x7FFFFFF0
bytes selects; they hold exactly representable data (see test_gemm_dispatch_gpu.py) and run in a test of their own.
"""
import numpy as np

FF, FT, TF, TT = '<false, false>', '<false, true>', '<true, false>', '<true, true>'
FT1, TF2 = '<false, true, 1>', '<true, false, 2>'
RED, RED_SMALL = 'splitk_reduce_k', 'splitk_reduce_small_k'


def _row(kernel, entry, shape, expect, env=None, a_split=0, c_split=0, bias=False, act='none', mask=None, off=(0, 0, 0, 0), also=(),
         note='', **more):
    e = expect if isinstance(expect, tuple) else (expect,)
    return dict(kernel=kernel, entry=entry, shape=shape, a_split=a_split, c_split=c_split, bias=bias, act=act, mask=mask, off=off,
                env={'GGAN_GEMM_SK': str(env)} if env is not None else {}, expect=e, also=tuple(also), note=note, **more)


def _x(waves, fast, ns, SK, kps, grid, **more):
    return dict(waves=waves, fast=fast, ns=ns, SK=SK, kps=kps, grid=grid, **more)


ROWS = [
    # ---- gemm_kernel: four waves, kps < 2 * KSTEP (16, 32, 48) ------------------------------------------------------------------------
    _row('gemm_kernel' + FF, 'gemm', (0, 0, 72, 68, 48), _x(4, 1, 0, 1, 48, (2, 2, 1)), env=1,
         note='kps 48 = 1.5 steps: the second step is half empty; SK == 1'),
    _row('gemm_kernel' + FF, 'gemm', (0, 0, 72, 68, 48), _x(4, 2, 0, 3, 16, (2, 2, 3)), off=(1, 0, 0, 0), also=(RED,), bias=True, act='lrelu',
         note='FAST 2 by a base offset of A, all dimensions multiples of 4; kps 16 = half a step'),
    _row('gemm_kernel' + FF, 'gemm', (0, 0, 72, 68, 63), _x(4, 2, 0, 2, 32, (2, 2, 2)), also=(RED,),
         note='K = 63: below the skinny range; last split 31 long'),
    _row('gemm_kernel' + FF, 'gemm', (0, 0, 512, 512, 136), _x(4, 1, 0, 3, 48, (8, 8, 3)), also=(RED,),
         note='64 tiles of 64 x 64: one too many for the skinny kernel; last split 40 long'),
    _row('gemm_kernel' + FT, 'gemm', (0, 1, 72, 68, 32), _x(4, 1, 0, 2, 16, (2, 2, 2)), also=(RED,), bias=True, act='relu',
         note='bias + ReLU applied by the reduce helper'),
    _row('gemm_kernel' + FT, 'gemm', (0, 1, 70, 70, 47), _x(4, 2, 0, 2, 32, (2, 2, 2)), also=(RED,),
         note='FAST 2 by the leading dimensions of A and B (K = 47); last split 15 long, K % KSTEP != 0'),
    _row('gemm_kernel' + FT, 'gemm', (0, 1, 31, 68, 100), _x(4, 1, 0, 4, 32, (2, 1, 4)), also=(RED,),
         note='M = 31: below the skinny range; last split 4 long'),
    _row('gemm_kernel' + TF, 'gemm', (1, 0, 72, 68, 1040), _x(4, 1, 0, 33, 32, (2, 2, 33)), env=33, also=(RED_SMALL,),
         note='one step per split, last split half a step'),
    _row('gemm_kernel' + TF, 'gemm', (1, 0, 72, 68, 96), _x(4, 2, 0, 2, 48, (2, 2, 2)), env=2, off=(0, 0, 1, 0), also=(RED,),
         note='FAST 2 by a base offset of B; kps 48'),
    _row('gemm_kernel' + TT, 'gemm', (1, 1, 72, 68, 48), _x(4, 1, 0, 1, 48, (2, 2, 1)), env=1, bias=True),
    _row('gemm_kernel' + TT, 'gemm', (1, 1, 70, 68, 40), _x(4, 2, 0, 2, 32, (2, 2, 2)), also=(RED,),
         note='FAST 2 by the leading dimension of A (M = 70); last split 8 long'),
    _row('gemm_kernel' + FT1, 'linear_bwd_data_act', (0, 1, 72, 68, 48), _x(4, 1, 0, 3, 16, (2, 2, 3)), mask='lrelu', also=(RED,)),
    _row('gemm_kernel' + FT1, 'linear_bwd_data_act', (0, 1, 72, 68, 48), _x(4, 2, 0, 1, 48, (2, 2, 1)), env=1, mask='relu', off=(1, 0, 0, 0),
         note='FAST 2 by a base offset of the gradient operand'),
    _row('gemm_kernel' + TF2, 'linear_bwd_weight_act', (1, 0, 72, 68, 48), _x(4, 1, 0, 1, 48, (2, 2, 1)), mask='lrelu',
         note='column sums of the masked operand, unsplit'),
    _row('gemm_kernel' + TF2, 'linear_bwd_weight_act', (1, 0, 72, 70, 40), _x(4, 2, 0, 1, 48, (2, 2, 1)), mask='relu',
         note='FAST 2 by the leading dimension of B (N = 70); K = 40 inside kps 48'),
    _row('gemm_kernel' + FF, 'gemm_colsum', (0, 0, 72, 68, 48), _x(4, 1, 0, 1, 48, (2, 2, 1)),
         note='column sums, unsplit (K < 512)'),
    _row('gemm_kernel' + TF, 'gemm_colsum', (1, 0, 72, 68, 1040), _x(4, 1, 0, 33, 32, (2, 2, 33)), also=(RED_SMALL,),
         note='column sums split (4 workgroups, K >= 512): they travel as slab tails'),
    _row('gemm_kernel' + FF, 'gemm_split', (0, 0, 72, 68, 1112), _x(4, 1, 0, 35, 32, (2, 2, 35)), a_split=1088, also=(RED_SMALL,),
         note='two sources split k; the second is 24 wide, narrower than a step: the last split reads it alone'),
    _row('gemm_kernel' + TF, 'gemm_split', (1, 0, 70, 68, 48), _x(4, 2, 0, 1, 48, (2, 2, 1)), env=1, a_split=64,
         note='two sources split m; the second is 6 wide (FAST 2 by its leading dimension)'),
    # ---- gemm_kernel8: eight waves, kps >= 2 * KSTEP ----------------------------------------------------------------------------------
    _row('gemm_kernel8' + FF, 'gemm', (0, 0, 72, 68, 1040), _x(8, 1, 0, 17, 64, (2, 2, 17)), env=17, also=(RED_SMALL,),
         note='2 steps per split, last split half a step (K % KSTEP != 0)'),
    _row('gemm_kernel8' + FF, 'gemm', (0, 0, 72, 68, 1056), _x(8, 2, 0, 11, 96, (2, 2, 11)), env=11, off=(1, 0, 0, 0), also=(RED_SMALL,),
         note='3 steps per split; FAST 2 by a base offset of A'),
    _row('gemm_kernel8' + FF, 'gemm', (0, 0, 256, 512, 128), _x(8, 1, 0, 1, 128, (8, 4, 1)),
         note='K <= 128 on 32 tiles: neither skinny nor split'),
    _row('gemm_kernel8' + FT, 'gemm', (0, 1, 72, 68, 1120), _x(8, 1, 0, 9, 128, (2, 2, 9)), env=9, also=(RED_SMALL,), bias=True, act='lrelu',
         note='4 steps per split, last split 3 steps'),
    _row('gemm_kernel8' + FT, 'gemm', (0, 1, 72, 68, 1040), _x(8, 2, 0, 4, 272, (2, 2, 4)), env=4, off=(0, 0, 1, 0), also=(RED,),
         note='8.5 steps per split, last split 7; FAST 2 by a base offset of B'),
    _row('gemm_kernel8' + TF, 'gemm', (1, 0, 72, 68, 64), _x(8, 1, 0, 1, 64, (2, 2, 1)), env=1, note='2 steps; SK == 1'),
    _row('gemm_kernel8' + TF, 'gemm', (1, 0, 72, 70, 96), _x(8, 2, 0, 1, 96, (2, 2, 1)), env=1,
         note='3 steps; FAST 2 by the leading dimension of B (N = 70)'),
    _row('gemm_kernel8' + TT, 'gemm', (1, 1, 72, 68, 160), _x(8, 1, 0, 1, 160, (2, 2, 1)), env=1, note='5 steps'),
    _row('gemm_kernel8' + TT, 'gemm', (1, 1, 72, 68, 128), _x(8, 2, 0, 1, 128, (2, 2, 1)), env=1, off=(1, 0, 0, 0), bias=True,
         note='4 steps; FAST 2 by a base offset of A'),
    _row('gemm_kernel8' + TT, 'gemm', (1, 1, 70, 68, 80), _x(8, 2, 0, 1, 80, (2, 2, 1)), env=1,
         note='2.5 steps; FAST 2 by the leading dimension of A (M = 70)'),
    _row('gemm_kernel8' + FT1, 'linear_bwd_data_act', (0, 1, 72, 68, 1040), _x(8, 1, 0, 17, 64, (2, 2, 17)), env=17, mask='lrelu',
         also=(RED_SMALL,)),
    _row('gemm_kernel8' + FT1, 'linear_bwd_data_act', (0, 1, 72, 68, 1056), _x(8, 2, 0, 11, 96, (2, 2, 11)), env=11, mask='relu',
         off=(0, 0, 0, 1), also=(RED_SMALL,), note='FAST 2 by a base offset of the reference tensor'),
    _row('gemm_kernel8' + TF2, 'linear_bwd_weight_act', (1, 0, 72, 68, 520), _x(8, 1, 0, 7, 80, (2, 2, 7)), env=8, mask='lrelu', also=(RED,),
         note='column sums of the masked operand as slab tails; 2.5 steps per split, last split 40 long'),
    _row('gemm_kernel8' + TF2, 'linear_bwd_weight_act', (1, 0, 72, 70, 100), _x(8, 2, 0, 1, 112, (2, 2, 1)), mask='relu',
         note='FAST 2 by the leading dimension of B; column sums unsplit'),
    _row('gemm_kernel8' + FF, 'gemm_split', (0, 0, 72, 68, 1112), _x(8, 1, 0, 9, 128, (2, 2, 9)), env=9, a_split=1088, bias=True,
         also=(RED_SMALL,), note='two sources split k: the last split (88 long) reads 64 of the first and the 24 of the second'),
    _row('gemm_kernel8' + TF, 'gemm_split', (1, 0, 72, 68, 96), _x(8, 1, 0, 1, 96, (2, 2, 1)), a_split=64, colsum=True,
         note='two sources split m, the second 8 wide; column sums (so no split-K below K = 512)'),
    _row('gemm_kernel8' + FT, 'gemm_split', (0, 1, 72, 72, 1040), _x(8, 1, 0, 1, 1040, (2, 2, 1)), c_split=64,
         note='split output: columns >= 64 (8 of them) go to the second buffer; never split-K'),
    # ---- gemv_rows_k ---------------------------------------------------------------------------------------------------------------
    _row('gemv_rows_k', 'gemm', (0, 0, 70, 1, 100), _x(4, -1, 0, 1, 100, (18, 1, 1)), bias=True, act='lrelu', note='N == 1'),
    # ---- gemm_skinny_k: NS = loads in flight per wave (K <= 128, 256, 512, 1024) -------------------------------------------------------
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 72, 68, 64), _x(8, -1, 1, 1, 64, (5, 5, 1)), note='K = 64: the shortest skinny product'),
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 70, 70, 200), _x(8, -1, 2, 1, 200, (5, 5, 1)), bias=True, act='relu'),
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 33, 50, 300), _x(8, -1, 4, 1, 300, (4, 3, 1))),
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 72, 68, 1024), _x(8, -1, 8, 1, 1024, (5, 5, 1)), note='K = 1024: the longest (1040 is a tile row)'),
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 448, 576, 136), _x(8, -1, 2, 1, 136, (36, 28, 1)),
         note='63 tiles of 64 x 64 (1008 of 16 x 16): the largest skinny grid'),
    _row('gemm_skinny_k' + FF, 'gemm', (0, 0, 256, 448, 128), _x(8, -1, 1, 1, 128, (28, 16, 1)),
         note='K <= 128 on 28 tiles: still skinny (32 tiles are not)'),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 32, 68, 100), _x(8, -1, 1, 1, 100, (5, 2, 1)), note='M = 32: the fewest rows'),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 72, 68, 130), _x(8, -1, 2, 1, 130, (5, 5, 1)), bias=True, note='K % 4 != 0: dword loads'),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 70, 70, 500), _x(8, -1, 4, 1, 500, (5, 5, 1)), bias=True, act='lrelu'),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 72, 70, 1000), _x(8, -1, 8, 1, 1000, (5, 5, 1))),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 72, 68, 128), _x(8, -1, 1, 1, 128, (5, 5, 1)), off=(1, 0, 0, 0), note='vecA == 0 by a base offset'),
    _row('gemm_skinny_k' + TF, 'gemm', (0, 1, 72, 68, 256), _x(8, -1, 2, 1, 256, (5, 5, 1)), off=(0, 0, 3, 0), note='vecB == 0 by a base offset'),
    _row('gemm_skinny_k' + TT, 'linear_bwd_data_act', (0, 1, 72, 68, 128), _x(8, -1, 1, 1, 128, (5, 5, 1)), mask='lrelu'),
    _row('gemm_skinny_k' + TT, 'linear_bwd_data_act', (0, 1, 72, 68, 256), _x(8, -1, 2, 1, 256, (5, 5, 1)), mask='relu'),
    _row('gemm_skinny_k' + TT, 'linear_bwd_data_act', (0, 1, 70, 70, 400), _x(8, -1, 4, 1, 400, (5, 5, 1)), mask='lrelu'),
    _row('gemm_skinny_k' + TT, 'linear_bwd_data_act', (0, 1, 72, 68, 1024), _x(8, -1, 8, 1, 1024, (5, 5, 1)), mask='relu'),
    _row('gemm_skinny_k' + FF, 'gemm_split', (0, 0, 72, 68, 200), _x(8, -1, 2, 1, 200, (5, 5, 1)), a_split=80, bias=True,
         note='two sources, split on a 16-step boundary that is not a 64 boundary'),
    _row('gemm_skinny_k' + TF, 'gemm_split', (0, 1, 72, 68, 202), _x(8, -1, 2, 1, 202, (5, 5, 1)), a_split=96,
         note='K - a_split = 106: vecA2 == 0'),
    _row('gemm_skinny_k' + TF, 'gemm_split', (0, 1, 72, 80, 200), _x(8, -1, 2, 1, 200, (5, 5, 1)), c_split=48,
         note='split output on a 16 boundary'),
    # ---- the critic heads ----------------------------------------------------------------------------------------------------------
    _row('head_out_fwd_k', 'critic_head_fwd', (72, 64, 8, 36), _x(4, -1, 0, 3, 32, (36, 1, 1)), off=(0, 0, 0), also=('gemm_kernel' + FF,),
         note='the product leaves 3 slabs (the last reads the 8-wide second source alone); the tail kernel sums them'),
    _row('head_out_fwd_k', 'critic_head_fwd', (72, 72, 0, 36), _x(4, -1, 0, 1, 80, (36, 1, 1)), env=1, off=(0, 0, 0),
         also=('gemm_kernel8' + FF,), note='SK == 1: the product already sits in h'),
    _row('head_out_fwd_bce_k', 'critic_head_fwd_bce', (72, 64, 8, 36), _x(4, -1, 0, 3, 32, (36, 1, 1)), off=(0, 0, 0),
         also=('gemm_kernel' + FF,), terms=((40, 1.0, 1.0), (32, 0.0, 0.5))),
    _row('gemm_group_kernel<8>', 'critic_head_bwd', (72, 64, 8, 36),
         (_x(8, 1, 0, 1, 48, (2, 2, 1), wgs=(0, 4)), _x(8, 1, 0, 1, 80, (1, 2, 1), wgs=(4, 6))), off=(0, 0, 0), need='all',
         also=('head_out_bwd_k',), note='two products: the data gradient (split output), then the weight gradient (two sources, column sums)'),
    _row('gemm_group_kernel<8>', 'critic_head_bwd_tail', (72, 64, 8, 36),
         (_x(8, 1, 0, 1, 48, (2, 2, 1), wgs=(0, 4)), _x(8, 1, 0, 1, 80, (1, 2, 1), wgs=(4, 6))), off=(0, 0, 0), need='all', tail=(6, 10),
         terms=((40, 1.0, 1.0), (32, 0.0, 0.5)), note='two products plus the cost tail'),
    _row('gemm_group_kernel<8>', 'critic_head_bwd_tail', (72, 64, 8, 36), _x(8, 1, 0, 1, 48, (2, 2, 1), wgs=(0, 4)), off=(0, 0, 0),
         need='data', tail=(4, 8), terms=((40, 1.0, 1.0), (32, 0.0, 0.5)), note='one product plus the tail'),
    _row('gemm_kernel8' + TF, 'critic_head_bwd', (72, 64, 8, 36), _x(8, 2, 0, 1, 80, (1, 2, 1)), off=(1, 0, 0), need='all',
         also=('head_out_bwd_k', 'gemm_kernel' + FT), note='a1 not 16-byte aligned: separate launches, no tail'),
    _row('gemm_kernel' + FT, 'critic_head_bwd_tail', (72, 64, 8, 36), _x(4, 2, 0, 1, 48, (2, 2, 1)), off=(0, 0, 1), need='all',
         terms=((40, 1.0, 1.0), (32, 0.0, 0.5)), also=('head_tail_k', 'gemm_kernel8' + TF),
         note='w not 16-byte aligned: separate launches, the tail in head_tail_k'),
]

# ---- the generic loader: FAST == 0, an operand of at least 0x7FFFFFF0 bytes ------------------------------------------------------------
# big: the operand that is that large, built on the device as `reps` copies of a small block along `along`, each with its own multiplier
BIG_ROWS = [
    _row('gemm_kernel' + FF, 'gemm', (0, 0, 2359296, 8, 512), _x(4, 0, 0, 1, 512, (1, 36864, 1)), big='A', along='M', reps=288,
         note='A of 4.5 GiB: byte offsets beyond 2^31 and 2^32'),
    _row('gemm_kernel' + FT, 'gemm', (0, 1, 2883584, 8, 192), _x(4, 0, 0, 2, 96, (1, 45056, 2)), env=2, big='A', along='M', reps=176,
         also=(RED,), note='3 steps per split on four waves'),
    _row('gemm_kernel' + FT1, 'linear_bwd_data_act', (0, 1, 2097152, 8, 256), _x(4, 0, 0, 2, 128, (1, 32768, 2)), env=2, mask='relu',
         big='A', along='M', reps=128, also=(RED,), note='4 steps per split on four waves; the reference tensor is as large as A'),
    _row('gemm_kernel' + TF, 'gemm', (1, 0, 64, 8, 10485760), _x(4, 0, 0, 256, 40960, (1, 1, 256)), big='A', along='K', reps=160,
         also=(RED_SMALL,), note='A stored [K, M], 2.5 GiB along K: a tall reduction over 256 slabs'),
    _row('gemm_kernel' + TT, 'gemm', (1, 1, 64, 8, 10485760), _x(4, 0, 0, 256, 40960, (1, 1, 256)), big='A', along='K', reps=160,
         also=(RED_SMALL,)),
    _row('gemm_kernel' + TF2, 'linear_bwd_weight_act', (1, 0, 64, 8, 10485760), _x(4, 0, 0, 256, 40960, (1, 1, 256)), mask='lrelu',
         big='A', along='K', reps=160, also=(RED_SMALL,), note='mask on B, column sums as slab tails'),
    _row('gemm_kernel' + FT, 'gemm', (0, 1, 8, 2359296, 256), _x(4, 0, 0, 1, 256, (36864, 1, 1)), big='B', along='N', reps=144,
         note='B is the large operand'),
    _row('gemm_kernel' + FF, 'gemm_split', (0, 0, 2359296, 8, 280), _x(4, 0, 0, 1, 288, (1, 36864, 1)), a_split=256, big='A', along='M',
         reps=144, note='two sources; the second starts 2.25 GiB behind the first'),
]


def row_id(row):
    return '%s-%s-%s%s%s%s%s' % (row['kernel'].replace(' ', ''), row['entry'], 'x'.join(str(v) for v in row['shape']),
                                 '-a%d' % row['a_split'] if row['a_split'] else '', '-c%d' % row['c_split'] if row['c_split'] else '',
                                 '-off%s' % ''.join(str(v) for v in row['off']) if any(row['off']) else '',
                                 ''.join('-%s%s' % (k.replace('GGAN_GEMM_', ''), v) for k, v in sorted(row['env'].items()))
                                 + ('-' + row['need'] if 'need' in row else '') + ('-' + row['mask'] if row['mask'] else ''))


# ---- BIG_ROWS: exactly representable operands built from small generating blocks ---------------------------------------------------------
# Entries are -1, 0 or 1 (the mask's reference tensor: -1 or 1; LeakyReLU slope 1/2), so every product is a multiple of 1/2 and every
# partial sum of fewer than 2^23 non-zero products is exact in fp32 in any order: the device result must EQUAL the reference.  The large
# operand is `reps` copies of a block along its long dimension, copy r scaled by mult[r]; the cycle (-1, 0, 1) from a random phase makes
# copies r and r - d differ for every distance d that is no multiple of 3 -- neighbours, and the copies 2^31 and 2^32 bytes apart
# whenever a block is a power of two bytes long -- so a read that lands in the wrong copy changes the result.
BIG_ALPHA = 0.5


def multipliers(reps, rng):
    start, step = int(rng.integers(3)), int(rng.integers(1, 3))
    return ((start + step * np.arange(reps)) % 3 - 1).astype(np.float64)


def _signs(reps, rng):
    return rng.integers(0, 2, reps).astype(np.float64) * 2 - 1


def _tern(rng, shape):
    return rng.integers(-1, 2, shape).astype(np.float64)


def _slope(ref, mask):
    return np.where(ref > 0, 1.0, BIG_ALPHA if mask == 'lrelu' else 0.0)


def big_block_bytes(row):
    """bytes of one copy of the large operand's generating block"""
    ta, tb, M, N, K = row['shape']
    long_, other = dict(M=(M, row['a_split'] or K), K=(K, M), N=(N, K))[row['along']]
    return 4 * (long_ // row['reps']) * other


def big_operands(row, rng):
    """the generating blocks, multipliers and small operands of a BIG_ROWS row (float64 arrays holding small integers)"""
    ta, tb, M, N, K = row['shape']
    reps = row['reps']
    d = dict(mult=multipliers(reps, rng))
    if row['along'] == 'M':                                   # A stored [M, K] (and its reference tensor), copies along M
        mb, ka = M // reps, row['a_split'] or K
        d['blockA'] = _tern(rng, (mb, ka))
        if row['a_split']:
            d['mult2'], d['block2'] = _signs(reps, rng), _tern(rng, (mb, K - ka))
        if row['mask']:
            d['multR'], d['blockR'] = _signs(reps, rng), _signs(mb * K, rng).reshape(mb, K)
        d['B'] = _tern(rng, (N, K) if tb else (K, N))
    elif row['along'] == 'K':                                 # A stored [K, M], copies along K; B follows with its own signs
        kb = K // reps
        d['blockA'] = _tern(rng, (kb, M))
        d['multB'], d['blockB'] = _signs(reps, rng), _tern(rng, (N, kb) if tb else (kb, N))
        if (d['mult'] * d['multB']).sum() == 0:               # (the copies must not cancel: the product would be all zeros)
            d['multB'][np.flatnonzero(d['mult'])[0]] *= -1
        if row['mask']:
            d['multR'], d['blockR'] = _signs(reps, rng), _signs(kb * N, rng).reshape(kb, N)
    else:                                                     # B stored [N, K], copies along N
        d['blockB'] = _tern(rng, (N // reps, K))
        d['A'] = _tern(rng, (M, K))
    return d


def big_bound(row, d):
    """the largest number of non-zero products any output element sums"""
    ta, tb, M, N, K = row['shape']
    if row['along'] == 'M':
        A = np.concatenate([d['blockA'], d['block2']], 1) if row['a_split'] else d['blockA']
        return (np.abs(A) @ np.abs(d['B'].T if tb else d['B'])).max()
    if row['along'] == 'N':
        return (np.abs(d['A']) @ np.abs(d['blockB']).T).max()
    return np.abs(d['mult']).sum() * (np.abs(d['blockA']).T @ np.abs(d['blockB'].T if tb else d['blockB'])).max()


def big_reference(row, d):
    """-> {output: float64 reference} from the blocks and multipliers alone"""
    ta, tb, M, N, K = row['shape']
    mult, reps = d['mult'], row['reps']
    if row['along'] == 'M':
        Bop = d['B'].T if tb else d['B']
        ka = d['blockA'].shape[1]
        if row['mask']:
            P = {s: (d['blockA'] * _slope(s * d['blockR'], row['mask'])) @ Bop for s in (1.0, -1.0)}
            return dict(C=np.concatenate([mult[r] * P[d['multR'][r]] for r in range(reps)]))
        P1 = d['blockA'] @ Bop[:ka]
        P2 = d['block2'] @ Bop[ka:] if row['a_split'] else None
        return dict(C=np.concatenate([mult[r] * P1 + (d['mult2'][r] * P2 if P2 is not None else 0.0) for r in range(reps)]))
    if row['along'] == 'N':
        P = d['A'] @ d['blockB'].T
        return dict(C=np.concatenate([mult[r] * P for r in range(reps)], 1))
    Bb = d['blockB'].T if tb else d['blockB']
    if not row['mask']:
        return dict(C=(mult * d['multB']).sum() * (d['blockA'].T @ Bb))
    C, cs = 0.0, 0.0
    for s in (1.0, -1.0):
        sel = d['multR'] == s
        Bm = Bb * _slope(s * d['blockR'], row['mask'])
        C = C + (mult * d['multB'])[sel].sum() * (d['blockA'].T @ Bm)
        cs = cs + d['multB'][sel].sum() * Bm.sum(0)
    return dict(C=C, colsum=cs)


def big_dense(row, d, displaced=None):
    """the same outputs from the materialised operands (for a reduced repeat count); displaced = (r, dist): copy r of the large operand
    is read from copy r - dist"""
    ta, tb, M, N, K = row['shape']
    reps = row['reps']
    used = d['mult'].copy()
    if displaced:
        used[displaced[0]] = d['mult'][displaced[0] - displaced[1]]
    if row['along'] == 'N':
        return dict(C=d['A'] @ np.concatenate([used[r] * d['blockB'] for r in range(reps)]).T)
    A = np.concatenate([used[r] * d['blockA'] for r in range(reps)])
    if row['along'] == 'M':
        if row['mask']:
            A = A * _slope(np.concatenate([d['multR'][r] * d['blockR'] for r in range(reps)]), row['mask'])
        if row['a_split']:
            A = np.concatenate([A, np.concatenate([d['mult2'][r] * d['block2'] for r in range(reps)])], 1)
        return dict(C=A @ (d['B'].T if tb else d['B']))
    B = np.concatenate([d['multB'][r] * (d['blockB'].T if tb else d['blockB']) for r in range(reps)])
    if row['mask']:
        B = B * _slope(np.concatenate([d['multR'][r] * d['blockR'] for r in range(reps)]), row['mask'])
        return dict(C=A.T @ B, colsum=B.sum(0))
    return dict(C=A.T @ B)
