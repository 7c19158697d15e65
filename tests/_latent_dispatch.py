"""Which path of the latent-space and noise kernels (csrc/latent.hip) each dispatch test runs: one row per scenario and edge (plain data),
the rows' inputs, a float32 restatement of every kernel in the kernel's summation order (run32: the CPU stand-in for the device), the
float64 restatements and derived bounds every output is held to in stages (check), `planned()`, a transcription of each entry point's
label, grid, block and dynamic LDS, MUTANTS, the wrong kernels run32 can play, and REJECTED, the calls that must be refused before any launch.

tests/test_latent_dispatch_gpu.py runs every row through the C ABI between sentinel pads, asserts that the profiler saw exactly the row's
launches and hands the outputs to check().  tests/test_latent_dispatch_cpu.py holds labels, kernel instances and constants against the
source text, recomputes every row's launches with planned(), asserts from the rows which edges the table reaches, checks the Philox known
answers and the extreme seeds, and proves that run32 passes every bound while each wrong kernel of MUTANTS misses one or breaks a bitwise
stage.

A row: entry (below), its parameters, launches ((label, launches, grid, block, kernel, dynamic LDS bytes), ...) and a note.  One row makes
every call of its scenario, so that the bitwise relations between entry points can be held:
  noise   seed, draws (the draw number written to state[1] before each call; None: what the call before left), specs ((kind, n, a, b, K), ...):
          one ggan_noise_fill per entry of draws, the tensors in slot order
  latent  B, K, D, temp, gl, gk, dz, dmu (False: that pointer NULL), bwd (False: B > 256, forward only), u_one: gmm_latent_fwd with and
          without logits, gmm_latent_st_fwd in both modes, gmm_latent_bwd, gmm_latent_st_bwd in both modes, both again with g_k NULL
          and the CONCRETE backward again with one output each
  mix     B, K, D, onehot: mix_mean
  post    K, D, batches ((row0, B), ...): gmm_posterior_assign per batch with probs and again, on a second colbest, without;
          cluster_accuracy over what they left
  acc     N, K: cluster_accuracy on a prepared assign / colbest

Inputs (inputs()), float32 on the host.  Latent: z and mu are normal draws scaled by 2 / sqrt(D), log_pi = -log K, u is drawn as the noise
kernel draws it ((24-bit word + .5) 2^-24) and carries 2^-25, 0.5 and 1 - 2^-24; the u_one row carries 1.0, which the generator no longer
produces but the kernel accepts.  Row 0 of every K >= 2 row is a tie: two components hold bitwise equal means, z is that mean and both u
are 1 - 2^-24, so that logits, soft and k tie at the top bit for bit.  inputs() redraws (seed + 1000, ...) until every row's float64 top
value is further from every smaller value than the two derived errors (margins(): logits for ST, (logits + g) / temp for STC, where the
bound on the softmax argument + 64 u keeps the float32 softmax strictly ordered); the CPU module asserts that no row is left out.

Stages and bounds (u = 2^-24; no stage carries another's error).  P_LOG = 3, P_EXP = 3, P_SQRT = 3, P_SIN = 4 ulps (1 ulp = 2 u relative):
the OpenCL conformance limits of logf, expf, sqrtf, sinf / cosf -- conditions, not measurements, as P_EXP in _cost_dispatch.
  uniform   (0, 1) and (0, 1/128): the host's float32 u01 bit for bit (a power of two scales exactly).  Any other (a, b):
            u (|a| + |b - a| u01 + |v|) of float64 -- the product's and the sum's rounding, either of which an fma may spare.  a <= v <= b
            always; 0 < v < b where a = 0 (what include/ggan.h and noise_fill_ promise: half-open for a = 0, closed otherwise -- (1, 2)
            with the word ffffff7f gives exactly 2, and the seed-39075 row with that spec asserts it).
  one-hot   min(int(fl(u01 K)), K - 1) of word 0 of the ROW's counter, exactly: one float32 product is deterministic.
  normal    float64 Box-Muller of the host's float32 u01 values and of the float32 product 6.28318530718f u.  r = sqrt(-2 log u): log's
            2 P_LOG u halves under the root, + 2 P_SQRT u; cos / sin 2 P_SIN u; the products b r and (b r) c one u each:
            K_NORMAL = P_LOG + 2 P_SQRT + 2 P_SIN + 2 = 19 u on |b r c|, + u |v| for the sum.
  state     state[1] + 1 and state[2] = 0 after every call; the same seed, draw and slot give the same bits; the draw's high word counts.
  logits    from the inputs: (cdiv(D, 64) + 9) / 2 u S + u |lg|, S = sum (z - mu)^2: the difference's u twice in the square, the fmaf
            chain of cdiv(D, 64) steps, 6 levels of wave_sum, the product with -.5 (exact) and the sum with log_pi (or one fma).
  gumbel    g = -log(-log(u + 1e-20) + 1e-20): u + 1e-20f is u in float32 for u >= 2^-25.  (2 P_LOG + 1) u + 2 P_LOG u |g|: absolute, the outer
            log turns the inner one's relative error and the sum's into an absolute one.  g cannot be read back: the bound enters k's.
  k, soft   from the device's own logits.  The argument (lg + g) inv_temp, inv_temp the float32 1.f / temp: da = inv (e_g + u |lg + g|) + u |a|.
            Relative error of p_j: expm1(da_j + sum_i p_i da_i + x_j + sum_i p_i x_i + (chain + 2) u), x = u |a - max| + 2 P_EXP u (the
            subtraction and expf), chain = cdiv(K, 256) + 10 (the thread loop, wave_sum, block_sum's 4 waves), 2 for the reciprocal and
            the product; + TINY where a value below 2^-126 may be flushed.  Rows sum to 1 within (chain + 2) u.
  k of the straight-through modes   (h - v) + v bit for bit from the device's v (soft, logits), h the one-hot of np.argmax(v): first index.
  argmax    of the device's v against np.argmax of the float64 value from the INPUTS, every row (see margins above).
  dz, dmu   from the inputs and the k the backward read; dlog cannot be read back.  dlog = gl + k (gk - dot) inv_temp: the dot product's
            chain is 12 in a row block (thread loop 1, wave_sum 6, block_sum 4, the product 1) and cdiv(K, 64) + 7 <= 11 in a component
            block; e_dlog = |k| inv 12 u sum|gk k| + 3 u |k (gk - dot) inv| + u |dlog|.  Then sum_j e_dlog_j |z - mu_j| + (K + 2) u
            sum_j |dlog_j (z - mu_j)| for dz (the difference, the K-long fmaf chain), with B for K and the sum over b for dmu.  ST:
            dlog = gl + gk, e_dlog = u |dlog| (0 with one of them NULL).
  mix_mean  one-hot rows: fl(mu_j + noise) bit for bit.  Dense: (K + 1) u sum|k mu| + u |out|.
  probs     against the float64 softmax of float64 logits: as k with da = the logits bound, chain = cdiv(K, 256) + 10.
  assign, colbest   np.argmax of the device's own probs along each axis, exactly, rows in test-set order whatever order the launches ran
            in; the key's high word is the winner's bits.  The same without probs.  correct = the host decode of what the device left.
  bitwise   STC soft = CONCRETE k; the three forward kernels' logits; k with logits NULL; STC backward = CONCRETE backward on soft; ST
            backward with g_k NULL = CONCRETE backward with g_k NULL; an output whether or not the other was requested.

Extreme words (test_latent_dispatch_cpu.py re-derives each with the host Philox; slot 0, draw 0, group / row 0): seed 39075 word 3 =
ffffff7f (u01 would be 1: the uniform value would equal b, which the kernel before this table's fix returned), 2871038 word 2 = ffffffa1
(the radius of the second normal pair), 1343428 word 3 = 00000000 (u01 = 2^-25, the smallest), 56065608 one-hot word 0 = ffffff25 (the index
product reaches K: the min decides).  A zero word in a radius position was not searched for.

Found unreachable or wrong: u01() returned exactly 1.0 for words ffffffxx (fixed: clamped to 1 - 2^-24, no other draw changes);
evaluate.decode_cluster_accuracy indexed label_of with an assign of -1 or K where the kernel counts no match (fixed).  latent.hip has 9
launch sites and 9 kernel instances (gmm_latent_st_fwd_k twice).  noise_fill_k's `step` is always 0.

Worst observed fraction of the bound per kernel, MI355X, 2026-10-20 (test_latent_dispatch_gpu.py prints every row's; above 1 fails):
  gmm_latent_bwd_k         dmu 0.47   dz 0.42
  gmm_latent_fwd_k         k 0.38   logits 0.72   rowsum 0.21
  gmm_latent_st_bwd_k      dmu 0.47   dz 0.42
  gmm_posterior_assign_k   probs 0.25
  mix_mean_k               out 0.80
  noise_fill_k             normal 0.16   uniform 0.25
  gmm_latent_st_fwd_k<kModeKStc>, gmm_latent_st_fwd_k<kModeKSt>, cluster_accuracy_k: exact stages only
mix_mean_k comes near its bound at K = 1, where the bound is two roundings."""
import ctypes as C

import numpy as np

from _cost_dispatch import (U, TINY, P_EXP, P_LOG, PAD, SENTINEL, f32, cdiv, d64, r32, bits, same_bits, _frac, within, _lanes, block_sum32,  # noqa: F401
                            Alloc, _ptrs, _floats, _ints, source_kernels)

# ---- constants the transcription copies (test_latent_dispatch_cpu.py holds them against the source text) ---------------------------------
GMM_MAX_K = 256                # kGmmMaxK
NOISE_MAX = 16                 # GGAN_NOISE_MAX
POSTERIOR_MAX_K = 8192         # GGAN_POSTERIOR_MAX_K
NOISE_PER_WG = 1024            # elements a workgroup of noise_fill_k covers per trip
NOISE_GRID_CAP = 256
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
TWO_PI32 = np.float32(6.28318530718)
E20 = np.float32(1e-20)
U01_MAX = np.float32(1.0 - 2.0 ** -24)
MODE_STC, MODE_ST = 1, 2
P_SQRT, P_SIN = 3, 4
K_NORMAL = P_LOG + 2 * P_SQRT + 2 * P_SIN + 2
DOT_CHAIN = 12
NORMAL, UNIFORM, ONEHOT = 0, 1, 2
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)
# seed -> (one-hot counter?, word index, the word): slot 0, draw 0, group / row 0
EXTREME_SEEDS = {39075: (False, 3, 0xffffff7f), 2871038: (False, 2, 0xffffffa1), 1343428: (False, 3, 0x00000000), 56065608: (True, 0, 0xffffff25)}
BIG_N = 262144 + 1027          # the capped grid, a second trip and a tail of 3: about 1 MB


def softmax_chain(K):
    return cdiv(K, 256) + 10


# ---- rows --------------------------------------------------------------------------------------------------------------------------------
def _row(entry, note, **kw):
    r = dict(entry=entry, note=note, **kw)
    r['launches'] = planned(r)
    return r


def _merge(launches):
    out = {}
    for label, grid, block, kernel, lds in launches:
        k = (label, grid, block, kernel, lds)
        out[k] = out.get(k, 0) + 1
    return tuple((k[0], v, k[1], k[2], k[3], k[4]) for k, v in out.items())


def noise_grid(specs):
    return (min(max(cdiv(max(s[1] for s in specs), NOISE_PER_WG), 1), NOISE_GRID_CAP), len(specs))


def bwd_calls(row):
    """the backward calls of a latent row: (name, entry st?, mode, gl, gk, dz, dmu)"""
    if not row['bwd']:
        return []
    gl, gk, dz, dmu = row['gl'], row['gk'], row['dz'], row['dmu']
    calls = [('', False, 0, gl, gk, dz, dmu), ('_stc', True, MODE_STC, gl, gk, dz, dmu), ('_st', True, MODE_ST, gl, gk, dz, dmu)]
    if gl and gk:
        calls += [('_nogk', False, 0, True, False, dz, dmu), ('_st_nogk', True, MODE_ST, True, False, dz, dmu)]
    if dz and dmu:
        calls += [('_only_dz', False, 0, gl, gk, True, False), ('_only_dmu', False, 0, gl, gk, False, True)]
    return calls


def planned(row):
    """-> the launches the transcription derives for a row, those of one (label, grid, block, kernel, LDS) counted together"""
    e, b = row['entry'], (256,)
    if e == 'noise':
        return _merge([('noise_fill', noise_grid(row['specs']), b, 'noise_fill_k', 0)] * len(row['draws']))
    if e == 'latent':
        B, K = row['B'], row['K']
        out = [('gmm_latent_fwd', (B,), b, 'gmm_latent_fwd_k', 0)] * 2
        out += [('gmm_latent_stc_fwd', (B,), b, 'gmm_latent_st_fwd_k<kModeKStc>', 0), ('gmm_latent_st_fwd', (B,), b, 'gmm_latent_st_fwd_k<kModeKSt>', 0)]
        for _, st, mode, gl, gk, dz, dmu in bwd_calls(row):
            grid = (B + (K if dmu else 0),)
            out.append(('gmm_latent_st_bwd', grid, b, 'gmm_latent_st_bwd_k', 0) if mode == MODE_ST else ('gmm_latent_bwd', grid, b, 'gmm_latent_bwd_k', 0))
        return _merge(out)
    if e == 'mix':
        return _merge([('mix_mean', (cdiv(row['B'] * (row['D'] // 4), 256),), b, 'mix_mean_k', 0)])
    if e == 'post':
        K = row['K']
        return _merge([('gmm_posterior_assign', (B,), b, 'gmm_posterior_assign_k', 4 * K) for _, B in row['batches']] * 2 +
                      [('cluster_accuracy', (1,), b, 'cluster_accuracy_k', 4 * K)])
    return _merge([('cluster_accuracy', (1,), b, 'cluster_accuracy_k', 4 * row['K'])])


def threads(launch):
    """the profiler's grid figure of a launch: work-items"""
    return int(np.prod(launch[2])) * int(np.prod(launch[3]))


ROWS = []
_U, _N, _O = UNIFORM, NORMAL, ONEHOT
_SIZES = ((_U, 1, 0.0, 1.0, 0), (_N, 2, 0.0, 1.0, 0), (_U, 3, 0.0, 1.0 / 128, 0), (_N, 5, 0.5, 2.0, 0), (_U, 1027, -1.0, 3.0, 0), (_N, 1027, 0.0, 1.0, 0),
          (_O, 21, 0.0, 0.0, 3), (_O, 5, 0.0, 0.0, 1), (_O, 330, 0.0, 0.0, 30), (_O, 512, 0.0, 0.0, 256), (_U, 5, 0.0, 1.0, 0), (_U, 2, 0.0, 1.0 / 128, 0))
ROWS.append(_row('noise', 'n = 1, 2, 3, 5, 1027 of every kind, one-hot widths 1, 3, 30, 256; a seed with a high half', seed=0x123456789abcdef0, draws=(5,), specs=_SIZES))
ROWS.append(_row('noise', 'about 1 MB: the capped grid of 256, a second trip of the grid-stride loop, a tail of 3; idle workgroups beside n = 5',
                 seed=11, draws=(0,), specs=((_U, BIG_N, 0.0, 1.0, 0), (_N, 5, 0.0, 1.0, 0))))
ROWS.append(_row('noise', 'count = GGAN_NOISE_MAX: slots 0..15, each with its own counter word', seed=12, draws=(3,),
                 specs=tuple(((_U, 37, 0.0, 1.0, 0), (_N, 37, 0.0, 1.0, 0), (_O, 36, 0.0, 0.0, 3), (_U, 37, -1.0, 3.0, 0))[i % 4] for i in range(NOISE_MAX))))
ROWS.append(_row('noise', 'the draw number crosses 2^32: counter words (ffffffff, 0), then (0, 1)', seed=13, draws=(2 ** 32 - 1, None),
                 specs=((_U, 9, 0.0, 1.0, 0), (_N, 9, 0.0, 1.0, 0), (_O, 9, 0.0, 0.0, 3))))
ROWS.append(_row('noise', 'the same seed, draw and slot twice, then the next draw', seed=14, draws=(7, 7, None),
                 specs=((_U, 9, 0.0, 1.0, 0), (_N, 9, 0.0, 1.0, 0), (_O, 9, 0.0, 0.0, 3))))
ROWS.append(_row('noise', 'word 3 = ffffff7f: element 3 would be b', seed=39075, draws=(0,), specs=((_U, 4, 0.0, 1.0, 0),)))
ROWS.append(_row('noise', 'word 3 = ffffff7f under (0, 1/128)', seed=39075, draws=(0,), specs=((_U, 4, 0.0, 1.0 / 128, 0),)))
ROWS.append(_row('noise', 'word 3 = ffffff7f under (1, 2): closed, the value rounds onto b', seed=39075, draws=(0,), specs=((_U, 4, 1.0, 2.0, 0),)))
ROWS.append(_row('noise', 'word 2 = ffffffa1: the radius of the second normal pair', seed=2871038, draws=(0,), specs=((_N, 4, 0.0, 1.0, 0),)))
ROWS.append(_row('noise', 'word 3 = 00000000: u01 = 2^-25', seed=1343428, draws=(0,), specs=((_U, 4, 0.0, 1.0, 0),)))
ROWS.append(_row('noise', 'word 3 = 00000000 as the angle of the second normal pair', seed=1343428, draws=(0,), specs=((_N, 4, 0.0, 1.0, 0),)))
ROWS.append(_row('noise', 'one-hot word 0 = ffffff25: the index product reaches K', seed=56065608, draws=(0,), specs=((_O, 30, 0.0, 0.0, 30),)))

_ALL = dict(gl=True, gk=True, dz=True, dmu=True)
_LATENT = [
    (1, 1, 1, 1.0, _ALL, 'everything 1'),
    (5, 4, 63, 0.5, _ALL, 'a lane idle, every wave one component'),
    (5, 5, 65, 0.1, _ALL, 'a ragged second trip of d += 64, a second trip of j += 4'),
    (255, 255, 1, 1.0, _ALL, 'B, K = 255'),
    (256, 5, 257, 0.5, _ALL, 'B = kGmmMaxK fills sv of a component block; a second trip of d += 256'),
    (5, 256, 130, 0.1, _ALL, 'K = kGmmMaxK; a third trip of d += 64'),
    (5, 30, 300, 0.1, _ALL, 'D = 300: a ragged second trip of d += 256'),
]
for _B, _K, _D, _t, _kw, _note in _LATENT:
    ROWS.append(_row('latent', _note, B=_B, K=_K, D=_D, temp=_t, bwd=True, u_one=False, **_kw))
ROWS.append(_row('latent', 'B = 300: forward only', B=300, K=5, D=65, temp=1.0, bwd=False, u_one=False, **_ALL))
ROWS.append(_row('latent', 'u carries 1.0: g = -log(1e-20)', B=5, K=5, D=63, temp=0.1, bwd=True, u_one=True, **_ALL))
for _i, (_gl, _gk) in enumerate(((True, True), (True, False), (False, True))):
    for _j, (_dz, _dmu) in enumerate(((True, True), (True, False), (False, True))):
        if _i or _j:
            ROWS.append(_row('latent', 'NULL combination', B=5, K=(4, 5)[_j % 2], D=(63, 65)[_i % 2], temp=(1.0, 0.5, 0.1)[(_i + _j) % 3], bwd=True, u_one=False,
                             gl=_gl, gk=_gk, dz=_dz, dmu=_dmu))
for _B, _K, _D, _oh in ((255, 1, 4, False), (64, 30, 16, True), (257, 100, 4, False), (257, 30, 4, True)):
    ROWS.append(_row('mix', 'B D / 4 = %d' % (_B * _D // 4), B=_B, K=_K, D=_D, onehot=_oh))
_THREE = ((128, 3), (0, 3), (64, 3))
for _K, _D, _batches in ((1, 1, ((0, 1),)), (1, 65, _THREE), (255, 65, _THREE), (257, 130, _THREE), (300, 1, _THREE), (POSTERIOR_MAX_K, 65, _THREE)):
    ROWS.append(_row('post', 'launches at rows %s' % ', '.join(str(r) for r, _ in _batches), K=_K, D=_D, batches=_batches))
ROWS.append(_row('acc', 'N ragged over 256 threads; assign of -1 and K; a key of 0; an underflowed column; a row past N', N=300, K=7))


def row_id(row):
    e = row['entry']
    if e == 'noise':
        return 'noise-s%x-c%d-n%d-d%s' % (row['seed'], len(row['specs']), max(s[1] for s in row['specs']),
                                          '_'.join('x' if d is None else '%x' % d for d in row['draws'])) + \
            ('-k%d-%g-%g' % (row['specs'][0][:1] + row['specs'][0][2:4]) if len(row['specs']) == 1 else '')
    if e == 'latent':
        return 'latent-%dx%dx%d-t%g%s%s%s%s%s%s' % (row['B'], row['K'], row['D'], row['temp'], '' if row['gl'] else '-nogl', '' if row['gk'] else '-nogk',
                                                    '' if row['dz'] else '-nodz', '' if row['dmu'] else '-nodmu', '' if row['bwd'] else '-fwd', '-u1' if row['u_one'] else '')
    if e == 'mix':
        return 'mix-%dx%dx%d%s' % (row['B'], row['K'], row['D'], '-onehot' if row['onehot'] else '')
    if e == 'post':
        return 'post-k%d-d%d-%s' % (row['K'], row['D'], '_'.join('%d+%d' % b for b in row['batches']))
    return 'acc-n%d-k%d' % (row['N'], row['K'])


# ---- Philox4x32-10 and the noise kernel's use of it, on the host ---------------------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def philox(counter, key, rounds=10, swapped=False):
    """Philox4x32 (Salmon et al. 2011): per round (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the
    key grows by the Weyl constants.  counter: four uint arrays (broadcast), key: two ints -> uint32 array [..., 4]"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint64) for c in counter])
    k0, k1 = int(key[0]), int(key[1])
    m0, m1 = (PHILOX_M1, PHILOX_M0) if swapped else (PHILOX_M0, PHILOX_M1)
    for _ in range(rounds):
        p0, p1 = np.uint64(m0) * c0, np.uint64(m1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _M32
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def u01(x, mut=None):
    """the kernel's u01 in float32: (top 24 bits + .5) 2^-24, the one value that rounds to 1 moved to 1 - 2^-24"""
    top = (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32)
    if mut == 'u01_no_half':
        return top * f32(2.0 ** -24)
    v = (top + f32(0.5)) * f32(2.0 ** -24)
    return v if mut == 'u01_unclamped' else np.minimum(v, U01_MAX)


def words(seed, slot, draw, idx, onehot, mut=None):
    """the four words of counter (idx, slot [| bit 31], draw low, draw high) under key = the seed's halves"""
    w1 = (0 if mut == 'slot_left_out' else slot) | (0x80000000 if onehot else 0)
    hi = 0 if mut == 'draw_high_dropped' else (draw >> 32) & 0xFFFFFFFF
    return philox((idx, w1, draw & 0xFFFFFFFF, hi), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF),
                  rounds=9 if mut == 'philox_9_rounds' else 10, swapped=mut == 'multipliers_swapped')


def noise_u(spec, seed, slot, draw, mut=None):
    """the float32 u01 values a tensor is made of: [groups, 4] (uniform, normal) or one per row (one-hot; per element under the mutant)"""
    kind, n, _, _, K = spec
    if kind == ONEHOT:
        idx = np.arange(n) if mut == 'onehot_keyed_by_element' else np.arange(n // K)
        return u01(words(seed, slot, draw, idx, True, mut)[:, 0], mut)
    return u01(words(seed, slot, draw, np.arange(cdiv(n, 4)), False, mut), mut)


def noise32(spec, seed, slot, draw, mut=None):
    """one tensor of noise_fill_k in float32 -> n values"""
    kind, n, a, b, K = spec
    a, b = f32(a), f32(b)
    u = noise_u(spec, seed, slot, draw, mut)
    with np.errstate(all='ignore'):
        if kind == ONEHOT:
            idx = np.minimum((u * f32(K)).astype(np.uint32), np.uint32(K - 1))
            if mut == 'onehot_keyed_by_element':
                return (np.arange(n) % K == idx).astype(np.float32)
            v = np.zeros((n // K, K), np.float32)
            v[np.arange(n // K), idx] = 1
            return v.ravel()
        if kind == UNIFORM:
            return (a + (b - a) * u).ravel()[:n]
        r0, r1 = np.sqrt(f32(-2) * np.log(u[:, 0])), np.sqrt(f32(-2) * np.log(u[:, 2]))
        t0, t1 = TWO_PI32 * u[:, 1], TWO_PI32 * u[:, 3]
        v = np.stack([a + b * r0 * np.cos(t0), a + b * r0 * np.sin(t0), a + b * r1 * np.cos(t1), a + b * r1 * np.sin(t1)], -1)
        return v.astype(np.float32).ravel()[:n]


def normal64(spec, seed, slot, draw):
    """-> (float64 Box-Muller of the float32 u01 values and float32 angles, its bound)"""
    _, n, a, b, _ = spec
    a, b = r32(a), r32(b)
    u = noise_u(spec, seed, slot, draw)
    rad = np.sqrt(-2.0 * np.log(d64(u[:, [0, 0, 2, 2]])))
    th = d64(np.stack([TWO_PI32 * u[:, 1], TWO_PI32 * u[:, 3]], -1))
    cs = np.stack([np.cos(th[:, 0]), np.sin(th[:, 0]), np.cos(th[:, 1]), np.sin(th[:, 1])], -1)
    v = a + b * rad * cs
    return v.ravel()[:n], (K_NORMAL * U * np.abs(b * rad * cs) + U * np.abs(v) + TINY).ravel()[:n]


def draws_of(row):
    out = []
    for d in row['draws']:
        out.append(out[-1] + 1 if d is None else d)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
_c32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)


def _draw_u(rng, shape):
    return np.minimum((rng.integers(0, 1 << 24, size=shape).astype(np.float32) + f32(0.5)) * f32(2.0 ** -24), U01_MAX)


def tie_pair(K):
    return K // 3, K - 1


def _latent_inputs(row, seed):
    rng = np.random.default_rng(seed)
    B, K, D = row['B'], row['K'], row['D']
    sc = 2.0 / np.sqrt(D)
    z, mu = _c32(sc * rng.standard_normal((B, D))), _c32(sc * rng.standard_normal((K, D)))
    u = _draw_u(rng, (B, K))
    edge = [f32(2.0 ** -25), f32(0.5), U01_MAX] + ([f32(1.0)] if row['u_one'] else [])
    for i, v in enumerate(edge[:B * K]):
        u.flat[B * K - 1 - i] = v
    if K >= 2:
        j1, j2 = tie_pair(K)
        mu[j2] = mu[j1]
        z[0] = mu[j1]
        u[0, j1] = u[0, j2] = U01_MAX
    return dict(z=z, mu=mu, u=u, gl=_c32(rng.standard_normal((B, K))), gk=_c32(rng.standard_normal((B, K))), log_pi=f32(-np.log(K)))


def inputs(row, seed):
    """-> dict of host arrays (float32 unless said)"""
    e = row['entry']
    if e == 'noise':
        return {}
    if e == 'latent':
        for attempt in range(50):
            inp = _latent_inputs(row, seed + 1000 * attempt)
            if min(m.min() for m in margins(row, inp).values()) > 0:
                inp['attempt'] = attempt
                return inp
        raise AssertionError('no draw with every top-two gap above the bound: %s' % row_id(row))
    rng = np.random.default_rng(seed)
    if e == 'mix':
        B, K, D = row['B'], row['K'], row['D']
        k = _c32(rng.standard_normal((B, K)))
        if row['onehot']:
            k = np.zeros((B, K), np.float32)
            k[np.arange(B), rng.integers(0, K, B)] = 1
        return dict(k=k, mu=_c32(rng.standard_normal((K, D))), noise=_c32(rng.standard_normal((B, D))))
    if e == 'post':
        K, D = row['K'], row['D']
        sc = 2.0 / np.sqrt(D)
        mu = _c32(sc * rng.standard_normal((K, D)))
        jstar = K // 2
        if K > 1:
            mu[jstar] = mu[jstar] + f32(8.0)
        zs = [_c32(sc * rng.standard_normal((B, D))) for _, B in row['batches']]
        if len(zs) > 1:                                              # rows 129 and 1, in the first and the second launch: the same bits
            zs[0][1] = mu[jstar]
            zs[1][1] = mu[jstar]
        N = max(r0 + B for r0, B in row['batches'])
        return dict(mu=mu, zs=zs, log_pi=f32(-np.log(K)), labels=rng.integers(0, 4, N).astype(np.int32), jstar=jstar)
    N, K = row['N'], row['K']
    labels = rng.integers(0, 3, N).astype(np.int32)
    assign = rng.integers(0, K, N).astype(np.int32)
    assign[3], assign[4], assign[N - 1], assign[256] = -1, K, 1, 0
    rows = rng.integers(0, N, K).astype(np.uint64)
    p = _c32(rng.random(K) * 0.9 + 0.05)
    col = (p.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - rows)
    col[0] = 0                                                       # nobody wrote it
    col[1] = np.uint64(0xFFFFFFFF)                                   # every probability underflowed: p = 0, the lowest row
    col[K - 1] = (np.uint64(0x3F000000) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.uint64(N))     # a row past N
    return dict(assign=assign, labels=labels, colbest=col)


# ---- the kernels in float32, in their summation order (no contraction: a device fmaf rounds once where this rounds twice) ----------------
MUTANTS = ('philox_9_rounds', 'multipliers_swapped', 'slot_left_out', 'draw_high_dropped', 'onehot_keyed_by_element', 'u01_no_half', 'u01_unclamped',
           'tail_guard_off_by_one', 'single_log_gumbel', 'softmax_no_max', 'temp_multiplied', 'dlog_without_dot', 'dz_wrong_sign', 'dmu_summed_over_K',
           'last_index_wins_tie', 'half_dropped', 'highest_row_wins_tie')
NAN32 = f32(np.nan)


def wave_sum32(s):
    """wave_sum's xor butterfly over the last axis of 64 lanes (lane 0's view)"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., idx ^ o]
    return s[..., 0]


def logits32(z, mu, log_pi, mut=None):
    t = z[:, None, :] - mu[None, :, :]
    s = wave_sum32(_lanes(t * t, 64))
    return (f32(-1.0) if mut == 'half_dropped' else f32(-0.5)) * s + f32(log_pi)


def gumbel32(u, mut=None):
    if mut == 'single_log_gumbel':
        return -np.log(u + E20)
    return -np.log(-np.log(u + E20) + E20)


def softmax32(sv, mut=None):
    m = np.zeros(sv.shape[0], np.float32) if mut == 'softmax_no_max' else sv.max(1)
    t = np.exp(sv - m[:, None])
    inv = f32(1) / block_sum32(_lanes(t, 256))
    return t * inv[:, None]


def argmax_first(v, mut=None):
    if mut == 'last_index_wins_tie':
        return v.shape[1] - 1 - np.argmax(v[:, ::-1], 1)
    return np.argmax(v, 1)


def st_value32(v, hot):
    h = np.zeros_like(v)
    h[np.arange(v.shape[0]), hot] = 1
    return (h - v) + v


def inv_temp32(temp, mut=None):
    return f32(temp) if mut == 'temp_multiplied' else f32(1) / f32(temp)


def bwd32(z, mu, kk, gl, gk, inv, dz, dmu, st, mut=None):
    """gmm_latent_bwd_k (st: gmm_latent_st_bwd_k) -> (dz or None, dmu or None); the row blocks' and the component blocks' dlog apart"""
    B, K = z.shape[0], mu.shape[0]
    zero = np.zeros((B, K), np.float32)
    base = gl if gl is not None else zero
    if gk is None:
        dl_row = dl_col = base
    elif st:
        dl_row = dl_col = base + gk
    else:
        prod = gk * kk
        dots = [block_sum32(_lanes(prod, 256)), wave_sum32(_lanes(prod, 64))]
        if mut == 'dlog_without_dot':
            dots = [np.zeros(B, np.float32)] * 2
        dl_row, dl_col = [base + (kk * (gk - d[:, None])) * inv for d in dots]
    out_dz = out_dmu = None
    if dz:
        acc = np.zeros_like(z)
        for j in range(K):
            acc = acc + dl_row[:, j, None] * (z - mu[j][None, :])
        out_dz = acc if mut == 'dz_wrong_sign' else -acc
    if dmu:
        acc = np.zeros_like(mu)
        for b in range(min(K, B) if mut == 'dmu_summed_over_K' else B):
            acc = acc + dl_col[b][:, None] * (z[b][None, :] - mu)
        out_dmu = acc
    return out_dz, out_dmu


def _latent32(row, inp, mut):
    z, mu, u = inp['z'], inp['mu'], inp['u']
    inv = inv_temp32(row['temp'], mut)
    lg = logits32(z, mu, inp['log_pi'], mut)
    k = softmax32((lg + gumbel32(u, mut)) * inv, mut)
    out = dict(lg=lg, k=k, k_nolog=k, lg_stc=lg, soft=k, k_stc=st_value32(k, argmax_first(k, mut)), lg_st=lg, k_st=st_value32(lg, argmax_first(lg, mut)))
    for name, st, mode, gl, gk, dz, dmu in bwd_calls(row):
        a, b = bwd32(z, mu, k, inp['gl'] if gl else None, inp['gk'] if gk else None, inv, dz, dmu, mode == MODE_ST, mut)
        out['dz' + name], out['dmu' + name] = a, b
    return out


def _noise32(row, inp, mut):
    vals = []
    for d in draws_of(row):
        call = []
        for slot, spec in enumerate(row['specs']):
            v = np.concatenate([noise32(spec, row['seed'], slot, d, mut), np.full(PAD, SENTINEL, np.float32)])
            if mut == 'tail_guard_off_by_one' and spec[1] % 4:
                more = noise32((spec[0], spec[1] + 1) + spec[2:], row['seed'], slot, d)
                if spec[0] != ONEHOT:
                    v[spec[1]] = more[spec[1]]
            call.append(v)
        vals.append(call)
    ds = draws_of(row)
    return dict(vals=vals, states=[(row['seed'], d + 1, 0) for d in ds])


def _mix32(row, inp, mut):
    acc = np.zeros((row['B'], row['D']), np.float32)
    for j in range(row['K']):
        acc = acc + inp['k'][:, j, None] * inp['mu'][j][None, :]
    return dict(out=acc + inp['noise'])


def column_keys(P, grows, mut=None):
    """colbest of probabilities P [rows, K] whose test-set rows are grows"""
    low = np.asarray(grows, np.uint64) if mut == 'highest_row_wins_tie' else np.uint64(0xFFFFFFFF) - np.asarray(grows, np.uint64)
    keys = (np.ascontiguousarray(P, np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | low[:, None]
    return keys.max(0)


def decode_accuracy(assign, labels, colbest):
    """cluster_accuracy_k on the host"""
    assign, labels = np.asarray(assign, np.int64), np.asarray(labels, np.int64)
    N, K = labels.size, len(colbest)
    rows = 0xFFFFFFFF - (np.asarray(colbest, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    label_of = np.where(rows < N, labels[np.minimum(rows, N - 1)], np.iinfo(np.int64).min)
    ok = (assign >= 0) & (assign < K)
    return int(np.sum(ok & (label_of[np.clip(assign, 0, K - 1)] == labels)))


def _post32(row, inp, mut):
    K = row['K']
    N = inp['labels'].size
    probs, assign, col = [], np.full(N, -1, np.int32), np.zeros(K, np.uint64)
    for (r0, B), z in zip(row['batches'], inp['zs']):
        lg = logits32(z, inp['mu'], inp['log_pi'], mut)
        p = softmax32(lg, mut)
        probs.append(p)
        assign[r0:r0 + B] = argmax_first(p, mut)
        col = np.maximum(col, column_keys(p, np.arange(r0, r0 + B), mut))
    return dict(probs=probs, assign=assign, colbest=col, assign2=assign.copy(), colbest2=col.copy(), correct=decode_accuracy(assign, inp['labels'], col))


def _acc32(row, inp, mut):
    return dict(correct=decode_accuracy(inp['assign'], inp['labels'], inp['colbest']))


_RUN32 = dict(noise=_noise32, latent=_latent32, mix=_mix32, post=_post32, acc=_acc32)


def run32(row, inp, mut=None):
    """every output of a row's calls from the float32 restatement; `mut` names one wrong kernel of MUTANTS"""
    with np.errstate(all='ignore'):
        return _RUN32[row['entry']](row, inp, mut)


# ---- float64 restatements and the staged checks ------------------------------------------------------------------------------------------
def logits64(z, mu, log_pi):
    """-> (float64 logits from the float32 inputs, their bound)"""
    D = z.shape[1]
    S = ((d64(z)[:, None, :] - d64(mu)[None, :, :]) ** 2).sum(2)
    lg = -0.5 * S + r32(log_pi)
    return lg, (cdiv(D, 64) + 9) / 2.0 * U * S + U * np.abs(lg) + TINY


def gumbel64(u):
    """-> (g in float64 from the float32 u as the kernel reads it, its bound); u + 1e-20f is u in float32 for u >= 2^-25"""
    assert np.all(u >= f32(2.0 ** -25))
    with np.errstate(divide='ignore'):
        g = -np.log(-np.log(d64(u)) + float(E20))
    return g, (2 * P_LOG + 1) * U + 2 * P_LOG * U * np.abs(g)


def softmax64(a, da, K):
    """-> (softmax of the float64 arguments a, its bound when the device's arguments are within da of them)"""
    m = a.max(1, keepdims=True)
    e = np.exp(a - m)
    p = e / e.sum(1, keepdims=True)
    x = U * np.abs(a - m) + 2 * P_EXP * U
    rel = da + (p * da).sum(1, keepdims=True) + x + (p * x).sum(1, keepdims=True) + (softmax_chain(K) + 2) * U
    return p, p * np.expm1(rel) + TINY


def margins(row, inp):
    """{mode: per row, how far the float64 top value is above every smaller one beyond the two derived errors} -- all must be positive"""
    K = row['K']
    lg, elg = logits64(inp['z'], inp['mu'], inp['log_pi'])
    g, eg = gumbel64(inp['u'])
    inv = float(f32(1) / f32(row['temp']))
    a = (lg + g) * inv
    ea = inv * (elg + eg + U * np.abs(lg + g)) + U * np.abs(a) + 64 * U
    out = {}
    for name, v, e in (('st', lg, elg), ('stc', a, ea)):
        top = np.argmax(v, 1)
        r = np.arange(v.shape[0])
        gap = v[r, top][:, None] - v - e - e[r, top][:, None]
        out[name] = np.where(v < v[r, top][:, None], gap, np.inf).min(1) if K > 1 else np.full(v.shape[0], np.inf)
    return out


def dlog64(kk, gl, gk, inv, st):
    """-> (dlog in float64, its bound) from the float32 k, g_logits, g_k (None: NULL)"""
    base = d64(gl) if gl is not None else np.zeros(kk.shape)
    if gk is None:
        return base, np.zeros(kk.shape)
    gk = d64(gk)
    if st:
        dl = base + gk
        return dl, (U * np.abs(dl) if gl is not None else np.zeros(kk.shape))
    k = d64(kk)
    dot = (gk * k).sum(1, keepdims=True)
    t3 = k * (gk - dot) * inv
    dl = base + t3
    return dl, np.abs(k) * inv * DOT_CHAIN * U * np.abs(gk * k).sum(1, keepdims=True) + 3 * U * np.abs(t3) + U * np.abs(dl)


def bwd64(z, mu, kk, gl, gk, inv, st):
    """-> ((dz, bound), (dmu, bound)) in float64"""
    B, K = kk.shape
    dl, edl = dlog64(kk, gl, gk, inv, st)
    diff = d64(z)[:, None, :] - d64(mu)[None, :, :]
    t, et = dl[:, :, None] * diff, edl[:, :, None] * np.abs(diff)
    return ((-t.sum(1), et.sum(1) + (K + 2) * U * np.abs(t).sum(1) + TINY), (t.sum(0), et.sum(0) + (B + 2) * U * np.abs(t).sum(0) + TINY))


def _chk_latent(row, inp, out, fr, broken):
    B, K, D = row['B'], row['K'], row['D']
    z, mu, u = inp['z'], inp['mu'], inp['u']
    inv = float(f32(1) / f32(row['temp']))
    lg64, elg = logits64(z, mu, inp['log_pi'])
    fr['logits'] = _frac(np.abs(d64(out['lg']) - lg64), elg)
    # k from the device's own logits
    g, eg = gumbel64(u)
    s = d64(out['lg']) + g
    a = s * inv
    p, ep = softmax64(a, inv * (eg + U * np.abs(s)) + U * np.abs(a), K)
    fr['k'] = _frac(np.abs(d64(out['k']) - p), ep)
    fr['rowsum'] = _frac(np.abs(d64(out['k']).sum(1) - 1.0), np.full(B, (softmax_chain(K) + 2) * U + K * TINY))
    for a_, b_, what in (('k_nolog', 'k', 'k differs with logits NULL'), ('soft', 'k', 'STC soft is not the CONCRETE k'),
                         ('lg_stc', 'lg', 'STC logits differ'), ('lg_st', 'lg', 'ST logits differ')):
        if not same_bits(out[a_], out[b_]):
            broken.append(what)
    # the straight-through values from the device's own v; the argmax against float64 from the inputs
    ga, _ = gumbel64(u)
    for key, v, ref in (('k_stc', out['soft'], (lg64 + ga) * inv), ('k_st', out['lg_st'], lg64)):
        v = np.asarray(v, np.float32)
        hot = np.argmax(v, 1)
        if not same_bits(out[key], st_value32(v, hot)):
            broken.append('%s is not (h - v) + v with h at the first maximum of v' % key)
        if not np.array_equal(hot, np.argmax(ref, 1)):
            broken.append('%s: argmax differs from float64 in rows %s' % (key, np.nonzero(hot != np.argmax(ref, 1))[0][:5]))
    if K >= 2:
        j1, j2 = tie_pair(K)
        for key in ('lg', 'soft'):
            v = np.asarray(out[key], np.float32)
            if bits(v[0, j1]) != bits(v[0, j2]) or np.argmax(v[0]) != j1:
                broken.append('the tie of row 0 is not a tie at the top of %s' % key)
    # the backward calls, each from the inputs and the k it read
    for name, st, mode, gl, gk, dz, dmu in bwd_calls(row):
        if name in ('_stc', '_only_dz', '_only_dmu'):
            continue
        st_ = mode == MODE_ST
        (rz, bz), (rm, bm) = bwd64(z, mu, np.asarray(out['k'], np.float32), inp['gl'] if gl else None, inp['gk'] if gk else None, inv, st_)
        if dz:
            fr['dz' + name] = _frac(np.abs(d64(out['dz' + name]) - rz), bz)
        if dmu:
            fr['dmu' + name] = _frac(np.abs(d64(out['dmu' + name]) - rm), bm)
    if row['bwd']:
        pairs = [('_stc', '', 'the STC backward is not the CONCRETE backward on soft')]
        if row['gl'] and row['gk']:
            pairs.append(('_st_nogk', '_nogk', 'ST backward with g_k NULL differs from the CONCRETE backward with g_k NULL'))
        if not row['gk']:
            pairs.append(('_st', '', 'ST backward with g_k NULL differs from the CONCRETE backward with g_k NULL'))
        for a_, b_, what in pairs:
            for o in ('dz', 'dmu'):
                if row[o] and not same_bits(out[o + a_], out[o + b_]):
                    broken.append('%s: %s' % (o, what))
        if row['dz'] and row['dmu']:
            if not same_bits(out['dz_only_dz'], out['dz']) or not same_bits(out['dmu_only_dmu'], out['dmu']):
                broken.append('an output changes when the other one is not requested')
        for name, _, _, _, _, dz, dmu in bwd_calls(row):
            for o, want in (('dz', dz), ('dmu', dmu)):
                if not want and out[o + name] is not None and not np.all(np.isnan(out[o + name])):
                    broken.append('%s%s was NULL and something was written' % (o, name))


def _chk_noise(row, inp, out, fr, broken):
    ds = draws_of(row)
    fr.update(uniform=0.0, normal=0.0)
    for c, d in enumerate(ds):
        if tuple(int(x) for x in out['states'][c]) != (row['seed'], d + 1, 0):
            broken.append('state after call %d: %s' % (c, out['states'][c]))
        for slot, spec in enumerate(row['specs']):
            kind, n, a, b, K = spec
            got = np.asarray(out['vals'][c][slot], np.float32)
            v, tail = got[:n], got[n:]
            if tail.size != PAD or not np.all(bits(tail) == bits(SENTINEL)):
                broken.append('call %d slot %d: the pad behind the tensor changed' % (c, slot))
            if not np.all(np.isfinite(v)):
                broken.append('call %d slot %d: not finite' % (c, slot))
                continue
            if kind == ONEHOT:
                if not same_bits(v, noise32(spec, row['seed'], slot, d)):
                    broken.append('call %d slot %d: one-hot rows differ from the host' % (c, slot))
            elif kind == UNIFORM:
                a32, b32 = f32(a), f32(b)
                if a == 0.0 and float(b32) in (1.0, 1.0 / 128):
                    if not same_bits(v, noise32(spec, row['seed'], slot, d)):
                        broken.append('call %d slot %d: uniform differs from the host u01 bit for bit' % (c, slot))
                un = d64(noise_u(spec, row['seed'], slot, d).ravel()[:n])
                ref = float(a32) + (float(b32) - float(a32)) * un
                fr['uniform'] = max(fr['uniform'], _frac(np.abs(d64(v) - ref), U * (abs(float(a32)) + abs(float(b32) - float(a32)) * un + np.abs(d64(v))) + TINY))
                if not (np.all(v >= a32) and np.all(v <= b32)):
                    broken.append('call %d slot %d: a uniform value outside [a, b]' % (c, slot))
                if a == 0.0 and not (np.all(v > 0) and np.all(v < b32)):
                    broken.append('call %d slot %d: a uniform value with a = 0 outside (0, b)' % (c, slot))
            else:
                ref, bound = normal64(spec, row['seed'], slot, d)
                fr['normal'] = max(fr['normal'], _frac(np.abs(d64(v) - ref), bound))
    for c in range(1, len(ds)):
        for c0 in range(c):
            if ds[c] == ds[c0] and not all(same_bits(x, y) for x, y in zip(out['vals'][c], out['vals'][c0])):
                broken.append('calls %d and %d have the same seed, draw and slots and differ' % (c0, c))


def _chk_mix(row, inp, out, fr, broken):
    k, mu, noise = inp['k'], inp['mu'], inp['noise']
    if row['onehot']:
        fr['out'] = 0.0 if same_bits(out['out'], mu[np.argmax(k, 1)] + noise) else np.inf
        return
    t = d64(k)[:, :, None] * d64(mu)[None, :, :]
    ref = t.sum(1) + d64(noise)
    fr['out'] = _frac(np.abs(d64(out['out']) - ref), (row['K'] + 1) * U * np.abs(t).sum(1) + U * np.abs(d64(out['out'])) + TINY)


def _chk_post(row, inp, out, fr, broken):
    K = row['K']
    fr['probs'] = 0.0
    grows, P = [], []
    for (r0, B), z, p in zip(row['batches'], inp['zs'], out['probs']):
        lg, elg = logits64(z, inp['mu'], inp['log_pi'])
        ref, bound = softmax64(lg, elg, K)
        fr['probs'] = max(fr['probs'], _frac(np.abs(d64(p) - ref), bound))
        grows += list(range(r0, r0 + B))
        P.append(np.asarray(p, np.float32))
    order = np.argsort(grows)
    grows, P = np.asarray(grows)[order], np.concatenate(P)[order]
    want = np.full(inp['labels'].size, -1, np.int64)
    want[grows] = np.argmax(P, 1)
    if not np.array_equal(want, np.asarray(out['assign'], np.int64)):
        broken.append('assign is not np.argmax of the device probs (-1 where no launch wrote)')
    best = np.argmax(P, 0)                                           # the lowest test-set row on a tie
    keys = (P[best, np.arange(K)].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - grows[best].astype(np.uint64))
    if not np.array_equal(keys, np.asarray(out['colbest'], np.uint64)):
        broken.append('colbest is not the column argmax of the device probs, lowest row first')
    if len(row['batches']) > 1:
        r_first, r_second = row['batches'][0][0] + 1, row['batches'][1][0] + 1
        i1, i2 = int(np.nonzero(grows == r_first)[0][0]), int(np.nonzero(grows == r_second)[0][0])
        j = inp['jstar']
        if not same_bits(P[i1], P[i2]) or P[i1, j] != P[:, j].max() or r_second >= r_first:
            broken.append('the two tie rows do not hold the bitwise-equal column maximum')
    if not np.array_equal(out['assign2'], out['assign']) or not np.array_equal(out['colbest2'], out['colbest']):
        broken.append('assign / colbest change with probs NULL')
    if int(out['correct']) != decode_accuracy(out['assign'], inp['labels'], out['colbest']):
        broken.append('correct %d is not the host decode %d' % (out['correct'], decode_accuracy(out['assign'], inp['labels'], out['colbest'])))


def _chk_acc(row, inp, out, fr, broken):
    want = decode_accuracy(inp['assign'], inp['labels'], inp['colbest'])
    if int(out['correct']) != want:
        broken.append('correct %d, the host decode %d' % (out['correct'], want))


_CHECK = dict(noise=_chk_noise, latent=_chk_latent, mix=_chk_mix, post=_chk_post, acc=_chk_acc)
_INTS = ('assign', 'assign2', 'colbest', 'colbest2', 'correct', 'states', 'vals')


def check(row, inp, out):
    """-> ({check: worst fraction of its bound}, [exact stages that do not hold]) for the outputs `out` of a row's calls"""
    fr, broken = {}, []
    with np.errstate(all='ignore'):
        _CHECK[row['entry']](row, inp, out, fr, broken)
    for k, v in out.items():
        for a in (v if isinstance(v, list) else [v]):
            if a is not None and k not in _INTS and not np.all(np.isfinite(np.asarray(a, np.float64))):
                broken.append('%s is not finite' % k)
    return fr, broken


def kernels_of(row):
    """{check name: the kernel it measures} -- for the per-kernel worst figures"""
    e = row['entry']
    if e == 'noise':
        return dict(uniform='noise_fill_k', normal='noise_fill_k')
    if e == 'latent':
        out = dict(logits='gmm_latent_fwd_k', k='gmm_latent_fwd_k', rowsum='gmm_latent_fwd_k')
        for name, _, mode, _, _, _, _ in bwd_calls(row):
            for o in ('dz', 'dmu'):
                out[o + name] = 'gmm_latent_st_bwd_k' if mode == MODE_ST else 'gmm_latent_bwd_k'
        return out
    return dict(out='mix_mean_k') if e == 'mix' else dict(probs='gmm_posterior_assign_k') if e == 'post' else {}


# ---- calls that must be refused before any launch ----------------------------------------------------------------------------------------
def _off(p, nbytes):
    return C.c_void_p(p.value + nbytes)


def _rej_noise(count=1, size=8, kind=UNIFORM, width=0, null=None, real_count=None):
    def call(L, A, S):
        n = max(real_count or count, 1)
        bufs = [A.buf(64, out=True) for _ in range(n)]
        args = dict(dsts=_ptrs(bufs), sizes=(C.c_size_t * n)(*[size] * n), kinds=_ints([kind] * n), a=_floats([0.0] * n), b=_floats([1.0] * n),
                    widths=_ints([width] * n), state=A.buf(6, out=True))
        if null == 'dst':
            args['dsts'] = (C.c_void_p * n)(*[None] * n)
        elif null:
            args[null] = None
        return L.ggan_noise_fill(args['dsts'], args['sizes'], args['kinds'], args['a'], args['b'], args['widths'], count, args['state'], S)
    return call


def _rej_latent(fn, B=4, K=4, D=8, temp=1.0, mode=None, null=()):
    def call(L, A, S):
        b, k = min(max(B, 1), 300), min(max(K, 1), 300)
        p = dict(z=A.buf(b * max(D, 1)), mu=A.buf(k * max(D, 1)), u=A.buf(b * k), kk=A.buf(b * k), gl=A.buf(b * k), gk=A.buf(b * k),
                 logits=A.buf(b * k, out=True), k=A.buf(b * k, out=True), soft=A.buf(b * k, out=True), dz=A.buf(b * max(D, 1), out=True),
                 dmu=A.buf(k * max(D, 1), out=True))
        for name in null:
            p[name] = None
        if fn == 'ggan_gmm_latent_fwd':
            return L.ggan_gmm_latent_fwd(p['z'], p['mu'], p['u'], p['logits'], p['k'], B, K, D, 0.0, temp, S)
        if fn == 'ggan_gmm_latent_bwd':
            return L.ggan_gmm_latent_bwd(p['z'], p['mu'], p['kk'], p['gl'], p['gk'], p['dz'], p['dmu'], B, K, D, temp, S)
        if fn == 'ggan_gmm_latent_st_fwd':
            return L.ggan_gmm_latent_st_fwd(p['z'], p['mu'], p['u'], p['logits'], p['k'], p['soft'], B, K, D, 0.0, temp, mode, S)
        return L.ggan_gmm_latent_st_bwd(p['z'], p['mu'], p['kk'], p['gl'], p['gk'], p['dz'], p['dmu'], B, K, D, temp, mode, S)
    return call


def _rej_mix(D=8, off=None, null=None):
    def call(L, A, S):
        p = dict(k=A.buf(16), mu=A.buf(64), noise=A.buf(64), out=A.buf(64, out=True))
        keep = A.buf(1, out=True)                                    # (an output to hold even where `out` is the NULL one)
        if off:
            p[off] = _off(p[off], 4)
        if null:
            p[null] = None
        return L.ggan_mix_mean(p['k'], p['mu'], p['noise'], p['out'], 4, 4, D, S) + 0 * bool(keep)
    return call


def _rej_post(K=4, B=2, row0=0, null=None):
    def call(L, A, S):
        p = dict(z=A.buf(16), mu=A.buf(64), probs=A.buf(64, out=True), assign=A.buf(64, out=True), colbest=A.buf(64, out=True))
        if null:
            p[null] = None
        return L.ggan_gmm_posterior_assign(p['z'], p['mu'], 0.0, B, K, 2, row0, p['probs'], p['assign'], p['colbest'], S)
    return call


def _rej_acc(N=4, K=4, null=None):
    def call(L, A, S):
        p = dict(assign=A.buf(16), labels=A.buf(16), colbest=A.buf(16), correct=A.buf(2, out=True))
        keep = A.buf(1, out=True)
        if null:
            p[null] = None
        return L.ggan_cluster_accuracy(p['assign'], p['labels'], p['colbest'], N, K, p['correct'], S) + 0 * bool(keep)
    return call


def _item(id_, fn, call):
    return dict(id=id_, fn=fn, call=call)


_NF, _FW, _BW, _SF, _SB = 'ggan_noise_fill', 'ggan_gmm_latent_fwd', 'ggan_gmm_latent_bwd', 'ggan_gmm_latent_st_fwd', 'ggan_gmm_latent_st_bwd'
REJECTED = [
    _item('noise-count0', _NF, _rej_noise(count=0)), _item('noise-count17', _NF, _rej_noise(count=NOISE_MAX + 1)),
    _item('noise-size0', _NF, _rej_noise(size=0)), _item('noise-size7fffffff', _NF, _rej_noise(size=0x7FFFFFFF)),
    _item('noise-kind-1', _NF, _rej_noise(kind=-1)), _item('noise-kind3', _NF, _rej_noise(kind=3)),
    _item('noise-width0', _NF, _rej_noise(kind=ONEHOT, width=0)), _item('noise-width-does-not-divide', _NF, _rej_noise(kind=ONEHOT, size=8, width=3)),
]
REJECTED += [_item('noise-null-%s' % n, _NF, _rej_noise(null=n)) for n in ('dsts', 'sizes', 'kinds', 'a', 'b', 'widths', 'state', 'dst')]
for _fn, _short, _m in ((_FW, 'fwd', None), (_SF, 'stc_fwd', MODE_STC), (_SF, 'st_fwd', MODE_ST)):
    REJECTED += [_item('%s-null-%s' % (_short, n), _fn, _rej_latent(_fn, mode=_m, null=(n,))) for n in ('z', 'mu', 'k')]
    REJECTED += [_item('%s-K257' % _short, _fn, _rej_latent(_fn, K=GMM_MAX_K + 1, mode=_m)), _item('%s-D0' % _short, _fn, _rej_latent(_fn, D=0, mode=_m)),
                 _item('%s-B0' % _short, _fn, _rej_latent(_fn, B=0, mode=_m))]
    if _m != MODE_ST:
        REJECTED += [_item('%s-temp0' % _short, _fn, _rej_latent(_fn, temp=0.0, mode=_m)), _item('%s-temp-1' % _short, _fn, _rej_latent(_fn, temp=-1.0, mode=_m)),
                     _item('%s-null-u' % _short, _fn, _rej_latent(_fn, mode=_m, null=('u',)))]
REJECTED += [_item('stc_fwd-null-soft', _SF, _rej_latent(_SF, mode=MODE_STC, null=('soft',))),
             _item('st_fwd-mode0', _SF, _rej_latent(_SF, mode=0)), _item('st_fwd-mode3', _SF, _rej_latent(_SF, mode=3)),
             _item('st_bwd-mode0', _SB, _rej_latent(_SB, mode=0)), _item('st_bwd-mode3', _SB, _rej_latent(_SB, mode=3)),
             _item('stc_bwd-null-soft', _SB, _rej_latent(_SB, mode=MODE_STC, null=('kk',))), _item('bwd-null-k', _BW, _rej_latent(_BW, null=('kk',)))]
for _fn, _short, _m in ((_BW, 'bwd', None), (_SB, 'stc_bwd', MODE_STC), (_SB, 'st_bwd', MODE_ST)):
    REJECTED += [_item('%s-null-%s' % (_short, n), _fn, _rej_latent(_fn, mode=_m, null=(n,))) for n in ('z', 'mu')]
    REJECTED += [_item('%s-both-gradients-null' % _short, _fn, _rej_latent(_fn, mode=_m, null=('gl', 'gk'))),
                 _item('%s-both-outputs-null' % _short, _fn, _rej_latent(_fn, mode=_m, null=('dz', 'dmu'))),
                 _item('%s-K257' % _short, _fn, _rej_latent(_fn, K=GMM_MAX_K + 1, mode=_m)), _item('%s-B257' % _short, _fn, _rej_latent(_fn, B=GMM_MAX_K + 1, mode=_m)),
                 _item('%s-D0' % _short, _fn, _rej_latent(_fn, D=0, mode=_m))]
    if _m != MODE_ST:
        REJECTED += [_item('%s-temp0' % _short, _fn, _rej_latent(_fn, temp=0.0, mode=_m)), _item('%s-temp-1' % _short, _fn, _rej_latent(_fn, temp=-1.0, mode=_m))]
REJECTED += [_item('mix-D6', 'ggan_mix_mean', _rej_mix(D=6))]
REJECTED += [_item('mix-%s-4-bytes-off' % n, 'ggan_mix_mean', _rej_mix(off=n)) for n in ('mu', 'noise', 'out')]
REJECTED += [_item('mix-null-%s' % n, 'ggan_mix_mean', _rej_mix(null=n)) for n in ('k', 'mu', 'noise', 'out')]
REJECTED += [_item('post-K8193', 'ggan_gmm_posterior_assign', _rej_post(K=POSTERIOR_MAX_K + 1)), _item('post-row0-1', 'ggan_gmm_posterior_assign', _rej_post(row0=-1)),
             _item('post-row0+B-past-2^31-1', 'ggan_gmm_posterior_assign', _rej_post(row0=0x7FFFFFFF - 1, B=2))]
REJECTED += [_item('post-null-%s' % n, 'ggan_gmm_posterior_assign', _rej_post(null=n)) for n in ('z', 'mu', 'assign', 'colbest')]
REJECTED += [_item('acc-N0', 'ggan_cluster_accuracy', _rej_acc(N=0)), _item('acc-K8193', 'ggan_cluster_accuracy', _rej_acc(K=POSTERIOR_MAX_K + 1))]
REJECTED += [_item('acc-null-%s' % n, 'ggan_cluster_accuracy', _rej_acc(null=n)) for n in ('assign', 'labels', 'colbest', 'correct')]
