"""row glue of the objectives: joins / splits / fan-out of row blocks, mixture and reparameterisation ops, the wali-gp interpolates."""
import collections
import ctypes as C
import math
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from .. import _lib
from .._lib import ACT_NONE, POSTERIOR_MAX_K, check  # noqa: F401
from ._core import _L, _p, _stream, _dev, _c, _DATA_ONLY, _is_param, _skip_undefined, _new_out, _adjacent  # noqa: F401
from .linear import Gemm  # noqa: F401


class JoinRows(Function):
    """cat([a, b], 0) for the critic evaluated once on [fake; real].  When the two operands already sit back to back in one
    buffer (their producers were handed RowSlots) the result is an alias of that memory: no copy kernel; the backward hands
    out the two row ranges of the incoming gradient (views)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.n = a.shape[0]
        if _adjacent(a, b):
            out = torch.empty(0, dtype=a.dtype, device=a.device)
            out.set_(a.untyped_storage(), a.storage_offset(), (a.shape[0] + b.shape[0],) + tuple(a.shape[1:]), a.stride())
            return out
        return torch.cat([a, b], 0)

    @staticmethod
    def backward(ctx, g):
        return g[:ctx.n], g[ctx.n:]


class Fanout(Function):
    """n aliases of a tensor that several branches of a step read (the mixture scripts: the code p_z feeds the Generator and the
    critics, q_z the mixture posterior and the critics, [p_z; q_z] both critics, the component means both hyper nets).  Their
    gradients are summed HERE, in alias order, by this library's pointwise launch (ggan_axpby through Axpby, differentiable) --
    not by at::add wherever autograd happens to meet the second contribution."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.set_materialize_grads(False)      # (an alias nobody differentiates contributes None, not a zero tensor + an addition launch)
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        gs = [g for g in gs if g is not None]
        if not gs:
            return None, None
        acc = gs[0]
        for g in gs[1:]:
            acc = Axpby.apply(acc, g, 1.0, 1.0, 0.0)
        return acc, None


def fanout(x, n=2):
    """n aliases of x whose gradients meet in one Fanout node (x itself n times where no gradient can flow)"""
    if not torch.is_tensor(x) or not x.is_cuda or not x.requires_grad or not torch.is_grad_enabled():
        return (x,) * n
    return Fanout.apply(x, n)


class SplitRows(Function):
    """(x[:n], x[n:]) for the critic evaluated once on [fake; real]; the backward is ONE concatenation instead of two
    zero-padded slice gradients and their sum."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.rows = n, x.shape[0]
        return x[:n], x[n:]

    @staticmethod
    def backward(ctx, ga, gb):
        if ga is None and gb is None:
            return None, None
        like = ga if ga is not None else gb
        if ga is None:
            ga = like.new_zeros((ctx.n,) + tuple(like.shape[1:]))
        if gb is None:
            gb = like.new_zeros((ctx.rows - ctx.n,) + tuple(like.shape[1:]))
        if (ga.is_contiguous() and gb.is_contiguous() and ga.dtype == gb.dtype
                and ga.untyped_storage().data_ptr() == gb.untyped_storage().data_ptr()
                and gb.storage_offset() == ga.storage_offset() + ga.numel()):
            # the two halves already sit back to back in one buffer (BceSum.backward): no copy
            return torch.as_strided(ga, (ctx.rows,) + tuple(ga.shape[1:]), ga.stride(), ga.storage_offset()), None
        return torch.cat([ga, gb], 0), None


@_skip_undefined
class CastScaleI32(Function):
    """real_x = mul*(float(x)/div - .5) + noise  (no gradient: the input is data)."""

    @staticmethod
    def forward(ctx, x_int, noise, div, mul, slot=None, ring=None):
        """ring: (int32 [R, ...] tensor of pre-staged minibatches, counter a, counter b, offset) -- the minibatch is slot
        (a + b + offset) mod R of the ring instead of x_int (ggan_cast_scale_ring_i32)"""
        _dev(x_int)
        assert x_int.dtype == torch.int32
        x_int = x_int.contiguous()
        y = _new_out(slot, x_int.shape, x_int.device)
        nz = _p(_c(noise)) if noise is not None else _p(None)
        if ring is not None:
            rt, ca, cb, off = ring
            assert rt.dtype == torch.int32 and rt.is_contiguous() and rt[0].numel() == x_int.numel()
            check(_L().ggan_cast_scale_ring_i32(_p(rt), rt.shape[0], _p(ca), _p(cb), int(off), nz, _p(y), x_int.numel(), div, mul,
                                                _stream()), 'ggan_cast_scale_ring_i32')
            return y
        check(_L().ggan_cast_scale_i32(_p(x_int), nz, _p(y), x_int.numel(), div, mul, _stream()), 'ggan_cast_scale_i32')
        return y

    @staticmethod
    def backward(ctx, g):
        return (None,) * len(ctx.needs_input_grad)


@_skip_undefined
class Axpby(Function):
    """out = a*x + b*y + c"""

    @staticmethod
    def forward(ctx, x, y, a, b, c, slot=None):
        x = _c(x)
        y = _c(y) if y is not None else None
        out = _new_out(slot, x.shape, x.device)
        check(_L().ggan_axpby(_p(x), _p(y), _p(out), x.numel(), a, b, c, _stream()), 'ggan_axpby')
        ctx.a, ctx.b, ctx.has_y = a, b, y is not None
        return out

    @staticmethod
    def backward(ctx, g):
        gx = Axpby.apply(g, None, ctx.a, 0.0, 0.0) if ctx.needs_input_grad[0] else None
        gy = Axpby.apply(g, None, ctx.b, 0.0, 0.0) if (ctx.has_y and ctx.needs_input_grad[1]) else None
        return (gx, gy) + (None,) * (len(ctx.needs_input_grad) - 2)


@_skip_undefined
class MixMean(Function):
    """p_z[B,D] = k[B,K] @ mu[K,D] + noise[B,D]: HyperGenerator of the gmgan scripts (gmgan_inference_cifar10.py:150-153) as ONE pointwise
    launch (ggan_mix_mean) instead of Gemm + Axpby at the head of the Generator chain; backward: d mu = k^T g (one product), d noise = g."""

    @staticmethod
    def usable(k, mu, noise):
        return k.dim() == 2 and mu.dim() == 2 and mu.shape[1] % 4 == 0 and k.is_cuda

    @staticmethod
    def forward(ctx, k, mu, noise, slot=None):
        k, mu, noise = _c(k), _c(mu), _c(noise)
        B, K = k.shape
        D = mu.shape[1]
        assert mu.shape[0] == K and tuple(noise.shape) == (B, D), (k.shape, mu.shape, noise.shape)
        out = _new_out(slot, (B, D), k.device)
        check(_L().ggan_mix_mean(_p(k), _p(mu), _p(noise), _p(out), B, K, D, _stream()), 'ggan_mix_mean')
        ctx.mu_param = _is_param(mu)
        ctx.save_for_backward(k, mu)
        return out

    @staticmethod
    def backward(ctx, g):
        k, mu = ctx.saved_tensors
        dk = dmu = None
        if ctx.needs_input_grad[1] and not (_DATA_ONLY[0] and ctx.mu_param):
            dmu = Gemm.apply(k, g, None, True, False, ACT_NONE, 0.0)          # k^T g
        if ctx.needs_input_grad[0]:
            dk = Gemm.apply(g, mu, None, False, True, ACT_NONE, 0.0)          # g mu^T
        return dk, dmu, (g if ctx.needs_input_grad[2] else None), None


class GmmLatent(Function):
    """HyperExtractor of the gmgan scripts in one launch per direction (ggan_gmm_latent_*): component logits of z under the
    mixture prior and the Gumbel-softmax relaxation of the component assignment.  Returns (logits, k)."""

    @staticmethod
    def forward(ctx, z, mu, gumbel_u, log_pi, temp, slot=None):
        z, mu, gumbel_u = _c(z), _c(mu), _c(gumbel_u)
        B, D = z.shape
        K = mu.shape[0]
        assert tuple(mu.shape) == (K, D) and tuple(gumbel_u.shape) == (B, K)
        logits = torch.empty((B, K), dtype=torch.float32, device=z.device)
        k = _new_out(slot, (B, K), z.device)
        check(_L().ggan_gmm_latent_fwd(_p(z), _p(mu), _p(gumbel_u), _p(logits), _p(k), B, K, D, float(log_pi), float(temp),
                                       _stream()), 'ggan_gmm_latent_fwd')
        ctx.temp = float(temp)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(z, mu, k)
        return logits, k

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_k):
        z, mu, k = ctx.saved_tensors
        n_in = len(ctx.needs_input_grad)
        if (g_logits is None and g_k is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * n_in
        B, D = z.shape
        K = mu.shape[0]
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        dmu = torch.empty_like(mu) if ctx.needs_input_grad[1] else None
        gl = _c(g_logits) if g_logits is not None else None
        gk = _c(g_k) if g_k is not None else None
        check(_L().ggan_gmm_latent_bwd(_p(z), _p(mu), _p(k), _p(gl), _p(gk), _p(dz), _p(dmu), B, K, D, ctx.temp, _stream()),
              'ggan_gmm_latent_bwd')
        return (dz, dmu) + (None,) * (n_in - 2)


class GmmLatentST(Function):
    """HyperExtractor under the straight-through MODE_K values (ggan_gmm_latent_st_*): mode = 'STRAIGHT_THROUGHT_CONCRETE' (the
    Gumbel-softmax s, its hard one-hot h in the forward value (h - s) + s, the gradient through s) or 'STRAIGHT_THROUGHT' (h = one-hot of
    the logits' argmax, value (h - logits) + logits, the gradient to the logits unchanged; gumbel_u None, temp unused).  Returns (logits, k)."""

    @staticmethod
    def forward(ctx, z, mu, gumbel_u, log_pi, temp, mode, slot=None):
        m = _lib.MODE_K[mode]
        assert m in (1, 2), mode
        z, mu = _c(z), _c(mu)
        B, D = z.shape
        K = mu.shape[0]
        assert tuple(mu.shape) == (K, D)
        st = m == 2
        if st:
            assert gumbel_u is None, 'STRAIGHT_THROUGHT draws no Gumbel noise'
            soft = None
        else:
            gumbel_u = _c(gumbel_u)
            assert tuple(gumbel_u.shape) == (B, K)
            soft = torch.empty((B, K), dtype=torch.float32, device=z.device)      # s: what the backward differentiates
        logits = torch.empty((B, K), dtype=torch.float32, device=z.device)
        k = _new_out(slot, (B, K), z.device)
        check(_L().ggan_gmm_latent_st_fwd(_p(z), _p(mu), _p(gumbel_u), _p(logits), _p(k), _p(soft), B, K, D, float(log_pi),
                                          float(temp), m, _stream()), 'ggan_gmm_latent_st_fwd')
        ctx.temp, ctx.mode = float(temp), m
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(z, mu, *([] if st else [soft]))
        return logits, k

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_k):
        z, mu = ctx.saved_tensors[:2]
        soft = ctx.saved_tensors[2] if ctx.mode == 1 else None
        n_in = len(ctx.needs_input_grad)
        if (g_logits is None and g_k is None) or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return (None,) * n_in
        B, D = z.shape
        K = mu.shape[0]
        dz = torch.empty_like(z) if ctx.needs_input_grad[0] else None
        dmu = torch.empty_like(mu) if ctx.needs_input_grad[1] else None
        gl = _c(g_logits) if g_logits is not None else None
        gk = _c(g_k) if g_k is not None else None
        check(_L().ggan_gmm_latent_st_bwd(_p(z), _p(mu), _p(soft), _p(gl), _p(gk), _p(dz), _p(dmu), B, K, D, ctx.temp, ctx.mode,
                                          _stream()), 'ggan_gmm_latent_st_bwd')
        return (dz, dmu) + (None,) * (n_in - 2)


def _mmd2_forward(ctx, name, x, y, sigmas, wts):
    x, y = _c(x), _c(y)
    m, d = x.shape
    n = y.shape[0]
    assert y.shape[1] == d
    ns = len(sigmas)
    sg = (C.c_float * ns)(*[float(v) for v in sigmas])
    wt = (C.c_float * ns)(*[float(v) for v in wts]) if wts is not None else None
    out = torch.empty((), dtype=torch.float32, device=x.device)
    scratch = torch.empty((m + n,), dtype=torch.float32, device=x.device)
    check(getattr(_L(), name)(_p(x), _p(y), m, n, d, sg, wt, ns, _p(out), _p(scratch), _stream()), name)
    ctx.sg, ctx.wt, ctx.ns = sg, wt, ns
    ctx.save_for_backward(x, y)
    return out


def _mmd2_backward(ctx, name, g):
    x, y = ctx.saved_tensors
    m, d = x.shape
    n = y.shape[0]
    dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
    dy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
    if dx is None and dy is None:
        return None, None, None, None
    check(getattr(_L(), name)(_p(x), _p(y), m, n, d, ctx.sg, ctx.wt, ctx.ns, _p(_c(g)), _p(dx), _p(dy), _stream()), name)
    return dx, dy, None, None


class MixRbfMmd2(Function):
    """biased MMD^2 between two sets of codes under a mixture of RBF kernels (tflib/objs/mmd.py:65-67) -> 0-dim tensor"""

    @staticmethod
    def forward(ctx, x, y, sigmas, wts):
        return _mmd2_forward(ctx, 'ggan_mix_rbf_mmd2_fwd', x, y, sigmas, wts)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _mmd2_backward(ctx, 'ggan_mix_rbf_mmd2_bwd', g)


class MixRbfMmd2Unbiased(Function):
    """the unbiased estimator (tflib/objs/mmd.py:53-61): same-set diagonals left out, means over m (m - 1) and n (n - 1) pairs; m, n >= 2"""

    @staticmethod
    def forward(ctx, x, y, sigmas, wts):
        return _mmd2_forward(ctx, 'ggan_mix_rbf_mmd2_unbiased_fwd', x, y, sigmas, wts)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _mmd2_backward(ctx, 'ggan_mix_rbf_mmd2_unbiased_bwd', g)


MMD_FUSED_MAX_ROWS = 512      # include/ggan.h: ggan_mix_rbf_mmd2_* take m + n <= 512


def mix_rbf_sums(x, y, sigmas, wts=None):
    """the three pairwise kernel sums of two row sets x [m, d], y [n, d] (ggan_mix_rbf_sums; x and y may be the same tensor) -> float64 device
    tensor [S_xx, S_yy, S_xy], the same-set sums over ordered pairs i != j.  Forward only: inputs that require grad are refused."""
    _no_grad('mix_rbf_sums', [x, y], ' (the differentiable op takes m + n <= %d rows)' % MMD_FUSED_MAX_ROWS)
    x, y = _row_shapes('mix_rbf_sums', [_c(x), _c(y)])
    (m, d), n = x.shape, y.shape[0]
    ns = len(sigmas)
    sg = (C.c_float * ns)(*[float(v) for v in sigmas])
    wt = (C.c_float * ns)(*[float(v) for v in wts]) if wts is not None else None
    ws, nbytes = _workspace(_L().ggan_mix_rbf_sums_workspace(m, n), x.device)
    out = torch.empty((3,), dtype=torch.float64, device=x.device)
    check(_L().ggan_mix_rbf_sums(_p(x), _p(y), m, n, d, sg, wt, ns, _p(out), _p(ws), nbytes, _stream()), 'ggan_mix_rbf_sums')
    return out


def mmd2_from_sums(sums3, m, n, wt_sum, biased):
    """either estimator from [S_xx, S_yy, S_xy] (float64 tensor or array): the reference's diagonal is the constant sum(wts), mmd.py:52-67"""
    sxx, syy, sxy = sums3[0], sums3[1], sums3[2]
    if biased:
        return (sxx + m * wt_sum) / (float(m) * m) + (syy + n * wt_sum) / (float(n) * n) - 2.0 * sxy / (float(m) * n)
    return sxx / (float(m) * (m - 1)) + syy / (float(n) * (n - 1)) - 2.0 * sxy / (float(m) * n)


PRDC_MAX_K = 8                # include/ggan.h: ggan_knn_radii keeps 1 <= k <= 8 neighbours per row


def _workspace(nbytes, device):
    """(an op's scratch buffer, the size to tell the op): what its *_workspace entry asks for (0: shapes the entry itself refuses)"""
    nbytes = int(nbytes)
    return torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=device), nbytes


def _row_shapes(name, sets):
    """[rows, d] sets of one width (ValueError otherwise) -> the sets"""
    if any(t.dim() != 2 for t in sets) or len(set(t.shape[1] for t in sets)) != 1:
        raise ValueError('%s: [rows, d] sets of one width expected, got %s' % (name, ', '.join(str(tuple(t.shape)) for t in sets)))
    return sets


def _no_grad(name, sets, hint=''):
    """the set-level ops are forward only: inputs that require grad are refused"""
    if torch.is_grad_enabled() and any(t.requires_grad for t in sets):
        raise _lib.GganError('%s has no backward: detach the inputs%s' % (name, hint))


def _row_sets(name, sets, k=None, radii=None):
    """the checks the k-NN ball ops share, in this order: [rows, d] sets of one width, 1 <= k <= min(8, fewest rows - 1), one radius per row of
    the last set (ValueError, before anything else); no gradient; fp32 on the device -> the sets, contiguous"""
    _row_shapes(name, sets)
    rows = min(t.shape[0] for t in sets)
    if k is not None and (not 1 <= int(k) <= PRDC_MAX_K or int(k) > rows - 1):
        raise ValueError('%s: 1 <= k <= min(%d, rows - 1) expected, got k = %s with %d rows' % (name, PRDC_MAX_K, k, rows))
    if radii is not None and (radii.dim() != 1 or radii.shape[0] != sets[-1].shape[0]):
        raise ValueError('%s: one radius per row of the second set expected, got %s for %d rows' % (name, tuple(radii.shape), sets[-1].shape[0]))
    _no_grad(name, sets)
    return [_c(t) for t in sets]


def knn_radii(z, k):
    """squared distance from every row of z [n, d] to its k-th nearest OTHER row (ggan_knn_radii: self left out by index, duplicates
    count) -> float32 [n] device tensor.  Forward only."""
    (z,), k = _row_sets('knn_radii', [z], k=k), int(k)
    n, d = z.shape
    ws, nbytes = _workspace(_L().ggan_knn_radii_workspace(n, k), z.device)
    r2 = torch.empty((n,), dtype=torch.float32, device=z.device)
    check(_L().ggan_knn_radii(_p(z), n, d, k, _p(r2), _p(ws), nbytes, _stream()), 'ggan_knn_radii')
    return r2


def ball_counts(a, b, r2_b):
    """per row of a [m, d]: in how many of b's balls it lies (squared radii r2_b [n], inclusive) and its squared distance to the nearest
    row of b (ggan_ball_counts) -> (int32 [m], float32 [m]) device tensors.  Forward only."""
    (a, b), r2_b = _row_sets('ball_counts', [a, b], radii=r2_b), _c(r2_b)
    (m, d), n = a.shape, b.shape[0]
    ws, nbytes = _workspace(_L().ggan_ball_counts_workspace(m, n), a.device)
    cnt = torch.empty((m,), dtype=torch.int32, device=a.device)
    mn = torch.empty((m,), dtype=torch.float32, device=a.device)
    check(_L().ggan_ball_counts(_p(a), _p(b), m, n, d, _p(r2_b), _p(cnt), _p(mn), _p(ws), nbytes, _stream()), 'ggan_ball_counts')
    return cnt, mn


def prdc(x, y, k=5):
    """(precision, recall, density, coverage) of the generated set y [n, d] against the real set x [m, d] from k-NN balls (Kynkaanniemi
    et al. 2019; Naeem et al. 2020; include/ggan.h) -> float64 [4] device tensor, formed on the device: the caller takes the one host
    synchronisation.  Forward only."""
    (x, y), k = _row_sets('prdc', [x, y], k=k), int(k)
    m, n = x.shape[0], y.shape[0]
    r_x, r_y = knn_radii(x, k), knn_radii(y, k)
    cnt_y, _ = ball_counts(y, x, r_x)                    # generated rows in real balls
    cnt_x, mn_x = ball_counts(x, y, r_y)                 # real rows in generated balls, and their nearest generated row
    f8 = torch.float64
    sums = torch.stack([(cnt_y > 0).sum(dtype=f8), (cnt_x > 0).sum(dtype=f8), cnt_y.sum(dtype=f8), (mn_x <= r_x).sum(dtype=f8)])
    # (a quotient of two tensors is a true division -- by a Python number torch multiplies by its rounded reciprocal --; the denominators
    #  are filled on the device: a tensor made from host numbers would be an upload the host waits for)
    den = lambda v: torch.full((), float(v), dtype=f8, device=x.device)
    return sums / torch.stack([den(n), den(m), den(k * n), den(m)])


KNN_MAX_K = 8                 # include/ggan.h: GGAN_KNN_MAX_K neighbours per list
KNN_MAX_CLASSES = 1024        # ... and the widest confusion matrix of ggan_knn_vote


def knn_lists(q, c, k, skip_diag=False, return_d2=False):
    """per row of q [m, d]: the indices of its k nearest rows of c [n, d], ascending in the total order (squared distance, index) -- a tie
    in distance goes to the lower index (ggan_knn_lists) -> int32 [m, k] device tensor, with return_d2 also the float32 [m, k] squared
    distances.  skip_diag (m == n): candidate i is left out for query i, by index.  Forward only."""
    name = 'knn_lists'
    _row_shapes(name, [q, c])
    (m, d), n, k, skip = q.shape, c.shape[0], int(k), bool(skip_diag)
    if skip and m != n:
        raise ValueError('%s: skip_diag needs as many candidates as queries, got %d and %d' % (name, n, m))
    if not 1 <= k <= KNN_MAX_K or k > n - (1 if skip else 0):
        raise ValueError('%s: 1 <= k <= min(%d, candidates%s) expected, got k = %s with %d candidates'
                         % (name, KNN_MAX_K, ' - 1' if skip else '', k, n))
    _no_grad(name, [q, c])
    q, c = _c(q), _c(c)
    ws, nbytes = _workspace(_L().ggan_knn_lists_workspace(m, n, k), q.device)
    idx = torch.empty((m, k), dtype=torch.int32, device=q.device)
    d2 = torch.empty((m, k), dtype=torch.float32, device=q.device) if return_d2 else None
    check(_L().ggan_knn_lists(_p(q), _p(c), m, n, d, k, 1 if skip else 0, _p(idx), _p(d2), _p(ws), nbytes, _stream()), 'ggan_knn_lists')
    return (idx, d2) if return_d2 else idx


def _labels(name, what, t, rows, device):
    if t.dim() != 1 or t.dtype != torch.int32 or (rows is not None and t.shape[0] != rows) or t.device != device:
        raise ValueError('%s: %s must be int32 [%s] on %s, got %s %s on %s'
                         % (name, what, 'rows' if rows is None else rows, device, t.dtype, tuple(t.shape), t.device))
    return t.contiguous()


def knn_vote(idx, labels_c, labels_q=None, classes=None):
    """the k-NN vote of neighbour lists idx [m, k] (int32, rows of the candidate set) over the candidates' labels_c (int32): pred[i] = the
    most frequent label of the list, the smallest one on a tied vote (ggan_knn_vote) -> pred int32 [m]; with labels_q (int32 [m]) also
    correct = #{pred == labels_q} (int32 [1]): (pred, correct); with classes (<= 1024) too the confusion matrix int32 [classes, classes],
    rows the queries' labels: (pred, correct, confusion).  Every index must be a row of labels_c.  Device tensors; forward only."""
    name = 'knn_vote'
    if idx.dim() != 2 or idx.dtype != torch.int32 or not 1 <= idx.shape[1] <= KNN_MAX_K or idx.shape[0] < 1:
        raise ValueError('%s: int32 lists [m, 1 <= k <= %d] expected, got %s %s' % (name, KNN_MAX_K, idx.dtype, tuple(idx.shape)))
    if idx.device.type != 'cuda':
        raise _lib.GganError('%s has no CPU path' % name)
    (m, k), dev = idx.shape, idx.device
    idx, labels_c = idx.contiguous(), _labels(name, 'labels_c', labels_c, None, dev)
    if classes is not None and labels_q is None:
        raise ValueError('%s: a confusion matrix needs labels_q' % name)
    if classes is not None and not 1 <= int(classes) <= KNN_MAX_CLASSES:
        raise ValueError('%s: 1 <= classes <= %d expected, got %s' % (name, KNN_MAX_CLASSES, classes))
    pred = torch.empty((m,), dtype=torch.int32, device=dev)
    correct = confusion = None
    if labels_q is not None:
        labels_q = _labels(name, 'labels_q', labels_q, m, dev)
        correct = torch.zeros((1,), dtype=torch.int32, device=dev)
        if classes is not None:
            confusion = torch.zeros((int(classes), int(classes)), dtype=torch.int32, device=dev)
    check(_L().ggan_knn_vote(_p(idx), _p(labels_c), _p(labels_q), m, k, int(classes or 0), _p(pred), _p(correct), _p(confusion), _stream()),
          'ggan_knn_vote')
    if labels_q is None:
        return pred
    return (pred, correct) if confusion is None else (pred, correct, confusion)


def knn_accuracy(z, y, k, classes=None, return_pred=False):
    """leave-one-out k-NN accuracy of the labelled set (z [n, d], y int32 [n]): every row is classified by the vote of its k nearest OTHER
    rows (knn_lists with skip_diag, knn_vote) -> float64 [1] device tensor, formed on the device: the caller takes the host
    synchronisation.  classes only checks the bound of the vote's optional outputs.  return_pred: (accuracy, pred int32 [n])."""
    if classes is not None and not 1 <= int(classes) <= KNN_MAX_CLASSES:
        raise ValueError('knn_accuracy: 1 <= classes <= %d expected, got %s' % (KNN_MAX_CLASSES, classes))
    idx = knn_lists(z, z, k, skip_diag=True)
    pred, correct = knn_vote(idx, y, y)
    acc = correct.double() / torch.full((1,), float(z.shape[0]), dtype=torch.float64, device=z.device)
    return (acc, pred) if return_pred else acc


PARZEN_MAX_SIGMAS = 16        # include/ggan.h: GGAN_PARZEN_MAX_SIGMAS bandwidths per call


def _sigmas(name, sigmas):
    """the bandwidths as a list of 1 .. 16 finite positive floats (ValueError otherwise)"""
    try:
        sig = [float(v) for v in sigmas]
    except TypeError:                  # one number
        sig = [float(sigmas)]
    if not 1 <= len(sig) <= PARZEN_MAX_SIGMAS:
        raise ValueError('%s: 1 <= ns <= %d bandwidths expected, got %d' % (name, PARZEN_MAX_SIGMAS, len(sig)))
    if any(not (math.isfinite(v) and v > 0.0) for v in sig):
        raise ValueError('%s: every sigma must be finite and positive, got %s' % (name, sig))
    return sig


def parzen_lse(q, s, sigmas):
    """lse[g, i] = log sum_j exp(-D(q_i, s_j) / (2 sigmas[g]^2)) over the rows of s [n, d], per row of q [m, d] and per bandwidth (at most
    16 host numbers), D the squared distance of knn_lists; the sums are carried shifted by the row's minimum distance, so the result is
    finite where a plain sum of kernel values is log 0 (ggan_parzen_lse) -> float32 [ns, m] device tensor.  Forward only."""
    _row_shapes('parzen_lse', [q, s])
    sig = _sigmas('parzen_lse', sigmas)
    _no_grad('parzen_lse', [q, s])
    q, s = _c(q), _c(s)
    (m, d), n, ns = q.shape, s.shape[0], len(sig)
    ws, nbytes = _workspace(_L().ggan_parzen_lse_workspace(m, n, ns), q.device)
    lse = torch.empty((ns, m), dtype=torch.float32, device=q.device)
    host = (C.c_float * ns)(*sig)
    check(_L().ggan_parzen_lse(_p(q), _p(s), m, n, d, C.cast(host, C.c_void_p), ns, _p(lse), _p(ws), nbytes, _stream()), 'ggan_parzen_lse')
    return lse


def parzen_ll(q, s, sigmas, scale=1.0):
    """the Gaussian Parzen-window log-likelihood of every row of q under the kernel density of the rows of s, per bandwidth, in the
    UNIT-INTERVAL pixel scale: ll[g, i] = parzen_lse(q, s, scale * sigmas)[g, i] - log n - (d / 2) log(2 pi sigmas[g]^2).  The rows are
    handed in as the nets see them; scale is the width of their pixel range (1 for sigmoid outputs, 2 for tanh outputs): the bandwidth
    times scale in the nets' units, normalised with the unscaled one, is exactly the density of the data mapped to [0, 1]
    -> float64 [ns, m] device tensor, formed on the device: the caller takes the host synchronisation.  Forward only."""
    sig, scale = _sigmas('parzen_ll', sigmas), float(scale)
    if not (math.isfinite(scale) and scale > 0.0):
        raise ValueError('parzen_ll: scale must be finite and positive, got %s' % scale)
    lse = parzen_lse(q, s, [scale * v for v in sig])
    n, d = s.shape
    # (the constants are filled on the device, one launch per bandwidth: a tensor made from host numbers would be an upload the host waits for)
    const = torch.empty((len(sig), 1), dtype=torch.float64, device=lse.device)
    for g, v in enumerate(sig):
        const[g].fill_(math.log(n) + 0.5 * d * math.log(2.0 * math.pi * v * v))
    return lse.double() - const


SSIM_MAX_ROWS, SSIM_MAX_C, SSIM_MIN_SIDE, SSIM_MAX_SIDE = 131072, 4, 11, 64        # include/ggan.h: the ranges ggan_ssim_pairs accepts


def _unit_map(name, m):
    """a unit-scale map as two finite floats (scale, shift) (ValueError otherwise)"""
    try:
        scale, shift = (float(v) for v in m)
    except (TypeError, ValueError):
        raise ValueError('%s: a map is a (scale, shift) pair, got %r' % (name, m))
    if not (math.isfinite(scale) and math.isfinite(shift)):
        raise ValueError('%s: a map must be finite, got %r' % (name, m))
    return scale, shift


def ssim_pairs(a, b, shape, map_a=(1., 0.), map_b=None):
    """per-image reconstruction fidelity of rows a[i] against b[i] (ggan_ssim_pairs): a, b [n, C*H*W] fp32 device rows of channel-major
    planes (or [B, LEN, C*H*W]: n = B*LEN frames), shape = (C, H, W), C in 1..4 and 11 <= H, W <= 64.  The pixel of an input in unit scale
    is scale * x + shift with (scale, shift) = map_a for a and map_b (default: map_a) for b -- (0.5, 0.5) for the tanh range, (1, 0) for the
    sigmoid range, (1/255, 0) for data in 0..255.  -> (mse [n], ssim [n]) float32 device tensors: the mean squared error, and the mean
    structural similarity under the 11x11 Gaussian window of sigma 1.5 (Wang et al. 2004; data range 1).  a is b is allowed.  Forward only."""
    name = 'ssim_pairs'
    try:
        c, h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError('%s: shape = (C, H, W) expected, got %r' % (name, shape))
    if not (1 <= c <= SSIM_MAX_C and SSIM_MIN_SIDE <= h <= SSIM_MAX_SIDE and SSIM_MIN_SIDE <= w <= SSIM_MAX_SIDE):
        raise ValueError('%s: 1 <= C <= %d and %d <= H, W <= %d expected, got %r' % (name, SSIM_MAX_C, SSIM_MIN_SIDE, SSIM_MAX_SIDE, (c, h, w)))
    if a.shape != b.shape or a.dim() < 2 or a.shape[-1] != c * h * w:
        raise ValueError('%s: two sets of rows [n, %d] expected, got %s, %s' % (name, c * h * w, tuple(a.shape), tuple(b.shape)))
    n = a.numel() // (c * h * w)
    if not 1 <= n <= SSIM_MAX_ROWS:
        raise ValueError('%s: 1 <= n <= %d images expected, got %d' % (name, SSIM_MAX_ROWS, n))
    (sa, ha), (sb, hb) = _unit_map(name, map_a), _unit_map(name, map_a if map_b is None else map_b)
    if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad):
        raise _lib.GganError('%s has no backward: detach the inputs' % name)
    same = a is b
    a = _c(a)
    b = a if same else _c(b)
    ws, nbytes = _workspace(_L().ggan_ssim_pairs_workspace(n, c, h, w), a.device)
    mse = torch.empty((n,), dtype=torch.float32, device=a.device)
    ssim = torch.empty((n,), dtype=torch.float32, device=a.device)
    check(_L().ggan_ssim_pairs(_p(a), _p(b), n, c, h, w, sa, ha, sb, hb, _p(mse), _p(ssim), _p(ws), nbytes, _stream()), 'ggan_ssim_pairs')
    return mse, ssim


def psnr_from_mse(mse):
    """-10 log10(max(mse, 1e-10)) per element of a tensor of unit-range mean squared errors, in dB: a perfect image scores 100 dB and not
    inf, which would poison a mean -> float64 tensor on the same device (plain torch arithmetic on n numbers: the caller keeps the one host
    synchronisation)"""
    return -10.0 * torch.log10(torch.clamp(mse.double(), min=1e-10))


PROBE_MAX_DIM, PROBE_MAX_CLASSES, PROBE_MAX_ROWS, PROBE_ROW_BLOCK = 128, 32, 131072, 256   # include/ggan.h: GGAN_PROBE_MAX_DIM / _MAX_CLASSES, the row range, GGAN_PROBE_ROW_BLOCK
PROBE_BAD_LABEL, PROBE_NONFINITE, PROBE_BAD_PIVOT = 1, 2, 4                                # ... and the bits of the status word

ProbeFit = collections.namedtuple('ProbeFit', 'mean inv_std W bias counts status')
ProbeFit.__doc__ = """a fitted least-squares probe, device tensors: mean, inv_std float32 [d] (inv_std 0 for a constant column), W float32 [d, classes], bias
float32 [classes] (the class frequencies), counts int32 [classes], status int32 [1] (0, or PROBE_BAD_LABEL | PROBE_NONFINITE | PROBE_BAD_PIVOT;
W is NaN where the solve failed)"""


def _probe_rows(name, z, y, d=None, least=1):
    """float32 rows [rows, d <= PROBE_MAX_DIM] and (or None) int32 labels [rows] on the rows' device (ValueError otherwise) -> (z, y) contiguous"""
    if z.dim() != 2 or z.dtype != torch.float32 or z.shape[0] > PROBE_MAX_ROWS:
        raise ValueError('%s: float32 rows [rows <= %d, d] expected, got %s %s' % (name, PROBE_MAX_ROWS, z.dtype, tuple(z.shape)))
    if z.shape[0] < least:
        raise ValueError('%s: at least %d rows expected, got %d' % (name, least, z.shape[0]))
    if not 1 <= z.shape[1] <= PROBE_MAX_DIM or (d is not None and z.shape[1] != d):
        raise ValueError('%s: %s columns expected, got %d' % (name, '1 <= d <= %d' % PROBE_MAX_DIM if d is None else d, z.shape[1]))
    if y is not None:
        y = _labels(name, 'y', y, z.shape[0], z.device)
    _no_grad(name, [z])
    return _c(z), y


def lsq_probe_fit(z, y, classes, ridge):
    """the ridge-regularised least-squares classifier of the labelled rows (z float32 [n, d], y int32 [n] in [0, classes)) on standardised
    columns, in closed form (ggan_probe_moments / _normal / _solve): with zs = (z - mean) * inv_std, G = zs^T zs / n and R[:, c] = (1/n) the sum of
    the zs rows of class c, W = (G + ridge I)^-1 R and the unpenalised intercept is the class frequencies -> ProbeFit.  d <= PROBE_MAX_DIM,
    classes <= PROBE_MAX_CLASSES, n >= 2, ridge > 0.  Nothing is read back: a label out of range, a non-finite moment or a failed
    factorisation is a bit of the record's status word.  Forward only."""
    name = 'lsq_probe_fit'
    classes, ridge = int(classes), float(ridge)
    if not 1 <= classes <= PROBE_MAX_CLASSES:
        raise ValueError('%s: 1 <= classes <= %d expected, got %d' % (name, PROBE_MAX_CLASSES, classes))
    if not (math.isfinite(ridge) and ridge > 0.0):
        raise ValueError('%s: ridge must be finite and positive, got %s' % (name, ridge))
    z, y = _probe_rows(name, z, y, least=2)
    n, d = z.shape
    dev = z.device
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
    fit = ProbeFit(new((d,)), new((d,)), new((d, classes)), new((classes,)), new((classes,), torch.int32), new((1,), torch.int32))
    G, R = new((d, d)), new((d, classes))
    L = _L()
    ws, nbytes = _workspace(max(L.ggan_probe_moments_workspace(n, d, classes), L.ggan_probe_normal_workspace(n, d, classes)), dev)
    check(L.ggan_probe_moments(_p(z), _p(y), n, d, classes, _p(fit.mean), _p(fit.inv_std), _p(fit.counts), _p(fit.status), _p(ws), nbytes,
                               _stream()), 'ggan_probe_moments')
    check(L.ggan_probe_normal(_p(z), _p(y), n, d, classes, _p(fit.mean), _p(fit.inv_std), _p(G), _p(R), _p(ws), nbytes, _stream()),
          'ggan_probe_normal')
    check(L.ggan_probe_solve(_p(G), _p(R), _p(fit.counts), n, d, classes, ridge, _p(fit.W), _p(fit.bias), _p(fit.status), _stream()),
          'ggan_probe_solve')
    return fit


def lsq_probe_predict(fit, z, y=None, return_pred=False):
    """a fitted probe on the rows z float32 [m, d] (ggan_probe_predict): the class of the largest score ((z - mean) * inv_std) W + bias, the
    lowest class on a tie.  With y (int32 [m]): correct int32 [1] = the number of rows that hit their label; with return_pred: (correct,
    pred int32 [m]); without y: pred.  Device tensors, nothing is read back.  Forward only."""
    name = 'lsq_probe_predict'
    d, classes = fit.W.shape
    z, y = _probe_rows(name, z, y, d)
    if any(t.device != z.device for t in fit):
        raise ValueError('%s: the fit lives on %s, the rows on %s' % (name, fit.W.device, z.device))
    m = z.shape[0]
    pred = torch.empty((m,), dtype=torch.int32, device=z.device) if (return_pred or y is None) else None
    correct = torch.empty((1,), dtype=torch.int32, device=z.device) if y is not None else None
    check(_L().ggan_probe_predict(_p(z), _p(y), m, d, classes, _p(fit.mean), _p(fit.inv_std), _p(fit.W), _p(fit.bias), _p(pred), _p(correct),
                                  _stream()), 'ggan_probe_predict')
    if y is None:
        return pred
    return (correct, pred) if return_pred else correct


WPROBE_MAX_DIM, WPROBE_TILE, WPROBE_PANEL, WPROBE_CHUNK = 4096, 64, 64, 128      # include/ggan.h: GGAN_WPROBE_MAX_DIM / _TILE / _PANEL / _CHUNK


def _wprobe_rows(name, z, y, d=None, least=1):
    """_probe_rows with the wide chain's column range, 1 <= d <= WPROBE_MAX_DIM"""
    if z.dim() != 2 or z.dtype != torch.float32 or z.shape[0] > PROBE_MAX_ROWS:
        raise ValueError('%s: float32 rows [rows <= %d, d] expected, got %s %s' % (name, PROBE_MAX_ROWS, z.dtype, tuple(z.shape)))
    if z.shape[0] < least:
        raise ValueError('%s: at least %d rows expected, got %d' % (name, least, z.shape[0]))
    if not 1 <= z.shape[1] <= WPROBE_MAX_DIM or (d is not None and z.shape[1] != d):
        raise ValueError('%s: %s columns expected, got %d' % (name, '1 <= d <= %d' % WPROBE_MAX_DIM if d is None else d, z.shape[1]))
    if y is not None:
        y = _labels(name, 'y', y, z.shape[0], z.device)
    _no_grad(name, [z])
    return _c(z), y


def lsq_probe_fit_wide(z, y, classes, ridge):
    """lsq_probe_fit for 1 <= d <= WPROBE_MAX_DIM columns (ggan_wprobe_moments / _normal / _factor / _solve): the same classifier and the
    same record, the normal equations and their Cholesky factor in float64 on the device (8 d (d + classes) bytes for the call: 134 MB at
    d = 4096).  Device float32 / int32 inputs, nothing is read back, a failure is a bit of the record's status word.  Forward only."""
    name = 'lsq_probe_fit_wide'
    classes, ridge = int(classes), float(ridge)
    if not 1 <= classes <= PROBE_MAX_CLASSES:
        raise ValueError('%s: 1 <= classes <= %d expected, got %d' % (name, PROBE_MAX_CLASSES, classes))
    if not (math.isfinite(ridge) and ridge > 0.0):
        raise ValueError('%s: ridge must be finite and positive, got %s' % (name, ridge))
    z, y = _wprobe_rows(name, z, y, least=2)
    n, d = z.shape
    dev = z.device
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
    fit = ProbeFit(new((d,)), new((d,)), new((d, classes)), new((classes,)), new((classes,), torch.int32), new((1,), torch.int32))
    G, R = new((d, d), torch.float64), new((d, classes), torch.float64)
    L = _L()
    ws, nbytes = _workspace(L.ggan_wprobe_moments_workspace(n, d, classes), dev)
    check(L.ggan_wprobe_moments(_p(z), _p(y), n, d, classes, _p(fit.mean), _p(fit.inv_std), _p(fit.counts), _p(fit.status), _p(ws), nbytes,
                                _stream()), 'ggan_wprobe_moments')
    check(L.ggan_wprobe_normal(_p(z), _p(y), n, d, classes, _p(fit.mean), _p(fit.inv_std), _p(G), _p(R), _stream()), 'ggan_wprobe_normal')
    check(L.ggan_wprobe_factor(_p(G), d, ridge, _p(fit.status), _stream()), 'ggan_wprobe_factor')
    check(L.ggan_wprobe_solve(_p(G), _p(R), _p(fit.counts), n, d, classes, _p(fit.W), _p(fit.bias), _p(fit.status), _stream()),
          'ggan_wprobe_solve')
    return fit


def lsq_probe_predict_wide(fit, z, y=None, return_pred=False):
    """lsq_probe_predict for a record of lsq_probe_fit_wide (ggan_wprobe_predict): the same arguments and results"""
    name = 'lsq_probe_predict_wide'
    d, classes = fit.W.shape
    z, y = _wprobe_rows(name, z, y, d)
    if any(t.device != z.device for t in fit):
        raise ValueError('%s: the fit lives on %s, the rows on %s' % (name, fit.W.device, z.device))
    m = z.shape[0]
    pred = torch.empty((m,), dtype=torch.int32, device=z.device) if (return_pred or y is None) else None
    correct = torch.empty((1,), dtype=torch.int32, device=z.device) if y is not None else None
    check(_L().ggan_wprobe_predict(_p(z), _p(y), m, d, classes, _p(fit.mean), _p(fit.inv_std), _p(fit.W), _p(fit.bias), _p(pred), _p(correct),
                                   _stream()), 'ggan_wprobe_predict')
    if y is None:
        return pred
    return (correct, pred) if return_pred else correct


FRECHET_MAX_DIM, FRECHET_MAX_ROWS = 128, 131072             # include/ggan.h: GGAN_FRECHET_MAX_DIM, the row range
FRECHET_NONFINITE, FRECHET_NOT_CONVERGED = 1, 2             # ... and the bits of the status word


def _frechet_rows(name, x):
    """float32 rows [2 <= rows <= FRECHET_MAX_ROWS, 1 <= d <= FRECHET_MAX_DIM] (ValueError otherwise), no gradient"""
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] > FRECHET_MAX_ROWS:
        raise ValueError('%s: float32 rows [rows <= %d, d] expected, got %s %s' % (name, FRECHET_MAX_ROWS, x.dtype, tuple(x.shape)))
    if x.shape[0] < 2:
        raise ValueError('%s: at least 2 rows expected, got %d' % (name, x.shape[0]))
    if not 1 <= x.shape[1] <= FRECHET_MAX_DIM:
        raise ValueError('%s: 1 <= d <= %d columns expected, got %d' % (name, FRECHET_MAX_DIM, x.shape[1]))
    _no_grad(name, [x])


def _frechet_moments(name, x):
    """(mean, cov, status) of checked rows, made contiguous on the device"""
    x = _c(x)
    n, d = x.shape
    mean = torch.empty((d,), dtype=torch.float64, device=x.device)
    cov = torch.empty((d, d), dtype=torch.float64, device=x.device)
    status = torch.empty((1,), dtype=torch.int32, device=x.device)
    ws, nbytes = _workspace(_L().ggan_frechet_moments_workspace(n, d), x.device)
    check(_L().ggan_frechet_moments(_p(x), n, d, _p(mean), _p(cov), _p(status), _p(ws), nbytes, _stream()), 'ggan_frechet_moments')
    return mean, cov, status


def frechet_moments(x):
    """(mean float64 [d], covariance float64 [d, d] over n - 1) of the rows x float32 [n, d] (ggan_frechet_moments): the mean from fp64 sums,
    the covariance from rows centred by that mean, a block of 256 rows summed in fp32, the blocks in fp64; kept in fp64.  2 <= n <= 131072,
    d <= FRECHET_MAX_DIM.  Device tensors, nothing is read back; a non-finite entry shows as a non-finite moment.  Forward only."""
    _frechet_rows('frechet_moments', x)
    mean, cov, _ = _frechet_moments('frechet_moments', x)
    return mean, cov


def frechet_distance(x, y):
    """the Frechet distance between Gaussians fitted to the row sets x [m, d] and y [n, d] (float32, one width d <= FRECHET_MAX_DIM, at least
    two rows each): |mu_x - mu_y|^2 + tr S_x + tr S_y - 2 tr (S_x S_y)^(1/2) (ggan_frechet_moments, ggan_frechet_distance: all fp64 behind
    the moments, singular covariances allowed) -> (values float64 [4] = [the distance, |dmu|^2, tr S_x + tr S_y, 2 tr (S_x S_y)^(1/2)],
    status int32 [1]: 0, or FRECHET_NONFINITE | FRECHET_NOT_CONVERGED).  The distance is not clipped at 0: two samples of one distribution
    may land a hair below.  Device tensors, no host synchronisation.  Forward only."""
    name = 'frechet_distance'
    _row_shapes(name, [x, y])
    _frechet_rows(name, x)
    _frechet_rows(name, y)
    m1, c1, s1 = _frechet_moments(name, x)
    m2, c2, s2 = _frechet_moments(name, y)
    d = x.shape[1]
    out = torch.empty((4,), dtype=torch.float64, device=m1.device)
    status = torch.empty((1,), dtype=torch.int32, device=m1.device)
    ws, nbytes = _workspace(_L().ggan_frechet_distance_workspace(d), m1.device)
    check(_L().ggan_frechet_distance(_p(m1), _p(c1), _p(m2), _p(c2), d, _p(out), _p(status), _p(ws), nbytes, _stream()), 'ggan_frechet_distance')
    return out, status | s1 | s2


SWD_MAX_ROWS, SWD_MAX_DIRS = 16384, 4096                   # include/ggan.h: GGAN_SWD_MAX_ROWS, GGAN_SWD_MAX_DIRS
SWD_NONFINITE = 1                                           # ... and the status word


def _swd_rows(name, x, what='d'):
    """float32 rows [1 <= rows <= SWD_MAX_ROWS, 1 <= columns] (ValueError otherwise)"""
    if x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] > SWD_MAX_ROWS:
        raise ValueError('%s: float32 rows [rows <= %d, %s] expected, got %s %s' % (name, SWD_MAX_ROWS, what, x.dtype, tuple(x.shape)))
    if x.shape[0] < 1:
        raise ValueError('%s: at least 1 row expected, got %d' % (name, x.shape[0]))
    if x.shape[1] < 1:
        raise ValueError('%s: at least 1 column expected, got %d' % (name, x.shape[1]))


def _swd_p(name, p):
    if p not in (1, 2):
        raise ValueError('%s: p must be 1 or 2, got %s' % (name, p))
    return int(p)


def _swd_dirs(name, L):
    if not 1 <= L <= SWD_MAX_DIRS:
        raise ValueError('%s: 1 <= L <= %d directions expected, got %d' % (name, SWD_MAX_DIRS, L))


def sliced_wasserstein_projected(px, py, p=2):
    """the sliced Wasserstein distance of two row sets already projected onto L directions, px float32 [m, L] and py float32 [n, L] (one
    width 1 <= L <= SWD_MAX_DIRS, 1 <= m, n <= SWD_MAX_ROWS, p 1 or 2; ggan_swd): per direction W_p^p between the empirical measures of the
    two columns -- both sorted on the device, the quantile integral with integer weights in fp64 -> (values float64 [2] = [(mean_l
    per_l)^(1/p), (max_l per_l)^(1/p)], per float64 [L], status int32 [1]: 0, or SWD_NONFINITE when a value of either set is NaN or
    +-inf; values and per are then NaN).  The result depends on the multiset of each column only: permuted rows give the same bits.  Device
    tensors, no host synchronisation.  Forward only."""
    name = 'sliced_wasserstein_projected'
    _row_shapes(name, [px, py])
    _swd_rows(name, px, 'L')
    _swd_rows(name, py, 'L')
    _swd_dirs(name, px.shape[1])
    p = _swd_p(name, p)
    _no_grad(name, [px, py])
    same = px is py
    px = _c(px)
    py = px if same else _c(py)
    (m, L), n = px.shape, py.shape[0]
    dev = px.device
    per = torch.empty((L,), dtype=torch.float64, device=dev)
    out = torch.empty((2,), dtype=torch.float64, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(_L().ggan_swd_workspace(m, n, L), dev)
    check(_L().ggan_swd(_p(px), _p(py), m, n, L, p, _p(per), _p(out), _p(status), _p(ws), nbytes, _stream()), 'ggan_swd')
    return out, per, status


def sliced_wasserstein(x, y, theta, p=2):
    """the sliced Wasserstein distance of the row sets x float32 [m, d] and y float32 [n, d] over the directions theta float32 [d, L], used
    as given (normalising the columns is the caller's business): both sets through linear.Gemm onto the directions, then
    sliced_wasserstein_projected -> (values float64 [2], per float64 [L], status int32 [1]).  No column cap: d is the full pixel space
    if the caller wants it.  Device tensors, no host synchronisation.  Forward only."""
    name = 'sliced_wasserstein'
    _row_shapes(name, [x, y])
    _swd_rows(name, x)
    _swd_rows(name, y)
    if theta.dim() != 2 or theta.dtype != torch.float32 or theta.shape[0] != x.shape[1]:
        raise ValueError('%s: float32 directions [%d, L] expected, got %s %s' % (name, x.shape[1], theta.dtype, tuple(theta.shape)))
    _swd_dirs(name, theta.shape[1])
    p = _swd_p(name, p)
    _no_grad(name, [x, y, theta])
    same = x is y
    theta = _c(theta)
    px = Gemm.apply(_c(x), theta, None, False, False, _lib.ACT_NONE, 0.0)
    py = px if same else Gemm.apply(_c(y), theta, None, False, False, _lib.ACT_NONE, 0.0)
    return sliced_wasserstein_projected(px, py, p)


class Reparam(Function):
    """(z, std) = (mean + eps * exp(log_std), exp(log_std)): the stochastic encoder head (gan_inference_cifar10.py:173-188)"""

    @staticmethod
    def forward(ctx, mean, log_std, eps):
        mean, log_std, eps = _c(mean), _c(log_std), _c(eps)
        z, sd = torch.empty_like(mean), torch.empty_like(mean)
        check(_L().ggan_reparam_fwd(_p(mean), _p(log_std), _p(eps), _p(z), _p(sd), mean.numel(), _stream()), 'ggan_reparam_fwd')
        ctx.save_for_backward(eps, sd)
        return z, sd

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gsd):
        eps, sd = ctx.saved_tensors
        gmean, glog = torch.empty_like(sd), torch.empty_like(sd)
        check(_L().ggan_reparam_bwd(_p(_c(gz)) if gz is not None else _p(None), _p(_c(gsd)) if gsd is not None else _p(None), _p(eps), _p(sd),
                                    _p(gmean), _p(glog), sd.numel(), _stream()), 'ggan_reparam_bwd')
        return gmean, glog, None


AGG_KL, AGG_IKL, AGG_JSD = 0, 1, 2


class AggDiv(Function):
    """Monte-Carlo KL / inverse KL / JSD between the aggregated posterior (mixture of the minibatch's diagonal Gaussians mu, sd [nx, d])
    and N(0, I) (tflib/objs/kl_aggregated.py:46-74) -> 0-dim tensor.  k_onehot [nz, nx], eps_q [nz, d]: the component draws and noise
    of the samples from q (kl, jsd); z_p [nz, d]: the samples from the prior (ikl, jsd)."""

    @staticmethod
    def forward(ctx, mu, sd, k_onehot, eps_q, z_p, kind, n_coms):
        mu, sd = _c(mu), _c(sd)
        nx, d = mu.shape
        nz = (z_p if kind != AGG_KL else eps_q).shape[0]
        ns = 2 * nz if kind == AGG_JSD else nz
        k_onehot = _c(k_onehot) if kind != AGG_IKL else None
        eps_q = _c(eps_q) if kind != AGG_IKL else None
        z_p = _c(z_p) if kind != AGG_KL else None
        assert k_onehot is None or (tuple(k_onehot.shape) == (nz, nx) and tuple(eps_q.shape) == (nz, d))
        assert z_p is None or tuple(z_p.shape) == (nz, d)
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=mu.device)
        out, Z, A, Bv, T = new(), new(ns, d), new(ns, nx), new(ns), new(ns)
        check(_L().ggan_agg_div_fwd(kind, _p(mu), _p(sd), _p(k_onehot), _p(eps_q), _p(z_p), nx, nz, d, int(n_coms), _p(out), _p(Z), _p(A),
                                    _p(Bv), _p(T), _stream()), 'ggan_agg_div_fwd')
        ctx.dims = (kind, nx, nz, d, int(n_coms), ns)
        ctx.save_for_backward(mu, sd, k_onehot, eps_q, Z, A, Bv)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        mu, sd, k_onehot, eps_q, Z, A, Bv = ctx.saved_tensors
        kind, nx, nz, d, n_coms, ns = ctx.dims
        gmu, gsd = torch.empty_like(mu), torch.empty_like(sd)
        W = torch.empty((ns, nx), dtype=torch.float32, device=mu.device)
        GZ = torch.empty((nz, d), dtype=torch.float32, device=mu.device)
        check(_L().ggan_agg_div_bwd(kind, _p(mu), _p(sd), _p(k_onehot), _p(eps_q), nx, nz, d, n_coms, _p(Z), _p(A), _p(Bv), _p(_c(g)),
                                    _p(W), _p(GZ), _p(gmu), _p(gsd), _stream()), 'ggan_agg_div_bwd')
        return gmu, gsd, None, None, None, None, None




@_skip_undefined
class RowLerp(Function):
    """out[r,:] = x[r,:] + alpha[r]*(y[r,:]-x[r,:])  (the wali-gp interpolates)."""

    @staticmethod
    def forward(ctx, x, y, alpha):
        x, y, alpha = _c(x), _c(y), _c(alpha)
        rows, cols = x.shape
        out = torch.empty_like(x)
        check(_L().ggan_row_lerp(_p(x), _p(y), _p(alpha), _p(out), rows, cols, _stream()), 'ggan_row_lerp')
        ctx.save_for_backward(alpha)
        return out

    @staticmethod
    def backward(ctx, g):
        (alpha,) = ctx.saved_tensors
        z = torch.zeros_like(g)
        gx = RowLerp.apply(g, z, alpha) if ctx.needs_input_grad[0] else None
        gy = RowLerp.apply(z, g, alpha) if ctx.needs_input_grad[1] else None
        return gx, gy, None


# ---- the test-set pass of the gmgan scripts (forward only: no autograd) -------------------------------------------------------------
def gmm_posterior_assign_(z, mu, log_pi, row0, assign, colbest, probs=None):
    """q_k_probs = softmax(q_k_logits) of the rows row0 .. row0+B-1 (gmgan_inference_mnist.py:338; the logits of GmmLatent, no Gumbel
    noise, no temperature) in ONE launch (ggan_gmm_posterior_assign): assign[row0 + b] = the row's argmax, colbest (uint64 as int64[K],
    zeroed by the caller at the start of a pass) takes the running column argmax; probs (optional [B, K]) receives p.  In place."""
    z, mu = _c(z), _c(mu)
    B, D = z.shape
    K = mu.shape[0]
    assert tuple(mu.shape) == (K, D) and K <= POSTERIOR_MAX_K, (z.shape, mu.shape)
    assert assign.dtype == torch.int32 and assign.is_contiguous() and row0 >= 0 and row0 + B <= assign.numel()
    assert colbest.dtype == torch.int64 and colbest.is_contiguous() and colbest.numel() == K
    if probs is not None:
        assert probs.dtype == torch.float32 and probs.is_contiguous() and tuple(probs.shape) == (B, K)
    check(_L().ggan_gmm_posterior_assign(_p(z), _p(mu), float(log_pi), B, K, D, int(row0), _p(probs), _p(assign), _p(colbest), _stream()),
          'ggan_gmm_posterior_assign')


def cluster_accuracy_(assign, labels, colbest, correct):
    """gmgan_inference_mnist.py:518-528 on the device (ggan_cluster_accuracy): correct[0] = the number of rows whose cluster's label (the
    label of the row that maximises that cluster's probability) is their own.  assign / labels int32[N], colbest int64[K]."""
    N, K = assign.numel(), colbest.numel()
    assert labels.dtype == torch.int32 and labels.numel() == N and labels.is_contiguous() and assign.dtype == torch.int32
    assert correct.dtype == torch.int32 and correct.numel() >= 1 and K <= POSTERIOR_MAX_K
    check(_L().ggan_cluster_accuracy(_p(assign), _p(labels), _p(colbest), N, K, _p(correct), _stream()), 'ggan_cluster_accuracy')
    return correct


def sheet_grid(rows):
    """(nh, nw) of tflib.save_images.large_image's size=None rule: nh the largest divisor of the sample count not above its square root"""
    nh = int(rows ** 0.5)
    while (nh + 1) * (nh + 1) <= rows:
        nh += 1
    while nh * nh > rows:
        nh -= 1
    while rows % nh:
        nh -= 1
    return nh, rows // nh


def video_sheet_u8(gen, data, shape, a=0.5, b=255.99, d=255.99, interleave=False):
    """The two byte tensors of one video sheet in ONE launch (ggan_video_sheet_u8; ssgan_inference_moving_mnist.py:568-576 vis):
    gen [n, LEN, C*H*W] generated frames in [-1, 1] or None, data [n, LEN, C*H*W] as the feed holds it or None, shape = (C, H, W);
    interleave: rows alternate data / generated.  q = trunc(((x + 1) * a) * b) for generated, trunc(x * d) for data values, clamped to
    0..255.  -> (sheet uint8 [rows*H, LEN*W, C], index planes uint8 [LEN, nh*H, nw*W]) on the device."""
    C_, H, W = (int(v) for v in shape)
    src = gen if gen is not None else data
    if src is None:
        raise _lib.GganError('video_sheet_u8 needs generated frames or data')
    gen, data = (_c(gen) if gen is not None else None), (_c(data) if data is not None else None)
    n, LEN = int(src.shape[0]), int(src.shape[1])
    for t in (gen, data):
        assert t is None or (t.numel() == n * LEN * C_ * H * W and t.shape[0] == n and t.shape[1] == LEN), (t.shape, n, LEN, shape)
    rows = 2 * n if interleave else n
    nh, nw = sheet_grid(rows)
    sheet = torch.empty((rows * H, LEN * W, C_), dtype=torch.uint8, device=src.device)
    gif = torch.empty((LEN, nh * H, nw * W), dtype=torch.uint8, device=src.device)
    check(_L().ggan_video_sheet_u8(_p(gen), _p(data), _p(sheet), _p(gif), n, rows, LEN, C_, H, W, nh, nw, 1 if interleave else 0,
                                   float(a), float(b), float(d), _stream()), 'ggan_video_sheet_u8')
    return sheet, gif
