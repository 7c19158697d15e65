"""tflib/objs/mmd.py: the MMD objective of MODE vegan-mmd (gan_inference_cifar10.py:327-329).  `mix_rbf_mmd2` is one fused kernel
per direction (ggan_mix_rbf_mmd2_*) at training-minibatch sizes, and the set-level MFMA kernel (ggan_mix_rbf_sums, forward only) beyond
them; `vegan_mmd` returns (gen_cost, gen_train_op) -- there is no critic in this mode."""
import torch

from ... import functional as F
from ...optim import TrainOp, get_optimizer

SIGMAS = [2., 5., 10., 20., 40., 80.]


def mix_rbf_mmd2(X, Y, sigmas=SIGMAS, wts=None, biased=True):
    """tflib/objs/mmd.py:65-67 -> 0-dim float32 device tensor.  Up to m + n = 512 rows the fused differentiable ops (biased: the one the
    scripts train with; unbiased: mmd.py:53-61).  Inputs that need no gradient take the set-level kernel for the unbiased estimator and
    for any larger sets; larger sets that require grad are refused (the set-level op has no backward)."""
    m, n = int(X.shape[0]), int(Y.shape[0])
    if not biased and (m < 2 or n < 2):
        raise ValueError('the unbiased MMD estimator needs at least 2 rows per set (got %d and %d)' % (m, n))
    sg, wt = tuple(sigmas), (tuple(wts) if wts is not None else None)
    small = m + n <= F.MMD_FUSED_MAX_ROWS
    needs_grad = torch.is_grad_enabled() and (X.requires_grad or Y.requires_grad)
    if not needs_grad and (not biased or not small):
        wt_sum = float(sum(wt)) if wt is not None else float(len(sg))
        return F.mmd2_from_sums(F.mix_rbf_sums(X, Y, sg, wt), m, n, wt_sum, biased).to(torch.float32)
    if not small:
        raise ValueError('mix_rbf_mmd2 is differentiable up to m + n = %d rows (got %d + %d); detach the sets to score them'
                         % (F.MMD_FUSED_MAX_ROWS, m, n))
    return (F.MixRbfMmd2 if biased else F.MixRbfMmd2Unbiased).apply(X, Y, sg, wt)


def vegan_mmd(q_z, p_z, rec_penalty, gen_params, batch_size, lamb, lr=2e-4, beta1=.5):
    """tflib/objs/mmd.py:69-80"""
    gen_cost = mix_rbf_mmd2(q_z, p_z) * float(lamb)
    gen_cost = gen_cost + rec_penalty
    gen_opt = get_optimizer('gen', gen_params, lr=lr, beta1=beta1, beta2=0.999)
    return gen_cost, TrainOp(gen_opt, gen_cost)
