"""float64 restatements for the classifier-score tests (test_cls_cpu.py, test_cls_gpu.py), written from the formulas: the mean softmax
cross-entropy with its gradient, the inception-score formula per split, and a small conv classifier with TF-flavoured Adam.  The shared
case tables and the gates.

Gates for values -- the loss, every split score, their mean and std, the two entropies: the project's set-level gate,
|got - ref| <= 2e-5 max(1, |ref|) (tests/_parzen_ref.py, tests/test_mmd_sets_gpu.py).

Gate for dlogits, from float32 unit roundoff u = 2^-24 and the operations of a row (first order, x the logits, m their maximum, d = x - m <= 0,
e = exp(d), s = sum e >= 1, p = e / s):
  d_c = x_c - m              one rounding, |delta d_c| <= u |d_c|, which exp turns into a relative error u |d_c| of e_c;
  e_c = expf(d_c)            the accurate expf the kernel calls is documented at 1 ulp = 2 u relative (no fast form is used);
  s   = a 6-level tree       6 u relative from the additions (all terms positive), and from the terms' own errors
                             sum_c e_c (|d_c| + 2) u / s = (sum_c p_c |d_c| + 2) u <= (ln C + 2) u, since sum_c p_c (-d_c) = H(p) - ln s <= ln C;
  p_c = e_c / s              one rounding: |delta p_c| <= p_c (|d_c| + 2 + 6 + ln C + 2 + 1) u, and p_c |d_c| <= e_c |d_c| <= 1 / e < 0.37;
  p_c - onehot, then / B     two roundings of a value of magnitude at most 1: 2 u.
With p_c <= 1: |delta dlogits_bc| <= (0.37 + 11 + ln C + 2) u / B.  The gate is DL_ULPS(C) u / B with DL_ULPS(C) = 16 + ln C: the sum above with
its constant rounded up from 13.37 to 16 for the second-order terms.  A row of dlogits sums to 0 exactly in real arithmetic, so the float64 sum
of a device row is gated at C times the element gate.  None of this was fitted to device output.

Every check prints the observed fraction of its bound."""
import math

import numpy as np

GATE = 2e-5
U32 = 2.0 ** -24
PAD, SENTINEL = 64, -7.5e8
BAD_LABEL, NONFINITE = 1, 2
MAX_CLASSES, MAX_SPLITS, MAX_BATCH, MAX_ROWS, ROW_BLOCK, XENT_ROWS_PER_WG = 64, 64, 65536, 1 << 20, 256, 64

# (B, C): the smallest shape; a class count that is no power of two; ...; the reference's minibatch; every lane, several workgroups and a tail; ...
XENT_ROWS = [(1, 2), (3, 33), (64, 10), (100, 10), (257, 64), (4099, 7)]
XENT_SCALES = [1.0, 80.0]          # 80: posteriors that underflow in float32
# (N, C, S, scale): one row per split; ...; uneven splits; ...; one split, underflow; a score of about 1, the cancellation case; the pass's own size
SCORE_ROWS = [(10, 2, 10, 1.0), (1000, 10, 10, 1.0), (1003, 10, 10, 3.0), (4099, 64, 7, 5.0), (2048, 33, 1, 80.0), (640, 10, 10, 0.01),
              (49984, 10, 10, 8.0)]


def gate(ref):
    return GATE * np.maximum(1.0, np.abs(ref))


def fraction(got, ref):
    """the largest |got - ref| in units of the value gate (nan if either is not finite)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if not (np.all(np.isfinite(got)) and np.all(np.isfinite(ref))):
        return float('nan')
    return float(np.max(np.abs(got - ref) / gate(ref)))


def dl_ulps(C):
    return 16.0 + math.log(C)


def dl_gate(B, C):
    return dl_ulps(C) * U32 / B


# ---- the two formulas ------------------------------------------------------------------------------------------------------------------------
def log_softmax(logits):
    x = np.asarray(logits, np.float64)
    d = x - x.max(axis=1, keepdims=True)
    return d - np.log(np.exp(d).sum(axis=1, keepdims=True))


def xent(logits, labels):
    """-> (loss, dlogits [B, C], hits): mean_b (logsumexp(x_b) - x_b,label), (softmax - onehot) / B, #{argmax_b == label_b} (lowest class on a tie)"""
    x = np.asarray(logits, np.float64)
    B, C = x.shape
    lp = log_softmax(x)
    y = np.asarray(labels, np.int64)
    loss = float(-np.mean(lp[np.arange(B), y]))
    dl = np.exp(lp)
    dl[np.arange(B), y] -= 1.0
    return loss, dl / B, int(np.sum(np.argmax(np.asarray(logits), axis=1) == y))


def split_bounds(N, S):
    return [((s * N) // S, ((s + 1) * N) // S) for s in range(S)]


def _xlogy(p, logq):
    return np.where(p > 0, p * np.where(p > 0, logq, 0.0), 0.0)


def class_score(logits, S):
    """the direct two-pass form, log p from the log-softmax -> (scores [S], mean, population std, mean row entropy, entropy of the marginal)"""
    lp = log_softmax(logits)
    p = np.exp(lp)
    scores = []
    for a, b in split_bounds(p.shape[0], S):
        pb = p[a:b].mean(axis=0, keepdims=True)
        with np.errstate(divide='ignore'):
            kl = _xlogy(p[a:b], lp[a:b] - np.log(pb)).sum(axis=1)
        scores.append(math.exp(kl.mean()))
    scores = np.array(scores)
    pb = p.mean(axis=0)
    with np.errstate(divide='ignore'):
        return scores, float(scores.mean()), float(scores.std()), float(-_xlogy(p, lp).sum(axis=1).mean()), float(-_xlogy(pb, np.log(pb)).sum())


def class_score_identity(logits, S):
    """exp(H(pbar) - mean_i H(p_i)) per split: what the device computes, here in float64"""
    lp = log_softmax(logits)
    p = np.exp(lp)
    out = []
    for a, b in split_bounds(p.shape[0], S):
        pb = p[a:b].mean(axis=0)
        with np.errstate(divide='ignore'):
            out.append(math.exp(-_xlogy(pb, np.log(pb)).sum() + _xlogy(p[a:b], lp[a:b]).sum(axis=1).mean()))
    return np.array(out)


def class_score_literal32(logits, S):
    """the published formula to the letter in float32, posteriors first and then their logarithm: NaN once a posterior underflows"""
    x = np.asarray(logits, np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    p = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    out = []
    with np.errstate(divide='ignore', invalid='ignore'):
        for a, b in split_bounds(p.shape[0], S):
            part = p[a:b]
            kl = part * (np.log(part) - np.log(np.mean(part, 0, keepdims=True)))
            out.append(np.exp(np.mean(np.sum(kl, 1))))
    return np.array(out)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
def xent_id(B, C, scale):
    return 'B%d-C%d-x%g' % (B, C, scale)


def xent_inputs(B, C, scale):
    """float32 logits, int32 labels, the row with an exact two-way tie at its maximum (its label is the HIGHER of the two classes: no hit)"""
    rng = np.random.default_rng(1000 * B + 10 * C + int(scale))
    x = (rng.standard_normal((B, C)) * scale).astype(np.float32)
    y = rng.integers(0, C, size=B).astype(np.int32)
    y[::3] = np.argmax(x, axis=1)[::3].astype(np.int32)          # (a third of the rows hit)
    t = B // 2
    a, b = sorted(rng.choice(C, size=2, replace=False).tolist())
    x[t, a] = x[t, b] = np.float32(x[t].max() + np.float32(scale))
    y[t] = b
    return x, y, t


def xent_launches(B):
    return {('softmax_xent', -(-B // XENT_ROWS_PER_WG) * 256): 1, ('softmax_xent_final', 256): 1}


def score_id(N, C, S, scale):
    return 'N%d-C%d-S%d-x%g' % (N, C, S, scale)


def score_inputs(N, C, S, scale):
    rng = np.random.default_rng(7 * N + 13 * C + S)
    return (rng.standard_normal((N, C)) * scale).astype(np.float32)


def score_launches(N, S):
    return {('class_score', S * -(-(-(-N // S)) // ROW_BLOCK) * 256): 1, ('class_score_final', 256): 1}


# ---- the fit ---------------------------------------------------------------------------------------------------------------------------------
# A synthetic four-class task: 28 x 28 images in [0, 1], a bright block of FIT_CONTRAST in one of the four quadrants over uniform noise
# of FIT_NOISE.  FIT_ROWS rows to fit on, FIT_HELD rows held out, minibatches of FIT_B in file order, FIT_EPOCHS passes: 32 steps.
# Chosen on the CPU so that the float64 restatement below reaches 100 % held-out accuracy with every held-out top-two logit margin above 1
# (measured there: accuracy 1.0, the smallest margin FIT_MARGIN64); the device fit must then reach 100 % too -- a condition on the inputs.
FIT_SEED, FIT_ROWS, FIT_HELD, FIT_B, FIT_EPOCHS, FIT_CLASSES, FIT_DIM = 5, 512, 256, 32, 2, 4, 8
FIT_CONTRAST, FIT_NOISE = 0.8, 0.2
FIT_TRAJECTORY = 20          # leading per-step losses compared with the float64 restatement
FIT_MARGIN64 = 12.89         # the smallest held-out top-two logit margin of the float64 restatement after the 32 steps (float32: 12.89 too)
# The trajectory gate.  tests/test_step_gpu.py gates WEIGHTS after a step (1e-4 of their scale, median and l2): it says nothing about a
# scalar loss along 20 Adam steps, so it does not carry over.  Measured instead, on the CPU: the largest gap between the float32 and the
# float64 restatement over the first FIT_TRAJECTORY losses is FIT_GAP32; the gate is 4 x that, because the device's summation orders differ
# from both.  Not tuned to device output.
# What the figure consists of.  The float32 restatement rounds EVERY operation of A.5 to float32, its scalars included, as a float32
# implementation does (the library's Adam kernels: csrc/optim.hip, adam_lr_t = lr sqrtf(1.f - powf(b2, t)) / (1.f - powf(b1, t)); TF1's
# AdamOptimizer likewise).  In 1 - b2^t the power, 0.998 .., carries half an ulp of 1 (3e-8) into a difference of 0.002: the step size of
# steps 2 .. 6 is off by 1.1e-6 .. 3.3e-6 relative, for all parameters together.  A common relative error d of one step's size moves the
# next loss by about d times the loss's change per step (0.2 .. 0.25 here): 7.1e-7 of the gap, at step 2.  The rest is summation order,
# about 1e-7: with the scalars kept in double the float32 restatement sits 0.8e-7 .. 1.4e-7 from the float64 one, and random errors do
# not add up as a common one does -- a relative gradient noise of 1e-4 per element moves the float64 losses by 1.2e-7 only.
FIT_GAP32 = 7.34e-7
FIT_LOSS_GATE = 4.0 * FIT_GAP32


def fit_config():
    from graphical_gan_amd.models import Config
    return Config('mnist', batch_size=FIT_B, dim=FIT_DIM, dim_latent=16)


def fit_task():
    """-> (fit_x float32 [FIT_ROWS, 784], fit_y int32, held_x float32 [FIT_HELD, 784], held_y int32)"""
    rng = np.random.default_rng(FIT_SEED)
    n = FIT_ROWS + FIT_HELD
    y = rng.integers(0, FIT_CLASSES, size=n).astype(np.int32)
    x = (FIT_NOISE * rng.random((n, 28, 28))).astype(np.float32)
    for i in range(n):
        r, c = 14 * (y[i] // 2), 14 * (y[i] % 2)
        x[i, r + 3:r + 11, c + 3:c + 11] += np.float32(FIT_CONTRAST)
    x = x.reshape(n, 784)
    return x[:FIT_ROWS], y[:FIT_ROWS], x[FIT_ROWS:], y[FIT_ROWS:]


def fit_batches(x, y):
    return [(x[i:i + FIT_B], y[i:i + FIT_B]) for i in range(0, x.shape[0] - FIT_B + 1, FIT_B)]


class RefClassifier(object):
    """classifier.ImageClassifier restated in PyTorch on the CPU at a given dtype: the same initial values, TF 'SAME' padding (the extra row
    and column at the bottom and right), LeakyReLU 0.2 as max(0.2 x, x), the mean softmax cross-entropy, TF-flavoured Adam (SURVEY.md App. A.5:
    lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), theta -= lr_t m / (sqrt(v) + eps))"""

    def __init__(self, cfg, classes, seed, dtype):
        import torch
        from graphical_gan_amd import classifier as K
        self.cfg, self.dtype, self.t = cfg, dtype, 0
        self.p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in K.initial_values(cfg, classes, seed).items()}
        self.m = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.lr, self.b1, self.b2, self.eps = K.CLS_LR, K.CLS_BETA1, K.CLS_BETA2, 1e-8

    def forward(self, x):
        import torch
        import torch.nn.functional as TF
        c = self.cfg
        out = torch.as_tensor(x, dtype=self.dtype).reshape(-1, c.C, c.S, c.S)
        for i in range(c.nl):
            w = self.p['Conv%d.Filters' % (i + 1)].permute(3, 2, 0, 1)            # HWIO -> OIHW
            pads = []
            for size in (out.shape[3], out.shape[2]):                               # (F.pad: the last dimension first)
                total = max((-(-size // 2) - 1) * 2 + 5 - size, 0)
                pads += [total // 2, total - total // 2]
            out = TF.conv2d(TF.pad(out, pads), w, self.p['Conv%d.Biases' % (i + 1)], stride=2)
            out = torch.maximum(0.2 * out, out)
        out = out.reshape(-1, c.flat)
        feat = out @ self.p['Feature.W'] + self.p['Feature.b']
        feat = torch.maximum(0.2 * feat, feat)
        return feat @ self.p['Output.W'] + self.p['Output.b']

    def step(self, x, y):
        import torch
        logits = self.forward(x)
        lp = logits - torch.logsumexp(logits, dim=1, keepdim=True)
        loss = -lp[torch.arange(len(y)), torch.as_tensor(np.asarray(y), dtype=torch.long)].mean()
        grads = torch.autograd.grad(loss, list(self.p.values()))
        self.t += 1
        # A.5's scalars at the restatement's own precision, as written: each operation of lr sqrt(1 - b2^t) / (1 - b1^t), 1 - b1 and 1 - b2
        # is rounded to self.dtype (in float32 the cancellation in 1 - b2^t costs the first steps' size about 3e-6 relative)
        f = np.float32 if self.dtype == torch.float32 else np.float64
        one, t = f(1), f(self.t)
        lr_t = float(f(self.lr) * np.sqrt(one - np.power(f(self.b2), t)) / (one - np.power(f(self.b1), t)))
        b1, b2, c1, c2 = float(f(self.b1)), float(f(self.b2)), float(one - f(self.b1)), float(one - f(self.b2))
        with torch.no_grad():
            for (k, p), g in zip(self.p.items(), grads):
                self.m[k].mul_(b1).add_(g, alpha=c1)
                self.v[k].mul_(b2).addcmul_(g, g, value=c2)
                p.sub_(lr_t * self.m[k] / (self.v[k].sqrt() + self.eps))
        return float(loss.detach())

    def fit(self, batches, epochs):
        return [self.step(x, y) for _ in range(epochs) for x, y in batches]

    def logits(self, x):
        import torch
        with torch.no_grad():
            return self.forward(x).double().numpy()


_FIT_CACHE = {}


def fit_reference(dtype_name='float64'):
    """the restated fit on the task, computed once per dtype -> dict(losses [steps], held_logits [FIT_HELD, classes], accuracy, margin)"""
    import torch
    if dtype_name not in _FIT_CACHE:
        fx, fy, hx, hy = fit_task()
        ref = RefClassifier(fit_config(), FIT_CLASSES, FIT_SEED, getattr(torch, dtype_name))
        losses = np.array(ref.fit(fit_batches(fx, fy), FIT_EPOCHS))
        lg = ref.logits(hx)
        top = np.sort(lg, axis=1)
        _FIT_CACHE[dtype_name] = dict(losses=losses, held_logits=lg, accuracy=float(np.mean(np.argmax(lg, axis=1) == hy)),
                                      margin=float(np.min(top[:, -1] - top[:, -2])))
    return _FIT_CACHE[dtype_name]
