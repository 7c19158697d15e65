"""A small image classifier fitted on the device, the scorer of evaluate.Evaluator.classifier_scores.

The reference scores its samples with a frozen Inception graph that tflib/inception_score.py:56-90 downloads at import; nothing is downloaded
here.  ImageClassifier is the stand-in a run can make for itself in seconds: the Extractor's conv stack for the data set (cfg.nl layers, 5x5,
stride 2, widths cfg.dim * 2^i, LeakyReLU in the fused epilogue) WITHOUT BatchNorm -- a scorer whose logits depend on who else is in the
minibatch is wrong --, then Linear(flat, 128) + LeakyReLU (the feature) and Linear(128, classes).  Built from functional.ConvFwd / Gemm
directly, trained by functional.SoftmaxXent and an optim.AdamOptimizer of its own.

Its parameters are private to the object: they are not in the tflib.param registry, so named_params(), checkpoints and the reference-trace
tests do not see them and delete_all_params() does not free them; its optimizer is under no Trainer role, keeps no average and its update
makes no collective call.  Initial values: the uniform He schemes of tflib/ops/conv2d.py (sqrt(4 / (fan_in + fan_out))) and linear.py ('he':
sqrt(2 / fan_in)), drawn from a numpy RandomState(seed) of the classifier's own -- numpy's global state is not touched.

Inputs are what model.real_x(feed) returns and the Generator emits: [rows, C * S * S] float32 in [-1, 1] ([0, 1] for MNIST)."""
import collections

import numpy as np
import torch

from . import functional as F
from . import optim

CLS_LR, CLS_BETA1, CLS_BETA2 = 1e-3, 0.9, 0.999
CLS_FEATURES = 128            # width of the feature layer: functional.FRECHET_MAX_DIM, the column cap of the Frechet kernels
META_KEYS = ('dataset', 'classes', 'dim', 'seed', 'fit_rows', 'epochs', 'accuracy')
_MUST_MATCH = ('dataset', 'classes', 'dim')


class _LocalBucket(optim.GradBucket):
    """the gradient bucket of an optimizer that belongs to ONE process whatever process group exists: world 1, scale 1, and all_reduce
    issues nothing.  The classifier is fitted by the one rank that evaluates; an exchange from there would meet no partner -- or the other
    ranks' next training exchange."""

    def __init__(self, flat):
        self.flat, self.group, self.world, self.scale = flat, None, 1, 1.0

    def all_reduce(self, async_op=False, lo=0, hi=None):
        return None


def _uniform(rng, stdev, shape):
    return rng.uniform(low=-stdev * np.sqrt(3), high=stdev * np.sqrt(3), size=shape).astype('float32')


def initial_values(cfg, classes, seed):
    """OrderedDict name -> float32 array, in the order the values are drawn: '<layer>.Filters' / '.Biases' for Conv1 .. Conv<nl>, then
    'Feature.W' / '.b' and 'Output.W' / '.b'"""
    rng = np.random.RandomState(int(seed))
    out = collections.OrderedDict()
    ch = cfg.C
    for i in range(cfg.nl):
        cout = cfg.dim * 2 ** i
        fan_in, fan_out = ch * 25, cout * 25 / 4.0
        out['Conv%d.Filters' % (i + 1)] = _uniform(rng, np.sqrt(4.0 / (fan_in + fan_out)), (5, 5, ch, cout))
        out['Conv%d.Biases' % (i + 1)] = np.zeros(cout, dtype='float32')
        ch = cout
    for name, nin, nout in (('Feature', cfg.flat, CLS_FEATURES), ('Output', CLS_FEATURES, int(classes))):
        out[name + '.W'] = _uniform(rng, np.sqrt(2.0 / nin), (nin, nout))
        out[name + '.b'] = np.zeros(nout, dtype='float32')
    return out


class ImageClassifier(object):
    def __init__(self, cfg, classes, seed, device=None):
        """cfg: the run's models.Config (dataset, C, S, nl, dim, flat, B); 2 <= classes <= functional.CLS_MAX_CLASSES; device: the tflib device
        by default"""
        classes = int(classes)
        if not 2 <= classes <= F.CLS_MAX_CLASSES:
            raise ValueError('ImageClassifier: 2 <= classes <= %d expected, got %d' % (F.CLS_MAX_CLASSES, classes))
        if device is None:
            from . import tflib as lib
            device = lib.get_device()
        self.cfg, self.classes, self.seed, self.device = cfg, classes, int(seed), torch.device(device)
        self.params = collections.OrderedDict()
        for name, value in initial_values(cfg, classes, seed).items():
            self.params[name] = torch.as_tensor(value).to(self.device).contiguous().requires_grad_()
        self.opt = optim.AdamOptimizer(list(self.params.values()), lr=CLS_LR, beta1=CLS_BETA1, beta2=CLS_BETA2)
        # single-replica whatever torch.distributed says: no exchange, no 1 / world on the gradient, the fused pack + update stays on
        self.opt.bucket = _LocalBucket(self.opt.g)
        self.opt.world = 1
        self.fit_rows, self.epochs, self.held_out = 0, 0, float('nan')

    # ---- the net ---------------------------------------------------------------------------------------------------------------------
    def _forward(self, x):
        c, p = self.cfg, self.params
        out = x.reshape(-1, c.C, c.S, c.S)
        ch = c.C
        for i in range(c.nl):
            cout = c.dim * 2 ** i
            geom = F.conv_geom(out.shape[0], ch, out.shape[2], out.shape[3], cout, 5, 2)
            out = F.ConvFwd.apply(out, p['Conv%d.Filters' % (i + 1)], p['Conv%d.Biases' % (i + 1)], geom, F.ACT_LRELU, 0.2, None)
            ch = cout
        out = out.reshape(-1, c.flat)
        feat = F.Gemm.apply(out, p['Feature.W'], p['Feature.b'], False, False, F.ACT_LRELU, 0.2, None)
        return F.Gemm.apply(feat, p['Output.W'], p['Output.b'], False, False, F.ACT_NONE, 0.0, None), feat

    def logits(self, x, features=False):
        """logits float32 [rows, classes] of images x [rows, C * S * S] (any shape with that many elements a row); features: (logits, the
        128-wide feature rows).  No tape."""
        with torch.no_grad():
            out, feat = self._forward(x)
        return (out, feat) if features else out

    def fit(self, batches, epochs):
        """eager Adam steps on the current stream over the minibatches [(x float32 [B, C * S * S], y int32 [B])] (device tensors), in the order
        given, `epochs` times -> the per-step losses, float32 [steps] on the device (nothing is read back)"""
        batches = list(batches)
        losses = []
        with torch.enable_grad():
            for _ in range(int(epochs)):
                for x, y in batches:
                    loss, _, _ = F.SoftmaxXent.apply(self._forward(x.detach())[0], y)
                    self.opt.minimize(loss)
                    losses.append(loss.detach())
        self.fit_rows, self.epochs = sum(int(y.shape[0]) for _, y in batches), self.epochs + int(epochs)
        return torch.stack(losses) if losses else torch.empty((0,), dtype=torch.float32, device=self.device)

    def hits(self, batches):
        """(rows whose argmax is their label: int32 [1] on the device, the row count) over minibatches [(x, y)]"""
        total, rows = torch.zeros((1,), dtype=torch.int32, device=self.device), 0
        for x, y in batches:
            total = total + F.softmax_xent(self.logits(x), y)[1]
            rows += int(y.shape[0])
        return total, rows

    def accuracy(self, batches):
        """the share of rows of the minibatches [(x, y)] whose argmax is their label (one host synchronisation)"""
        total, rows = self.hits(batches)
        return int(total.item()) / float(max(rows, 1))

    # ---- state -----------------------------------------------------------------------------------------------------------------------
    def meta(self):
        return dict(dataset=self.cfg.dataset, classes=self.classes, dim=int(self.cfg.dim), seed=self.seed, fit_rows=int(self.fit_rows),
                    epochs=int(self.epochs), accuracy=float(self.held_out))

    def state_dict(self):
        """{'classifier/<layer>.<Filters|Biases|W|b>': float32 array, 'classifier/meta': the META_KEYS as one string array}"""
        st = {'classifier/' + k: v.detach().cpu().numpy().copy() for k, v in self.params.items()}
        m = self.meta()
        st['classifier/meta'] = np.array(['%s=%s' % (k, m[k]) for k in META_KEYS])
        return st

    @staticmethod
    def _parse_meta(arr):
        m = dict(str(s).split('=', 1) for s in np.asarray(arr).reshape(-1))
        missing = [k for k in META_KEYS if k not in m]
        if missing:
            raise ValueError('classifier file: classifier/meta lacks %s' % ', '.join(missing))
        return dict(dataset=m['dataset'], classes=int(m['classes']), dim=int(m['dim']), seed=int(m['seed']), fit_rows=int(m['fit_rows']),
                    epochs=int(m['epochs']), accuracy=float(m['accuracy']))

    def load_state_dict(self, st):
        """takes a state_dict() whose meta names this run's data set, class count and width (ValueError naming the field otherwise); the
        optimizer's moments restart"""
        if 'classifier/meta' not in st:
            raise ValueError('classifier file: no classifier/meta key')
        m, mine = self._parse_meta(st['classifier/meta']), self.meta()
        for k in _MUST_MATCH:
            if m[k] != mine[k]:
                raise ValueError('classifier file: %s is %r, this run has %r' % (k, m[k], mine[k]))
        for k, p in self.params.items():
            a = st.get('classifier/' + k)
            if a is None or tuple(np.shape(a)) != tuple(p.shape):
                raise ValueError('classifier file: classifier/%s is %s, this run has %s' % (k, 'missing' if a is None else np.shape(a), tuple(p.shape)))
        with torch.no_grad():
            for k, p in self.params.items():
                p.copy_(torch.as_tensor(np.asarray(st['classifier/' + k], dtype=np.float32)))
            self.opt.m.zero_()
            self.opt.v.zero_()
            self.opt.step.zero_()
        self.seed, self.fit_rows, self.epochs, self.held_out = m['seed'], m['fit_rows'], m['epochs'], m['accuracy']

    def save(self, path):
        with open(path, 'wb') as f:
            np.savez(f, **self.state_dict())

    def load(self, path):
        with np.load(path, allow_pickle=False) as z:
            self.load_state_dict({k: z[k] for k in z.files})
