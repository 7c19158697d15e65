"""Device time of the wide probe chain (csrc/probe_wide.hip) at a script's default row counts, entry by entry, beside the time the probe
pass spends building its sets (docs/KERNELS.md, the wide probe section).  Random labelled rows for the kernels; synthetic labelled images
and a randomly initialised model for the pass: timing only.  Per entry: one warm-up, then REPEATS timed calls between device events --
median and range.  `python tools/probe_wide_time.py [script] [d ...]` (default: gan_inference_cifar10 3072 4096)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from graphical_gan_amd import run, _lib, functional as F  # noqa: E402
from graphical_gan_amd import tflib as lib  # noqa: E402
from graphical_gan_amd.engine import Trainer  # noqa: E402
from graphical_gan_amd.evaluate import Evaluator, PROBE_FIT_ROWS, PROBE_MAX_ROWS, PROBE_RIDGE  # noqa: E402

REPEATS = 5
FP64_MFMA_PEAK = 78.6e12      # MI355X, dense fp64 matrix flop/s


def _timed(fn):
    """fn() once to warm up, then REPEATS times between events -> sorted milliseconds"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)


def chain(n, m, d, classes, device):
    """the five entries on n fit rows and m scoring rows of d columns -> {entry: sorted ms}; the factor's launches by label from one
    profiled call"""
    L, S, p = _lib.load(), F._stream(), F._p
    g = torch.Generator(device='cpu').manual_seed(0)
    y = torch.randint(0, classes, (n,), generator=g, dtype=torch.int32)
    Z = (torch.randn(n, d, generator=g) + 0.35 * torch.randn(classes, d, generator=g)[y.long()]).to(device)
    y = y.to(device)
    new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=device)
    mean, inv_std, W, bias, counts, status = new((d,)), new((d,)), new((d, classes)), new((classes,)), new((classes,), torch.int32), new((1,), torch.int32)
    G, G0, R, correct = new((d, d), torch.float64), new((d, d), torch.float64), new((d, classes), torch.float64), new((1,), torch.int32)
    nbytes = L.ggan_wprobe_moments_workspace(n, d, classes)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)

    def ok(rc):
        assert rc == 0, L.ggan_last_error()
    out = {}
    out['moments'] = _timed(lambda: ok(L.ggan_wprobe_moments(p(Z), p(y), n, d, classes, p(mean), p(inv_std), p(counts), p(status), p(ws), nbytes, S)))
    out['normal'] = _timed(lambda: ok(L.ggan_wprobe_normal(p(Z), p(y), n, d, classes, p(mean), p(inv_std), p(G0), p(R), S)))

    def factor():
        ok(L.ggan_wprobe_factor(p(G), d, PROBE_RIDGE, p(status), S))
    ms = []
    for i in range(REPEATS + 1):                      # (in place: every call gets a fresh copy, outside the timed span)
        G.copy_(G0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        factor()
        b.record()
        torch.cuda.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    out['factor'] = sorted(ms)
    out['solve'] = _timed(lambda: ok(L.ggan_wprobe_solve(p(G), p(R), p(counts), n, d, classes, p(W), p(bias), p(status), S)))
    out['predict'] = _timed(lambda: ok(L.ggan_wprobe_predict(p(Z[:m]), p(y[:m]), m, d, classes, p(mean), p(inv_std), p(W), p(bias), None, p(correct), S)))
    assert int(status.item()) == 0 and bool(torch.isfinite(W).all())
    G.copy_(G0)
    L.ggan_prof_reset()
    L.ggan_prof_enable(1)
    factor()
    torch.cuda.synchronize()
    L.ggan_prof_enable(0)
    parts = {}
    for r in _lib.prof_report(cap=1024):
        parts[r['name']] = parts.get(r['name'], 0.0) + r['total_ms']
    L.ggan_prof_reset()
    return out, parts


def main(script='gan_inference_cifar10', *widths):
    widths = [int(w) for w in widths] or [3072, 4096]
    S = run.reference_block(script)
    S.update(SYNTHETIC='force')
    cfg = run.config(S)
    device = lib.get_device()
    B, D = S['BATCH_SIZE'], cfg.output_dim
    n, m = PROBE_FIT_ROWS // B * B, PROBE_MAX_ROWS // B * B
    med = lambda v: v[len(v) // 2]
    for d in widths:
        out, parts = chain(n, m, d, 10, device)
        print('d = %d, %d fit rows, %d scoring rows, 10 classes: median ms [min, max] of %d' % (d, n, m, REPEATS))
        for k, v in out.items():
            print('  %-8s %9.3f [%9.3f, %9.3f]' % (k, med(v), v[0], v[-1]))
        fit = sum(med(out[k]) for k in ('moments', 'normal', 'factor', 'solve'))
        print('  fit %.3f ms; fit + the predictions of the dev and the fit rows %.3f ms' % (fit, fit + med(out['predict']) * (1.0 + n / float(m))))
        print('  factor: %.1f %% of the fp64 MFMA peak (d^3 / 3 flop); its launches under the profiler: %s'
              % (100.0 * (d ** 3 / 3.0) / (med(out['factor']) * 1e-3) / FP64_MFMA_PEAK, {k: round(v, 3) for k, v in sorted(parts.items())}))
    tr = Trainer(cfg, device=device, graph=False)
    rng = np.random.default_rng(0)
    proto = rng.integers(0, 256, size=(10, D))

    def batches(k):
        res = []
        for _ in range(k):
            y = rng.integers(0, 10, size=B)
            x = np.clip(0.5 * proto[y] + 0.5 * rng.integers(0, 256, size=(B, D)), 0, 255)
            res.append(((x / 255.0).astype(np.float32) if cfg.dataset == 'mnist' else x.astype(np.int32), y.astype(np.int64)))
        return res
    fit, dev = batches(PROBE_FIT_ROWS // B), batches(PROBE_MAX_ROWS // B)
    for wide in (False, True):
        ev = Evaluator(tr, dict(S, PROBE_WIDE=wide))
        secs = []
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.time()
            res = ev.probe_scores(fit, dev)
            torch.cuda.synchronize()
            secs.append(time.time() - t0)
        print('%s: the pass %s: wall seconds %s (the first call warms up), x %d and h %d columns, %s'
              % (script, 'with PROBE_WIDE' if wide else 'as it is', ['%.3f' % s for s in secs], D, cfg.flat, res))


if __name__ == '__main__':
    main(*sys.argv[1:])
