"""Time of the set-level MMD op (functional.mix_rbf_sums, csrc/mmd_sets.hip) and of the dev-set MMD pass on an MI355X, for docs/KERNELS.md.

  python tools/mmd_time.py [--n 10000] [--dims 128 3072] [--repeat 7] [--chunk 2048] [--no-pass]

Per width d: two sets of n rows each, every shape warmed twice, then the op timed `--repeat` times between HIP events (median, min, max
printed).  Beside it what a user of torch would write: the same three sums from `x @ y.T`, the row norms and `exp`, in row chunks of
`--chunk` so that no n x n matrix is held (whole same-set blocks: it does not use the symmetry), summed in float64; the two results are
compared.  FLOP: the kernel launch's own count (tiles computed x 2 x 128 x 128 x d, the figure it hands to the profiler) over the op's
time, against the fp32-MFMA peak of 157.3 TFLOP/s; libggan's per-kernel timers give the three launches' shares.  Then the wall time of one
Evaluator.mmd_scores pass beside one dev_costs pass on the synthetic dev set of gan_inference_cifar10 (host clock around a device
synchronise).  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIGMAS = [2., 5., 10., 20., 40., 80.]
PEAK_TFLOPS = 157.3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--dims', type=int, nargs='+', default=[128, 3072])
    ap.add_argument('--repeat', type=int, default=7)
    ap.add_argument('--chunk', type=int, default=2048)
    ap.add_argument('--no-pass', action='store_true')
    a = ap.parse_args()
    import torch
    from graphical_gan_amd import functional as F, run, _lib
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.evaluate import Evaluator
    assert torch.cuda.is_available(), 'a timing needs the GPU'
    dev = torch.device('cuda:0')

    def timed(fn, reps):
        fn(); fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))

    def torch_sums(x, y):
        def block(p, q, same):
            nq = (q * q).sum(1)
            tot = torch.zeros((), dtype=torch.float64, device=dev)
            for r0 in range(0, p.shape[0], a.chunk):
                pc = p[r0:r0 + a.chunk]
                D = ((pc * pc).sum(1)[:, None] + nq[None, :] - 2.0 * (pc @ q.t())).clamp_(min=0)
                K = torch.zeros_like(D)
                for s in SIGMAS:
                    K += torch.exp(D * (-1.0 / (2 * s * s)))
                if same:
                    K[torch.arange(pc.shape[0], device=dev), torch.arange(r0, r0 + pc.shape[0], device=dev)] = 0
                tot += K.sum(dtype=torch.float64)
            return tot
        return torch.stack([block(x, x, True), block(y, y, True), block(x, y, False)])

    out, L = {}, _lib.load()
    for d in a.dims:
        g = torch.Generator(device=dev)
        g.manual_seed(d)
        if d <= 256:          # codes
            x, y = torch.randn(a.n, d, device=dev, generator=g), torch.randn(a.n, d, device=dev, generator=g) * 1.1 + 0.1
        else:                 # pixels in [-1, 1]
            x, y = torch.rand(a.n, d, device=dev, generator=g) * 2 - 1, torch.tanh(torch.randn(a.n, d, device=dev, generator=g))
        ours, ref = F.mix_rbf_sums(x, y, SIGMAS).cpu().tolist(), torch_sums(x, y).cpu().tolist()
        rec = dict(sums=ours, rel_diff_to_torch=[abs(p - q) / abs(q) for p, q in zip(ours, ref)])
        rec['op'] = timed(lambda: F.mix_rbf_sums(x, y, SIGMAS), a.repeat)
        rec['torch_chunk%d' % a.chunk] = timed(lambda: torch_sums(x, y), max(3, a.repeat // 2))
        L.ggan_prof_reset(); L.ggan_prof_enable(1)
        for _ in range(3):
            F.mix_rbf_sums(x, y, SIGMAS)
        torch.cuda.synchronize()
        rec['kernels_ms'] = {r['name']: r['total_ms'] / r['launches'] for r in _lib.prof_report() if r['name'].startswith('mmd_set')}
        flop = [r['flops'] / r['launches'] for r in _lib.prof_report() if r['name'] == 'mmd_set_sums'][0]
        L.ggan_prof_enable(0)
        rec['launch_flop'] = flop
        rec['tflops'] = flop / (rec['op']['median_ms'] * 1e-3) / 1e12
        rec['of_fp32_mfma_peak'] = rec['tflops'] / PEAK_TFLOPS
        out['d%d' % d] = rec
        print('d = %d: %s' % (d, json.dumps(rec)))
        del x, y
    if not a.no_pass:
        S = run.reference_block('gan_inference_cifar10')
        S.update(SYNTHETIC='force', DATA_DIR='')
        tr = Trainer(run.config(S), device=dev, graph=False)
        ev = Evaluator(tr, S)
        dset, _ = run.eval_sets(S, tr.model, dev)
        res = dict(rows=len(dset) * S['BATCH_SIZE'])
        for name, fn in (('dev_costs', lambda: ev.dev_costs(dset)), ('mmd_scores', lambda: ev.mmd_scores(dset))):
            fn(); fn()
            ts = []
            for _ in range(5):
                torch.cuda.synchronize(); t0 = time.time(); fn(); torch.cuda.synchronize(); ts.append((time.time() - t0) * 1e3)
            res[name + '_ms'] = dict(median=float(np.median(ts)), all=ts)
        out['pass'] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
