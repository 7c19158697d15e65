"""Wall time of functional.tsne on an MI355X, split into its stages, for docs/KERNELS.md ("t-SNE").

  python tools/tsne_time.py [--n 10000] [--dims 128 784] [--repeat 3] [--iters 1000] [--sklearn] [--prof]

Every shape is warmed once, then each stage is timed `--repeat` times by a host clock around work that ends in a device synchronise;
all repeats are printed so that the spread is seen beside the figure.  Pair counts and FLOP come from the shapes: the repulsive kernel
touches N^2 pairs per iteration at 12 float operations each (3 subtract / 2 multiply-add for the distance, 1 add, the reciprocal counted
as 1, 1 multiply, 1 add and 2 multiply-adds into the accumulators).  --sklearn: TSNE() of scikit-learn on the same data, where it is
importable, on the CPUs the process may use.  --prof: libggan's own per-kernel timers around one run (they serialise the launches, so
the sum of the kernel times against the unprofiled wall time of the loop gives the share of launch gaps).  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--dims', type=int, nargs='+', default=[128, 784])
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--iters', type=int, default=1000)
    ap.add_argument('--sklearn', action='store_true')
    ap.add_argument('--prof', action='store_true')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('tsne_time: no GPU -- nothing is measured')
    from graphical_gan_amd import _lib
    from graphical_gan_amd import functional as F
    dev = torch.device('cuda')
    sync = lambda: torch.cuda.synchronize(dev)
    N, K, perp = a.n, 90, 30.
    out = dict(N=N, iters=a.iters, splits=F.tsne_splits(N), device=torch.cuda.get_device_name(0), shapes=[])

    def clock(fn):
        sync()
        t = time.time()
        r = fn()
        sync()
        return r, time.time() - t

    for D in a.dims:
        rng = np.random.RandomState(D)
        centres = 3.0 * rng.normal(size=(10, D))
        Xh = (centres[rng.randint(0, 10, size=N)] + rng.normal(size=(N, D))).astype(np.float32)
        X = torch.as_tensor(Xh).to(dev)
        y0 = torch.as_tensor((1e-4 * np.random.RandomState(0).standard_normal((N, 2))).astype(np.float32)).to(dev)

        def loop(P):
            Y = y0.clone()
            return F.tsne_step(P, Y, torch.zeros_like(Y), torch.ones_like(Y), 0, a.iters)

        rec = dict(D=D, neighbours_s=[], affinities_s=[], loop_s=[], total_s=[])
        for rep in range(a.repeat + 1):                 # (the first round warms every shape and is not reported)
            (idx, dist), t_n = clock(lambda: F.tsne_neighbours(X, K))
            P, t_a = clock(lambda: F.tsne_symmetrise(idx, F.tsne_affinities(dist, perp)[0]))
            Y, t_l = clock(lambda: loop(P))
            _, t_all = clock(lambda: F.tsne(X, n_iter=a.iters))
            if rep:
                rec['neighbours_s'].append(t_n); rec['affinities_s'].append(t_a); rec['loop_s'].append(t_l); rec['total_s'].append(t_all)
        assert bool(torch.isfinite(Y).all())
        best = min(rec['loop_s'])
        rec['pairs_per_iter'] = float(N) * N
        rec['repulse_gflops_if_loop_were_all_repulse'] = 12.0 * N * N * a.iters / best * 1e-9
        rec['neighbour_gemm_tflops'] = 2.0 * N * N * D / min(rec['neighbours_s']) * 1e-12
        if a.prof:
            L = _lib.load()
            L.ggan_prof_reset(); L.ggan_prof_enable(1)
            _, t_p = clock(lambda: F.tsne(X, n_iter=a.iters))
            L.ggan_prof_enable(0)
            kern = {}
            for r in _lib.prof_report():
                k = kern.setdefault(r['name'], dict(ms=0.0, launches=0))
                k['ms'] += r['total_ms']; k['launches'] += r['launches']
            rec['prof'] = dict(wall_s=t_p, kernels=kern)
            rep_ms, step_ms = kern.get('tsne_repulse', {}).get('ms', 0.0), kern.get('tsne_step', {}).get('ms', 0.0)
            rec['loop_kernel_s'] = (rep_ms + step_ms) * 1e-3
            rec['loop_gap_share'] = 1.0 - rec['loop_kernel_s'] / best
            if rep_ms:
                rec['repulse_gflops'] = 12.0 * N * N * kern['tsne_repulse']['launches'] / (rep_ms * 1e-3) * 1e-9
        if a.sklearn:
            try:
                from sklearn.manifold import TSNE
                t = time.time()
                TSNE().fit_transform(Xh)
                rec['sklearn_s'] = time.time() - t
            except ImportError:
                rec['sklearn_s'] = None
        print(json.dumps(rec), flush=True)
        out['shapes'].append(rec)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
