"""Writes tests/golden/tsne_reference.json and tsne_reference_bh.npy: what scikit-learn's TSNE (the reference's TSNE().fit_transform,
gmgan_inference_mnist.py:545) and the float64 restatement tests/_tsne_ref.py compute on the recipe's inputs.  Needs scikit-learn; run
from the repository root: python tests/golden/make_tsne_fixture.py   (about ten minutes)"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import _tsne_ref as R  # noqa: E402

RECIPE = dict(seed=0, clusters=10, dim=32, per_cluster=120, centre_scale=3.0)
SEEDS = (0, 1, 2)
PREFIX_ITERS = (1, 5, 10)       # (by iteration 50 a change of 1e-16 in P has grown to 1e-6 of the extent: too sensitive to pin)
PREFIX_POINTS = 50


def main():
    import sklearn
    from sklearn.manifold import TSNE
    X, y = R.fixture_inputs(RECIPE)
    P = R.sparse_P(X, 30.)
    out = dict(recipe=RECIPE, sklearn=sklearn.__version__, perplexity=30., seeds=list(SEEDS), runs=[], restatement=[],
               prefix_iters=list(PREFIX_ITERS), prefix_points=PREFIX_POINTS)
    bh = np.zeros((len(SEEDS), len(X), 2), np.float32)
    for method in ('exact', 'barnes_hut'):
        for k, seed in enumerate(SEEDS):
            ts = TSNE(method=method, init='random', learning_rate=200., perplexity=30., early_exaggeration=12., max_iter=1000, random_state=seed)
            Y = ts.fit_transform(X)
            if method == 'barnes_hut':
                bh[k] = Y
            run = dict(method=method, seed=seed, kl_divergence_=float(ts.kl_divergence_), n_iter_=int(ts.n_iter_),
                       purity=R.purity(Y, y), kl_s=R.kl_sparse(P, Y.astype(np.float32)))
            print(run, flush=True)
            out['runs'].append(run)
    for seed in SEEDS:
        Y, kept = R.run(P, R.initial(len(X), seed), 1000, keep=PREFIX_ITERS)
        rec = dict(seed=seed, kl_s=R.kl_sparse(P, Y), purity=R.purity(Y, y),
                   prefix={str(it): kept[it][:PREFIX_POINTS].tolist() for it in PREFIX_ITERS},
                   extent={str(it): float(np.abs(kept[it]).max()) for it in PREFIX_ITERS})
        print({k: v for k, v in rec.items() if k != 'prefix'}, flush=True)
        out['restatement'].append(rec)
    np.save(os.path.join(HERE, 'tsne_reference_bh.npy'), bh)
    with open(os.path.join(HERE, 'tsne_reference.json'), 'w') as f:
        json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
