#!/usr/bin/env python
"""Record what the reference's gmgan scripts do under the straight-through MODE_K values (BUILD CONTAINER ONLY, as
make_reference_trace.py, whose run_script / trace_case this reuses with one more source patch, `MODE_K = ...`):

  tests/golden/reference_trace_mode_k.json    '<script>:<MODE>:<MODE_K>' -> the part of the trace_case record the replay reads
                                              (session.run order, draws, minibatches, costs, the first step's gradient digests,
                                              the largest gradient of each tensor over the runs, FINAL_SAMPLES entries of the
                                              final weights, random nodes; 7 significant digits) + the argmax margins

A hard argmax that flips between the shim's float64 and the HIP path's float32 changes every gradient behind it.  So every
tf.argmax the scripts evaluate is watched: per row, the gap between the largest and the second largest entry of its input,
relative to the largest entry's magnitude.  A case whose smallest gap is below MARGIN_BOUND is refused, not committed.

  python tests/golden/make_mode_k_trace.py [--only gmgan_inference_mnist:local_ep:STRAIGHT_THROUGHT_CONCRETE]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_trace as MRT            # noqa: E402

shim, tp = MRT.shim, MRT.shim.tp

STC, ST = 'STRAIGHT_THROUGHT_CONCRETE', 'STRAIGHT_THROUGHT'
MARGIN_BOUND = 1e-3             # smallest relative top-two gap of an argmax input a committed case may have
FINAL_SAMPLES = 4               # entries kept per final weight tensor (the first 4 of reftrace's 64 positions: the same draws)
SMALL_GM = dict(MRT.SMALL_IMG, N_COMS=5)
CASES = [
    ('gmgan_inference_mnist', 'local_ep', STC, SMALL_GM), ('gmgan_inference_cifar10', 'local_epce', STC, SMALL_GM),
    ('gmgan_inference_cifar10', 'local_ep', ST, SMALL_GM),
    # (svhn at DIM 8: the first run's argmax has a relative gap of 7.6e-4, below MARGIN_BOUND -- refused; at DIM 16 the smallest is 4.3e-3)
    ('gmgan_inference_svhn', 'local_ep', ST, dict(SMALL_GM, DIM=16)),
]


class MarginWatch(object):
    """shim.argmax with a record of the top-two gaps of every input it evaluates while a session runs"""

    def __init__(self):
        self.on, self.gaps, self.calls = False, [], 0

    def install(self):
        watch = self

        def argmax(x, axis=None, name=None, dimension=None):
            ax = axis if axis is not None else dimension

            def f(a):
                v = np.asarray(a.v, np.float64)
                if watch.on and v.ndim == 2 and v.shape[-1] > 1 and ax in (-1, 1):
                    top = np.sort(v, axis=-1)[:, ::-1]
                    gap = (top[:, 0] - top[:, 1]) / np.maximum(np.abs(top[:, 0]), 1e-30)
                    watch.gaps.append(float(gap.min()))
                    watch.calls += 1
                return tp.T(np.argmax(a.v, axis=ax))
            return shim._op(f, x)
        shim.argmax = argmax

    def reset(self):
        self.on, self.gaps, self.calls = False, [], 0


def _g(x):
    return float('%.7g' % x)


def slim(rec):
    """only what the replay reads, one column per weight tensor (`names`, sorted): its shape, the gradient digest of the first training
    run (None: no gradient), the largest |gradient| over all runs (None: never one), FINAL_SAMPLES entries of the final weights.  No critic logits, feed
    digests or optimizer records."""
    names = sorted(rec['params'])
    runs, first, gmax = [], None, dict.fromkeys(names)
    for r in rec['runs']:
        for t in r['train']:
            for n, d in t['grads'].items():
                if d is not None:
                    gmax[n] = max(gmax[n] or 0.0, _g(d[1]))
        if r['train'] and first is None:
            first = [None if r['train'][0]['grads'].get(n) is None else [_g(v) for v in r['train'][0]['grads'][n]] for n in names]
        runs.append(dict(run=r['run'], draws=r['draws'], feeds=[{k: f[k] for k in ('placeholder', 'stream', 'index', 'spec')} for f in r['feeds']],
                         train=[dict(optimizer=t['optimizer'], cost=_g(t['cost'])) for t in r['train']]))
    keep = ('constants', 'script_constants', 'critic_iters', 'random_nodes')
    return dict({k: rec[k] for k in keep}, names=names, shapes=[rec['params'][n] for n in names], runs=runs, first_grads=first,
                gmax=[gmax[n] for n in names], final=[[_g(v) for v in rec['final'][n][:2 + FINAL_SAMPLES]] for n in names],
                final_samples=FINAL_SAMPLES)


def trace_mode_k(script, mode, mode_k, extra, watch):
    watch.reset()
    orig = shim.Session.run

    def run(sess, *a, **k):                    # (argmax inputs of session.run only: not the static shapes of graph building)
        watch.on = True
        try:
            return orig(sess, *a, **k)
        finally:
            watch.on = False
    shim.Session.run = run
    try:
        rec = MRT.trace_case(script, mode, dict(extra, MODE_K=mode_k))
    finally:
        shim.Session.run = orig
    if not watch.calls:
        raise SystemExit('%s:%s:%s: no argmax was evaluated -- is MODE_K patched?' % (script, mode, mode_k))
    margin = min(watch.gaps)
    if margin < MARGIN_BOUND:
        raise SystemExit('%s:%s:%s: an argmax input has a top-two gap of %.3g (relative) < %g: float32 may pick another index'
                         % (script, mode, mode_k, margin, MARGIN_BOUND))
    rec = slim(rec)
    rec.update(mode_k=mode_k, argmax_margin=_g(margin), argmax_calls=watch.calls, margin_bound=MARGIN_BOUND)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='script:MODE:MODE_K[,...]')
    args = ap.parse_args()
    if not os.path.isdir(MRT.REF):
        raise SystemExit('%s is not here: this generator runs in the build container only' % MRT.REF)
    MRT.install()
    watch = MarginWatch()
    watch.install()
    want = set(args.only.split(',')) if args.only else None
    path = os.path.join(HERE, 'reference_trace_mode_k.json')
    traces = json.load(open(path)) if (want and os.path.exists(path)) else {}
    for script, mode, mode_k, extra in CASES:
        key = '%s:%s:%s' % (script, mode, mode_k)
        if want and key not in want:
            continue
        traces[key] = trace_mode_k(script, mode, mode_k, extra, watch)
        sys.stderr.write('[trace] %-60s %d runs, margin %.3g over %d argmax\n'
                         % (key, len(traces[key]['runs']), traces[key]['argmax_margin'], traces[key]['argmax_calls']))
    json.dump(traces, open(path, 'w'), sort_keys=True, separators=(',', ':'))


if __name__ == '__main__':
    main()
