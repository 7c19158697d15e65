#!/usr/bin/env python
"""Record what the reference's gmgan scripts do under their global-critic MODEs (BUILD CONTAINER ONLY, as make_reference_trace.py,
whose trace_case this reuses unchanged, and make_mode_k_trace.py, whose slim / trace_mode_k it reuses):

  tests/golden/reference_trace_gmgan_global.json    '<script>:<MODE>[:<MODE_K>]' -> the slimmed trace_case record (session.run order,
                                                    draws, minibatches, costs, the first step's gradient digests, the largest gradient
                                                    of each tensor, FINAL_SAMPLES entries of the final weights, random nodes)

MODE ali / alice: one joint critic Discriminator(x, z, k) (gmgan_inference_cifar10.py:306-336,376-398); MODE vegan: Discriminator(z, k)
on codes only (:233-251,359-361,405-407).  The CONCRETE cases evaluate no argmax; the STRAIGHT_THROUGHT case goes through
trace_mode_k and its argmax-margin rule.

  python tests/golden/make_gmgan_global_trace.py [--only gmgan_inference_mnist:vegan]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_trace as MRT            # noqa: E402
import make_mode_k_trace as MK                # noqa: E402

SMALL_GM = dict(MRT.SMALL_IMG, N_COMS=5)
SMALL_GM_FACE = dict(MRT.SMALL_FACE, N_COMS=5)
CASES = [
    ('gmgan_inference_cifar10', 'ali', None, SMALL_GM), ('gmgan_inference_cifar10', 'alice', None, SMALL_GM),
    ('gmgan_inference_cifar10', 'vegan', None, SMALL_GM),
    ('gmgan_inference_mnist', 'ali', None, SMALL_GM), ('gmgan_inference_mnist', 'vegan', None, SMALL_GM),
    ('gmgan_inference_svhn', 'alice', None, SMALL_GM),
    ('gmgan_inference_face', 'ali', None, SMALL_GM_FACE),
    ('gmgan_inference_cifar10', 'ali', MK.ST, SMALL_GM),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='script:MODE[:MODE_K][,...]')
    args = ap.parse_args()
    if not os.path.isdir(MRT.REF):
        raise SystemExit('%s is not here: this generator runs in the build container only' % MRT.REF)
    MRT.install()
    watch = MK.MarginWatch()
    watch.install()
    want = set(args.only.split(',')) if args.only else None
    path = os.path.join(HERE, 'reference_trace_gmgan_global.json')
    traces = json.load(open(path)) if (want and os.path.exists(path)) else {}
    for script, mode, mode_k, extra in CASES:
        key = '%s:%s' % (script, mode) + (':' + mode_k if mode_k else '')
        if want and key not in want:
            continue
        if mode_k:
            traces[key] = MK.trace_mode_k(script, mode, mode_k, extra, watch)
            sys.stderr.write('[trace] %-55s %d runs, margin %.3g over %d argmax\n'
                             % (key, len(traces[key]['runs']), traces[key]['argmax_margin'], traces[key]['argmax_calls']))
        else:
            traces[key] = dict(MK.slim(MRT.trace_case(script, mode, extra)), mode_k='CONCRETE')
            sys.stderr.write('[trace] %-55s %d runs\n' % (key, len(traces[key]['runs'])))
    json.dump(traces, open(path, 'w'), sort_keys=True, separators=(',', ':'))


if __name__ == '__main__':
    main()
