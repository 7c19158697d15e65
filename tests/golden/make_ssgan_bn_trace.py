#!/usr/bin/env python
"""Record what the reference's state-space scripts do with BN_FLAG = True (BUILD CONTAINER ONLY, as make_reference_trace.py,
whose run_script / trace_case this reuses with one more source patch, `BN_FLAG = True`; BN_FLAG_G / _E / _D follow it):

  tests/golden/reference_trace_ssgan_bn.json   '<script>:<MODE>[:<ALI_MODE>]' -> the part of the trace_case record the replay reads
                                               (make_mode_k_trace.slim: session.run order, draws, minibatches, costs, the first
                                               step's gradient digests, the largest gradient of each tensor over the runs,
                                               FINAL_SAMPLES entries of the final weights, random nodes; 7 significant digits) +
                                               the parameters the non-fused [0,1,2,3] BatchNorm branch created

  python tests/golden/make_ssgan_bn_trace.py [--only ssgan_inference_moving_mnist:ali:3dcnn]
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_trace as MRT            # noqa: E402
import make_mode_k_trace as MKT               # noqa: E402

SMALL_MM = dict(DIM=4, DIM_OP=16, BATCH_SIZE=10, LEN=4, ITERS=2)      # (moving_mnist: BATCH_SIZE a multiple of N_C = 10)
SMALL_CH = dict(DIM=4, DIM_OP=16, BATCH_SIZE=2, LEN=3, ITERS=2)
CASES = [
    ('ssgan_inference_moving_mnist', 'local_ep', None, SMALL_MM),
    ('ssgan_inference_moving_mnist', 'local_epce-z', None, SMALL_MM),
    ('ssgan_inference_moving_mnist', 'ali', '3dcnn', SMALL_MM),
    ('ssgan_inference_moving_mnist', 'ali', 'concat_x', SMALL_MM),
    ('ssgan_inference_moving_mnist', 'alice-z', 'concat_z', SMALL_MM),
    ('ssgan_inference_chairs', 'local_ep', None, SMALL_CH),
]


def trace_bn(script, mode, ali_mode, extra):
    consts = dict(extra, BN_FLAG=True)
    if ali_mode is not None:
        consts['ALI_MODE'] = ali_mode
    rec = MRT.trace_case(script, mode, consts)
    # the [0,1,2,3] branch (tf.nn.moments + tf.nn.batch_normalization) creates offset / scale only
    no_moving = sorted(n for n in rec['params'] if '.BN' in n and len(rec['params'][n]) == 5)
    out = MKT.slim(rec)
    out.update(bn_5d=no_moving, ali_mode=ali_mode)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default=None, help='script:MODE[:ALI_MODE][,...]')
    args = ap.parse_args()
    if not os.path.isdir(MRT.REF):
        raise SystemExit('%s is not here: this generator runs in the build container only' % MRT.REF)
    MRT.install()
    want = set(args.only.split(',')) if args.only else None
    path = os.path.join(HERE, 'reference_trace_ssgan_bn.json')
    traces = json.load(open(path)) if (want and os.path.exists(path)) else {}
    for script, mode, ali_mode, extra in CASES:
        key = '%s:%s' % (script, mode) + (':%s' % ali_mode if ali_mode else '')
        if want and key not in want:
            continue
        traces[key] = trace_bn(script, mode, ali_mode, extra)
        sys.stderr.write('[trace] %-60s %d runs, %d parameters\n' % (key, len(traces[key]['runs']), len(traces[key]['names'])))
    json.dump(traces, open(path, 'w'), sort_keys=True, separators=(',', ':'))


if __name__ == '__main__':
    main()
