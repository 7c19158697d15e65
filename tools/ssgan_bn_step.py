#!/usr/bin/env python
"""Time the captured state-space step (one iteration = critic step + generator step, one graph replay each) with BatchNorm off and
on (BN_FLAG of ssgan_inference_moving_mnist.py), at B 32, LEN 16, DIM 32 on synthetic sequences.  One JSON line per variant.

  python tools/ssgan_bn_step.py [--modes local_ep,ali:3dcnn] [--steps 30] [--warmup 5] [--bn off,on]
  python tools/ssgan_bn_step.py --kernels      (the existing rows kernels and the row-grouped pair alone on 65 536 x 64)

Under `rocprofv3 --kernel-trace --stats -- python tools/ssgan_bn_step.py ...` the per-launch times of bn_sp_* (the row-grouped
kernels) land in the stats table."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(mode, ali_mode, bn, steps, warmup, B=32, L=16, dim=32):
    import numpy as np
    import torch
    from graphical_gan_amd import tflib as lib, optim
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    optim.reset_optimizers()
    lib.delete_all_params()
    np.random.seed(0)
    dev = torch.device('cuda')
    cfg = SSConfig(batch_size=B, length=L, dim=dim, mode=mode, ali_mode=ali_mode, bn_g=bn, bn_e=bn, bn_d=bn)
    tr = Trainer(cfg, device=dev, graph=True, seed=4321, model=StateSpaceGAN(cfg))
    ring = tr.model.synthetic_ring(dev)
    feeds = iter(ring * (steps + warmup + 2))
    for it in range(warmup):
        tr.iteration(it, feeds)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for it in range(warmup, warmup + steps):
        res = tr.iteration(it, feeds)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    return dict(mode=mode, ali_mode=ali_mode, bn=bn, B=B, LEN=L, DIM=dim, step_ms=round(ms, 4),
                gen_cost=float(res.get('gen_cost', float('nan'))), disc_cost=float(res.get('disc_cost', float('nan'))))


def kernels(reps=50):
    """the 3dcnn critic's BN2 at full size ([fake; real] = 65 536 rows x 64 channels): the existing rows kernels (one workgroup per 32
    channels, no groups) against the row-grouped pair (groups = 2), forward and backward, microseconds per call (HIP events)"""
    import torch
    from graphical_gan_amd._lib import check
    from graphical_gan_amd.functional._core import _L, _p, _stream, workspace
    dev = torch.device('cuda')
    R, C = 65536, 64
    x, gy = torch.randn(R, C, device=dev), torch.randn(R, C, device=dev)
    sc, of = torch.rand(C, device=dev) + .5, torch.randn(C, device=dev)
    y, gx = torch.empty_like(x), torch.empty_like(x)
    m, v = torch.empty(2, C, device=dev), torch.empty(2, C, device=dev)
    gs, go = torch.empty(C, device=dev), torch.empty(C, device=dev)
    L, ws = _L(), workspace(dev)
    calls = {
        'bn_fwd_rows (existing)': lambda: check(L.ggan_bn_fwd_train(_p(x), _p(sc), _p(of), _p(y), _p(m), _p(v), R, C, 1, 1e-5, 1, 0.2,
                                                                    _stream()), 'fwd'),
        'bn_bwd_rows (existing)': lambda: check(L.ggan_bn_bwd_act(_p(x), _p(gy), _p(y), 1, 0.2, _p(sc), _p(m), _p(v), _p(gx), _p(gs),
                                                                  _p(go), _p(None), R, C, 1, _stream()), 'bwd'),
        'bn_split_fwd_train (groups 2)': lambda: check(L.ggan_bn_split_fwd_train(_p(x), _p(sc), _p(of), _p(y), _p(m), _p(v), R, C, 1, 2,
                                                                                 1e-5, 1, 0.2, _p(ws), ws.numel(), _stream()), 'sfwd'),
        'bn_split_bwd_act (groups 2)': lambda: check(L.ggan_bn_split_bwd_act(_p(x), _p(gy), 1, 0.2, _p(sc), _p(of), _p(m), _p(v), _p(gx),
                                                                             _p(gs), _p(go), _p(None), R, C, 1, 2, 2, _p(ws), ws.numel(),
                                                                             _stream()), 'sbwd'),
    }
    for name, f in calls.items():
        for _ in range(5):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        print(json.dumps(dict(kernel=name, rows=R, channels=C, us=round(1e3 * e0.elapsed_time(e1) / reps, 2))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--modes', default='local_ep,ali:3dcnn')
    ap.add_argument('--bn', default='off,on')
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--kernels', action='store_true', help='time the BatchNorm kernels alone on the 65 536 x 64 shape instead')
    a = ap.parse_args()
    if a.kernels:
        kernels()
        return
    for m in a.modes.split(','):
        mode, _, ali = m.partition(':')
        for bn in a.bn.split(','):
            print(json.dumps(measure(mode, ali or 'concat_x', bn == 'on', a.steps, a.warmup)), flush=True)


if __name__ == '__main__':
    main()
