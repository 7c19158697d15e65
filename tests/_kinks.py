"""Near-kink bookkeeping shared by the step tests (tests/test_step_gpu.py, tests/test_second_order_gpu.py)."""
import numpy as np


def _kink_samples(log, margin=1e-5):
    """(layer call, row) pairs whose Linear-layer ReLU / LeakyReLU inputs come within `margin` (relative to the row's rms) of zero
    in the float64 oracle forward pass (oracle.tape.KINK_LOG): the places where an fp32 evaluation can legitimately take the other
    branch for a unit that carries a macroscopic share of a weight-gradient entry"""
    rows = []
    for i, x in enumerate(log):
        rms = np.sqrt((x ** 2).mean(1, keepdims=True)) + 1e-30
        rows += [(i, int(r)) for r in np.nonzero((np.abs(x) / rms).min(1) < margin)[0]]
    return rows
