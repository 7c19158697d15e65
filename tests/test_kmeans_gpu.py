"""gpu: the k-means kernels against the float64 restatement tests/_kmeans_ref.py -- the assignment under the derived float32 Gram bound and
exactly on the integer lattice, ghost rows and limits, the seeding, the update, the fit, non-finite rows as a status, the bin test and the
clustering scores --, and the pass Evaluator.kmeans_scores on a tiny evaluator."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmeans_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a)).to(dev)


def _bits(*tensors):
    return b''.join(t.cpu().numpy().tobytes() for t in tensors)


def _odd(a, dev):
    """the same values as a contiguous view that starts one element into its buffer: the base is not 16-byte aligned"""
    import torch
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(*a.shape)
    v.copy_(_t(a, dev))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _wide(a, dev):
    """the same values as the leading columns of a wider parent array: not contiguous"""
    import torch
    parent = torch.full((a.shape[0], a.shape[1] + 3), 7.0, dtype=torch.float32, device=dev)
    parent[:, :a.shape[1]].copy_(_t(a, dev))
    v = parent[:, :a.shape[1]]
    assert not v.is_contiguous() or a.shape[0] == 1
    return v


# ---- 1. assign against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lloyd', (0, 3))
@pytest.mark.parametrize('d,k', R.ASSIGN_CASES)
def test_assign_against_float64(gpu, d, k, lloyd):
    """every row whose float64 gap between its two nearest centres exceeds 2 T_i (T_i = max_j (2 d + 4) u (|x|^2 + |c|^2), the derived float32
    Gram bound) has the float64 argmin; every distance is within T_i; the inertia is the fp64 sum of the device's own distances to 1e-12; at
    most 5 % of the rows may be ambiguous; views at an odd offset and of a wide parent give the bits of the contiguous call"""
    from graphical_gan_amd import functional as F
    X, C, D, T = R.assign_case(d, k, lloyd)
    ref = np.argmin(D, axis=1)
    amb = R.ambiguous(D, T)
    xd, cd = _t(X, gpu), _t(C, gpu)
    a, dist, inertia, moved, st = F.kmeans_assign(xd, cd)
    base = _bits(a, dist, inertia, moved, st)
    assert base == _bits(*F.kmeans_assign(xd, cd))
    assert base == _bits(*F.kmeans_assign(_odd(X, gpu), _odd(C, gpu)))
    assert base == _bits(*F.kmeans_assign(_wide(X, gpu), _wide(C, gpu)))
    an, dn = a.cpu().numpy(), dist.cpu().numpy().astype(np.float64)
    err = np.abs(dn - D.min(axis=1))
    dev_sum = math.fsum(dn.tolist())
    print('d %d k %d lloyd %d: ambiguous %.4f, wrong among the rest %d, distance error %.3e of its bound, inertia %.3e relative'
          % (d, k, lloyd, amb.mean(), int(np.sum(an[~amb] != ref[~amb])), float(np.max(err / T)), abs(float(inertia.item()) - dev_sum) / dev_sum))
    assert amb.mean() <= R.AMBIGUOUS_CAP
    assert str(a.dtype) == 'torch.int32' and int(st.item()) == 0 and int(moved.item()) == X.shape[0]
    assert an.min() >= 0 and an.max() < k
    assert np.array_equal(an[~amb], ref[~amb])
    assert np.all(err <= T)
    assert abs(float(inertia.item()) - dev_sum) <= 1e-12 * dev_sum


# ---- 2. assign on the integer lattice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', (3, 128))
def test_assign_on_the_integer_lattice_is_exact_ties_included(gpu, d):
    from graphical_gan_amd import functional as F
    X, C = R.lattice(257, 37, d)
    X, C = X.copy(), C.copy()
    C[3], C[33] = C[29], C[7]                     # duplicated centres, planted at a lower and at a higher index
    X[0], X[1], X[100] = C[29], C[7], C[3]
    D = R.d2(X, C)
    ref, rd = R.assign(X, C, D)
    ties = int(np.sum(np.sum(D == D.min(axis=1, keepdims=True), axis=1) > 1))
    assert ties >= 1
    a, dist, inertia, _, st = F.kmeans_assign(_t(X, gpu), _t(C, gpu))
    assert np.array_equal(a.cpu().numpy(), ref) and np.array_equal(dist.cpu().numpy().astype(np.float64), rd)
    assert float(inertia.item()) == float(rd.sum()) and int(st.item()) == 0
    assert ref[0] == 3 and ref[1] == 7 and ref[100] == 3          # the lower of the two equal centres


# ---- 3. ghost rows and limits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', (1, 2, 127, 128))
def test_ghost_rows_never_win_and_short_sets_are_legal(gpu, k):
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(k)
    for n in (1, 127, 128, 129, 257):
        X, C = rng.integers(0, 4, size=(n, 6)).astype(np.float32), (rng.integers(0, 4, size=(k, 6)) + 5).astype(np.float32)
        # every centre is farther from every row than the origin is: a ghost candidate row (zeros, norm 0) that took part would win
        ref, rd = R.assign(X, C)
        a, dist, _, _, st = F.kmeans_assign(_t(X, gpu), _t(C, gpu))
        an = a.cpu().numpy()
        assert an.min() >= 0 and an.max() < k and int(st.item()) == 0, (n, k)
        assert np.array_equal(an, ref) and np.array_equal(dist.cpu().numpy().astype(np.float64), rd), (n, k)
        u = rng.random(k)
        cen, idx = F.kmeans_seed(_t(X, gpu), k, u)          # n < k: repetition only where the total is 0
        ridx, rrows = R.seed(X, k, u)
        assert np.array_equal(idx.cpu().numpy(), ridx) and np.array_equal(cen.cpu().numpy().astype(np.float64), rrows), (n, k)


# ---- 4. seed ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', (3, 128))
def test_seeding_on_the_lattice_equals_the_restatement(gpu, d):
    from graphical_gan_amd import functional as F
    X = R.lattice(300, 1, d)[0]
    xd = _t(X, gpu)
    for k in (1, 8, 37):
        u = np.random.RandomState(100 * d + k).rand(k)
        cen, idx = F.kmeans_seed(xd, k, u)
        ridx, rrows = R.seed(X, k, u)
        assert np.array_equal(idx.cpu().numpy(), ridx), (d, k)
        assert np.array_equal(cen.cpu().numpy().astype(np.float64), rrows), (d, k)
        assert _bits(cen, idx) == _bits(*F.kmeans_seed(xd, k, u))


def test_seeding_of_equal_rows_and_the_pick_alone(gpu):
    from graphical_gan_amd import functional as F
    u = np.random.RandomState(5).rand(9)
    _, idx = F.kmeans_seed(_t(np.full((50, 7), 1.5, np.float32), gpu), 9, u)
    assert np.array_equal(idx.cpu().numpy(), np.floor(u * 50).astype(np.int64))            # the total == 0 rule
    rng = np.random.default_rng(11)
    mind = rng.random(20001).astype(np.float32)
    mind[rng.random(20001) < 0.3] = 0.0
    mind[:7] = 0.0
    mind[7], mind[12345], mind[20000] = 1e-40, 1e6, 0.0          # a denormal, one huge value, a trailing zero
    assert 0 < mind[7] < np.finfo(np.float32).tiny
    run = np.cumsum(mind.astype(np.float64))
    total = run[-1]
    cands = [0.5 / total, 1e-4, 0.003, 0.0065, 0.2, 0.5, 0.999, 0.9999995] + list(np.random.RandomState(3).rand(12) * 0.0066)
    used = [float(v) for v in cands if np.min(np.abs(v * total - run)) > 1e-9 * total]
    assert len(used) >= 12
    md = _t(mind, gpu)
    picks = [int(F.kmeans_pick(md, v).item()) for v in used]
    assert picks == [R.pick(mind, v) for v in used]
    assert 12345 in picks and min(picks) < 12345


# ---- 5. update against float64 -------------------------------------------------------------------------------------------------------------
def _check_update(F, gpu, X, a, C, ident):
    xd, ad, cd = _t(X, gpu), _t(np.asarray(a, np.int32), gpu), _t(C, gpu)
    keep = cd.clone()
    new, counts = F.kmeans_update(xd, ad, cd)
    assert _bits(new, counts) == _bits(*F.kmeans_update(xd, ad, cd)) and _bits(cd) == _bits(keep), ident
    rc, rcounts = R.update(X, a, C)
    assert np.array_equal(counts.cpu().numpy(), rcounts), ident
    nn = new.cpu().numpy()
    empty = rcounts == 0
    assert nn[empty].tobytes() == np.asarray(C)[empty].tobytes(), ident
    bound = (R.ROW_BLOCK - 1) * R.U * float(np.max(np.abs(X)))
    err = float(np.max(np.abs(nn.astype(np.float64) - rc)))
    print('%s: largest centre error %.3e, bound %.3e' % (ident, err, bound))
    assert err <= bound, ident


@pytest.mark.parametrize('d,k', R.ASSIGN_CASES)
def test_update_against_float64(gpu, d, k):
    """counts exact; an empty cluster's centre bit-identical to its input; every element within (KMEANS_ROW_BLOCK - 1) u max|x| of the float64
    mean -- derived: a block partial is an fp32 sum of at most that many members, the rest is fp64 --; two calls give the same bits"""
    from graphical_gan_amd import functional as F
    assert F.KMEANS_ROW_BLOCK == R.ROW_BLOCK
    X, C, D, _ = R.assign_case(d, k, 0)
    a = np.argmin(D, axis=1)
    _check_update(F, gpu, X, a, C, 'd %d k %d' % (d, k))
    _check_update(F, gpu, X, np.full(len(a), k // 2), C, 'd %d k %d, one cluster' % (d, k))
    _check_update(F, gpu, X, a % 3, C, 'd %d k %d, empty clusters' % (d, k))


@pytest.mark.parametrize('d', (1, 127, 3072))
def test_update_at_the_row_block_boundaries(gpu, d):
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(d)
    for n in (1, R.ROW_BLOCK - 1, R.ROW_BLOCK + 1):
        X = rng.standard_normal((n, d)).astype(np.float32)
        C = rng.standard_normal((5, d)).astype(np.float32)
        _check_update(F, gpu, X, rng.integers(0, 4, size=n), C, 'n %d d %d' % (n, d))


# ---- 6. fit -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('d', (16, 784))
def test_fit_of_separated_blobs_gives_the_partition_of_the_restatement(gpu, d):
    """both start from one seeding (the device's); which optimum Lloyd reaches is its own business: the assertion is equality with the
    float64 restatement, not recovery of the blobs"""
    from graphical_gan_amd import functional as F
    for s in range(5):
        rng = np.random.default_rng(1000 * d + s)
        cen = rng.standard_normal((8, d))
        X = (np.repeat(cen, 50, axis=0) + 0.05 * rng.standard_normal((400, d)))[rng.permutation(400)].astype(np.float32)
        fit = F.kmeans_fit(_t(X, gpu), 8, 6, rng.random(8))
        ref = R.fit(X, 8, 6, idx=fit.idx.cpu().numpy())
        assert int(fit.status.item()) == 0
        assert np.array_equal(fit.assign.cpu().numpy(), ref['assign']), (d, s)
        assert np.array_equal(fit.counts.cpu().numpy(), ref['counts']), (d, s)
        assert np.allclose(fit.inertia.cpu().numpy(), ref['inertia'], rtol=1e-3)


def test_fit_on_case_data_descends_converges_and_repeats(gpu):
    from graphical_gan_amd import functional as F
    X = R.case(1000, 67, 128)[0]
    xd, u = _t(X, gpu), np.random.RandomState(1).rand(37)
    fit = F.kmeans_fit(xd, 37, 20, u)
    assert _bits(*fit) == _bits(*F.kmeans_fit(xd, 37, 20, u))
    inertia, moved = fit.inertia.cpu().numpy(), fit.moved.cpu().numpy()
    # a centre is a row or a mean of rows, so its norm is at most the largest row's: the rows' T_i, summed
    n2 = (X.astype(np.float64) ** 2).sum(axis=1)
    slack = float(np.sum((2 * 128 + 4) * R.U * (n2 + n2.max())))
    print('inertia', inertia, 'moved', moved, 'slack', slack)
    assert moved[0] == 1000 and int(fit.status.item()) == 0
    assert np.all(inertia[1:] <= inertia[:-1] + slack)
    assert np.array_equal(fit.counts.cpu().numpy(), np.bincount(fit.assign.cpu().numpy(), minlength=37))
    still = np.nonzero(moved == 0)[0]
    if len(still):
        t0 = int(still[0])
        assert np.all(moved[t0:] == 0)
        assert _bits(F.kmeans_fit(xd, 37, t0, u).centres) == _bits(fit.centres)          # the centres stopped changing, bit for bit
    if moved[-1] == 0:
        a, _, _, mv, _ = F.kmeans_assign(xd, fit.centres, prev=fit.assign)
        new, _ = F.kmeans_update(xd, a, fit.centres)
        assert int(mv.item()) == 0 and _bits(a) == _bits(fit.assign) and _bits(new) == _bits(fit.centres)


# ---- 7. non-finite rows --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('where', ('row', 'centre'))
def test_a_non_finite_value_is_a_status_not_a_fault(gpu, where):
    import torch
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(3)
    for bad in (float('nan'), float('inf'), float('-inf')):
        X, C = rng.standard_normal((300, 20)).astype(np.float32), rng.standard_normal((5, 20)).astype(np.float32)
        (X if where == 'row' else C)[3, 11] = bad
        a, dist, inertia, moved, st = F.kmeans_assign(_t(X, gpu), _t(C, gpu))
        torch.cuda.synchronize()
        assert int(st.item()) == F.KMEANS_NONFINITE and 0 <= int(a.min().item()) and int(a.max().item()) < 5, (where, bad)
        if where == 'row':
            fit = F.kmeans_fit(_t(X, gpu), 5, 2, rng.random(5))
            assert int(fit.status.item()) == F.KMEANS_NONFINITE and 0 <= int(fit.assign.min().item()) and int(fit.assign.max().item()) < 5
    a, _, _, _, st = F.kmeans_assign(_t(rng.standard_normal((300, 20)).astype(np.float32), gpu), _t(np.ones((5, 20), np.float32), gpu))
    assert int(st.item()) == 0


# ---- 8. bin_test and cluster_scores -------------------------------------------------------------------------------------------------------
def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


@pytest.mark.parametrize('k', (1, 10, 100, 128))
def test_bin_test_and_cluster_scores_against_the_restatement(gpu, k):
    from graphical_gan_amd import functional as F
    rng = np.random.default_rng(k)
    for trial in range(3):
        p = rng.dirichlet(np.full(k, 2.0))
        q = p if trial == 0 else rng.dirichlet(np.full(k, 2.0) + 50 * p)
        ca, cb = rng.multinomial(20000, p).astype(np.int32), rng.multinomial((20000, 9984, 1)[trial], q).astype(np.int32)
        if trial == 2 and k > 1:
            ca[k // 2] = 0                                   # a 0 log 0 bin
        out = F.bin_test(_t(ca, gpu), _t(cb, gpu)).cpu().numpy()
        nd, share, js = R.bin_test(ca, cb)
        assert out[0] == nd and out[1] == share and _close(out[2], js), (k, trial, out, (nd, share, js))
    for classes in (2, 10, 32):
        for n in (1, 1000, 20001):
            y = rng.integers(0, classes, size=n).astype(np.int32)
            a = ((y + rng.integers(0, 3, size=n) * (rng.random(n) < 0.4)) % k).astype(np.int32)
            out, table, st = F.cluster_scores(_t(a, gpu), _t(y, gpu), k, classes)
            purity, nmi, rt = R.cluster_scores(a, y, k, classes)
            out = out.cpu().numpy()
            assert int(st.item()) == 0 and np.array_equal(table.cpu().numpy(), rt), (k, classes, n)
            assert _close(out[0], purity) and _close(out[1], nmi), (k, classes, n, out, purity, nmi)


def test_the_known_answers_on_the_device(gpu):
    from graphical_gan_amd import functional as F
    c = np.array([5, 0, 17, 3, 0, 40], np.int32)
    out = F.bin_test(_t(c, gpu), _t(3 * c, gpu)).cpu().numpy()
    assert out[0] == 0 and out[1] == 0 and out[2] == 0                                  # equal histograms
    out = F.bin_test(_t(np.array([4, 6, 0, 0], np.int32), gpu), _t(np.array([0, 0, 6, 4], np.int32), gpu)).cpu().numpy()
    assert out[0] == 4 and out[1] == 1.0 and _close(out[2], math.log(2.0))             # disjoint histograms
    out = F.bin_test(_t(np.array([7], np.int32), gpu), _t(np.array([9], np.int32), gpu)).cpu().numpy()
    assert out[0] == 0 and out[2] == 0                                                  # one bin: se == 0
    assert np.all(np.isnan(F.bin_test(_t(np.array([0, 0], np.int32), gpu), _t(np.array([1, 2], np.int32), gpu)).cpu().numpy()))
    y = np.arange(1200, dtype=np.int32) % 6
    out, _, st = F.cluster_scores(_t((y * 5 + 2) % 6, gpu), _t(y, gpu), 6, 6)           # a relabelling
    out = out.cpu().numpy()
    assert int(st.item()) == 0 and out[0] == 1.0 and _close(out[1], 1.0)
    i = np.arange(1200, dtype=np.int32)
    out, _, _ = F.cluster_scores(_t(i % 4, gpu), _t((i // 4) % 5, gpu), 4, 5)           # independent uniform partitions of a product grid
    assert out.cpu().numpy()[1] == 0.0 and _close(float(out.cpu().numpy()[0]), 0.2)
    out, _, st = F.cluster_scores(_t(np.zeros(9, np.int32), gpu), _t(np.zeros(9, np.int32), gpu), 1, 1)
    assert out.cpu().numpy().tolist() == [1.0, 1.0]                                     # both entropies 0
    for a, yv in ((np.array([0, 6], np.int32), np.array([0, 1], np.int32)), (np.array([0, 1], np.int32), np.array([0, -1], np.int32))):
        out, _, st = F.cluster_scores(_t(a, gpu), _t(yv, gpu), 6, 6)
        assert int(st.item()) == F.KMEANS_BAD_INDEX and np.all(np.isnan(out.cpu().numpy()))


# ---- 9. the pass, on a tiny evaluator ------------------------------------------------------------------------------------------------------
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)
from test_knn_gpu import _labelled_dev  # noqa: E402

KEYS = ['dev ndb x', 'dev ndb js x', 'dev ndb data', 'dev kmeans accuracy z', 'dev kmeans nmi z']


def _settings(B, mode, K, **more):
    return dict(dict(BATCH_SIZE=B, MODE=mode, N_COMS=K, KM_BINS=12, KM_FIT_ROWS=10 * B, KM_SAMPLES=7 * B + 3, KM_MAX_ROWS=5 * B, KM_ITERS=5), **more)


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_kmeans_scores_values_and_the_passes_it_leaves_alone(gpu, dataset, K, mode, capsys):
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 6
    tr = P._model(gpu, dataset, B, K, mode)
    both = _labelled_dev(dataset, B, 3 * n)
    fit, dev = both[:2 * n], both[2 * n:]
    S = _settings(B, mode, K)
    ev = Evaluator(tr, S)
    tr.model.sample_noise(tr.feed)
    torch.cuda.synchronize()
    before = P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']
    res, got = ev.kmeans_scores(fit, dev, return_sets=True)
    assert list(res) == KEYS and all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    assert (P._snapshot(tr.feed), np.random.get_state()[1].tobytes(), P._snapshot(ev.feed)['rng_state']) == before
    assert ev.km_fits == 1 and ev.km_z_fits == 1
    host = {k: v.cpu().numpy() for k, v in got.items()}
    kz = K if K else 4
    assert host['centres'].shape == (12, tr.cfg.output_dim) and host['centres'].min() >= 0.0 and host['centres'].max() <= 1.0
    assert host['counts_fit'].sum() == 10 * B and host['counts_x'].sum() == 7 * B and host['counts_data'].sum() == 5 * B
    assert host['moved'].shape == (6,) and host['inertia'].shape == (6,) and host['moved_z'].shape == (6,) and host['assign_z'].shape == (5 * B,)
    assert host['centres_z'].shape == (kz, tr.cfg.dim_latent)
    assert np.array_equal(host['labels'], np.concatenate([y for _, y in dev[:5]]))
    # each value is what the restatement gives from the returned sets
    _, share_x, js_x = R.bin_test(host['counts_fit'], host['counts_x'])
    _, share_d, _ = R.bin_test(host['counts_fit'], host['counts_data'])
    purity, nmi, table = R.cluster_scores(host['assign_z'], host['labels'], kz, 4)
    assert res[KEYS[0]] == share_x and _close(res[KEYS[1]], js_x) and res[KEYS[2]] == share_d
    assert _close(res[KEYS[3]], purity) and _close(res[KEYS[4]], nmi) and np.array_equal(host['table'], table)
    print(dataset, res)
    # the second firing does not refit the bins; the clusters of the codes are fitted again
    centres = got['centres'].clone()
    res2, got2 = ev.kmeans_scores(fit, dev, return_sets=True)
    assert ev.km_fits == 1 and ev.km_z_fits == 2 and got2['centres'] is got['centres'] and torch.equal(got2['centres'], centres)
    assert torch.equal(got2['counts_data'], got['counts_data']) and res2[KEYS[2]] == res[KEYS[2]]
    # every other pass logs the same values whether the k-means pass ran in between or not
    plain, mixed = Evaluator(tr, S), Evaluator(tr, S)
    a1 = plain.set_scores(dev, knn=True, mmd=True)
    mixed.kmeans_scores(fit, dev)
    b1 = mixed.set_scores(dev, knn=True, mmd=True)
    mixed.kmeans_scores(fit, dev)
    assert a1 == b1 and plain.dev_costs(dev) == mixed.dev_costs(dev)
    a3 = plain.swd_scores(dev)
    mixed.kmeans_scores(fit, dev)
    assert mixed.swd_scores(dev) == a3
    assert P._snapshot(plain.feed)['rng_state'] == P._snapshot(mixed.feed)['rng_state']
    # unlabelled dev data: the three NDB rows and one message over two firings
    capsys.readouterr()
    bare = Evaluator(tr, S)
    r1, r2 = bare.kmeans_scores([x for x, _ in fit], [x for x, _ in dev]), bare.kmeans_scores([x for x, _ in fit], [x for x, _ in dev])
    assert list(r1) == KEYS[:3] == list(r2) and capsys.readouterr().out.count('dev kmeans accuracy z / nmi z skipped') == 1
    assert r1[KEYS[2]] == res[KEYS[2]] and bare.km_z_fits == 0
    # the averaged weights' names
    tr.ema_loaded, mixed.weights = True, 'ema'
    try:
        assert list(mixed.tag(mixed.kmeans_scores(fit, dev))) == [k + ' ema' for k in KEYS] and mixed.km_fits == 1
    finally:
        tr.ema_loaded, mixed.weights = False, 'live'
    # a poisoned weight: nan and one message, no exception
    weights = tr.get_params()
    name = sorted(k for k in weights if k.startswith('Generator.') and k.endswith('.Filters'))[-1]      # the output layer: a ReLU's fmax would drop a NaN further up
    capsys.readouterr()
    tr.load_params(dict(weights, **{name: np.full_like(weights[name], np.nan)}))
    try:
        res3 = mixed.kmeans_scores(fit, dev)
    finally:
        tr.load_params(weights)
    out = capsys.readouterr().out
    assert list(res3) == KEYS and np.isnan(res3[KEYS[0]]) and np.isnan(res3[KEYS[1]]) and out.count('[evaluate] kmeans: status') == 1, (name, res3)
    assert res3[KEYS[2]] == res[KEYS[2]]
    assert P._snapshot(tr.feed) == before[0]


def test_training_bit_identical_with_the_kmeans_pass_and_the_flag_prints_the_rows(gpu, tmp_path, monkeypatch, capsys):
    from graphical_gan_amd import checkpoint, evaluate
    from graphical_gan_amd.models import Config
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    small = dict(KM_BINS=6, KM_SAMPLES=3 * B, KM_MAX_ROWS=2 * B, KM_FIT_ROWS=4 * B, KM_ITERS=3)
    base = dict(DATASET='mnist', BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config('mnist', batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base, MMD_EVERY=2), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, MMD_EVERY=2, KMEANS_EVERY=2, **small), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    rest = lambda seen: [(n, i, v) for n, i, v in seen if n not in KEYS and n != 'time']
    assert rest(seen0) == rest(seen1) and any(n.startswith('dev mmd') for n, _, _ in seen0)          # the training costs AND the following dev mmd
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [1, 3], key
    assert not [n for n, _, _ in seen0 if n in KEYS]
    ckpt = str(tmp_path / 'params.npz')
    checkpoint.save(ckpt, tr1)
    P._fresh()
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=K, BATCH_SIZE=B, **small)
    capsys.readouterr()
    res = evaluate.main([ckpt, '--script', 'gmgan_inference_mnist', '--kmeans'] + ['--set=%s=%s' % kv for kv in over.items()])
    out = capsys.readouterr().out
    assert all(k in res and ('%s\t' % k) in out for k in KEYS)
    plain = evaluate.main([ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()])
    assert not any(k in plain for k in KEYS) and all(plain[k] == res[k] for k in plain)
    # synthetic minibatches have no labels: the three NDB rows, one message
    capsys.readouterr()
    S = dict(DATASET='mnist', BATCH_SIZE=8, ITERS=2, LOG_EVERY=1, MODE='ali', SYNTHETIC='force', KMEANS_EVERY=1, **small)
    _, _, _, seen = P._train(S, Config('mnist', batch_size=8, n_coms=0, mode='ali', dim=8, dim_latent=16))
    assert [n for n, _, _ in seen if n in KEYS] == KEYS[:3] * 2 and capsys.readouterr().out.count('dev kmeans accuracy z / nmi z skipped') == 1
