"""-m gpu: the labelled neighbour lists (csrc/knn_lists.hip: functional.knn_lists / knn_vote / knn_accuracy) against the float64
direct-difference restatement tests/_knn_ref.py -- lists and distances, the lower index at a tie and exactness on an integer lattice,
planted neighbours in every row block and split, lists where everything ties, the vote and its tie rule, the accuracy end to end,
repeatability --, and the dev-set k-NN accuracy pass: its values, the Trainer it leaves untouched, the sets it shares with the MMD and
PRDC passes, the training it does not change, the CLI.

What float32 may decide differently is derived in _knn_ref, not measured: a row is held to the reference's list (as a set, and position by
position where the reference's distances are clear of each other) only if no other candidate lies within 2 T_i of its k-th distance, and
to the reference's vote only if the candidates within that band carry one label; test_knn_cpu asserts how few rows are let off."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knn_ref as R  # noqa: E402
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)

pytestmark = pytest.mark.gpu

KEYS = ['dev knn accuracy z', 'dev knn accuracy x']


def _t(a, dev, dtype=np.float32):
    import torch
    return torch.as_tensor(np.array(a, dtype=dtype), device=dev)          # (a copy: the shared cases are read-only)


def _lists(q, c, k, skip, dev):
    """functional.knn_lists with distances, checked for what holds whatever the input: int32 in range, distinct, never i, ascending"""
    import torch
    from graphical_gan_amd import functional as F
    tq = _t(q, dev)
    idx, d2 = F.knn_lists(tq, tq if c is q else _t(c, dev), k, skip_diag=skip, return_d2=True)
    assert idx.is_cuda and idx.dtype == torch.int32 and d2.dtype == torch.float32 and tuple(idx.shape) == tuple(d2.shape) == (len(q), k)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy().astype(np.float64)
    assert idx.min() >= 0 and idx.max() < len(c)
    assert all(len(set(row)) == k for row in idx.tolist())
    if skip:
        assert not np.any(idx == np.arange(len(q))[:, None])
    assert np.all(np.isfinite(d2)) and np.all(d2 >= 0) and np.all(np.diff(d2, axis=1) >= 0)
    return idx, d2


# ---- 1. lists against float64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d,skip,ks', [(1, 1, 5, False, (1,)),                  # minimum
                                           (2, 2, 1, True, (1,)),                   # the smallest leave-one-out; d = 1
                                           (5, 9, 16, False, (1, 3)),               # a ragged tile
                                           (67, 130, 33, False, (1, 3, 5)),         # two candidate blocks; rows that are not 16-byte aligned
                                           (130, 130, 33, True, (1, 3, 5)),         # the diagonal in two tiles
                                           (257, 300, 131, False, (1, 5, 8))])      # three blocks each way, three splits; the longest list
def test_lists_against_float64(gpu, m, n, d, skip, ks):
    for k in ks:
        r = R.reference(m, n, d, k, skip)
        idx, d2 = _lists(r['Q'], r['C'], k, skip, gpu)
        err = np.abs(d2 - r['dist'])
        closed = r['set_closed']
        print('lists', (m, n, d, skip, k), 'max err / T', (err / r['T'][:, None]).max(), 'set-open rows', int((~closed).sum()), 'pinned', int(r['pinned'].sum()))
        assert np.all(err <= r['T'][:, None]), (k, err.max())
        assert np.array_equal(np.sort(idx[closed], axis=1), np.sort(r['idx'][closed], axis=1))
        assert np.array_equal(idx[r['pinned']], r['idx'][r['pinned']])
        assert closed.mean() >= 0.95 and r['pinned'].any()


# ---- 2. the integer lattice: exact, ties included -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', [(130, 67, 33), (257, 300, 16), (192, 160, 3072),
                                   (5800, 5800, 16)])           # 46 blocks each way in 45 splits: split 0 walks a second, ragged tile
def test_integer_lattice_is_exact_lower_index_at_a_tie(gpu, m, n, d):
    """integer entries: every product and sum is exact in float32, so indices and distances must EQUAL the reference's -- and the
    reference sees distance ties at the k-th place, so it is the lower-index rule that decides"""
    X, Y = R.lattice(m, n, d)
    k = 3
    for Q, C, skip in ((X, Y, False), (Y, X, False), (X, X, True), (Y, Y, True)):
        D = R.distances(Q, C, skip)
        ref_idx, ref_d = R.lists_from(D, k)
        assert np.any(np.sort(D, axis=1)[:, k - 1] == np.sort(D, axis=1)[:, k])              # a tie between the k-th and the next
        idx, d2 = _lists(Q, C, k, skip, gpu)
        assert np.array_equal(d2, ref_d)
        assert np.array_equal(idx, ref_idx), np.flatnonzero(np.any(idx != ref_idx, axis=1))[:8]


# ---- 3. planted neighbours ----------------------------------------------------------------------------------------------------------------
def test_planted_copies_are_found_in_every_block_and_split(gpu):
    """(130, 300, 33): three candidate blocks, each a split of its own; six queries spread over both query blocks, both lane halves and
    all four waves get an exact copy at the first / last row of every candidate block"""
    Q, _, C, _ = R.split(130, 300, 33)
    C = np.array(C)
    where = {0: 0, 37: 127, 64: 128, 100: 255, 128: 256, 129: 299}              # query -> candidate position of its copy
    for qi, pos in where.items():
        C[pos] = Q[qi]
    D, T = R.distances(Q, C), R.row_tol(Q, C)
    for k in (1, 3):
        ref_idx, ref_d = R.lists_from(D, k)
        idx, d2 = _lists(Q, C, k, False, gpu)
        assert np.all(np.abs(d2 - ref_d) <= T[:, None])
        for qi, pos in where.items():
            assert ref_idx[qi, 0] == pos and ref_d[qi, 0] == 0.0 and np.sort(D[qi])[1] > 2 * T[qi]       # (the copy is the nearest beyond doubt)
            assert idx[qi, 0] == pos and d2[qi, 0] <= T[qi], (qi, idx[qi], d2[qi])


# ---- 4. everything ties ---------------------------------------------------------------------------------------------------------------------
def test_all_rows_equal_lists_are_the_lowest_indices(gpu):
    row = np.random.default_rng(3).standard_normal(16).astype(np.float32)
    Q, C = np.tile(row, (130, 1)), np.tile(row, (9, 1))
    idx, d2 = _lists(Q, C, 8, False, gpu)
    assert np.array_equal(idx, np.tile(np.arange(8), (130, 1)))
    assert np.all(d2 == d2[0, 0]) and d2[0, 0] <= R.row_tol(Q, C)[0]
    idx, _ = _lists(C, C, 8, True, gpu)                                          # leave-one-out: the first 8 indices other than i
    assert idx.tolist() == [[j for j in range(9) if j != i] for i in range(9)]


def test_k_equal_to_n_lists_every_candidate_and_no_ghost_row(gpu):
    Q, _, C, _ = R.split(130, 5, 16)
    idx, d2 = _lists(Q, C, 5, False, gpu)
    assert np.array_equal(np.sort(idx, axis=1), np.tile(np.arange(5), (130, 1)))
    ref_idx, ref_d = R.lists(Q, C, 5)
    assert np.all(np.abs(d2 - ref_d) <= R.row_tol(Q, C)[:, None])


# ---- 5. the vote ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('classes', [4, 1000])
def test_vote_against_the_reference(gpu, classes):
    import torch
    from graphical_gan_amd import functional as F
    m, n = 300, 500
    rng = np.random.default_rng(classes)
    lc, lq = rng.integers(0, classes, size=n), rng.integers(0, min(classes, 6), size=m)
    if classes == 1000:
        lc[:n // 2] = rng.integers(0, 6, size=n // 2)              # (so that some votes are correct, and some lists repeat a label)
    tc, tq = _t(lc, gpu, np.int32), _t(lq, gpu, np.int32)
    for k in (1, 2, 5, 8):
        idx = rng.integers(0, n, size=(m, k))
        ref = R.vote(idx, lc)
        ti = _t(idx, gpu, np.int32)
        pred = F.knn_vote(ti, tc)
        assert pred.is_cuda and pred.dtype == torch.int32 and np.array_equal(pred.cpu().numpy(), ref)
        p2, correct = F.knn_vote(ti, tc, tq)
        p3, c3, conf = F.knn_vote(ti, tc, tq, classes)
        assert np.array_equal(p2.cpu().numpy(), ref) and np.array_equal(p3.cpu().numpy(), ref)
        assert correct.dtype == conf.dtype == torch.int32 and tuple(correct.shape) == (1,) and tuple(conf.shape) == (classes, classes)
        n_ok = int(np.sum(ref == lq))
        conf = conf.cpu().numpy()
        print('vote', classes, k, 'correct', n_ok)
        assert int(correct.item()) == int(c3.item()) == n_ok and 0 < n_ok < m             # (neither trivial end)
        assert np.array_equal(conf, R.confusion(lq, ref, classes)) and conf.sum() == m and np.trace(conf) == n_ok
        shuffled = _t(rng.permuted(idx, axis=1), gpu, np.int32)     # the multiset decides, not the order in the list
        assert np.array_equal(F.knn_vote(shuffled, tc).cpu().numpy(), ref)


def test_a_tied_vote_goes_to_the_smallest_label(gpu):
    from graphical_gan_amd import functional as F
    labels = _t([3, 1, 3, 1, 7, 5, 6], gpu, np.int32)
    for lists, want in (([[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [0, 2, 1, 3]], 1),       # 2-2
                        ([[4, 5, 6], [6, 5, 4], [5, 6, 4], [4, 6, 5]], 5),                   # 1-1-1
                        ([[0, 2, 1, 4, 5], [4, 1, 5, 0, 2]], 3)):                            # (no tie: 2-1-1-1)
        pred = F.knn_vote(_t(lists, gpu, np.int32), labels).cpu().tolist()
        assert pred == [want] * len(lists) == R.vote(lists, [3, 1, 3, 1, 7, 5, 6]).tolist()


# ---- 6. the accuracy end to end -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,d', [(9, 16), (130, 33), (300, 131), (192, 3072)])
def test_knn_accuracy_end_to_end(gpu, n, d):
    import torch
    from graphical_gan_amd import functional as F
    Z, y = R.labelled(n, d)
    tz, ty = _t(Z, gpu), _t(y, gpu, np.int32)
    for k in (1, 5):
        r = R.reference(n, n, d, k, True)
        acc, pred = F.knn_accuracy(tz, ty, k, R.CLASSES, return_pred=True)
        assert acc.is_cuda and acc.dtype == torch.float64 and tuple(acc.shape) == (1,)
        junk = torch.full((1 << 16,), 3.0, device=gpu)               # (another allocation pattern in between)
        again = F.knn_accuracy(tz, ty, k, R.CLASSES)
        del junk
        assert acc.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
        acc, pred = float(acc.item()), pred.cpu().numpy()
        closed = r['label_closed']
        lo, hi = R.accuracy_bracket(r['pred'], y, closed)
        print('accuracy', (n, d, k), acc, (lo, hi), 'label-open rows', int((~closed).sum()))
        assert np.array_equal(pred[closed], r['pred'][closed])
        assert acc == float(np.mean(pred == y)) and lo <= acc <= hi, (acc, lo, hi)


def test_bank_and_query_vote_at_the_pixel_width(gpu):
    """160 queries against a bank of 192 rows at d = 3072: lists, vote, correct count and confusion matrix in one chain"""
    from graphical_gan_amd import functional as F
    m, n, d = 160, 192, 3072
    for k in (1, 5):
        r = R.reference(m, n, d, k, False)
        idx = F.knn_lists(_t(r['Q'], gpu), _t(r['C'], gpu), k)
        pred, correct, conf = F.knn_vote(idx, _t(r['yc'], gpu, np.int32), _t(r['yq'], gpu, np.int32), R.CLASSES)
        pred, conf = pred.cpu().numpy(), conf.cpu().numpy()
        closed = r['label_closed']
        lo, hi = R.accuracy_bracket(r['pred'], r['yq'], closed)
        print('bank / query', k, int(correct.item()) / float(m), (lo, hi), 'label-open rows', int((~closed).sum()))
        assert np.array_equal(pred[closed], r['pred'][closed])
        assert int(correct.item()) == int(np.sum(pred == r['yq'])) and lo <= int(correct.item()) / float(m) <= hi
        assert np.array_equal(conf, R.confusion(r['yq'], pred, R.CLASSES))


# ---- 7. the pass ------------------------------------------------------------------------------------------------------------------------------
def _labelled_dev(dataset, B, n, seed=21):
    """n labelled minibatches of B images that depend on their class (4 classes; a fifth of the labels redrawn, so that the accuracy is not
    1), plus a partial minibatch (dropped by the pass)"""
    rng = np.random.default_rng(seed)
    D = 784 if dataset == 'mnist' else 3072
    proto = rng.random((4, D))
    dev = []
    for _ in range(n):
        y = rng.integers(0, 4, size=B)
        x = np.clip(0.7 * proto[y] + 0.3 * rng.random((B, D)), 0, 1)
        y = np.where(rng.random(B) < 0.2, rng.integers(0, 4, size=B), y)
        dev.append((x.astype(np.float32) if dataset == 'mnist' else np.floor(x * 255.99).astype(np.int32), y.astype(np.int64)))
    return dev + [(dev[0][0][:B - 1], dev[0][1][:B - 1])]


def _inside(value, Z, y, k):
    """the bracket rule on a returned set: the reference's leave-one-out vote, its label-closed rows, the value between the two ends"""
    Dm, T = R.distances(Z, Z, True), R.row_tol(Z, Z)
    c = R.closed_rows(Dm, k, T, y)
    lo, hi = R.accuracy_bracket(R.vote(c['idx'], y), y, c['label_closed'])
    print('   bracket', (lo, hi), 'value', value, 'label-open rows', int((~c['label_closed']).sum()), 'of', len(y))
    return lo - 1e-12 <= value <= hi + 1e-12


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_knn_scores_values_shared_sets_and_an_untouched_trainer(gpu, dataset, K, mode):
    import torch
    from graphical_gan_amd import optim
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 12
    tr = P._model(gpu, dataset, B, K, mode)
    dev = _labelled_dev(dataset, B, n)
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    ev = Evaluator(tr, S, keep_noise=True)
    tr.model.sample_noise(tr.feed)                 # (the Trainer's buffers hold something to compare)
    torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        w = {k: v.tobytes() for k, v in tr.get_params().items()}
        adam = {key[0]: tuple(t.cpu().numpy().tobytes() for t in (o.step, o.m, o.v)) for key, o in optim._optimizers.items()}
        return w, adam, P._snapshot(tr.feed), torch.cuda.get_rng_state(gpu).numpy().tobytes(), np.random.get_state()[1].tobytes()
    before = state()
    assert 'rng_state' in before[2] and before[0]
    res, sets = ev.knn_scores(dev, return_sets=True)
    assert state() == before                       # weights, optimizer state, feed buffers and every RNG state: byte for byte
    assert list(res) == KEYS and all(isinstance(v, float) and 0.0 <= v <= 1.0 for v in res.values())
    c = tr.cfg
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z=(n * B, c.dim_latent), x=(n * B, c.output_dim), y=(n * B,))
    assert len(ev.kept) == n and sets['y'].dtype == torch.int32
    host = {k: v.cpu().numpy() for k, v in sets.items()}
    assert np.array_equal(host['y'], np.concatenate([y for _, y in dev[:n]]))          # row-aligned with the minibatches
    for space in ('z', 'x'):
        assert _inside(res['dev knn accuracy ' + space], host[space], host['y'], 5), space
    assert 0.5 < res['dev knn accuracy x'] < 1.0                                        # (the images DO depend on the class; neither trivial end)
    # KNN_K reaches the op; KNN_MAX_ROWS caps the sets at whole minibatches
    res2, capped = Evaluator(tr, dict(S, KNN_MAX_ROWS=2 * B + 3, KNN_K=2)).knn_scores(dev, return_sets=True)
    assert capped['z'].shape[0] == capped['y'].shape[0] == 2 * B and list(res2) == KEYS
    hc = {k: v.cpu().numpy() for k, v in capped.items()}
    assert _inside(res2['dev knn accuracy z'], hc['z'], hc['y'], 2) and _inside(res2['dev knn accuracy x'], hc['x'], hc['y'], 2)
    with pytest.raises(ValueError, match='KNN_K'):
        Evaluator(tr, dict(S, KNN_MAX_ROWS=B, KNN_K=8)).knn_scores(dev)                # 8 rows have 7 neighbours
    # the three set-level passes at once: ONE build of the sets, and every value that of its pass run alone from the same state
    alone = {name: Evaluator(tr, S).set_scores(dev, **{name: True}) for name in ('mmd', 'prdc', 'knn')}
    assert alone['knn'] == res
    both = Evaluator(tr, S, keep_noise=True)
    builds, build = [], both._score_sets
    both._score_sets = lambda *a, **kw: (builds.append(1), build(*a, **kw))[1]
    res_all, sets_all = both.set_scores(dev, mmd=True, prdc=True, knn=True, return_sets=True)
    assert len(builds) == 1 and len(both.kept) == n and sorted(sets_all) == ['gx', 'pz', 'x', 'y', 'z']
    assert list(res_all) == ['dev mmd z', 'dev mmd x'] + P.KEYS + KEYS
    for name in alone:
        assert all(res_all[k] == v for k, v in alone[name].items()), name
    assert all(torch.equal(sets_all[k], sets[k]) for k in sets)
    assert state() == before


# ---- 8. training unaffected ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset', ['cifar10', 'mnist'])
def test_training_bit_identical_with_the_knn_pass(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, KNN_EVERY=1), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    train_keys = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev ') and n != 'time']
    assert train_keys(seen0) == train_keys(seen1)            # the logged training costs too
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [0, 1, 2, 3], key
    assert all(0.0 <= v <= 1.0 for n, _, v in seen1 if n in KEYS)
    assert not [n for n, _, _ in seen0 if n.startswith('dev ')]
    assert not [n for n, _, _ in seen1 if n.startswith('dev ') and n not in KEYS]      # (no other pass was switched on)


def test_unlabelled_dev_data_skip_the_pass_with_one_message(gpu, capsys):
    from graphical_gan_amd.models import Config
    S = dict(DATASET='mnist', BATCH_SIZE=8, ITERS=2, LOG_EVERY=1, MODE='ali', SYNTHETIC='force', KNN_EVERY=1)
    capsys.readouterr()
    _, _, _, seen = P._train(S, Config('mnist', batch_size=8, n_coms=0, mode='ali', dim=8, dim_latent=16))
    out = capsys.readouterr().out
    assert out.count('[run] dev knn accuracy skipped: no labelled dev set') == 1
    assert not [n for n, _, _ in seen if n.startswith('dev ')]


# ---- 9. CLI -------------------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_two_rows_of_the_live_evaluator(gpu, tmp_path, monkeypatch, capsys):
    from graphical_gan_amd import checkpoint, run, evaluate
    from graphical_gan_amd.evaluate import Evaluator
    from graphical_gan_amd.engine import Trainer
    P._data_on_disk(tmp_path, monkeypatch)
    over = dict(DIM=8, DIM_LATENT=16, N_COMS=5, BATCH_SIZE=8)
    S = run.reference_block('gmgan_inference_mnist', **over)
    P._fresh()
    tr = Trainer(run.config(S), device=gpu, graph=False)
    for it in range(2):
        tr.iteration(it, iter(tr.model.synthetic_ring(gpu, n=4) * 2))
    ckpt = str(tmp_path / 'params_2.npz')
    checkpoint.save(ckpt, tr)
    np.random.seed(5)
    dev, test = run.eval_sets(S, tr.model, gpu)
    ev = Evaluator(tr, S)                          # the passes in evaluate_once's order: they share ONE stream of noise draws
    ev.dev_costs(dev)
    ev.cluster_accuracy(test)
    live = ev.set_scores(dev, knn=True)
    P._fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--knn'])
    out = capsys.readouterr().out
    for k in KEYS:
        assert res[k] == live[k], k
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    P._fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if k not in KEYS)
    assert all(plain[k] == res[k] for k in plain)
