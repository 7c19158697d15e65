"""-m gpu: the Parzen-window log-sums (csrc/parzen_sets.hip: functional.parzen_lse / parzen_ll) against the float64 direct-difference
restatement tests/_parzen_ref.py -- on an integer lattice, where the distances are exact and only the shifted exp / log arithmetic is under
test, and on image-like rows, where an unshifted sum is log 0 --, the limits (a huge bandwidth, a set against itself), repeatability,
bandwidths that do not depend on each other, the unit-interval scale, and the dev-set Parzen pass: its three values, the Trainer it leaves
untouched, the values of the other passes it does not move, the training it does not change, the CLI.

The gate is the project's one for set-level values: |got - ref| <= 2e-5 max(1, |ref|), per row and per bandwidth (_parzen_ref.gate)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _parzen_ref as R  # noqa: E402
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)

pytestmark = pytest.mark.gpu

KEYS = ['dev parzen ll x', 'dev parzen se x', 'dev parzen sigma x']


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32), device=dev)          # (a copy: the shared cases are read-only)


def _lse(Q, S, sig, dev):
    import torch
    from graphical_gan_amd import functional as F
    tq = _t(Q, dev)
    out = F.parzen_lse(tq, tq if S is Q else _t(S, dev), sig)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (len(sig), len(Q))
    return out.cpu().numpy().astype(np.float64)


# ---- 1. values against float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', R.LATTICE_CASES + R.IMAGE_CASES)
def test_values_against_float64(gpu, m, n, d):
    """(2, 1, 1) the minimum with one candidate; (5, 9, 16) a ragged tile; (130, 67, 33) two query blocks, rows that are not 16-byte
    aligned; (257, 300, 131) three blocks each way and three splits; (192, 160, 3072) pixel width; the two image-like cases"""
    Q, S, sig = R.case(m, n, d)
    ref = R.reference(m, n, d)
    got = _lse(Q, S, sig, gpu)
    assert np.all(np.isfinite(got))
    err = np.abs(got - ref) / R.gate(ref)
    print('lse', (m, n, d), 'max err / gate per sigma', err.max(axis=1), 'ref from', ref.min(), 'to', ref.max())
    assert np.all(err <= 1.0), err.max()


# ---- 2. limits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('m,n,d', [(130, 67, 33), (1, 1, 5), (5800, 5800, 16)])          # (the last: 46 blocks in 45 splits, two tiles in split 0)
def test_a_huge_bandwidth_counts_the_candidates(gpu, m, n, d):
    Q, S = R.lattice(m, n, d)[:2] if d != 5 else (np.ones((1, 5), np.float32), np.full((1, 5), 2.0, np.float32))
    got = _lse(Q, S, [1e6], gpu)
    assert np.all(np.abs(got - np.log(n)) <= 1e-6), np.abs(got - np.log(n)).max()


def test_a_set_against_itself(gpu):
    Q = R.lattice(130, 67, 33)[0]
    sig = R.lattice(130, 67, 33)[2]
    ref = R.lse(Q, Q, sig)
    got = _lse(Q, Q, sig, gpu)                       # (the same pointer twice)
    assert np.all(np.abs(got - ref) <= R.gate(ref))
    assert np.all(got >= 0.0)                        # every row meets itself: a term exp(0)


# ---- 3. repeatability -------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu):
    import torch
    from graphical_gan_amd import functional as F
    Q, S, sig = R.case(257, 300, 131)
    tq, ts = _t(Q, gpu), _t(S, gpu)
    a = F.parzen_lse(tq, ts, sig)
    pad = torch.full((12345,), 3.0, device=gpu)      # (another allocation in between: the workspace moves)
    b = F.parzen_lse(tq, ts, sig)
    assert torch.equal(a, b) and a.data_ptr() != b.data_ptr() and float(pad[0]) == 3.0


def test_sixteen_bandwidths_are_two_calls_of_eight(gpu):
    import torch
    from graphical_gan_amd import functional as F
    Q, S, _ = R.case(130, 300, 784)
    tq, ts = _t(Q, gpu), _t(S, gpu)
    sig = list(np.logspace(-1, 1, 16))
    all16 = F.parzen_lse(tq, ts, sig)
    assert torch.equal(all16, torch.cat([F.parzen_lse(tq, ts, sig[:8]), F.parzen_lse(tq, ts, sig[8:])]))
    ref = R.lse_from_d2(R.case_d2(130, 300, 784), sig)
    assert np.all(np.abs(all16.cpu().numpy() - ref) <= R.gate(ref))


# ---- 4. the unit-interval scale ---------------------------------------------------------------------------------------------------------
def test_parzen_ll_scale(gpu):
    """rows r in a range of width 1 against rows 2 r - 1 with scale = 2: the same density of the unit-scale data.  r from the lattice
    divided by 4 (and 2 r - 1 with it) is exact in float32, and so are both sets' distances"""
    import torch
    from graphical_gan_amd import functional as F
    Q, S, _ = R.lattice(130, 67, 33)
    q, s = np.asarray(Q, np.float64) / 4.0, np.asarray(S, np.float64) / 4.0
    sig = [0.1, 0.3, 1.0]
    one = F.parzen_ll(_t(q, gpu), _t(s, gpu), sig)
    two = F.parzen_ll(_t(2 * q - 1, gpu), _t(2 * s - 1, gpu), sig, scale=2.0)
    assert one.is_cuda and one.dtype == torch.float64 and tuple(one.shape) == (3, 130)
    ref = R.ll(q, s, sig)
    one, two = one.cpu().numpy(), two.cpu().numpy()
    print('ll scale: max err / gate', (np.abs(one - ref) / R.gate(ref)).max(), (np.abs(two - ref) / R.gate(ref)).max())
    assert np.all(np.abs(one - ref) <= R.gate(ref)) and np.all(np.abs(two - ref) <= R.gate(ref))
    assert np.all(np.abs(two - one) <= R.gate(ref))


# ---- 5. the pass ------------------------------------------------------------------------------------------------------------------------
def _dev(dataset, B, n, seed=21):
    """n minibatches of B synthetic images plus a partial one (dropped by the pass)"""
    rng = np.random.default_rng(seed)
    if dataset == 'mnist':
        xs = [(rng.random((B, 784)) ** 3).astype(np.float32) for _ in range(n)]
    else:
        xs = [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]
    return xs + [xs[0][:B - 1]]


def _check(res, sets, B, scale, sigmas=R.SIGMAS, valid=1000, rows=None):
    """the three values against the restatement on the sets the pass built"""
    x, gx = sets['x'].cpu().numpy(), sets['gx'].cpu().numpy()
    p = R.pass_values(x[:rows], gx[:rows], B, sigmas=sigmas, scale=scale, valid=valid)
    print('   pass', res, 'ref', {k: p[k] for k in ('ll', 'se', 'sigma', 'v', 'count')}, 'validation means', p['valid_means'])
    sig = np.asarray(sigmas, np.float64)
    chosen = int(np.argmin(np.abs(sig - res['dev parzen sigma x'])))
    assert res['dev parzen sigma x'] == sig[chosen]
    # float32 may choose another bandwidth only where the reference's validation means cannot tell the two apart
    assert p['valid_means'][chosen] >= p['valid_means'][p['best']] - 2 * R.gate(p['valid_means'][p['best']])
    held = p['rows'][chosen, p['v']:]
    assert abs(res['dev parzen ll x'] - held.mean()) <= R.gate(held.mean())
    # |std a - std b| <= max |a - b| for the population std (a projection and a norm), so the standard error moves by at most the
    # largest row gate / sqrt(count)
    se = held.std() / np.sqrt(len(held))
    assert abs(res['dev parzen se x'] - se) <= R.gate(held).max() / np.sqrt(len(held))
    assert res['dev parzen se x'] > 0.0
    return p


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_parzen_scores_values_and_an_untouched_trainer(gpu, dataset, K, mode):
    import torch
    from graphical_gan_amd import optim
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 6
    tr = P._model(gpu, dataset, B, K, mode)
    dev = _dev(dataset, B, n)
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    scale = 1.0 if dataset == 'mnist' else 2.0
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
    res, sets = ev.parzen_scores(dev, return_sets=True)
    assert state() == before                       # weights, optimizer state, feed buffers and every RNG state: byte for byte
    assert list(res) == KEYS and all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    c = tr.cfg
    assert {k: tuple(v.shape) for k, v in sets.items()} == dict(z=(n * B, c.dim_latent), pz=(n * B, c.dim_latent),
                                                                 x=(n * B, c.output_dim), gx=(n * B, c.output_dim))
    assert len(ev.kept) == n
    p = _check(res, sets, B, scale)
    assert p['v'] == 3 * B and p['count'] == 3 * B                                      # half the minibatches choose, half are scored
    # the settings reach the pass: the row cap (whole minibatches), the validation rows, the grid
    S2 = dict(S, PARZEN_MAX_ROWS=5 * B + 3, PARZEN_VALID_ROWS=B + 1, PARZEN_SIGMAS=[0.3, 0.6])
    res2, capped = Evaluator(tr, S2).parzen_scores(dev, return_sets=True)
    assert capped['x'].shape[0] == 5 * B and list(res2) == KEYS
    p2 = _check(res2, capped, B, scale, sigmas=[0.3, 0.6], valid=B + 1)
    assert p2['v'] == B and p2['count'] == 4 * B
    with pytest.raises(ValueError, match='at least 2 full minibatches'):
        Evaluator(tr, dict(S, PARZEN_MAX_ROWS=2 * B - 1)).parzen_scores(dev)
    # with the other passes: ONE build of the sets, the same stream of draws, and their ten values bit for bit those without parzen
    without = Evaluator(tr, S).set_scores(dev, mmd=True, prdc=True)
    both = Evaluator(tr, S, keep_noise=True)
    builds, build = [], both._score_sets
    both._score_sets = lambda *a, **kw: (builds.append(1), build(*a, **kw))[1]
    res_all, sets_all = both.set_scores(dev, mmd=True, prdc=True, parzen=True, return_sets=True)
    assert len(builds) == 1 and len(both.kept) == n
    assert list(res_all) == ['dev mmd z', 'dev mmd x'] + P.KEYS + KEYS and list(res_all)[:10] == list(without)
    assert all(res_all[k] == without[k] for k in without)
    assert all(res_all[k] == res[k] for k in KEYS)                                      # ... and the three are those of the pass alone
    assert all(torch.equal(sets_all[k], sets[k]) for k in sets)
    assert state() == before


# ---- 6. training unaffected -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dataset', ['cifar10', 'mnist'])
def test_training_bit_identical_with_the_parzen_pass(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=4, LOG_EVERY=2, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, PARZEN_EVERY=1), cfg())
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
    assert all(np.isfinite(v) for n, _, v in seen1 if n in KEYS)
    assert not [n for n, _, _ in seen0 if n.startswith('dev ')]
    assert not [n for n, _, _ in seen1 if n.startswith('dev ') and n not in KEYS]      # (no other pass was switched on)


# ---- 7. CLI -----------------------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_three_rows_of_the_live_evaluator(gpu, tmp_path, monkeypatch, capsys):
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
    live = ev.set_scores(dev, parzen=True)
    P._fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--parzen'])
    out = capsys.readouterr().out
    for k in KEYS:
        assert res[k] == live[k], k
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    P._fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if k not in KEYS)
    assert all(plain[k] == res[k] for k in plain)
