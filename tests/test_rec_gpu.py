"""-m gpu: reconstruction fidelity on the device (csrc/ssim_pairs.hip: functional.ssim_pairs / psnr_from_mse) against the float64
direct-window restatement tests/_ssim_ref.py -- per image, over the shapes at which the kernel takes another path (one window position, an
odd width, the MNIST and CIFAR shapes, the banded 64 x 64 planes, planes off a 16-byte boundary) and the kinds of data that can go wrong
(the bright flat planes tell a centred formulation from a raw one) --, exactness of a set against itself and of constant planes,
repeatability, locality, and the two dev-set passes: the image scripts' (its rows, its four values, the Trainer it leaves untouched, the
values of the other passes it does not move, the training it does not change, the CLI) and the state-space scripts' (rows are frames).

The gate is the project's one for set-level values: |got - ref| <= 2e-5 max(1, |ref|), per image (_ssim_ref.gate)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ssim_ref as R  # noqa: E402
import test_prdc_gpu as P  # noqa: E402  (its small oracle-weight models, data on disk and recorded training runs)

pytestmark = pytest.mark.gpu

KEYS = ['dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x']


def _t(a, dev):
    import torch
    return torch.as_tensor(np.array(a, dtype=np.float32), device=dev)          # (a copy: the shared cases are read-only)


def _pairs(a, b, shape, ma, mb, dev):
    import torch
    from graphical_gan_amd import functional as F
    ta = _t(a, dev)
    mse, ssim = F.ssim_pairs(ta, ta if b is a else _t(b, dev), shape, ma, mb)
    for v in (mse, ssim):
        assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (len(a),)
    return mse, ssim


# ---- 1. values against float64 ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,c,h,w', R.SHAPES + R.EXTRA_SHAPES)
@pytest.mark.parametrize('kind', R.KINDS)
def test_values_against_float64(gpu, kind, n, c, h, w):
    """(1, 1, 11, 11) one window position; (5, 1, 12, 17) an odd width; (67, 1, 28, 28) MNIST; (33, 3, 32, 32) CIFAR; (9, 1, 64, 64) and
    (6, 3, 64, 64) the largest LDS footprint, four bands; (7, 2, 13, 17) every second plane off a 16-byte boundary: both load paths;
    (3, 1, 64, 37) and (4, 4, 40, 64) two bands, the second ragged.  PSNR: against float64 of the kernel's own mse (the log arithmetic)"""
    from graphical_gan_amd import functional as F
    a, b, ma, mb = R.case(kind, n, c, h, w)
    ref_mse, ref_ssim = R.reference(kind, n, c, h, w)
    mse, ssim = _pairs(a, b, (c, h, w), ma, mb, gpu)
    psnr = F.psnr_from_mse(mse).cpu().numpy()
    mse, ssim = mse.cpu().numpy().astype(np.float64), ssim.cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(mse)) and np.all(np.isfinite(ssim))
    e_mse, e_ssim = np.abs(mse - ref_mse) / R.gate(ref_mse), np.abs(ssim - ref_ssim) / R.gate(ref_ssim)
    print('rec', kind, (n, c, h, w), 'max err / gate: mse %.4f ssim %.4f' % (e_mse.max(), e_ssim.max()),
          'ssim from', ref_ssim.min(), 'to', ref_ssim.max(), 'mse up to', ref_mse.max())
    assert np.all(e_mse <= 1.0), e_mse.max()
    assert np.all(e_ssim <= 1.0), e_ssim.max()
    ref_psnr = R.psnr(mse)
    assert psnr.dtype == np.float64 and np.all(np.abs(psnr - ref_psnr) <= R.gate(ref_psnr))


def test_the_scalar_load_path(gpu):
    """the same rows one float off a 16-byte boundary: the scalar staging path, and bit for bit the values of the vector path"""
    import torch
    from graphical_gan_amd import functional as F
    n, c, h, w = 33, 3, 32, 32
    a, b, ma, mb = R.case('smooth', n, c, h, w)
    ta, tb = _t(a, gpu), _t(b, gpu)
    assert ta.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0
    mse, ssim = F.ssim_pairs(ta, tb, (c, h, w), ma, mb)
    off = []
    for t in (ta, tb):
        buf = torch.empty((t.numel() + 1,), dtype=torch.float32, device=gpu)
        buf[1:].copy_(t.reshape(-1))
        off.append(buf[1:].view(n, -1))
        assert off[-1].data_ptr() % 16 == 4 and off[-1].is_contiguous()
    mse1, ssim1 = F.ssim_pairs(off[0], off[1], (c, h, w), ma, mb)
    assert torch.equal(mse, mse1) and torch.equal(ssim, ssim1)
    ref_mse, ref_ssim = R.reference('smooth', n, c, h, w)
    assert np.all(np.abs(ssim1.cpu().numpy() - ref_ssim) <= R.gate(ref_ssim)) and np.all(np.abs(mse1.cpu().numpy() - ref_mse) <= R.gate(ref_mse))


# ---- 2. exactness -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,c,h,w', [(5, 1, 12, 17), (33, 3, 32, 32), (6, 3, 64, 64)])
@pytest.mark.parametrize('kind', ['smooth', 'bright_flat', 'two_maps'])
def test_a_set_against_itself_is_exact(gpu, kind, n, c, h, w):
    import torch
    from graphical_gan_amd import functional as F
    a, _, ma, _ = R.case(kind, n, c, h, w)
    mse, ssim = _pairs(a, a, (c, h, w), ma, None, gpu)                 # (the same pointer twice)
    assert torch.equal(ssim, torch.ones_like(ssim)) and torch.equal(mse, torch.zeros_like(mse))
    psnr = F.psnr_from_mse(mse)
    assert torch.equal(psnr, torch.full_like(psnr, 100.0))


@pytest.mark.parametrize('c,h,w', [(1, 11, 11), (3, 32, 32), (1, 64, 64)])
def test_constant_planes_match_their_closed_forms(gpu, c, h, w):
    import torch
    from graphical_gan_amd import functional as F
    vals = [(0.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.98, 0.97), (1.0, 1.0), (0.5, 0.5)]
    a = np.repeat(np.array([[v[0]] for v in vals], np.float32), c * h * w, axis=1)
    b = np.repeat(np.array([[v[1]] for v in vals], np.float32), c * h * w, axis=1)
    mse, ssim = F.ssim_pairs(_t(a, gpu), _t(b, gpu), (c, h, w))
    va, vb = a[:, 0].astype(np.float64), b[:, 0].astype(np.float64)
    ref_ssim, ref_mse = (2 * va * vb + R.C1) / (va * va + vb * vb + R.C1), (va - vb) ** 2
    assert np.all(np.abs(ssim.cpu().numpy() - ref_ssim) <= R.gate(ref_ssim)), ssim
    assert np.all(np.abs(mse.cpu().numpy() - ref_mse) <= R.gate(ref_mse)), mse
    # the tanh range against data in 0..255: the maps are in the formula
    mse2, ssim2 = F.ssim_pairs(_t(2 * a - 1, gpu), _t(255 * b, gpu), (c, h, w), R.TANH, R.BYTES)
    assert np.all(np.abs(ssim2.cpu().numpy() - ref_ssim) <= R.gate(ref_ssim)) and np.all(np.abs(mse2.cpu().numpy() - ref_mse) <= R.gate(ref_mse))


# ---- 3. repeatability and locality ------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(gpu):
    import torch
    from graphical_gan_amd import functional as F
    n, c, h, w = 6, 3, 64, 64
    a, b, ma, mb = R.case('noise', n, c, h, w)
    ta, tb = _t(a, gpu), _t(b, gpu)
    m0, s0 = F.ssim_pairs(ta, tb, (c, h, w), ma, mb)
    pad = torch.full((12345,), 3.0, device=gpu)      # (another allocation in between: the workspace and the outputs move)
    m1, s1 = F.ssim_pairs(ta, tb, (c, h, w), ma, mb)
    assert torch.equal(m0, m1) and torch.equal(s0, s1) and s0.data_ptr() != s1.data_ptr() and m0.data_ptr() != m1.data_ptr()
    assert float(pad[0]) == 3.0


@pytest.mark.parametrize('kind,n,c,h,w', [('smooth', 33, 3, 32, 32), ('two_maps', 7, 2, 13, 17), ('noise', 9, 1, 64, 64)])
def test_an_image_does_not_depend_on_its_neighbours(gpu, kind, n, c, h, w):
    """image i of the n-image call equals the same image scored alone, bit for bit -- as a view (the same address) and as a copy of its
    own (another alignment where the plane size is no multiple of 4 floats)"""
    import torch
    from graphical_gan_amd import functional as F
    a, b, ma, mb = R.case(kind, n, c, h, w)
    ta, tb = _t(a, gpu), _t(b, gpu)
    mse, ssim = F.ssim_pairs(ta, tb, (c, h, w), ma, mb)
    for i in (0, 1, n // 2, n - 1):
        for one_a, one_b in ((ta[i:i + 1], tb[i:i + 1]), (ta[i:i + 1].clone(), tb[i:i + 1].clone())):
            m1, s1 = F.ssim_pairs(one_a, one_b, (c, h, w), ma, mb)
            assert torch.equal(m1, mse[i:i + 1]) and torch.equal(s1, ssim[i:i + 1]), i
    # ... nor on n: the leading rows alone
    m2, s2 = F.ssim_pairs(ta[:n // 2], tb[:n // 2], (c, h, w), ma, mb)
    assert torch.equal(m2, mse[:n // 2]) and torch.equal(s2, ssim[:n // 2])


def test_three_dimensional_rows_are_frames(gpu):
    import torch
    from graphical_gan_amd import functional as F
    n, c, h, w = 6, 3, 64, 64
    a, b, ma, mb = R.case('smooth', n, c, h, w)
    ta, tb = _t(a, gpu), _t(b, gpu)
    flat = F.ssim_pairs(ta, tb, (c, h, w))
    seq = F.ssim_pairs(ta.view(2, 3, -1), tb.view(2, 3, -1), (c, h, w))
    assert tuple(seq[0].shape) == (6,) and torch.equal(seq[0], flat[0]) and torch.equal(seq[1], flat[1])


# ---- 4. the image scripts' pass ---------------------------------------------------------------------------------------------------------
def _dev(dataset, B, n, seed=21):
    """n labelled minibatches of B synthetic images plus a partial one (dropped by the pass)"""
    rng = np.random.default_rng(seed)
    if dataset == 'mnist':
        xs = [(rng.random((B, 784)) ** 3).astype(np.float32) for _ in range(n)]
    else:
        xs = [rng.integers(0, 256, size=(B, 3072)).astype(np.int32) for _ in range(n)]
    return [(x, rng.integers(0, 10, size=B)) for x in xs] + [(xs[0][:B - 1], np.zeros(B - 1, np.int64))]


def _check_values(res, rows):
    """the four logged values against the float64 numpy statistics of the per-image rows"""
    mse, ssim = rows['mse'].cpu().numpy(), rows['ssim'].cpu().numpy()
    want = R.pass_values(mse, ssim)
    print('   pass', res, 'ref', want)
    assert list(res) == KEYS and all(isinstance(v, float) and np.isfinite(v) for v in res.values())
    for k in KEYS:
        assert abs(res[k] - want[k]) <= R.gate(want[k]), k
    assert res['dev rec ssim se x'] > 0.0 and res['dev rec mse x'] > 0.0
    assert np.all(np.abs(rows['psnr'].cpu().numpy() - R.psnr(mse)) <= R.gate(R.psnr(mse)))


@pytest.mark.parametrize('dataset,K,mode', [('mnist', 0, 'ali'), ('cifar10', 5, 'local_ep')])
def test_rec_scores_rows_values_and_an_untouched_trainer(gpu, dataset, K, mode):
    """deterministic-encoder MODEs: the rows of the pass are F.ssim_pairs on reconstructions(batch), minibatch by minibatch and bit for
    bit; the four values are the float64 statistics of those rows; the Trainer is byte for byte what it was; and the other passes' values
    are those of the call without rec"""
    import torch
    from graphical_gan_amd import functional as F, optim
    from graphical_gan_amd.evaluate import Evaluator
    B, n = 8, 6
    tr = P._model(gpu, dataset, B, K, mode)
    dev = _dev(dataset, B, n)
    S = dict(BATCH_SIZE=B, MODE=mode, N_COMS=K)
    c = tr.cfg
    shape, unit = (c.C, c.S, c.S), ((1.0, 0.0) if dataset == 'mnist' else (0.5, 0.5))
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
    res, rows = ev.rec_scores(dev, return_rows=True)
    assert state() == before                       # weights, optimizer state, feed buffers and every RNG state: byte for byte
    assert sorted(rows) == ['mse', 'psnr', 'ssim'] and all(tuple(v.shape) == (n * B,) and v.is_cuda for v in rows.values())
    assert len(ev.kept) == n
    _check_values(res, rows)
    assert list(ev.rec_scores(dev)) == KEYS                                             # (without the rows: the dict alone)
    # the rows are those of reconstructions(), a full minibatch at a time
    other = Evaluator(tr, S)
    for i in range(n):
        real, rec = other.reconstructions(dev[i])
        mse, ssim = F.ssim_pairs(_t(rec, gpu), _t(real, gpu), shape, unit)
        assert torch.equal(mse, rows['mse'][i * B:(i + 1) * B]) and torch.equal(ssim, rows['ssim'][i * B:(i + 1) * B]), i
        # ... and they are what the float64 restatement says of those pictures
        ref_mse, ref_ssim = R.pairs(rec, real, shape, unit)
        assert np.all(np.abs(ssim.cpu().numpy() - ref_ssim) <= R.gate(ref_ssim)) and np.all(np.abs(mse.cpu().numpy() - ref_mse) <= R.gate(ref_mse))
    # the row cap: whole minibatches, at least one
    res2, rows2 = Evaluator(tr, dict(S, REC_MAX_ROWS=3 * B + 5)).rec_scores(dev, return_rows=True)
    assert rows2['ssim'].shape[0] == 3 * B and torch.equal(rows2['ssim'], rows['ssim'][:3 * B])
    _check_values(res2, rows2)
    assert Evaluator(tr, dict(S, REC_MAX_ROWS=1)).rec_scores(dev, return_rows=True)[1]['mse'].shape[0] == B
    # with the other passes: ONE build of the sets, the same stream of draws, and their values bit for bit those without rec
    without, sets0 = Evaluator(tr, S).set_scores(dev, mmd=True, prdc=True, knn=True, parzen=True, return_sets=True)
    both = Evaluator(tr, S, keep_noise=True)
    builds, build = [], both._score_sets
    both._score_sets = lambda *a, **kw: (builds.append(1), build(*a, **kw))[1]
    res_all, sets_all = both.set_scores(dev, mmd=True, prdc=True, knn=True, parzen=True, rec=True, return_sets=True)
    assert len(builds) == 1 and len(both.kept) == n
    assert list(res_all) == list(without) + KEYS and len(without) == 15
    assert all(res_all[k] == without[k] for k in without)
    assert all(res_all[k] == res[k] for k in KEYS)                                      # ... and the four are those of the pass alone
    assert sorted(sets_all) == sorted(list(sets0) + ['rx']) and all(torch.equal(sets_all[k], sets0[k]) for k in sets0)
    assert state() == before


@pytest.mark.parametrize('dataset', ['cifar10', 'mnist'])
def test_training_bit_identical_with_the_rec_pass(gpu, tmp_path, monkeypatch, dataset):
    from graphical_gan_amd.models import Config
    P._data_on_disk(tmp_path, monkeypatch)
    K, B = 5, 8
    base = dict(DATASET=dataset, BATCH_SIZE=B, ITERS=6, LOG_EVERY=3, DATA_DIR=str(tmp_path), MODE='local_ep', N_COMS=K, N_VIS=10 * K)
    cfg = lambda: Config(dataset, batch_size=B, n_coms=K, dim=8, dim_latent=16)
    tr0, w0, a0, seen0 = P._train(dict(base), cfg())
    tr1, w1, a1, seen1 = P._train(dict(base, REC_EVERY=2), cfg())
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for x, y in zip(a0[r], a1[r]):
            assert np.array_equal(x, y), r
    train_keys = lambda seen: [(n, i, v) for n, i, v in seen if not n.startswith('dev ') and n != 'time']
    assert train_keys(seen0) == train_keys(seen1)            # the logged training costs too
    for key in KEYS:
        assert [i for n, i, _ in seen1 if n == key] == [1, 3, 5], key
    assert all(np.isfinite(v) for n, _, v in seen1 if n in KEYS)
    assert not [n for n, _, _ in seen0 if n.startswith('dev ')]
    assert not [n for n, _, _ in seen1 if n.startswith('dev ') and n not in KEYS]      # (no other pass was switched on)


def test_cli_prints_the_four_rows_of_the_live_evaluator(gpu, tmp_path, monkeypatch, capsys):
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
    live = ev.set_scores(dev, rec=True)
    P._fresh()
    args = [ckpt, '--script', 'gmgan_inference_mnist'] + ['--set=%s=%s' % kv for kv in over.items()]
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--rec'])
    out = capsys.readouterr().out
    for k in KEYS:
        assert res[k] == live[k], k
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    P._fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(plain) == sorted(k for k in res if k not in KEYS)
    assert all(plain[k] == res[k] for k in plain)


# ---- 5. the state-space scripts' pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 3])
def test_sequence_rec_scores_rows_are_frames(gpu, channels):
    import torch
    import test_ssgan_eval_gpu as SQ
    from graphical_gan_amd import functional as F, optim
    from graphical_gan_amd.evaluate import SequenceEvaluator
    from oracle import ssgan as O
    B, L = 2, 3
    ocfg, P0, cfg, tr = SQ._mk(gpu, 'naive_mean_field', 'res_w' if channels == 3 else 'res', B=B, L=L, channels=channels,
                               n_c=0 if channels == 3 else 2)
    S = dict(BATCH_SIZE=B, N_VIS=B, SEED=1)
    feeds = [O.make_feed(ocfg, np.random.default_rng(s)) for s in (3, 4, 5)]
    dev = [(f['real_x_unit'], f['real_y']) for f in feeds]
    dev.append((dev[0][0][:1], dev[0][1][:1]))                                          # (a partial minibatch: dropped)
    shape, maps = (cfg.C, 64, 64), ((0.5, 0.5), (1.0 / cfg.x_div, 0.0))
    assert cfg.x_div == (256.0 if channels == 3 else 1.0)
    ev = SequenceEvaluator(tr, S)
    torch.cuda.synchronize()

    def state():
        torch.cuda.synchronize()
        w = {k: v.tobytes() for k, v in tr.get_params().items()}
        adam = {key[0]: tuple(t.cpu().numpy().tobytes() for t in (o.step, o.m, o.v)) for key, o in optim._optimizers.items()}
        return w, adam, P._snapshot(tr.feed), torch.cuda.get_rng_state(gpu).numpy().tobytes(), np.random.get_state()[1].tobytes()
    before = state()
    res, rows = ev.rec_scores(dev, return_rows=True, per_frame=True)
    assert state() == before
    n = 3 * B * L
    assert all(tuple(rows[k].shape) == (n,) for k in ('mse', 'psnr', 'ssim'))
    curves = {k: res.pop(k) for k in ('mse_t', 'psnr_t', 'ssim_t')}
    _check_values(res, rows)
    # rows are frames, sequence-major: those of ssim_pairs on reconstructions(batch) against the data, minibatch by minibatch
    other = SequenceEvaluator(tr, S)
    for i in range(3):
        rec = other.reconstructions(dev[i])
        assert tuple(rec.shape) == (B, L, cfg.output_dim)
        data = _t(np.asarray(dev[i][0], np.float32).reshape(B, L, -1), gpu)
        mse, ssim = F.ssim_pairs(rec, data, shape, *maps)
        assert torch.equal(mse, rows['mse'][i * B * L:(i + 1) * B * L]) and torch.equal(ssim, rows['ssim'][i * B * L:(i + 1) * B * L]), i
        ref_mse, ref_ssim = R.pairs(rec.cpu().numpy().reshape(B * L, -1), data.cpu().numpy().reshape(B * L, -1), shape, *maps)
        assert np.all(np.abs(ssim.cpu().numpy() - ref_ssim) <= R.gate(ref_ssim)) and np.all(np.abs(mse.cpu().numpy() - ref_mse) <= R.gate(ref_mse))
    # the per-frame curves: the rows regrouped on the host
    for k in ('mse', 'psnr', 'ssim'):
        want = rows[k].cpu().numpy().astype(np.float64).reshape(-1, L).mean(axis=0)
        assert curves[k + '_t'].shape == (L,) and np.all(np.abs(curves[k + '_t'] - want) <= R.gate(want)), k
    plain = ev.rec_scores(dev)
    assert list(plain) == KEYS and all(plain[k] == res[k] for k in KEYS)
    # the frame cap: whole minibatches, at least one
    capped = SequenceEvaluator(tr, dict(S, REC_MAX_ROWS=2 * B * L + 1)).rec_scores(dev, return_rows=True)[1]
    assert capped['ssim'].shape[0] == 2 * B * L and torch.equal(capped['ssim'], rows['ssim'][:2 * B * L])
    assert SequenceEvaluator(tr, dict(S, REC_MAX_ROWS=1)).rec_scores(dev, return_rows=True)[1]['ssim'].shape[0] == B * L
    # data against itself through the two different maps: tanh range against the loader's units
    x = data
    mse, ssim = F.ssim_pairs(2.0 * (x / cfg.x_div) - 1.0, x, shape, *maps)
    assert np.all(np.abs(ssim.cpu().numpy() - 1.0) <= R.gate(1.0)) and np.all(mse.cpu().numpy() <= R.gate(0.0))


@pytest.mark.parametrize('script', ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs'])
def test_sequence_training_and_cli(gpu, tmp_path, capsys, script):
    """REC_EVERY leaves the training bit-identical and logs the four rows at the due iterations only; evaluate --rec prints them for a
    checkpoint without --out-dir, and with --out-dir writes the videos too"""
    import test_ssgan_eval_gpu as SQ
    from graphical_gan_amd import run, checkpoint, evaluate
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd.evaluate import SequenceEvaluator
    S0 = SQ._small(script)
    tr0, w0, a0 = SQ._train(dict(S0), run.config(S0))
    seen, orig, it0 = [], lib.plot.plot, lib.plot._iter[0]
    lib.plot.plot = lambda name, value: (seen.append((name, lib.plot._iter[0] - it0)), orig(name, value))[1]
    try:
        S1 = dict(S0, REC_EVERY=2)
        tr1, w1, a1 = SQ._train(S1, run.config(S1))
    finally:
        lib.plot.plot = orig
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1)
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for u, v in zip(a0[r], a1[r]):
            assert np.array_equal(u, v), r
    for key in KEYS:
        assert [i for n, i in seen if n == key] == [1, 3, 5], key
    assert not [n for n, _ in seen if n.startswith('dev ') and n not in KEYS]
    # the CLI on the checkpoint of those weights
    ckpt = str(tmp_path / 'params_6.npz')
    checkpoint.save(ckpt, tr1)
    live = SequenceEvaluator(tr1, S1).rec_scores(run.rec_sequences(S1, tr1.model, gpu))
    keys = ('BATCH_SIZE', 'LEN', 'DIM', 'DIM_LATENT_G', 'SYNTHETIC', 'SEED') + (('N_C',) if S0['N_C'] else ())
    args = [ckpt, '--script', script] + ['--set=%s=%s' % (k, S0[k]) for k in keys]
    P._fresh()
    capsys.readouterr()
    res = evaluate.main(args + ['--rec'])                                               # (no --out-dir: nothing is written)
    out = capsys.readouterr().out
    assert list(res) == KEYS
    for k in KEYS:
        assert res[k] == live[k], k
        assert '%s\t%s' % (k, live[k]) in out.splitlines()
    P._fresh()
    with pytest.raises(SystemExit):                                                     # without --rec the passes are files
        evaluate.main(args)
    P._fresh()
    both = evaluate.main(args + ['--rec', '--out-dir', str(tmp_path / 'cli')])
    assert all(both[k] == live[k] for k in KEYS) and len(both['files'].split()) == 8
    assert len(list((tmp_path / 'cli').iterdir())) == 8
