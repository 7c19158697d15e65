"""-m gpu: the evaluation-only exponential moving average of the generator-side weights -- the two kernels against a float64 restatement
of tf.train.ExponentialMovingAverage(decay, num_updates), the average riding in eager and captured steps without touching the training,
the visit of the averaged values in the parameters' own storage, checkpoints, and the evaluators / driver loop / CLI on top.

Bound of one ema_step_ launch per element: 4 * 2^-24 * max(|shadow|, |theta|) -- the kernel rounds four times (the quotient
(1 + t) / (10 + t), 1 - d, the difference, the product-and-subtract with or without contraction), each by at most half an ulp of a value
no larger than that maximum; after k launches k times that (the recurrence contracts earlier errors by d_t < 1)."""
import contextlib
import os

import numpy as np
import pytest

from test_ema_cpu import ema_ref

pytestmark = pytest.mark.gpu

U = 4.0 * 2.0 ** -24
GRID_CAP = 2048 * 256 * 4                  # elements one trip of the launcher's capped grid covers (2048 workgroups x 256 threads x float4)
SIZES = [1, 3, 4, 5, 255, 1025, GRID_CAP + 1027]
PAD = 8                                    # sentinel floats on both sides (a multiple of 4: the payload stays 16-byte aligned)
SENTINEL = -12345.678


def _fresh():
    from graphical_gan_amd import tflib as lib
    from graphical_gan_amd import optim
    optim.reset_optimizers()
    lib.delete_all_params()


def _padded(values, gpu):
    import torch
    buf = torch.full((values.size + 2 * PAD,), SENTINEL, dtype=torch.float32, device=gpu)
    buf[PAD:PAD + values.size].copy_(torch.as_tensor(values))
    return buf, buf[PAD:PAD + values.size]


def _sentinels_intact(buf):
    s = np.float32(SENTINEL)
    h = buf.cpu().numpy()
    return bool(np.all(h[:PAD] == s) and np.all(h[-PAD:] == s))


def _mixed(n, seed):
    """a shadow and weights around it at mixed scales (1e-3, 1, 100)"""
    rng = np.random.default_rng(seed)
    scale = np.asarray([1e-3, 1.0, 100.0])[rng.integers(0, 3, size=n)]
    shadow = (scale * rng.standard_normal(n)).astype(np.float32)
    theta = (shadow + scale * 0.1 * rng.standard_normal(n)).astype(np.float32)
    return shadow, theta


# ---- 1. ema_step_ ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_ema_step_against_float64(gpu, n):
    import torch
    from graphical_gan_amd import functional as F
    worst = 0.0
    for decay, ts in ((0.9, (1, 2, 79, 80, 81, 10 ** 6)), (0.999, (8989, 8990, 8991))):
        for t in ts:
            s0, th = _mixed(n, 1000 * n % 9973 + t % 97)
            sbuf, s = _padded(s0, gpu)
            tbuf, theta = _padded(th, gpu)
            step = torch.tensor([t], dtype=torch.int32, device=gpu)
            F.ema_step_(s, theta, step, decay)
            torch.cuda.synchronize()
            ref = ema_ref(s0, th, float(np.float32(decay)), t)              # (the kernel takes the decay as a float)
            err = np.abs(s.cpu().numpy().astype(np.float64) - ref)
            bound = U * np.maximum(np.abs(s0), np.abs(th)).astype(np.float64)
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (n, decay, t, float((err / bound).max()))
            assert np.array_equal(theta.cpu().numpy(), th) and int(step[0]) == t         # only read
            assert _sentinels_intact(sbuf) and _sentinels_intact(tbuf), (n, decay, t)
    print('ema_step_ n=%d: worst error %.2f of the bound 4 * 2^-24 * max(|shadow|, |theta|)' % (n, worst))


# ---- 2. swap_ --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_swap_is_bitwise_and_an_involution(gpu, n):
    import torch
    from graphical_gan_amd import functional as F
    a0, b0 = _mixed(n, n)
    a0[0], b0[-1] = np.float32(-0.0), np.float32('inf')                       # (bit patterns, not values)
    abuf, a = _padded(a0, gpu)
    bbuf, b = _padded(b0, gpu)
    F.swap_(a, b)
    torch.cuda.synchronize()
    bits = lambda x: x.cpu().numpy().view(np.uint32)
    assert np.array_equal(bits(a), b0.view(np.uint32)) and np.array_equal(bits(b), a0.view(np.uint32))
    assert _sentinels_intact(abuf) and _sentinels_intact(bbuf)
    F.swap_(a, b)
    torch.cuda.synchronize()
    assert np.array_equal(bits(a), a0.view(np.uint32)) and np.array_equal(bits(b), b0.view(np.uint32))
    assert _sentinels_intact(abuf) and _sentinels_intact(bbuf)


# ---- 3. trajectories -------------------------------------------------------------------------------------------------------------------
IMAGE_CASES = [('cifar10', 8, 0, 'ali', 8, 16), ('cifar10', 8, 5, 'local_ep', 8, 16), ('cifar10', 8, 0, 'wali', 8, 16),
               ('cifar10', 8, 0, 'wali-gp', 8, 16)]
SS_KW = dict(batch_size=4, length=3, dim=4, dim_op=16, dim_g=8, dim_l=4)
CASES = IMAGE_CASES + ['ssgan']
DECAY = 0.9


def _mk(case, graph, gpu, ema_decay=None, n_c=10):
    """as tests/test_step_gpu.py::_mk and tests/test_ssgan_gpu.py::_mk build them, with the Trainer's ema_decay -> (trainer, feeds)"""
    from graphical_gan_amd.engine import Trainer
    if case == 'ssgan':
        from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
        from oracle import ssgan as O
        kw = dict(SS_KW, pos_mode='naive_mean_field', op_dyn_mode='res', channels=1, n_c=n_c, mode='local_ep', ali_mode='concat_x')
        ocfg = O.Cfg(**kw)
        P0 = O.init_params(ocfg, seed=0)
        rng = np.random.default_rng(5)
        for k in P0:
            if k.endswith('.b') or k.endswith('.Biases'):
                P0[k] = (0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
        _fresh()
        cfg = SSConfig(dataset='moving_mnist', **kw)
        tr = Trainer(cfg, device=gpu, graph=graph, inject_noise=True, model=StateSpaceGAN(cfg), ema_decay=ema_decay)
        tr.load_params(P0)
        rng = np.random.default_rng(9)
        return tr, [O.make_feed(ocfg, rng) for _ in range(16)]
    from graphical_gan_amd.models import Config
    from oracle import nets as N, step as S
    dataset, B, K, mode, dim, dl = case
    ocfg = N.Cfg(dataset, batch_size=B, n_coms=K, dim=dim, dim_latent=dl, latent_critic=False, learn_std=False, z_samples=100, bn=None)
    P0 = N.init_params(ocfg, seed=0)
    rng = np.random.default_rng(7)
    for k in P0:
        if P0[k].ndim <= 2 and ('Biases' in k or k.endswith('.b') or 'offset' in k):
            P0[k] = (0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
        if k.endswith('.scale'):
            P0[k] = (1 + 0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
    _fresh()
    cfg = Config(dataset, batch_size=B, n_coms=K, mode=mode, dim=dim, dim_latent=dl, fuse=True, bn=None)
    tr = Trainer(cfg, device=gpu, graph=graph, inject_noise=True, ema_decay=ema_decay)
    tr.load_params(P0)
    omode = mode if mode in ('wali', 'wali-gp') else 'ali'
    return tr, [S.make_feed(ocfg, np.random.default_rng(100 + i), omode) for i in range(4 * (1 + 5))]


def _states():
    from graphical_gan_amd import optim
    return {key[0]: {k: v.cpu().numpy() for k, v in o.state_dict().items() if k in ('m', 'v', 'step')} for key, o in optim._optimizers.items()}


def _gen_names():
    from graphical_gan_amd import optim
    return [p.param_name for key, o in optim._optimizers.items() if key[0] == 'gen' for p in o.params]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_RUNS = {}


def _run(case, graph, ema, gpu, no_pack=False):
    """four iterations -> per iteration {costs, live weights, Adam states, averaged weights}; computed once per (case, graph, ema, no_pack)"""
    import torch
    from graphical_gan_amd import optim
    key = (str(case), graph, ema, no_pack)
    if key in _RUNS:
        return _RUNS[key]
    with _env(GGAN_NO_PACK_ADAM='1') if no_pack else contextlib.nullcontext():
        tr, feeds = _mk(case, graph, gpu, DECAY if ema else None)
        P0 = tr.get_params()
        it_feeds, rec = iter(feeds), []
        for it in range(4):
            res = tr.iteration(it, it_feeds)
            torch.cuda.synchronize()
            rec.append(dict(costs={k: float(v) for k, v in res.items()}, live=tr.get_params(), states=_states(),
                            ema=tr.get_params(weights='ema') if ema else None))
        shadows = {key[0]: o.shadow is not None for key, o in optim._optimizers.items()}
        fused = {key[0]: o.can_fuse_update() for key, o in optim._optimizers.items()}
    _RUNS[key] = dict(P0=P0, its=rec, gen=_gen_names(), shadows=shadows, fused=fused)
    return _RUNS[key]


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipgraph'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c if isinstance(c, str) else '-'.join(str(x) for x in c))
def test_trajectory_with_the_average_riding_along(gpu, case, graph):
    off, on = _run(case, graph, False, gpu), _run(case, graph, True, gpu)
    # (e) the generator side averages, the critic does not; with averaging off nobody does
    assert on['shadows'] == {'gen': True, 'disc': False} and off['shadows'] == {'gen': False, 'disc': False}
    gen = on['gen']
    assert gen and gen == off['gen'] and any(n.startswith('Generator') for n in gen) and not any(n.startswith('Discriminator') for n in gen)
    # (a) the training does not notice: weights, costs and both optimizer states bit for bit, after every iteration
    for it, (a, b) in enumerate(zip(off['its'], on['its'])):
        assert a['costs'] == b['costs'], (it, a['costs'], b['costs'])
        assert _same(a['live'], b['live']), it
        for role in ('gen', 'disc'):
            if role in a['states'] or role in b['states']:
                assert _same(a['states'][role], b['states'][role]), (it, role)
    # (b) the average: the initial weights until the first generator update, then the float64 recurrence on the recorded weights
    P0 = on['P0']
    assert _same(on['its'][0]['ema'], on['its'][0]['live'])                  # (iteration 0 is a critic step: the critic's are live values)
    assert all(np.array_equal(on['its'][0]['ema'][n], P0[n]) for n in gen)
    ref = {n: P0[n].astype(np.float64) for n in gen}
    top = {n: np.abs(ref[n]) for n in gen}
    d32 = float(np.float32(DECAY))
    worst = 0.0
    for k in (1, 2, 3):
        rec = on['its'][k]
        assert int(rec['states']['gen']['step'][0]) == k
        for n in gen:
            theta = rec['live'][n].astype(np.float64)
            top[n] = np.maximum(top[n], np.abs(theta))
            ref[n] = ema_ref(ref[n], theta, d32, k)
            err = np.abs(rec['ema'][n].astype(np.float64) - ref[n])
            bound = k * U * top[n]
            assert np.all(err <= bound), (k, n, float(err.max()))
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert any(not np.array_equal(rec['ema'][n], rec['live'][n]) for n in gen), k       # (an average, not a copy)
        for n in rec['live']:                                                # everything else reads as its live value
            if n not in gen:
                assert np.array_equal(rec['ema'][n], rec['live'][n]), (k, n)
    print('average after 3 updates, %s graph=%s: worst error %.2f of the bound' % (case, graph, worst))
    # (c) eager and captured steps keep the same average, bit for bit (the captures' warm-up and rehearsal steps left no trace in it)
    other = _run(case, not graph, True, gpu)
    for it in range(4):
        assert _same(other['its'][it]['ema'], on['its'][it]['ema']), it


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipgraph'])
@pytest.mark.parametrize('case', CASES, ids=lambda c: c if isinstance(c, str) else '-'.join(str(x) for x in c))
def test_the_separate_adam_launch_keeps_the_same_average(gpu, case, graph):
    """(d) GGAN_NO_PACK_ADAM=1: the update is a launch of its own (adam_k, then ema_k; captured as two nodes in the graph variant, as the
    data-parallel graphs capture them) instead of riding in the pack launch; the average follows either.  The wali case's RMSProp update
    never rides in the pack launch, so there the two runs take the same path and the check is that the switch changes nothing."""
    fused, apart = _run(case, graph, True, gpu), _run(case, graph, True, gpu, no_pack=True)
    assert not apart['fused']['gen'] and not apart['fused']['disc']
    if case != 'ssgan':
        assert fused['fused']['gen'] == (case[3] != 'wali'), case
    for it in range(4):
        assert _same(fused['its'][it]['ema'], apart['its'][it]['ema']), it
        assert _same(fused['its'][it]['live'], apart['its'][it]['live']), it


# ---- 4. ema_weights() ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'hipgraph'])
def test_the_averaged_weights_visit_the_live_storage_and_leave_no_trace(gpu, graph):
    import torch
    from graphical_gan_amd import tflib as lib
    case = IMAGE_CASES[0]
    never = _run(case, graph, True, gpu)                                      # four iterations, never entered
    tr, feeds = _mk(case, graph, gpu, DECAY)
    it_feeds = iter(feeds)
    with pytest.raises(RuntimeError, match='first generator step'):          # the generator-side optimizer does not exist yet
        with tr.ema_weights():
            pass
    for it in range(2):
        tr.iteration(it, it_feeds)
    live, avg = tr.get_params(), tr.get_params(weights='ema')
    gen = _gen_names()
    assert any(not np.array_equal(live[n], avg[n]) for n in gen)
    registry = lambda: {n: p.detach().cpu().numpy().copy() for n, p in lib.named_params().items()}
    ptrs = {n: p.data_ptr() for n, p in lib.named_params().items()}
    with tr.ema_weights():
        assert _same(registry(), avg)                                         # the parameters hold the averaged values, bitwise ...
        assert {n: p.data_ptr() for n, p in lib.named_params().items()} == ptrs            # ... in their own storage
        assert _same(tr.get_params(weights='ema'), avg) and _same(tr.get_params(), live)   # (both views stay what they are)
        with tr.ema_weights():                                                # entering twice is harmless
            assert _same(registry(), avg)
        assert _same(registry(), avg)
        with pytest.raises(RuntimeError, match='ema_weights'):               # no training step on the visiting weights
            tr.step('gen')
    assert _same(registry(), live) and _same(tr.get_params(weights='ema'), avg)

    class Boom(Exception):
        pass
    with pytest.raises(Boom):
        with tr.ema_weights():
            raise Boom()
    assert _same(registry(), live) and _same(tr.get_params(weights='ema'), avg)          # an exception still swaps back
    for it in range(2, 4):
        tr.iteration(it, it_feeds)
    torch.cuda.synchronize()
    assert _same(tr.get_params(), never['its'][3]['live']) and _same(tr.get_params(weights='ema'), never['its'][3]['ema'])
    # averaging off: a clear error, and no average to read
    tr, feeds = _mk(case, False, gpu, None)
    it_feeds = iter(feeds)
    for it in range(2):
        tr.iteration(it, it_feeds)
    with pytest.raises(RuntimeError, match='without ema_decay'):
        with tr.ema_weights():
            pass
    with pytest.raises(RuntimeError, match='without ema_decay'):
        tr.get_params(weights='ema')


def test_a_second_trainer_leaves_a_live_optimizer_as_it_was_built(gpu):
    """captured graphs hold the launch and the shadow's address: a Trainer built later, without a reset, neither drops nor adds either"""
    from graphical_gan_amd import optim
    from graphical_gan_amd.engine import Trainer
    case = IMAGE_CASES[0]
    never = _run(case, True, True, gpu)                                                 # four iterations, no second Trainer
    tr, feeds = _mk(case, True, gpu, DECAY)
    it_feeds = iter(feeds)
    for it in range(3):
        tr.iteration(it, it_feeds)
    opt = next(o for key, o in optim._optimizers.items() if key[0] == 'gen')
    ptr = opt.shadow.data_ptr()
    other = Trainer(tr.cfg, device=gpu, graph=False, inject_noise=True)                  # no average asked for, no reset
    assert opt.shadow is not None and opt.shadow.data_ptr() == ptr and opt.ema_decay == DECAY
    tr.iteration(3, it_feeds)                                                           # the first Trainer's graphs still have their buffer
    assert _same(tr.get_params(weights='ema'), never['its'][3]['ema']) and _same(tr.get_params(), never['its'][3]['live'])
    assert other.ema_decay is None
    # ... and the other way round: asking for an average over a live optimizer built without one says so
    tr, feeds = _mk(case, False, gpu, None)
    it_feeds = iter(feeds)
    for it in range(2):
        tr.iteration(it, it_feeds)
    late = Trainer(tr.cfg, device=gpu, graph=False, inject_noise=True, ema_decay=DECAY)
    assert next(o for key, o in optim._optimizers.items() if key[0] == 'gen').shadow is None
    with pytest.raises(RuntimeError, match='reset_optimizers'):
        with late.ema_weights():
            pass


# ---- 5. checkpoint ---------------------------------------------------------------------------------------------------------------------
def test_checkpoint_carries_the_average_and_resumes_bit_exact(gpu, tmp_path):
    from graphical_gan_amd import checkpoint
    case = IMAGE_CASES[0]
    tr, feeds = _mk(case, False, gpu, DECAY)
    it_feeds = iter(feeds)
    for it in range(3):
        tr.iteration(it, it_feeds)
    path = str(tmp_path / 'ck.npz')
    keys = checkpoint.save(path, tr)
    assert 'ema/gen/Generator.Input.W' in keys and 'ema/gen/decay' in keys and 'adam/gen/step' in keys
    assert not [k for k in keys if k.startswith('ema/disc') or k.startswith('ema/gen/Discriminator')]
    z = np.load(path)
    assert float(z['ema/gen/decay']) == DECAY and z['ema/gen/Generator.Input.W'].shape == z['Generator.Input.W'].shape
    assert np.array_equal(z['ema/gen/Generator.Input.W'], tr.get_params(weights='ema')['Generator.Input.W'])
    rest = feeds[5:]                                     # it 0: 1 feed, it 1-2: 2 feeds each
    a = iter(rest)
    for it in range(3, 5):
        tr.iteration(it, a)
    PA, EA = tr.get_params(), tr.get_params(weights='ema')
    tr2, _ = _mk(case, False, gpu, DECAY)                # fresh registry, initial weights
    checkpoint.restore(path, tr2)                        # no optimizer yet: the average is parked with the Adam state
    assert sorted(tr2.get_params()) == sorted(PA)        # (no ema/ key became a parameter)
    b = iter(rest)
    for it in range(3, 5):
        tr2.iteration(it, b)
    assert _same(tr2.get_params(), PA) and _same(tr2.get_params(weights='ema'), EA)
    # ... and into LIVE optimizers
    checkpoint.restore(path, tr2)
    assert np.array_equal(tr2.get_params(weights='ema')['Generator.Input.W'], z['ema/gen/Generator.Input.W'])
    b = iter(rest)
    for it in range(3, 5):
        tr2.iteration(it, b)
    assert _same(tr2.get_params(), PA) and _same(tr2.get_params(weights='ema'), EA)
    # a checkpoint with ema/ keys restores into a trainer that does not average: ignored
    tr3, _ = _mk(case, False, gpu, None)
    checkpoint.restore(path, tr3)
    b = iter(rest)
    for it in range(3, 5):
        tr3.iteration(it, b)
    assert _same(tr3.get_params(), PA)
    with pytest.raises(RuntimeError):
        tr3.get_params(weights='ema')
    plain = str(tmp_path / 'plain.npz')
    keys = checkpoint.save(plain, tr3)                   # saved with averaging off: today's keys
    assert not [k for k in keys if k.startswith('ema/')]
    # ... restored into an averaging trainer: the average starts from the restored weights (parked state and live optimizer alike)
    tr4, _ = _mk(case, False, gpu, DECAY)
    checkpoint.restore(plain, tr4)
    assert _same(tr4.get_params(weights='ema'), PA)
    c = iter(feeds)
    for it in range(5, 7):
        tr4.iteration(it, c)
    assert not _same(tr4.get_params(weights='ema'), tr4.get_params())
    checkpoint.restore(plain, tr4)
    assert _same(tr4.get_params(weights='ema'), PA) and _same(tr4.get_params(), PA)


# ---- 6. evaluators, the driver loop, the CLI -----------------------------------------------------------------------------------------------
def test_evaluator_on_averaged_weights_equals_a_trainer_holding_them(gpu):
    from graphical_gan_amd.evaluate import Evaluator
    case = IMAGE_CASES[0]
    S = dict(BATCH_SIZE=8, MODE='ali', SEED=3)
    tr, feeds = _mk(case, False, gpu, DECAY)
    it_feeds = iter(feeds)
    for it in range(3):
        tr.iteration(it, it_feeds)
    dev = tr.model.synthetic_ring(gpu, n=3, seed=4321)

    def scores(trainer, weights):
        ev = Evaluator(trainer, S)
        ev.weights = weights
        return dict(ev.dev_costs(dev), **ev.rec_scores(dev))
    live, avg = scores(tr, 'live'), scores(tr, 'ema')
    before = tr.get_params()
    assert sorted(live) == sorted(avg) and 'dev gen cost' in avg and 'dev rec ssim x' in avg
    assert all(avg[k] != live[k] for k in ('dev gen cost', 'dev rec mse x', 'dev rec ssim x')), (avg, live)
    P = tr.get_params(weights='ema')
    assert _same(tr.get_params(), before)                                     # the passes left the live weights as they were
    tr2, _ = _mk(case, False, gpu, None)
    tr2.load_params(P)
    assert scores(tr2, 'live') == avg                                         # the same kernels on the same inputs: bit for bit
    with pytest.raises(RuntimeError, match='without ema_decay'):
        scores(tr2, 'ema')
    ev = Evaluator(tr2, S)
    ev.weights = 'average'
    with pytest.raises(ValueError):
        ev.dev_costs(dev)


def test_sequence_evaluator_on_averaged_weights(gpu):
    """the state-space case with N_C = 2: SequenceEvaluator needs N_VIS = BATCH_SIZE = 4 to be a multiple of N_C, which the trajectories'
    N_C = 10 is not"""
    from graphical_gan_amd.evaluate import SequenceEvaluator
    S = dict(BATCH_SIZE=4, N_VIS=4, SEED=3)
    tr, feeds = _mk('ssgan', False, gpu, DECAY, n_c=2)
    it_feeds = iter(feeds)
    for it in range(3):
        tr.iteration(it, it_feeds)
    dev = [(f['real_x_unit'], f['real_y']) for f in feeds[8:10]]

    def scores(trainer, weights):
        ev = SequenceEvaluator(trainer, S)
        ev.weights = weights
        return ev.rec_scores(dev)
    live, avg = scores(tr, 'live'), scores(tr, 'ema')
    assert avg['dev rec mse x'] != live['dev rec mse x'] and avg['dev rec ssim x'] != live['dev rec ssim x']
    P = tr.get_params(weights='ema')
    tr2, _ = _mk('ssgan', False, gpu, None, n_c=2)
    tr2.load_params(P)
    assert scores(tr2, 'live') == avg


def _train(S, cfg):
    from graphical_gan_amd import run
    from graphical_gan_amd import tflib as lib
    _fresh()
    seen = []
    orig = lib.plot.plot
    it0 = lib.plot._iter[0]

    def rec(name, value):
        seen.append((name, lib.plot._iter[0] - it0, float(value)))
        orig(name, value)
    lib.plot.plot = rec
    try:
        tr = run.train(S, cfg)
    finally:
        lib.plot.plot = orig
    return tr, tr.get_params(), seen


def test_driver_loop_scores_both_and_the_cli_reads_the_average(gpu, tmp_path, capsys):
    from graphical_gan_amd import evaluate
    from graphical_gan_amd.models import Config
    cfg = lambda: Config('cifar10', batch_size=8, mode='ali', dim=8, dim_latent=16)
    base = dict(DATASET='cifar10', BATCH_SIZE=8, MODE='ali', ITERS=5, LOG_EVERY=2, SYNTHETIC='force', EMA_DECAY=.9, DEV_EVERY=2, REC_EVERY=2,
                SAVE_EVERY=5)
    out_live, out_both = tmp_path / 'live', tmp_path / 'both'
    _, w_live, seen_live = _train(dict(base, EMA_EVAL='live', OUT_DIR=str(out_live)), cfg())
    tr, w_both, seen_both = _train(dict(base, EMA_EVAL='both', OUT_DIR=str(out_both)), cfg())
    assert _same(w_live, w_both)                                              # the final weights do not depend on what was scored
    at = lambda seen, name: [i for n, i, _ in seen if n == name]
    for name in ('dev gen cost', 'dev rec mse x', 'dev rec ssim x'):
        assert at(seen_both, name) == [1, 3] and at(seen_both, name + ' ema') == [1, 3], name
        assert at(seen_live, name) == [1, 3] and at(seen_live, name + ' ema') == [], name
    val = lambda name, i: [v for n, j, v in seen_both if n == name and j == i][0]
    assert val('dev rec mse x ema', 3) != val('dev rec mse x', 3)
    names = sorted(os.listdir(str(out_both)))
    assert 'samples_5.png' in names and 'samples_5_ema.png' in names and 'params_5.npz' in names
    assert 'samples_5_ema.png' in os.listdir(str(out_live))                  # (the grid follows the average, not what the passes score)
    log = open(str(out_both / 'logfile.txt')).read()
    assert 'dev gen cost ema' in log and 'dev rec mse x ema' in log
    z = np.load(str(out_both / 'params_5.npz'))
    assert 'ema/gen/Generator.Input.W' in z.files and float(z['ema/gen/decay']) == .9
    avg = tr.get_params(weights='ema')
    assert np.array_equal(z['ema/gen/Generator.Input.W'], avg['Generator.Input.W'])
    # the CLI on that checkpoint: the ' ema' rows, from the averaged weights
    args = [str(out_both / 'params_5.npz'), '--script', 'gan_inference_cifar10', '--rec'] + \
           ['--set=%s=%s' % kv for kv in dict(DIM=8, DIM_LATENT=16, BATCH_SIZE=8, SYNTHETIC='force').items()]
    _fresh()
    np.random.seed(5)
    capsys.readouterr()
    res = evaluate.main(args + ['--ema'])
    printed = capsys.readouterr().out
    assert 'dev gen cost ema' in res and 'dev rec mse x ema' in res and not [k for k in res if not k.endswith(' ema')]
    assert 'dev rec mse x ema\t%s' % res['dev rec mse x ema'] in printed.splitlines()
    _fresh()
    np.random.seed(5)
    plain = evaluate.main(args)
    assert sorted(k + ' ema' for k in plain) == sorted(res) and plain['dev rec mse x'] != res['dev rec mse x ema']
    # a checkpoint of a run that did not average: refused with the keys it lacks
    off = tmp_path / 'off'
    _train(dict(base, EMA_DECAY=None, EMA_EVAL=None, OUT_DIR=str(off)), cfg())
    assert 'samples_5.png' in os.listdir(str(off)) and 'samples_5_ema.png' not in os.listdir(str(off))
    assert not [k for k in np.load(str(off / 'params_5.npz')).files if k.startswith('ema/')]
    _fresh()
    args[0] = str(off / 'params_5.npz')
    with pytest.raises(SystemExit):
        evaluate.main(args + ['--ema'])
    assert 'ema/gen/' in capsys.readouterr().err
