"""not-gpu: the float64 restatement of tests/_cls_ref.py against closed forms, the built library's new entry points, the switch, the flag and
the keyword of the classifier pass, and the host logic of classifier.ImageClassifier on CPU tensors (registry, numpy state, files)."""
import argparse
import ctypes as C
import glob
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cls_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_mnist', 'gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_face',
                 'gmgan_inference_mnist', 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_softmax_xent_workspace', 'ggan_softmax_xent_fwd_grad', 'ggan_class_score_workspace', 'ggan_class_score']


# ---- the restatement against closed forms ------------------------------------------------------------------------------------------------------
def test_uniform_posteriors_score_one_and_balanced_one_hot_posteriors_score_the_class_count():
    scores, mean, std, h_row, h_marg = R.class_score(np.zeros((120, 6)), 4)
    assert np.allclose(scores, 1.0, atol=1e-14) and abs(mean - 1.0) < 1e-14 and std < 1e-14
    assert abs(h_row - np.log(6)) < 1e-14 and abs(h_marg - np.log(6)) < 1e-14
    for Cc in (2, 7, 10):
        x = 200.0 * np.eye(Cc)[np.arange(12 * Cc) % Cc]             # confident, every class as often as every other in every split
        scores, mean, std, h_row, h_marg = R.class_score(x, 3)
        assert np.allclose(scores, Cc, rtol=1e-12) and abs(mean - Cc) < 1e-10 and std < 1e-10
        assert h_row < 1e-12 and abs(h_marg - np.log(Cc)) < 1e-12


def test_the_two_pass_form_and_the_entropy_identity_agree_in_float64():
    for row in R.SCORE_ROWS[:-1]:
        x = R.score_inputs(*row)
        a, b = R.class_score(x, row[2])[0], R.class_score_identity(x, row[2])
        assert np.max(np.abs(a - b) / a) < 1e-12, row


def test_split_boundaries_are_the_reference_integer_divisions_and_std_is_the_population_form():
    N, S = 1003, 10
    bounds = R.split_bounds(N, S)
    assert bounds == [((i * N) // S, ((i + 1) * N) // S) for i in range(S)]
    assert bounds[0] == (0, 100) and bounds[-1] == (902, 1003) and sorted(b - a for a, b in bounds) == [100] * 7 + [101] * 3
    assert all(bounds[i][1] == bounds[i + 1][0] for i in range(S - 1))
    x = R.score_inputs(N, 10, S, 3.0)
    scores, mean, std, _, _ = R.class_score(x, S)
    for s, (a, b) in enumerate(bounds):                                # a split's score is the score of its rows alone
        assert abs(R.class_score(x[a:b], 1)[0][0] - scores[s]) < 1e-12
    assert abs(std - np.sqrt(np.mean((scores - mean) ** 2))) < 1e-15 and abs(std - np.std(scores, ddof=1)) > 1e-3 * std


def test_the_literal_float32_form_is_nan_at_scale_80_where_the_restatement_stays_finite():
    rng = np.random.default_rng(0)
    x = (80.0 * rng.standard_normal((100, 10))).astype(np.float32)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    assert np.sum((e / e.sum(axis=1, keepdims=True)).astype(np.float32) == 0) > 100      # many posteriors underflow
    assert np.all(np.isnan(R.class_score_literal32(x, 2)))
    scores, mean, std, h_row, h_marg = R.class_score(x, 2)
    assert np.all(np.isfinite(scores)) and all(np.isfinite(v) for v in (mean, std, h_row, h_marg))
    mild = (rng.standard_normal((100, 10))).astype(np.float32)          # ... and where nothing underflows the two agree
    assert np.allclose(R.class_score_literal32(mild, 2), R.class_score(mild, 2)[0], rtol=1e-5)


def test_xent_restatement_against_closed_forms():
    loss, dl, hits = R.xent(np.zeros((5, 8)), np.arange(5))
    assert abs(loss - np.log(8)) < 1e-15 and hits == 1                   # (all tied: the lowest class, row 0's label)
    assert np.allclose(dl.sum(axis=1), 0, atol=1e-15) and np.allclose(dl[0], (np.full(8, 1 / 8) - np.eye(8)[0]) / 5)
    x, y, t = R.xent_inputs(100, 10, 80.0)
    loss, dl, hits = R.xent(x, y)
    assert np.isfinite(loss) and np.max(np.abs(dl.sum(axis=1))) < 1e-15 and hits == int(np.sum(np.argmax(x, 1) == y)) and np.argmax(x[t]) < y[t]
    eps = 1e-6                                                          # the gradient is the gradient
    xp = np.array(x[:4] / 80.0, np.float64)
    g = R.xent(xp, y[:4])[1]
    for (i, j) in ((0, 0), (1, 3), (3, 9)):
        d = np.zeros_like(xp)
        d[i, j] = eps
        assert abs((R.xent(xp + d, y[:4])[0] - R.xent(xp - d, y[:4])[0]) / (2 * eps) - g[i, j]) < 1e-8


def test_a_float32_evaluation_of_the_row_operations_stays_inside_the_derived_dlogits_gate():
    """the gate of _cls_ref's docstring against the operations it counts, each rounded to float32 by numpy: a derivation that forgot a term
    would be missed here on the CPU, and one that is orders too wide shows as a tiny fraction"""
    f = np.float32
    worst = 0.0
    for (B, Cc) in R.XENT_ROWS:
        for scale in R.XENT_SCALES:
            x, y, _ = R.xent_inputs(B, Cc, scale)
            d = x - x.max(axis=1, keepdims=True)
            e = np.exp(d, dtype=f)
            s = e.sum(axis=1, keepdims=True, dtype=f)
            dl = ((e / s) - np.eye(Cc, dtype=f)[y]) / f(B)
            assert dl.dtype == f
            frac = float(np.max(np.abs(dl.astype(np.float64) - R.xent(x, y)[1]))) / R.dl_gate(B, Cc)
            sums = float(np.max(np.abs(dl.astype(np.float64).sum(axis=1)))) / (Cc * R.dl_gate(B, Cc))
            print('float32 numpy %s: dlogits %.4f, row sums %.4f of the gate' % (R.xent_id(B, Cc, scale), frac, sums))
            assert frac <= 1.0 and sums <= 1.0, (B, Cc, scale, frac, sums)
            worst = max(worst, frac)
    assert worst >= 0.01            # (the gate is within two orders of what float32 really does)


# ---- the built library -----------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_declared_and_bound(lib_built):
    from graphical_gan_amd import _lib, build, functional as F
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert lib.ggan_version() == _lib.ABI_VERSION == int(re.search(r'#define GGAN_ABI_VERSION (\d+)', hdr).group(1))
    assert 'class_score.hip' in build.SOURCES
    raw = C.CDLL(lib_built)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    const = lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
    assert (F.CLS_MAX_CLASSES, F.CLS_MAX_SPLITS) == (const('GGAN_CLS_MAX_CLASSES'), const('GGAN_CLS_MAX_SPLITS')) == (R.MAX_CLASSES, R.MAX_SPLITS) == (64, 64)
    assert (F.CLS_BAD_LABEL, F.CLS_NONFINITE) == (const('GGAN_CLS_BAD_LABEL'), const('GGAN_CLS_NONFINITE')) == (R.BAD_LABEL, R.NONFINITE)
    assert const('GGAN_CLS_ROW_BLOCK') == R.ROW_BLOCK and (F.CLS_MAX_BATCH, F.CLS_SCORE_MAX_ROWS) == (R.MAX_BATCH, R.MAX_ROWS)
    # the workspace twins: 0 out of range, enough for the partials inside
    assert lib.ggan_softmax_xent_workspace(0, 10) == 0 and lib.ggan_softmax_xent_workspace(8, 1) == 0 and lib.ggan_softmax_xent_workspace(8, 65) == 0
    assert lib.ggan_softmax_xent_workspace(65537, 10) == 0 and lib.ggan_softmax_xent_workspace(4099, 7) >= 65 * 16
    assert lib.ggan_class_score_workspace(100, 10, 0) == 0 and lib.ggan_class_score_workspace(5, 10, 6) == 0 and lib.ggan_class_score_workspace(100, 10, 65) == 0
    assert lib.ggan_class_score_workspace(1 << 20, 64, 1) >= 4096 * 65 * 8 and lib.ggan_class_score_workspace((1 << 20) + 1, 64, 1) == 0
    # refused with a message before any launch: no device is needed to be told
    p = C.c_void_p(256)
    assert lib.ggan_softmax_xent_fwd_grad(p, p, 0, 10, p, p, p, p, p, 1 << 20, None) < 0 and b'classes' in lib.ggan_last_error()
    assert lib.ggan_class_score(p, 100, 10, 65, p, p, p, p, 1 << 20, None) < 0 and b'splits' in lib.ggan_last_error()
    assert lib.ggan_class_score(None, 100, 10, 10, p, p, p, p, 1 << 20, None) < 0 and b'null' in lib.ggan_last_error()


def test_the_functions_refuse_cpu_tensors(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    with pytest.raises(_lib.GganError):
        F.softmax_xent(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.GganError):
        F.SoftmaxXent.apply(torch.zeros(4, 10), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(_lib.GganError):
        F.class_score(torch.zeros(40, 10), 4)


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_classifier_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_CLS_EVERY', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.classifier_settings(s) == {} and run.classifier_settings('/somewhere/%s.py' % s) == {}
    others = lambda s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s), run.probe_settings(s), run.frechet_settings(s),
                        run.swd_settings(s))
    base = {s: others(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_CLS_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.classifier_settings(s) == {'CLS_EVERY': 20} and run.classifier_settings('/somewhere/%s.py' % s) == {'CLS_EVERY': 20}
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.classifier_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert others(s) == base[s]
    S = dict(run.reference_block('gan_inference_cifar10'), **run.classifier_settings('gan_inference_cifar10'))
    assert [it for it in range(60) if run.classifier_due(S, it)] == [19, 39, 59]
    assert run.eval_plan(S) is None and not any(run.scores_due(S, it) or run.probe_due(S, it) or run.frechet_due(S, it) or run.swd_due(S, it) for it in range(60))
    assert not any(run.classifier_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_the_eight_image_scripts_carry_the_line():
    line = 'SETTINGS.update(run.classifier_settings(__file__))'
    seen = {os.path.splitext(os.path.basename(p))[0]: open(p).read().count(line) for p in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py'))}
    assert seen == dict([(s, 1) for s in IMAGE_SCRIPTS] + [(s, 0) for s in SEQUENCE_SCRIPTS])


def test_classifier_sets_without_labelled_training_data_and_shared_with_the_probe(tmp_path, monkeypatch):
    from graphical_gan_amd import run
    state = np.random.get_state()[1].tobytes()
    assert run.classifier_sets(dict(DATASET='face', BATCH_SIZE=8)) is None
    assert run.classifier_sets(dict(DATASET='cifar10', BATCH_SIZE=8, SYNTHETIC='force')) is None
    assert run.classifier_sets(dict(DATASET='cifar10', BATCH_SIZE=8, DATA_DIR='/no/such/dir')) is None
    import gzip
    import pickle
    rng = np.random.default_rng(0)
    mk = lambda n: (rng.random((n, 784), dtype=np.float32), rng.integers(0, 10, size=n))
    with gzip.open(str(tmp_path / 'mnist.pkl.gz'), 'wb') as f:
        pickle.dump((mk(64), mk(24), mk(20)), f)
    monkeypatch.setenv('GGAN_MNIST', str(tmp_path / 'mnist.pkl.gz'))
    S = dict(DATASET='mnist', BATCH_SIZE=8, CLS_FIT_ROWS=40, PROBE_FIT_ROWS=16)
    fit, again, probe = run.classifier_sets(S), run.classifier_sets(S), run.probe_sets(S)
    assert len(fit) == 5 and len(probe) == 2 and all(x.shape == (8, 784) and y.shape == (8,) for x, y in fit)
    for (a, b), (c, d) in list(zip(fit, again)) + list(zip(fit, probe)):          # the same rows every time; the probe's rows lead them
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert np.random.get_state()[1].tobytes() == state
    assert inspect.getsource(run.classifier_sets).count('_leading_training_rows') == 1 == inspect.getsource(run.probe_sets).count('_leading_training_rows')


def test_the_flag_parses_and_the_state_space_scripts_refuse_it(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--cls']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert parsed[0].cls is False and parsed[1].cls is True and parsed[1].probe is False and parsed[1].frechet is False and parsed[1].swd is False
    for script in SEQUENCE_SCRIPTS:            # refused before anything is built: the checkpoint does not even exist
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--cls', '--out-dir', 'x'])
        assert e.value.code == 2 and '--cls: the state-space scripts have no single set of images' in capsys.readouterr().err


def test_the_pass_is_no_row_of_the_table_and_checks_its_settings():
    from graphical_gan_amd import evaluate
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    sig = inspect.signature(evaluate.evaluate_once)
    names = list(sig.parameters)
    assert names.index('swd') < names.index('cls') < names.index('scores') and sig.parameters['cls'].default is False
    assert evaluate.CLS_KEYS == ('dev classifier score x', 'dev classifier score std x', 'dev classifier score data', 'dev classifier accuracy',
                                 'dev classifier frechet x')
    assert not any('inception' in k for k in evaluate.CLS_KEYS)
    assert (evaluate.CLS_SAMPLES, evaluate.CLS_MAX_ROWS, evaluate.CLS_SPLITS, evaluate.CLS_FIT_ROWS, evaluate.CLS_EPOCHS) == (50000, 10000, 10, 20000, 4)

    class Cfg:
        B = 4
    ev = object.__new__(evaluate.Evaluator)
    ev.S, ev.cfg = {}, Cfg()
    xs = [(np.zeros((4, 6), np.float32), np.zeros(4, np.int64))]
    with pytest.raises(ValueError, match='labelled'):
        ev.classifier_scores(xs, [np.zeros((4, 6), np.float32)])
    with pytest.raises(ValueError, match='labelled'):
        ev.classifier_scores([], xs)
    with pytest.raises(ValueError, match='at most 64 classes'):
        ev.classifier_scores(xs, [(xs[0][0], np.full(4, 64))])
    for key, bad in (('CLS_SAMPLES', 3), ('CLS_SAMPLES', (1 << 20) + 1), ('CLS_MAX_ROWS', 1), ('CLS_SPLITS', 0), ('CLS_SPLITS', 65)):
        ev.S = {key: bad}
        with pytest.raises(ValueError, match=key):
            ev.classifier_scores(xs, xs)


# ---- the classifier's host logic, on CPU tensors ---------------------------------------------------------------------------------------------
def _cfg(dataset='mnist', dim=8):
    from graphical_gan_amd.models import Config
    return Config(dataset, batch_size=8, dim=dim, dim_latent=16)


def test_the_classifier_keeps_out_of_the_registry_and_of_the_global_numpy_state():
    import torch
    from graphical_gan_amd import classifier as K, optim
    from graphical_gan_amd import tflib as lib
    registry, optimizers = dict(lib.named_params()), dict(optim._optimizers)
    np.random.seed(1234)
    np.random.rand(3)
    state = np.random.get_state()
    cls = K.ImageClassifier(_cfg('cifar10'), 10, seed=77, device='cpu')
    after = np.random.get_state()
    assert state[0] == after[0] and state[1].tobytes() == after[1].tobytes() and state[2:] == after[2:]
    assert lib.named_params() == registry and optim._optimizers == optimizers
    assert list(cls.params) == ['Conv1.Filters', 'Conv1.Biases', 'Conv2.Filters', 'Conv2.Biases', 'Conv3.Filters', 'Conv3.Biases', 'Feature.W',
                                'Feature.b', 'Output.W', 'Output.b']
    shapes = {k: tuple(v.shape) for k, v in cls.params.items()}
    assert shapes['Conv1.Filters'] == (5, 5, 3, 8) and shapes['Conv3.Filters'] == (5, 5, 16, 32) and shapes['Feature.W'] == (512, 128)
    assert shapes['Output.W'] == (128, 10) and shapes['Output.b'] == (10,)
    assert all(getattr(p, 'param_name', None) is None and p.requires_grad and p._flat_owner is cls.opt for p in cls.params.values())
    assert not any('BN' in k or 'scale' in k for k in cls.params)                       # no BatchNorm
    assert (cls.opt.lr, cls.opt.beta1, cls.opt.beta2, cls.opt.shadow, cls.opt.world) == (1e-3, 0.9, 0.999, None, 1)
    # the He schemes, from a RandomState of its own: the same seed gives the same values, whatever the global stream holds
    np.random.seed(99)
    twin = K.ImageClassifier(_cfg('cifar10'), 10, seed=77, device='cpu')
    other = K.ImageClassifier(_cfg('cifar10'), 10, seed=78, device='cpu')
    for k in cls.params:
        assert torch.equal(cls.params[k], twin.params[k]), k
    assert not torch.equal(cls.params['Conv1.Filters'], other.params['Conv1.Filters'])
    w = cls.params['Conv2.Filters'].detach().numpy()
    bound = np.sqrt(4.0 / (8 * 25 + 16 * 25 / 4.0)) * np.sqrt(3)
    assert np.abs(w).max() <= bound and np.abs(w).max() > 0.98 * bound and abs(w.std() - bound / np.sqrt(3)) < 0.05 * bound
    f = cls.params['Feature.W'].detach().numpy()
    assert np.abs(f).max() <= np.sqrt(2.0 / 512) * np.sqrt(3) and np.all(cls.params['Feature.b'].detach().numpy() == 0)
    # the registry's clean-up does not reach it
    theta = cls.opt.theta.clone()
    lib.delete_all_params()
    assert torch.equal(cls.opt.theta, theta) and all(p._flat_owner is cls.opt for p in cls.params.values())
    with pytest.raises(ValueError, match='classes'):
        K.ImageClassifier(_cfg(), 1, seed=0, device='cpu')
    with pytest.raises(ValueError, match='classes'):
        K.ImageClassifier(_cfg(), 65, seed=0, device='cpu')


def _free_port():
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lone_rank_worker(rank, world, port, q):
    """rank 0 of a 2-rank gloo group builds a classifier and steps it, as the one evaluating rank of a data-parallel run does; rank 1 never
    joins an exchange.  A collective from the classifier's optimizer would find no partner and the step would not return."""
    import torch
    import torch.distributed as dist
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    os.environ['GGAN_FORCE_ALLREDUCE'] = '1'          # (the switch that makes even a single replica exchange: not this optimizer)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    from graphical_gan_amd import classifier as K, functional as F, optim
    try:
        if rank == 0:
            _lone_rank_checks(world, torch, K, F, optim)
        q.put((rank, 'done'))
    except BaseException as e:          # (reported, not waited for)
        q.put((rank, repr(e)))
    dist.barrier()
    dist.destroy_process_group()


def _lone_rank_checks(world, torch, K, F, optim):
    plain = optim.AdamOptimizer([torch.zeros(3, requires_grad=True)])
    assert plain.world == world and plain.bucket.scale == 1.0 / world           # what the classifier must NOT inherit
    cls = K.ImageClassifier(_cfg(), 4, seed=5, device='cpu')
    assert cls.opt.world == 1 and cls.opt.bucket.world == 1 and cls.opt.bucket.scale == 1.0 and cls.opt.bucket.flat is cls.opt.g
    # the step's device launches stood in for on the CPU (there is no CPU path): what is under test is the host logic between them
    seen = []

    def pack_(tensors, offsets, flat, bump=None, adam=None):
        for (o, n), t in zip(offsets, tensors):
            flat[o:o + n] = 0 if t is None else t.reshape(-1)
        seen.append(('pack_', adam is not None, None if adam is None else adam[-1]))
        if adam is None and bump is not None:
            bump += 1

    def adam_step_(theta, g, m, v, step, lr, b1, b2, eps=1e-8, grad_scale=1.0, counted=False):
        seen.append(('adam_step_', grad_scale))
    F.pack_, F.adam_step_ = pack_, adam_step_
    log = optim.EXCHANGE_LOG[0] = []
    grads = [torch.ones_like(p) for p in cls.opt.params]
    cls.opt.apply_gradients(grads)                 # pack, all_reduce, update -- and it returns
    assert cls.opt.all_reduce() is None and cls.opt.all_reduce(async_op=True, lo=0, hi=64) is None
    assert [e[0] for e in log] == ['pack', 'update'] and not any(e[0] == 'exchange' for e in log), log
    assert seen == [('pack_', False, None), ('adam_step_', 1.0)], seen          # the gradient is not scaled by 1 / world
    del os.environ['GGAN_FORCE_ALLREDUCE']
    assert cls.opt.can_fuse_update()               # ... and the fused pack + update stays available
    del log[:], seen[:]
    cls.opt.apply_gradients(grads)
    assert [e[:2] for e in log] == [('pack', 0), ('update', 'in the pack launch')] and seen == [('pack_', True, 1.0)], (log, seen)
    optim.EXCHANGE_LOG[0] = None


def test_the_classifier_optimizer_exchanges_nothing_in_a_process_group():
    import torch.multiprocessing as mp
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_lone_rank_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=120) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.terminate()
    assert res == {0: 'done', 1: 'done'} and all(p.exitcode == 0 for p in procs)


def test_save_load_round_trip_and_every_mismatching_field_is_named(tmp_path):
    import torch
    from graphical_gan_amd import classifier as K
    cls = K.ImageClassifier(_cfg(), 4, seed=5, device='cpu')
    with torch.no_grad():
        for p in cls.params.values():
            p.add_(0.25)
        cls.opt.m.fill_(1.0)
    cls.fit_rows, cls.epochs, cls.held_out = 512, 2, 0.96875
    path = str(tmp_path / 'cls.npz')
    cls.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(['classifier/' + k for k in cls.params] + ['classifier/meta'])
        assert sorted(s.split('=')[0] for s in z['classifier/meta']) == sorted(K.META_KEYS)
    fresh = K.ImageClassifier(_cfg(), 4, seed=6, device='cpu')
    with torch.no_grad():
        fresh.opt.m.fill_(3.0)
    fresh.load(path)
    for k in cls.params:
        assert torch.equal(cls.params[k], fresh.params[k]), k
    assert fresh.meta() == cls.meta() == dict(dataset='mnist', classes=4, dim=8, seed=5, fit_rows=512, epochs=2, accuracy=0.96875)
    assert float(fresh.opt.m.abs().max()) == 0.0 and torch.equal(fresh.opt.theta[:200], cls.opt.theta[:200])      # (the weights live in theta)
    st = cls.state_dict()
    fresh.load_state_dict(st)
    for field, other in (('dataset', K.ImageClassifier(_cfg('cifar10'), 4, seed=5, device='cpu')), ('classes', K.ImageClassifier(_cfg(), 10, seed=5, device='cpu')),
                         ('dim', K.ImageClassifier(_cfg(dim=16), 4, seed=5, device='cpu'))):
        before = {k: v.detach().clone() for k, v in other.params.items()}
        with pytest.raises(ValueError, match='classifier file: %s is' % field):
            other.load(path)
        assert all(torch.equal(before[k], other.params[k]) for k in before)              # a refused file changes nothing
    bad = dict(st)
    del bad['classifier/meta']
    with pytest.raises(ValueError, match='meta'):
        fresh.load_state_dict(bad)
    bad = dict(st)
    bad['classifier/Output.W'] = np.zeros((128, 5), np.float32)
    with pytest.raises(ValueError, match='Output.W'):
        fresh.load_state_dict(bad)


def test_the_restated_fit_meets_its_condition():
    """the condition on the fit test's inputs, checked where it was chosen: the float64 restatement reaches 100 % held-out accuracy with every
    top-two margin above 1, and the recorded figures are the measured ones"""
    ref = R.fit_reference('float64')
    print('float64 restatement: accuracy %.4f, smallest margin %.4f, first losses %s' % (ref['accuracy'], ref['margin'], ref['losses'][:4]))
    assert ref['accuracy'] == 1.0 and ref['margin'] > 1.0 and abs(ref['margin'] - R.FIT_MARGIN64) < 0.01
    assert len(ref['losses']) == R.FIT_EPOCHS * (R.FIT_ROWS // R.FIT_B) >= R.FIT_TRAJECTORY
    gap = float(np.max(np.abs(R.fit_reference('float32')['losses'][:R.FIT_TRAJECTORY] - ref['losses'][:R.FIT_TRAJECTORY])))
    print('float32 against float64 over %d steps: %.3e (recorded %.3e, gate %.3e)' % (R.FIT_TRAJECTORY, gap, R.FIT_GAP32, R.FIT_LOSS_GATE))
    # the recorded figure is the measured one: 7.1e-7 of it is the float32 step size, the same on every host; the rest, about 1e-7 either
    # way, follows the summation order of the host's float32 convolutions
    assert R.FIT_LOSS_GATE == 4.0 * R.FIT_GAP32 and abs(gap / R.FIT_GAP32 - 1.0) <= 0.2, (gap, R.FIT_GAP32)
