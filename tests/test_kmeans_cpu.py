"""not-gpu: the float64 restatement of tests/_kmeans_ref.py against known answers, the condition on the assignment cases for the
restatement alone, the built library's new entry points, and the switch, the flag and the keyword of the k-means pass."""
import argparse
import ctypes as C
import glob
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _kmeans_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_mnist', 'gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_face',
                 'gmgan_inference_mnist', 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_kmeans_workspace', 'ggan_kmeans_seed', 'ggan_kmeans_pick', 'ggan_kmeans_assign', 'ggan_kmeans_update', 'ggan_kmeans_fit',
           'ggan_bin_test', 'ggan_cluster_scores']
KEYS = ('dev ndb x', 'dev ndb js x', 'dev ndb data', 'dev kmeans accuracy z', 'dev kmeans nmi z')


# ---- the restatement's known answers ---------------------------------------------------------------------------------------------------------
def test_partitions_identical_under_a_relabelling_and_independent_partitions():
    y = np.arange(1200) % 6
    purity, nmi, table = R.cluster_scores((y * 5 + 2) % 6, y, 6, 6)
    assert purity == 1.0 and abs(nmi - 1.0) < 1e-14 and table.sum() == 1200 and np.count_nonzero(table) == 6
    i = np.arange(1200)
    purity, nmi, _ = R.cluster_scores(i % 4, (i // 4) % 5, 4, 5)          # independent uniform partitions of a product grid
    assert nmi == 0.0 and abs(purity - 0.2) < 1e-15
    assert R.cluster_scores(np.zeros(9, int), np.zeros(9, int), 1, 1)[:2] == (1.0, 1.0)          # both entropies 0
    purity, nmi, _ = R.cluster_scores(np.zeros(10, int), np.arange(10) % 2, 1, 2)                # one cluster, two classes
    assert purity == 0.5 and nmi == 0.0


def test_the_bin_test_against_hand_computed_values():
    c = [5, 0, 17, 3, 0, 40]
    assert R.bin_test(c, [3 * v for v in c]) == (0, 0.0, 0.0)                                     # equal histograms
    nd, share, js = R.bin_test([4, 6, 0, 0], [0, 0, 6, 4])                                         # disjoint histograms
    assert (nd, share) == (4, 1.0) and abs(js - math.log(2.0)) < 1e-15
    # a hand-computed z statistic: 30 of 100 against 50 of 100: P = 0.4, se = sqrt(0.4 * 0.6 * 0.02) = sqrt(0.0048), z = 0.2 / se
    z, se = R.z_statistic(30.0, 50.0, 100.0, 100.0)
    assert abs(se - math.sqrt(0.0048)) < 1e-17 and abs(z - 0.2 / math.sqrt(0.0048)) < 1e-13 and abs(z - 2.8867513459481287) < 1e-12
    assert R.bin_test([30, 70], [50, 50])[0] == 2 and R.bin_test([30, 70], [50, 50], z=2.9)[0] == 0
    assert R.z_statistic(7.0, 9.0, 7.0, 9.0) == (None, 0.0) and R.bin_test([7], [9]) == (0, 0.0, 0.0)          # an se == 0 bin does not differ
    assert R.z_statistic(0.0, 0.0, 7.0, 9.0)[0] is None
    nd, _, js = R.bin_test([0, 10], [5, 5])                                                       # a 0 log 0 bin
    assert math.isfinite(js) and abs(js - (0.5 * math.log(1 / 0.75) + 0.5 * (0.5 * math.log(0.5 / 0.25) + 0.5 * math.log(0.5 / 0.75)))) < 1e-15


def test_seed_assign_and_update_rules_of_the_restatement():
    X = np.array([[0.0], [1.0], [1.0], [5.0]])
    assert R.pick([0, 1, 1, 2], 0.0) == 1 and R.pick([0, 1, 1, 2], 0.25) == 2 and R.pick([0, 1, 1, 2], 0.5) == 3 and R.pick([0, 1, 1, 2], 0.49) == 2
    assert R.pick([0, 0, 0, 0], 0.6) == 2                                                          # the total == 0 rule
    idx, rows = R.seed(X, 3, [0.3, 0.5, 0.99])
    assert idx.tolist() == [1, 3, 0] and rows[:, 0].tolist() == [1.0, 5.0, 0.0]
    a, dist = R.assign(X, np.array([[1.0], [1.0], [4.0]]))
    assert a.tolist() == [0, 0, 0, 2] and dist.tolist() == [1.0, 0.0, 0.0, 1.0]                   # a tie goes to the lower centre index
    Cn, counts = R.update(X, a, np.array([[1.0], [7.5], [4.0]]))
    assert counts.tolist() == [3, 0, 1] and Cn[:, 0].tolist() == [2.0 / 3.0, 7.5, 5.0]            # an empty cluster keeps its centre
    f = R.fit(X, 2, 3, idx=[0, 3])
    assert f['assign'].tolist() == [0, 0, 0, 1] and f['moved'].tolist() == [4, 0, 0, 0] and np.all(np.diff(f['inertia']) <= 0)


@pytest.mark.parametrize('d,k', R.ASSIGN_CASES)
def test_the_cap_on_ambiguous_rows_holds_for_the_restatement_alone(d, k):
    """the GPU test excuses a row whose two nearest centres are within 2 T_i of each other in float64; here, without any device, at most
    5 % of the rows of each of its cases are that close, so it cannot leave out more"""
    for lloyd in (0, 3):
        X, Cn, D, T = R.assign_case(d, k, lloyd)
        share = float(R.ambiguous(D, T).mean())
        print('d %d k %d lloyd %d: ambiguous share %.4f' % (d, k, lloyd, share))
        assert X.shape == (600 if d == 3072 else 1000, d) and Cn.shape == (k, d) and Cn.dtype == np.float32
        assert share <= R.AMBIGUOUS_CAP


# ---- the built library -----------------------------------------------------------------------------------------------------------------------
def test_the_entry_points_are_exported_declared_and_bound(lib_built):
    from graphical_gan_amd import _lib, build, functional as F, evaluate
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert lib.ggan_version() == _lib.ABI_VERSION == int(re.search(r'#define GGAN_ABI_VERSION (\d+)', hdr).group(1)) == 800
    assert 'kmeans.hip' in build.SOURCES
    raw = C.CDLL(lib_built)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(raw, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    const = lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
    assert (F.KMEANS_MAX_K, F.KMEANS_ROW_BLOCK, F.KMEANS_NONFINITE) == (const('GGAN_KMEANS_MAX_K'), const('GGAN_KMEANS_ROW_BLOCK'), const('GGAN_KMEANS_NONFINITE'))
    assert (F.KMEANS_MAX_K, F.KMEANS_ROW_BLOCK, F.KMEANS_NONFINITE) == (R.MAX_K, R.ROW_BLOCK, R.NONFINITE) == (128, 512, 1)
    assert (F.KMEANS_MAX_CLASSES, F.KMEANS_BAD_INDEX, F.KMEANS_MAX_ITERS) == (const('GGAN_KMEANS_MAX_CLASSES'), const('GGAN_KMEANS_BAD_INDEX'), const('GGAN_KMEANS_MAX_ITERS'))
    assert evaluate.KM_BINS <= F.KMEANS_MAX_K
    # the partials of the workload's largest shape stay under 256 MB
    assert 0 < lib.ggan_kmeans_workspace(20000, 12288, 128) < 256 * 1024 * 1024 + 4 * 1024 * 1024
    assert -(-20000 // F.KMEANS_ROW_BLOCK) * 128 * 12288 * 4 < 256 * 1000 * 1000
    # the workspace twin: 0 out of range
    ws = lib.ggan_kmeans_workspace
    assert ws(0, 4, 4) == 0 and ws(131073, 4, 4) == 0 and ws(10, 0, 4) == 0 and ws(10, 4, 0) == 0 and ws(10, 4, 129) == 0 and ws(131072, 1, 128) > 0
    # refused with a message before any launch: no device is needed to be told
    p = C.c_void_p(256)
    big = 1 << 30
    for k in (0, 129):
        assert lib.ggan_kmeans_assign(p, p, 10, 4, k, None, p, p, p, p, None, p, p, big, None) < 0 and b'k <= 128' in lib.ggan_last_error()
        assert lib.ggan_kmeans_seed(p, 10, 4, k, p, p, p, p, big, None) < 0 and lib.ggan_kmeans_update(p, p, 10, 4, k, p, p, p, big, None) < 0
        assert lib.ggan_kmeans_fit(p, 10, 4, k, 3, p, p, p, p, p, p, p, p, p, big, None) < 0
        assert lib.ggan_bin_test(p, p, k, 1.96, p, None) < 0 and lib.ggan_cluster_scores(p, p, 10, k, 4, p, p, p, None) < 0
    assert lib.ggan_kmeans_assign(p, p, 0, 4, 4, None, p, p, p, p, None, p, p, big, None) < 0 and b'n <= 131072' in lib.ggan_last_error()
    assert lib.ggan_kmeans_pick(p, 0, p, p, None) < 0 and lib.ggan_cluster_scores(p, p, 0, 4, 4, p, p, p, None) < 0
    assert lib.ggan_cluster_scores(p, p, 10, 4, 33, p, p, p, None) < 0 and b'classes' in lib.ggan_last_error()
    assert lib.ggan_kmeans_assign(None, p, 10, 4, 4, None, p, p, p, p, None, p, p, big, None) < 0 and b'null' in lib.ggan_last_error()
    assert lib.ggan_kmeans_assign(p, p, 10, 4, 4, None, p, p, p, p, None, p, p, 16, None) < 0 and b'workspace' in lib.ggan_last_error()
    assert lib.ggan_kmeans_fit(p, 10, 4, 4, -1, p, p, p, p, p, p, p, p, p, big, None) < 0 and b'iters' in lib.ggan_last_error()


def test_the_functions_refuse_cpu_tensors_and_bad_shapes(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    x, c, a = torch.zeros(8, 3), torch.zeros(2, 3), torch.zeros(8, dtype=torch.int32)
    for call in (lambda: F.kmeans_seed(x, 2, [0.1, 0.2]), lambda: F.kmeans_assign(x, c), lambda: F.kmeans_update(x, a, c),
                 lambda: F.kmeans_fit(x, 2, 3, [0.1, 0.2]), lambda: F.bin_test(a, a), lambda: F.cluster_scores(a, a, 2, 2),
                 lambda: F.kmeans_pick(torch.zeros(8), 0.5)):
        with pytest.raises(_lib.GganError):
            call()


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_kmeans_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_KMEANS_EVERY', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.kmeans_settings(s) == {} and run.kmeans_settings('/somewhere/%s.py' % s) == {}
    others = lambda s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s), run.probe_settings(s), run.frechet_settings(s),
                        run.swd_settings(s), run.classifier_settings(s))
    base = {s: others(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_KMEANS_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.kmeans_settings(s) == {'KMEANS_EVERY': 20} and run.kmeans_settings('/somewhere/%s.py' % s) == {'KMEANS_EVERY': 20}
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.kmeans_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert others(s) == base[s]
    S = dict(run.reference_block('gan_inference_cifar10'), **run.kmeans_settings('gan_inference_cifar10'))
    assert [it for it in range(60) if run.kmeans_due(S, it)] == [19, 39, 59]
    assert run.eval_plan(S) is None and not any(run.scores_due(S, it) or run.probe_due(S, it) or run.classifier_due(S, it) for it in range(60))
    assert not any(run.kmeans_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_the_eight_image_scripts_carry_the_line_behind_the_classifier_line():
    line, before = 'SETTINGS.update(run.kmeans_settings(__file__))', 'SETTINGS.update(run.classifier_settings(__file__))'
    seen = {}
    for p in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py')):
        text = open(p).read()
        seen[os.path.splitext(os.path.basename(p))[0]] = text.count(line)
        assert text.count(line) == 0 or text.index(before) < text.index(line)
    assert seen == dict([(s, 1) for s in IMAGE_SCRIPTS] + [(s, 0) for s in SEQUENCE_SCRIPTS])


def test_kmeans_sets_lead_with_the_probe_rows_and_take_unlabelled_data(tmp_path, monkeypatch):
    from graphical_gan_amd import run
    import gzip
    import pickle
    state = np.random.get_state()[1].tobytes()
    assert run.kmeans_sets(dict(DATASET='cifar10', BATCH_SIZE=8, SYNTHETIC='force')) is None            # (no model to draw synthetic rows from)
    assert run.kmeans_sets(dict(DATASET='cifar10', BATCH_SIZE=8, DATA_DIR='/no/such/dir')) is None
    rng = np.random.default_rng(0)
    mk = lambda n: (rng.random((n, 784), dtype=np.float32), rng.integers(0, 10, size=n))
    with gzip.open(str(tmp_path / 'mnist.pkl.gz'), 'wb') as f:
        pickle.dump((mk(64), mk(24), mk(20)), f)
    monkeypatch.setenv('GGAN_MNIST', str(tmp_path / 'mnist.pkl.gz'))
    S = dict(DATASET='mnist', BATCH_SIZE=8, KM_FIT_ROWS=40, PROBE_FIT_ROWS=16)
    fit, again, probe = run.kmeans_sets(S), run.kmeans_sets(S), run.probe_sets(S)
    assert len(fit) == 5 and len(probe) == 2 and all(x.shape == (8, 784) for x, _ in fit)
    for (a, b), (c, d) in list(zip(fit, again)) + list(zip(fit, probe)):
        assert np.array_equal(a, c) and np.array_equal(b, d)
    assert np.random.get_state()[1].tobytes() == state
    assert inspect.getsource(run.kmeans_sets).count('_leading_training_rows') == 1


def test_the_flag_parses_and_the_state_space_scripts_refuse_it(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--kmeans']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert parsed[0].kmeans is False and parsed[1].kmeans is True and parsed[1].cls is False and parsed[1].swd is False
    for script in SEQUENCE_SCRIPTS:            # refused before anything is built: the checkpoint does not even exist
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--kmeans', '--out-dir', 'x'])
        assert e.value.code == 2 and '--kmeans: the state-space scripts have no single set of images to bin' in capsys.readouterr().err


def test_the_pass_is_no_row_of_the_table_and_checks_its_settings():
    from graphical_gan_amd import evaluate
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    sig = inspect.signature(evaluate.evaluate_once)
    names = list(sig.parameters)
    assert names.index('cls') + 1 == names.index('kmeans') == names.index('scores') - 1 and sig.parameters['kmeans'].default is False
    assert evaluate.KM_KEYS == KEYS
    assert (evaluate.KM_BINS, evaluate.KM_FIT_ROWS, evaluate.KM_SAMPLES, evaluate.KM_MAX_ROWS, evaluate.KM_ITERS) == (100, 20000, 20000, 10000, 50)
    assert evaluate.KM_Z_THRESHOLD == R.Z_5_PERCENT == 1.959963984540054
    seeds = [evaluate.KM_SEED, evaluate.PROBE_SEED, evaluate.FRECHET_SEED, evaluate.SWD_SEED, evaluate.CLS_SEED]
    assert len(set(seeds)) == 5 and len(set(s + d for s in seeds for d in (0, 1))) == 10          # (the pass's second seeding uses KM_SEED + 1)

    class Cfg:
        B = 4
        K = 0
    ev = object.__new__(evaluate.Evaluator)
    ev.S, ev.cfg = {}, Cfg()
    xs = [(np.zeros((4, 6), np.float32), np.zeros(4, np.int64))]
    with pytest.raises(ValueError, match='minibatches'):
        ev.kmeans_scores([], xs)
    with pytest.raises(ValueError, match='at most 32 classes'):
        ev.kmeans_scores(xs, [(xs[0][0], np.full(4, 32))])
    for key, bad in (('KM_BINS', 0), ('KM_BINS', 129), ('KM_FIT_ROWS', 3), ('KM_SAMPLES', 3), ('KM_MAX_ROWS', 1), ('KM_ITERS', -1),
                     ('KM_Z_CLUSTERS', 129)):
        ev.S = {key: bad}
        with pytest.raises(ValueError, match=key):
            ev.kmeans_scores(xs, xs)
