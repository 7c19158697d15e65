"""not-gpu: the Frechet distance away from the device -- the known answers of the float64 reference tests/_frechet_ref.py, the float64 model of
the kernel's own route (pivoted semi-definite Cholesky, round-robin Jacobi) against that reference over the grid of the GPU tests and within
the recorded sweep cap, the switch and the flag, the ABI, and the argument refusals of the C entry points and of functional."""
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
import _frechet_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_mnist', 'gan_inference_face',
                 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_mnist', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_frechet_moments_workspace', 'ggan_frechet_moments', 'ggan_frechet_distance_workspace', 'ggan_frechet_distance']


# ---- known answers of the reference ---------------------------------------------------------------------------------------------------------
def _two(n=300, d=12, seed=0):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=(n, d)) @ rng.normal(size=(d, d)) + rng.normal(size=d)).astype(np.float32)
    y = (1.5 * rng.normal(size=(n, d)) @ rng.normal(size=(d, d)) - 0.5).astype(np.float32)
    return x, y


def test_identical_sets_give_zero():
    x, _ = _two()
    v = R.reference(x, x.copy())
    assert abs(v[0]) <= 1e-9 * v[2] and v[1] == 0 and abs(v[2] - v[3]) <= 1e-9 * v[2]


def test_diagonal_covariances_give_the_sum_of_squared_differences():
    s1, s2 = np.array([0.5, 1.0, 2.0, 3.0]), np.array([1.5, 1.0, 0.25, 4.0])
    mu = np.zeros(4)
    v = R.distance(mu, np.diag(s1 ** 2), mu, np.diag(s2 ** 2))
    assert abs(v[0] - np.sum((s1 - s2) ** 2)) <= 1e-12 and v[1] == 0
    w, _, _ = R.model_distance(mu, np.diag(s1 ** 2), mu, np.diag(s2 ** 2))
    assert abs(w[0] - np.sum((s1 - s2) ** 2)) <= 1e-12


def test_a_shift_adds_its_squared_length():
    x, y = _two(seed=1)
    v = np.array([0.5, -2.0, 1.0] * 4)
    (m1, S1), (m2, S2) = R.moments(x), R.moments(y)
    a, b = R.distance(m1, S1, m2, S2), R.distance(m1, S1, m2 + v, S2)
    assert abs((b[0] - a[0]) - (np.sum(v * v) + 2.0 * np.dot(m2 - m1, v))) <= 1e-10 * b[2] and np.array_equal(a[2:], b[2:])
    same = R.distance(m1, S1, m1 + v, S1)            # a set against itself shifted: exactly |v|^2
    assert abs(same[0] - np.sum(v * v)) <= 1e-9 * same[2] and abs(same[1] - np.sum(v * v)) <= 1e-12


def test_scaling_both_sets_scales_the_value_by_the_square():
    x, y = _two(seed=2)
    a, b = R.reference(x, y), R.reference(4.0 * x, 4.0 * y)          # (a power of two: the float32 rows scale exactly)
    assert np.max(np.abs(b - 16.0 * a)) <= 1e-10 * b[2]


def test_rank_deficient_inputs_stay_finite():
    for kind in ('short', 'const', 'twin'):
        for n, d in ((2, 33), (600, 128)):
            x, y = R.sets(kind, n, d)
            assert np.linalg.matrix_rank(R.moments(x)[1]) < d
            v, (w, st, _) = R.case_reference(kind, n, d), R.case_model(kind, n, d)
            assert np.all(np.isfinite(v)) and np.all(np.isfinite(w)) and st == 0 and v[0] > 0
    z = np.full((5, 3), 2.5, np.float32)               # nothing varies at all
    assert np.array_equal(R.reference(z, z), np.zeros(4)) and np.array_equal(R.model_distance(*(R.moments(z) * 2))[0], np.zeros(4))
    assert R.model_distance(np.array([np.nan]), np.eye(1), np.zeros(1), np.eye(1))[1] == R.NONFINITE


# ---- the model of the kernel's route ------------------------------------------------------------------------------------------------------------
def test_the_grid():
    cases = R.cases()
    assert sorted(set(d for _, _, d in cases)) == [1, 2, 31, 33, 64, 127, 128] and sorted(set(n for _, n, _ in cases)) == [2, 255, 256, 257, 600]
    assert set(k for k, _, _ in cases) == set(R.KINDS) == {'gauss', 'self', 'shift', 'short', 'const', 'twin', 'scale'}
    assert all(R.sets('short', n, d)[0].shape[0] < d for _, n, d in R.cases(('short',)))
    assert R.SWEEP_CAP == 2 * R.SWEEPS_SEEN and R.WHOLE_OP_CEILING == 256 * 2.0 ** -24
    src = open(os.path.join(ROOT, 'graphical_gan_amd', 'csrc', 'frechet.hip')).read()
    assert 'kSweepCap = %d;' % R.SWEEP_CAP in src and 'kTol = %g;' % R.JACOBI_TOL in src


@pytest.mark.parametrize('kind', R.KINDS)
def test_the_model_matches_the_reference_and_converges_within_the_cap(kind):
    """the kernel's route in float64 against the symmetric square root, case by case within d sqrt(eps) of the traces.  That is the
    REFERENCE's own resolution, not the model's: eigh returns the zero eigenvalues of a singular S1 as +-eps of the largest, and the square
    root lifts each to sqrt(eps) -- at rank 1 (n = 2, d = 127) the reference calls a set against itself -3.2e-7 of the traces where the
    exact answer is 0, and the model, whose pivoted factorisation has exactly one column there, gives 1e-16.  So a set against itself is
    also held to 0 directly.  The sweeps stay within half the kernel's trip count."""
    worst, sweeps = 0.0, 0
    for k, n, d in R.cases((kind,)):
        v, st, sw = R.case_model(k, n, d)
        err = R.rel_err(v, R.case_reference(k, n, d))
        assert st == 0 and err <= d * np.sqrt(R.EPS), (R.case_id(k, n, d), err)
        worst, sweeps = max(worst, err), max(sweeps, sw)
        if k == 'self':
            assert abs(v[0]) <= 1e-9 * v[2], (R.case_id(k, n, d), v)
    print(kind, 'worst error against the reference %.2e, most sweeps %d' % (worst, sweeps))
    assert sweeps <= R.SWEEPS_SEEN


def test_round_robin_meets_every_pair_once():
    for m in (2, 4, 32, 34, 128):
        seen = set()
        for step in range(m - 1):
            p, q = R.round_robin(m, step)
            assert len(set(p) | set(q)) == m and np.all(p < q)          # m / 2 disjoint pairs
            seen |= set(zip(p.tolist(), q.tolist()))
        assert len(seen) == m * (m - 1) // 2


def test_an_unpivoted_factorisation_would_fail_on_float32_moments():
    """why the Cholesky factorisation is pivoted: float32 moments of a rank-deficient set are indefinite at 1e-8, and in the given order
    L L^T misses S by far more than the noise"""
    x, _ = R.sets('short', 600, 31)
    _, S = R.fp32_moments(x)
    assert np.linalg.eigvalsh(S)[0] < 0
    L = R.chol_psd(S)
    assert np.abs(L @ L.T - S).max() <= 1e-6 * np.abs(S).max()
    d, thr = S.shape[0], S.shape[0] * R.EPS * np.trace(S)
    U = np.zeros((d, d))
    for j in range(d):
        s = S[j:, j] - U[j:, :j] @ U[j, :j]
        if s[0] > thr:
            U[j:, j] = s / np.sqrt(s[0])
    assert np.abs(U @ U.T - S).max() > 1e-5 * np.abs(S).max()


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_frechet_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_FRECHET_EVERY', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.frechet_settings(s) == {} and run.frechet_settings('/somewhere/%s.py' % s) == {}
    others = lambda s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s), run.probe_settings(s))
    base = {s: others(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_FRECHET_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.frechet_settings(s) == {'FRECHET_EVERY': 20} and run.frechet_settings('/somewhere/%s.py' % s) == {'FRECHET_EVERY': 20}
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.frechet_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert others(s) == base[s]
    S = dict(run.reference_block('gan_inference_cifar10'), **run.frechet_settings('gan_inference_cifar10'))
    assert [it for it in range(60) if run.frechet_due(S, it)] == [19, 39, 59]
    assert run.eval_plan(S) is None and not any(run.scores_due(S, it) or run.probe_due(S, it) for it in range(60))
    assert not any(run.frechet_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_the_eight_image_scripts_carry_the_line():
    line = 'SETTINGS.update(run.frechet_settings(__file__))'
    seen = {os.path.splitext(os.path.basename(p))[0]: open(p).read().count(line) for p in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py'))}
    assert seen == dict([(s, 1) for s in IMAGE_SCRIPTS] + [(s, 0) for s in SEQUENCE_SCRIPTS])


def test_the_flag_parses_and_the_state_space_scripts_refuse_it(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--frechet']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert parsed[0].frechet is False and parsed[1].frechet is True and parsed[1].probe is False
    assert not any(getattr(parsed[1], r.name) for r in evaluate.SET_SCORES)
    for script in SEQUENCE_SCRIPTS:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--frechet', '--out-dir', 'x'])
        assert e.value.code == 2 and '--frechet: the state-space scripts have no single code' in capsys.readouterr().err


def test_the_pass_is_no_row_of_the_table():
    from graphical_gan_amd import evaluate, functional as F
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    sig = inspect.signature(evaluate.evaluate_once)
    names = list(sig.parameters)
    assert names.index('probe') < names.index('frechet') < names.index('scores') and sig.parameters['frechet'].default is False
    assert sig.parameters['scores'].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError, match='no set-level score frechet'):
        evaluate._known('set_scores', dict(frechet=True))
    assert evaluate.FRECHET_KEYS == ('dev frechet z', 'dev frechet mean z', 'dev frechet xr', 'dev frechet mean xr')
    assert (evaluate.FRECHET_MAX_ROWS, evaluate.FRECHET_PROJ_DIM) == (10000, 128) and evaluate.FRECHET_PROJ_DIM == F.FRECHET_MAX_DIM
    assert evaluate.FRECHET_SEED != evaluate.PROBE_SEED


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_800_and_the_entry_points_are_bound(lib_built):
    from graphical_gan_amd import _lib, build, functional as F
    lib = _lib.load()
    assert lib.ggan_version() == _lib.ABI_VERSION == 800
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert '#define GGAN_ABI_VERSION 800' in hdr and 'frechet.hip' in build.SOURCES
    assert 'tflib/inception_score.py' in hdr and 'gan_inference_cifar10.py:381-391' in hdr
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    const = lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
    assert F.FRECHET_MAX_DIM == const('GGAN_FRECHET_MAX_DIM') == R.MAX_DIM == 128
    assert (F.FRECHET_NONFINITE, F.FRECHET_NOT_CONVERGED) == (const('GGAN_FRECHET_NONFINITE'), const('GGAN_FRECHET_NOT_CONVERGED')) == (R.NONFINITE, R.NOT_CONVERGED)
    assert const('GGAN_PROBE_ROW_BLOCK') == R.ROW_BLOCK and F.FRECHET_MAX_ROWS == R.MAX_ROWS


def test_the_entry_points_refuse_bad_arguments_before_any_launch(lib_built):
    """d = 0, d = 129, n = 1, a null pointer, a short or misaligned workspace: a negative code and a message, on a machine with no device to
    launch on"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    p, big = C.c_void_p(4096), 1 << 30

    def refused(rc, what):
        assert rc < 0 and what.encode() in L.ggan_last_error(), (rc, what, L.ggan_last_error())
    assert L.ggan_frechet_moments_workspace(600, 128) >= 3 * (128 * 8 + 128 * 128 * 4) and L.ggan_frechet_distance_workspace(128) >= 2 * 128 * 128 * 8
    for bad in ((1, 8), (100, 0), (100, 129), (131073, 8)):
        assert L.ggan_frechet_moments_workspace(*bad) == 0, bad
    assert L.ggan_frechet_distance_workspace(0) == 0 and L.ggan_frechet_distance_workspace(129) == 0
    mom = lambda n=100, d=8, X=p, cov=p, ws=p, nb=big: L.ggan_frechet_moments(X, n, d, p, cov, p, ws, nb, None)
    dist = lambda d=8, m1=p, out=p, st=p, ws=p, nb=big: L.ggan_frechet_distance(m1, p, p, p, d, out, st, ws, nb, None)
    for fn in (mom, dist):
        refused(fn(d=0), 'd <= 128')
        refused(fn(d=129), 'd <= 128')
        refused(fn(nb=16), 'workspace too small')
        refused(fn(ws=C.c_void_p(4100)), '16-byte aligned')
        refused(fn(ws=None), 'null pointer')
    refused(mom(n=1), 'n < 2')
    refused(mom(n=131073), '131072')
    refused(mom(X=None), 'null pointer')
    refused(mom(cov=None), 'null pointer')
    refused(mom(cov=C.c_void_p(4100)), '8-byte aligned')
    refused(dist(m1=None), 'null pointer')
    refused(dist(out=None), 'null pointer')
    refused(dist(st=None), 'null pointer')


def test_functional_refuses_what_it_must_before_the_device():
    import torch
    from graphical_gan_amd import functional as F, _lib
    x = torch.zeros(10, 4)
    for bad, what in ((torch.zeros(10, 129), 'columns'), (torch.zeros(10, 0), 'columns'), (torch.zeros(1, 4), 'at least 2 rows'),
                      (x.double(), 'float32'), (torch.zeros(10), 'float32 rows'), (torch.zeros(2, 3, 4), 'float32 rows')):
        with pytest.raises(ValueError, match=what):
            F.frechet_moments(bad)
    for a, b, what in ((x, torch.zeros(10, 5), 'one width'), (x, torch.zeros(1, 4), 'at least 2 rows'), (torch.zeros(10, 129), torch.zeros(10, 129), 'columns'),
                       (x, x.double(), 'float32'), (x, torch.zeros(10), 'one width')):
        with pytest.raises(ValueError, match=what):
            F.frechet_distance(a, b)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.frechet_distance(x.clone().requires_grad_(), x)
    with pytest.raises(_lib.GganError, match='no CPU path'):           # no fall-back
        F.frechet_distance(x, x)
    with pytest.raises(_lib.GganError, match='no CPU path'):
        F.frechet_moments(x)
