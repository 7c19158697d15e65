"""not-gpu: the sliced Wasserstein distance away from the device -- the integer-breakpoint formula of tests/_swd_ref.py against the brute force and
against closed forms, the numpy model of the kernel's bitonic network over every padded size of the GPU tests' grid, the perturbation
inequality the GPU tests lean on, the switch and the flag, the ABI, and the argument refusals of the C entry points and of functional."""
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
import _swd_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_SCRIPTS = ['gan_inference_cifar10', 'gan_inference_svhn', 'gan_inference_mnist', 'gan_inference_face',
                 'gmgan_inference_cifar10', 'gmgan_inference_svhn', 'gmgan_inference_mnist', 'gmgan_inference_face']
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
ENTRIES = ['ggan_swd_workspace', 'ggan_swd']


# ---- the yardstick --------------------------------------------------------------------------------------------------------------------------
def test_the_breakpoint_formula_against_the_brute_force():
    """w_pp against every point repeated to the least common multiple, on the small pairs, both exponents: a few roundings of float64"""
    worst = 0.0
    for m, n in R.SMALL_PAIRS:
        rng = np.random.default_rng(m * 100003 + n)
        a, b = rng.normal(size=(m, 5)).astype(np.float32), (1.7 * rng.normal(size=(n, 5)) + 0.3).astype(np.float32)
        for p in R.PS:
            got, want = R.w_pp(a, b, p), R.w_pp_lcm(a, b, p)
            worst = max(worst, float(np.max(np.abs(got - want) / want)))
            assert np.all(np.abs(got - want) <= 64 * R.EPS * want), (m, n, p)
    print('worst relative difference %.1e' % worst)


def test_the_grid():
    cases = R.cases()
    assert set(k for k, _, _, _ in cases) == set(R.KINDS) == {'gauss', 'shift', 'ties', 'self', 'sorted', 'reversed', 'scale'}
    assert sorted(set(n for _, m, n, _ in cases if m == n)) == [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1024, 1025, 4097, 16384]
    assert [(m, n) for k, m, n, L in cases if m != n and k == 'gauss' and L == 3] == \
        [(1, 7), (7, 1), (3, 5), (4, 6), (256, 1000), (1000, 999), (512, 1024), (16384, 16383)]
    assert sorted(set(L for _, _, _, L in cases)) == [1, 3, 64] and all(L == 3 for _, m, n, L in cases if max(m, n) >= 16383)
    assert R.PS == (1, 2)
    x, y = R.sets('scale', 257, 257, 3)
    assert np.any(np.signbit(x) & (x == 0)) and np.any(~np.signbit(x) & (x == 0)) and np.abs(x).max() > 1e6 and 0 < np.abs(y).max() < 1e-5
    x, y = R.sets('ties', 1000, 999, 64)
    assert set(np.unique(x)) <= {0, 1, 2, 3} and np.all(x[:, 0] == 1) and np.all(y[:, 0] == 3) and np.all(x[:, 63] == y[0, 63])


def test_closed_forms():
    for m, n, L in ((257, 257, 3), (1000, 1000, 64), (1, 1, 1)):
        c = R.shift_of(m, n, L)
        x, y = R.sets('shift', m, n, L)
        assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + c)              # (exact in float32: multiples of 2^-10)
        for p in R.PS:
            v, per = R.reference(x, y, p)
            assert np.all(np.abs(per - np.abs(c) ** p) <= 4 * R.EPS * np.abs(c) ** p), (m, L, p)
            assert abs(v[1] - np.max(np.abs(c))) <= 4 * R.EPS * v[1] and v[0] <= v[1]
    for m, n, L in ((257, 257, 3), (1000, 999, 64), (16384, 16384, 3)):
        x, y = R.sets('self', m, m, L)
        for p in R.PS:
            v, per = R.reference(x, y, p)
            assert np.array_equal(per, np.zeros(L)) and np.array_equal(v, np.zeros(2))
    # two points against one: each carries half of the one's mass
    for p in R.PS:
        assert R.w_pp(np.array([1.0, 4.0]), np.array([2.0]), p)[0] == 0.5 * 1.0 ** p + 0.5 * 2.0 ** p
        assert R.w_pp(np.array([2.0]), np.array([4.0, 1.0]), p)[0] == 0.5 * 1.0 ** p + 0.5 * 2.0 ** p
    # three against two: thirds and halves meet at sixths -- a1 b1 | a2 b1 | a2 b2 | a3 b2 with lengths 2 1 1 2
    a, b = np.array([0.0, 1.0, 5.0]), np.array([0.5, 3.0])
    assert abs(R.w_pp(a, b, 1)[0] - (2 * 0.5 + 0.5 + 2.0 + 2 * 2.0) / 6.0) <= R.EPS
    x, y = R.sets('ties', 1000, 999, 64)
    assert R.w_pp(x, y, 2)[0] == 4.0 and R.w_pp(x, y, 1)[0] == 2.0 and R.w_pp(x, y, 2)[63] == 0.0


def test_the_network_model_sorts_every_padded_size_of_the_grid():
    """the kernel's stage order and index arithmetic, in numpy: every row count of the grid (so every padded size 64 .. 16384), random keys,
    ties, -0 / +0, descending input; the padding stays at the end; the stage list is the bitonic network's, fixed by the padded size alone"""
    sizes = sorted(set(R.EQUAL) | set(v for pair in R.UNEQUAL for v in pair))
    assert sorted(set(R.padded(n) for n in sizes)) == [64, 128, 256, 512, 1024, 2048, 8192, 16384]
    rng = np.random.default_rng(0)
    for n in sizes + [2048, 2049]:
        for kind in ('gauss', 'ties', 'reversed'):
            keys = rng.normal(size=n).astype(np.float32)
            if kind == 'ties':
                keys = rng.integers(-1, 2, size=n).astype(np.float32) * np.where(rng.random(n) < 0.5, 0.0, 1.0).astype(np.float32)
            if kind == 'reversed':
                keys = np.sort(keys)[::-1].copy()
            trace = []
            out = R.network_sort(keys, trace)
            P = R.padded(n)
            assert out.shape == (P,) and np.array_equal(out[:n], np.sort(keys)) and np.all(np.isinf(out[n:])), (n, kind)
            assert trace == R.network_stages(P), (n, kind)          # every stage of the network once, in the network's order
    # a NaN key may leave the order undefined, but the stage list is the same: trip counts depend on the padded size alone
    keys = rng.normal(size=300).astype(np.float32)
    t0, t1 = [], []
    R.network_sort(keys, t0)
    keys[17] = np.nan
    out = R.network_sort(keys, t1)
    assert t0 == t1 and np.isnan(out).sum() == 1


def test_the_source_holds_the_models_constants():
    src = open(os.path.join(ROOT, 'graphical_gan_amd', 'csrc', 'swd.hip')).read()
    assert 'kMinPad = %d;' % R.MIN_PAD in src and 'kSortThreads = %d;' % R.SORT_THREADS in src and 'kKeys = %d;' % R.KEYS in src
    assert 'base = lane | ((tid >> 6) * (64 * KPT))' in src and 'exchange(v[s], v[s | jb], ((base | (s << 6)) & k) == 0)' in src
    assert '(((base | (s << 6)) & k) == 0) == ((lane & j) == 0)' in src and 'exchange(u[s], u[s | jb], ((s * G) & k) == 0)' in src
    for P, (kpt, lw) in ((64, (1, 0)), (128, (2, 0)), (256, (4, 0)), (512, (8, 0)), (1024, (16, 0)), (2048, (16, 1)), (4096, (16, 2)), (8192, (16, 3))):
        assert R.layout(P) == (kpt, lw) and 'case %d: sort_column<%s, %d>' % (P, 'kKeys' if kpt == 16 else kpt, lw) in src, P
    assert R.layout(16384) == (16, 4) and 'default: sort_column<kKeys, 4>' in src
    assert 'powf(' not in src and 'log1pf(' not in src and 'atomicAdd' not in src
    for name in ('"swd_transpose"', '"swd_sort"', '"swd_final"'):
        assert name in src, name


@pytest.mark.parametrize('d', [3, 128, 3072])
def test_a_perturbation_moves_the_distance_by_at_most_twice_its_size(d):
    """the inequality gate (b) of the GPU tests leans on, here between float32 and float64 numpy projections of the same float32 inputs:
    W_p is a metric and moving every point by at most delta moves a measure by at most delta, so |W_p(l) - ref W_p(l)| <= 2 delta per
    direction, for unequal sizes too, and through the p-mean and the max over directions"""
    rng = np.random.default_rng(d)
    theta = rng.normal(size=(d, 16))
    theta = (theta / np.sqrt(np.sum(theta * theta, axis=0))).astype(np.float32)
    x, y = rng.random((257, d), dtype=np.float32), (0.9 * rng.random((200, d), dtype=np.float32) + 0.05)
    p32 = [a @ theta for a in (x, y)]
    p64 = [a.astype(np.float64) @ theta.astype(np.float64) for a in (x, y)]
    delta = max(float(np.max(np.abs(a - b))) for a, b in zip(p32, p64))
    assert 0 < delta <= d * 2.0 ** -24 * np.sqrt(d) * 1.0001
    for p in R.PS:
        (v, per), (rv, rper) = R.reference(p32[0], p32[1], p), R.reference(p64[0], p64[1], p)
        assert np.all(np.abs(per ** (1.0 / p) - rper ** (1.0 / p)) <= 2 * delta) and np.all(np.abs(v - rv) <= 2 * delta)
        assert np.all(rper > 100 * delta ** p)


# ---- switch, flag, keyword -----------------------------------------------------------------------------------------------------------------
def test_swd_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    monkeypatch.delenv('GGAN_SWD_EVERY', raising=False)
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.swd_settings(s) == {} and run.swd_settings('/somewhere/%s.py' % s) == {}
    others = lambda s: (run.eval_settings(s), run.score_settings(s), run.manifold_settings(s), run.probe_settings(s), run.frechet_settings(s))
    base = {s: others(s) for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS}
    monkeypatch.setenv('GGAN_SWD_EVERY', '20')
    for s in IMAGE_SCRIPTS:
        assert run.swd_settings(s) == {'SWD_EVERY': 20} and run.swd_settings('/somewhere/%s.py' % s) == {'SWD_EVERY': 20}
    for s in SEQUENCE_SCRIPTS + ['no_such_script']:
        assert run.swd_settings(s) == {}
    for s in IMAGE_SCRIPTS + SEQUENCE_SCRIPTS:           # (no other settings function learns the variable)
        assert others(s) == base[s]
    S = dict(run.reference_block('gan_inference_cifar10'), **run.swd_settings('gan_inference_cifar10'))
    assert [it for it in range(60) if run.swd_due(S, it)] == [19, 39, 59]
    assert run.eval_plan(S) is None and not any(run.scores_due(S, it) or run.probe_due(S, it) or run.frechet_due(S, it) for it in range(60))
    assert not any(run.swd_due(run.reference_block('gan_inference_cifar10'), it) for it in range(60))


def test_the_eight_image_scripts_carry_the_line():
    line, before = 'SETTINGS.update(run.swd_settings(__file__))', 'SETTINGS.update(run.frechet_settings(__file__))'
    seen = {}
    for path in glob.glob(os.path.join(ROOT, 'scripts', '*_inference_*.py')):
        text = open(path).read()
        seen[os.path.splitext(os.path.basename(path))[0]] = text.count(line)
        if text.count(line):
            assert text.count(before) == 1 and text.index(before) < text.index(line), path
    assert seen == dict([(s, 1) for s in IMAGE_SCRIPTS] + [(s, 0) for s in SEQUENCE_SCRIPTS])


def test_the_flag_parses_and_the_state_space_scripts_refuse_it(monkeypatch, capsys):
    from graphical_gan_amd import evaluate
    parsed, real = [], argparse.ArgumentParser.parse_args

    def parse(self, argv=None):                # (main's own parser, stopped once it has read the command line)
        parsed.append(real(self, argv))
        raise SystemExit(0)
    with monkeypatch.context() as mp:
        mp.setattr(argparse.ArgumentParser, 'parse_args', parse)
        for flags in ([], ['--swd']):
            with pytest.raises(SystemExit):
                evaluate.main(['nowhere.npz', '--script', 'gan_inference_mnist'] + flags)
    assert parsed[0].swd is False and parsed[1].swd is True and parsed[1].probe is False and parsed[1].frechet is False
    assert not any(getattr(parsed[1], r.name) for r in evaluate.SET_SCORES)
    for script in SEQUENCE_SCRIPTS:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            evaluate.main(['nowhere.npz', '--script', script, '--swd', '--out-dir', 'x'])
        assert e.value.code == 2 and '--swd: the state-space scripts have no single code' in capsys.readouterr().err


def test_the_pass_is_no_row_of_the_table():
    from graphical_gan_amd import evaluate, functional as F
    assert [r.name for r in evaluate.SET_SCORES] == ['mmd', 'prdc', 'knn', 'parzen', 'rec']
    sig = inspect.signature(evaluate.evaluate_once)
    names = list(sig.parameters)
    assert names.index('probe') < names.index('frechet') < names.index('swd') < names.index('scores') and sig.parameters['swd'].default is False
    assert sig.parameters['scores'].kind is inspect.Parameter.VAR_KEYWORD
    with pytest.raises(TypeError, match='no set-level score swd'):
        evaluate._known('set_scores', dict(swd=True))
    assert evaluate.SWD_KEYS == ('dev swd z', 'dev swd max z', 'dev swd x', 'dev swd max x')
    assert (evaluate.SWD_MAX_ROWS, evaluate.SWD_DIRS, evaluate.SWD_P) == (10000, 512, 2)
    assert evaluate.SWD_MAX_ROWS <= F.SWD_MAX_ROWS and evaluate.SWD_DIRS <= F.SWD_MAX_DIRS
    assert len({evaluate.SWD_SEED, evaluate.PROBE_SEED, evaluate.FRECHET_SEED, 0}) == 4


def test_the_documents_name_the_switch_and_the_limits():
    table = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    assert '| `GGAN_SWD_EVERY` |' in table and 'Evaluator.swd_scores' in table
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert 'GGAN_SWD_EVERY' in readme and 'not comparable with published SWD figures' in readme and 'out of scope' in readme
    kernels = open(os.path.join(ROOT, 'docs', 'KERNELS.md')).read()
    assert 'swd_sort_k' in kernels and 'swd_final_k' in kernels and 'swd_transpose_k' in kernels


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_800_and_the_entry_points_are_bound(lib_built):
    from graphical_gan_amd import _lib, build, functional as F
    lib = _lib.load()
    assert lib.ggan_version() == _lib.ABI_VERSION == 800
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert '#define GGAN_ABI_VERSION 800' in hdr and 'swd.hip' in build.SOURCES
    assert hdr.count('tflib/inception_score.py') >= 2
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret, decl = re.search(r'\b(size_t|int) %s\(([^;]*)\);' % name, hdr).groups()
        assert len(decl.split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    const = lambda n: int(re.search(r'#define %s (\d+)' % n, hdr).group(1))
    assert F.SWD_MAX_ROWS == const('GGAN_SWD_MAX_ROWS') == R.MAX_ROWS == 16384
    assert F.SWD_MAX_DIRS == const('GGAN_SWD_MAX_DIRS') == R.MAX_DIRS == 4096
    assert F.SWD_NONFINITE == const('GGAN_SWD_NONFINITE') == R.NONFINITE == 1


def test_the_entry_points_refuse_bad_arguments_before_any_launch(lib_built):
    """m or n = 0 and 16385, L = 0 and 4097, p = 3, a null pointer, a short or misaligned workspace, a misaligned fp64 output: a negative
    code and a message, on a machine with no device to launch on"""
    from graphical_gan_amd import _lib
    L = _lib.load()
    ptr, big = C.c_void_p(4096), 1 << 40

    def refused(rc, what):
        assert rc < 0 and what.encode() in L.ggan_last_error(), (rc, what, L.ggan_last_error())
    assert L.ggan_swd_workspace(1000, 999, 3) >= 4 * 3 * 1999 and L.ggan_swd_workspace(1000, 999, 3) % 16 == 0
    assert L.ggan_swd_workspace(16384, 16384, 4096) == 2 * 4 * 16384 * 4096
    for bad in ((0, 5, 3), (5, 0, 3), (16385, 5, 3), (5, 16385, 3), (5, 5, 0), (5, 5, 4097), (-1, 5, 3)):
        assert L.ggan_swd_workspace(*bad) == 0, bad
    swd = lambda m=100, n=90, dirs=3, p=2, PX=ptr, PY=ptr, per=ptr, out=ptr, st=ptr, ws=ptr, nb=big: \
        L.ggan_swd(PX, PY, m, n, dirs, p, per, out, st, ws, nb, None)
    for kw in (dict(m=0), dict(n=0), dict(m=16385), dict(n=16385)):
        refused(swd(**kw), '1 <= m, n <= 16384')
    refused(swd(dirs=0), '1 <= L <= 4096')
    refused(swd(dirs=4097), '1 <= L <= 4096')
    refused(swd(p=3), 'p must be 1 or 2')
    refused(swd(p=0), 'p must be 1 or 2')
    for name in ('PX', 'PY', 'per', 'out', 'st', 'ws'):
        refused(swd(**{name: None}), 'null pointer')
    refused(swd(nb=4 * 3 * 190 - 16), 'workspace too small')
    refused(swd(nb=0), 'workspace too small')
    refused(swd(ws=C.c_void_p(4100)), '16-byte aligned')
    refused(swd(per=C.c_void_p(4100)), '8-byte aligned')
    refused(swd(out=C.c_void_p(4100)), '8-byte aligned')


def test_functional_refuses_what_it_must_before_the_device():
    import torch
    from graphical_gan_amd import functional as F, _lib
    x = torch.zeros(10, 4)
    th = torch.zeros(4, 3)
    for a, b, what in ((x, x.double(), 'float32'), (x.double(), x, 'float32'), (x, torch.zeros(10), 'one width'), (torch.zeros(2, 3, 4), x, 'one width'),
                       (x, torch.zeros(10, 5), 'one width'), (torch.zeros(16385, 4), x, 'rows <= 16384'), (x, torch.zeros(16385, 4), 'rows <= 16384'),
                       (torch.zeros(0, 4), x, 'at least 1 row'), (x, torch.zeros(0, 4), 'at least 1 row'),
                       (torch.zeros(10, 0), torch.zeros(10, 0), 'at least 1 column')):
        with pytest.raises(ValueError, match=what):
            F.sliced_wasserstein_projected(a, b)
        with pytest.raises(ValueError, match=what):
            F.sliced_wasserstein(a, b, torch.zeros(a.shape[-1], 3))
    with pytest.raises(ValueError, match='1 <= L <= 4096'):
        F.sliced_wasserstein_projected(torch.zeros(3, 4097), torch.zeros(3, 4097))
    for bad, what in ((torch.zeros(4, 4097), '1 <= L <= 4096'), (torch.zeros(4, 0), '1 <= L <= 4096'), (torch.zeros(5, 3), r'directions \[4, L\]'),
                      (th.double(), 'float32 directions'), (torch.zeros(4), 'float32 directions')):
        with pytest.raises(ValueError, match=what):
            F.sliced_wasserstein(x, x, bad)
    for p in (0, 3, 1.5, None):
        with pytest.raises(ValueError, match='p must be 1 or 2'):
            F.sliced_wasserstein_projected(x, x, p)
        with pytest.raises(ValueError, match='p must be 1 or 2'):
            F.sliced_wasserstein(x, x, th, p)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.sliced_wasserstein_projected(x.clone().requires_grad_(), x)
    with pytest.raises(_lib.GganError, match='no backward'):
        F.sliced_wasserstein(x, x, th.clone().requires_grad_())
    for p in R.PS:
        with pytest.raises(_lib.GganError, match='no CPU path'):           # no fall-back
            F.sliced_wasserstein_projected(x, x + 1, p)
        with pytest.raises(_lib.GganError, match='no CPU path'):
            F.sliced_wasserstein(x, x + 1, th, p)
