"""not-gpu: the reconstruction-fidelity op's ABI (header, binding, built library, argument errors without a GPU), what the Python ops
refuse, the cadence settings of the dev-set reconstruction pass for all ten scripts, what the CLI refuses before a
checkpoint is read, and the float64 restatement tests/_ssim_ref.py: its closed forms by hand, its agreement with scipy's Gaussian filter,
and the condition on the shared cases under which the GPU tests test something (raw one-pass moments in float32 miss the gate on the bright
flat planes; centred ones do not)."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ssim_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('ggan_ssim_pairs_workspace', 'ggan_ssim_pairs')
IMAGE_SCRIPTS = ['%s_inference_%s' % (f, d) for f in ('gan', 'gmgan') for d in ('cifar10', 'svhn', 'mnist', 'face')]
SEQUENCE_SCRIPTS = ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs']
SCORE_VARS = ['GGAN_%s_EVERY' % n for n in ('MMD', 'PRDC', 'KNN', 'PARZEN', 'REC')]
KEYS = ['dev rec mse x', 'dev rec psnr x', 'dev rec ssim x', 'dev rec ssim se x']


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def test_window():
    g, W = R.taps(), R.window()
    assert g.shape == (11,) and W.shape == (11, 11) and abs(g.sum() - 1) < 1e-15 and abs(W.sum() - 1) < 1e-15
    assert np.array_equal(g, g[::-1]) and np.argmax(g) == 5
    assert np.allclose(g[5 + 1] / g[5], np.exp(-0.5 / 2.25), rtol=1e-15)               # sigma 1.5
    assert (R.C1, R.C2) == (1e-4, 9e-4)


@pytest.mark.parametrize('shape', [(1, 11, 11), (3, 12, 17), (1, 64, 64)])
def test_constant_planes_closed_form(shape):
    c, h, w = shape
    for a, b in ((0.0, 0.0), (0.0, 1.0), (0.25, 0.75), (0.98, 0.97), (1.0, 1.0)):
        mse, ssim = R.pairs(np.full((2, c * h * w), a, np.float32), np.full((2, c * h * w), b, np.float32), shape)
        a64, b64 = float(np.float32(a)), float(np.float32(b))
        assert np.allclose(ssim, (2 * a64 * b64 + R.C1) / (a64 ** 2 + b64 ** 2 + R.C1), rtol=0, atol=1e-12)
        assert np.allclose(mse, (a64 - b64) ** 2, rtol=0, atol=1e-15)


def test_a_set_against_itself():
    for kind in ('smooth', 'noise', 'bright_flat'):
        a = R.case(kind, 5, 1, 12, 17)[0]
        mse, ssim = R.pairs(a, a, (1, 12, 17))
        assert np.array_equal(ssim, np.ones(5)) and np.array_equal(mse, np.zeros(5))
    assert np.array_equal(R.psnr([0.0, 1e-12, 1e-10, 0.01, 1.0]), [100.0, 100.0, 100.0, 20.0, 0.0])


def test_one_window_position_by_hand():
    """h = w = 11: the map has one entry, the weighted moments of the whole plane -- written out with loops"""
    a, b, ma, mb = R.case('two_maps', 1, 1, 11, 11)
    ua, ub = ma[0] * a.astype(np.float64).reshape(11, 11) + ma[1], mb[0] * b.astype(np.float64).reshape(11, 11) + mb[1]
    g = [np.exp(-(k - 5) ** 2 / (2 * 1.5 ** 2)) for k in range(11)]
    tot = sum(g)
    mx = my = 0.0
    for i in range(11):
        for j in range(11):
            wt = g[i] * g[j] / tot ** 2
            mx += wt * ua[i, j]
            my += wt * ub[i, j]
    sxx = syy = sxy = 0.0
    for i in range(11):
        for j in range(11):
            wt = g[i] * g[j] / tot ** 2
            sxx += wt * (ua[i, j] - mx) ** 2
            syy += wt * (ub[i, j] - my) ** 2
            sxy += wt * (ua[i, j] - mx) * (ub[i, j] - my)
    want = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    mse, ssim = R.reference('two_maps', 1, 1, 11, 11)
    assert ssim.shape == (1,) and abs(ssim[0] - want) < 1e-13
    assert abs(mse[0] - np.mean((ua - ub) ** 2)) < 1e-15


@pytest.mark.parametrize('kind', ['smooth', 'noise', 'binary_dimmed'])
def test_restatement_against_scipy_gaussian_filter(kind):
    """scikit-image's recipe with scipy's filter: gaussian_filter(sigma=1.5, truncate=3.5) of x, y, xx, yy, xy, E[xy] - mx my, cropped by 5
    on every side (inside the crop no border mode is seen)"""
    ndi = pytest.importorskip('scipy.ndimage')
    n, c, h, w = 5, 1, 12, 17
    a, b, ma, mb = R.case(kind, n, c, h, w)
    ua, ub = R.unit(a, ma).reshape(n, h, w), R.unit(b, mb).reshape(n, h, w)
    f = lambda v: ndi.gaussian_filter(v, sigma=1.5, truncate=3.5, mode='reflect')
    _, ref = R.reference(kind, n, c, h, w)
    for i in range(n):
        x, y = ua[i], ub[i]
        mx, my = f(x), f(y)
        sxx, syy, sxy = f(x * x) - mx * mx, f(y * y) - my * my, f(x * y) - mx * my
        m = ((2 * mx * my + R.C1) * (2 * sxy + R.C2)) / ((mx * mx + my * my + R.C1) * (sxx + syy + R.C2))
        assert abs(m[5:-5, 5:-5].mean() - ref[i]) < 1e-10, (i, m[5:-5, 5:-5].mean(), ref[i])


def test_the_bright_flat_planes_tell_the_two_formulations_apart():
    """a condition on the inputs, from the host alone: in float32 the raw one-pass moments miss the gate on the bright flat planes where an
    image has few window positions to average its error over (and stay a thousand times worse where it has many); the centred ones stay
    far inside it -- on every shape and every kind"""
    for shape in R.SHAPES + R.EXTRA_SHAPES:
        a, b, ma, mb = R.case('bright_flat', *shape)
        _, ref = R.reference('bright_flat', *shape)
        raw = (np.abs(R.pairs_f32(a, b, shape[1:], ma, mb, centred=False) - ref) / R.gate(ref)).max()
        cen = (np.abs(R.pairs_f32(a, b, shape[1:], ma, mb, centred=True) - ref) / R.gate(ref)).max()
        print('bright flat planes', shape, 'float32 error / gate: raw %.2f, centred %.5f' % (raw, cen))
        assert cen < 0.05 and raw > 100 * cen, shape
        if shape[2] * shape[3] <= 28 * 28:
            assert raw > 1.0, shape
    for kind in R.KINDS:
        a, b, ma, mb = R.case(kind, 5, 1, 12, 17)
        _, ref = R.reference(kind, 5, 1, 12, 17)
        assert (np.abs(R.pairs_f32(a, b, (1, 12, 17), ma, mb) - ref) / R.gate(ref)).max() < 0.5, kind


def test_the_shared_cases_are_what_they_say():
    for kind in R.KINDS:
        a, b, ma, mb = R.case(kind, 5, 1, 12, 17)
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (5, 204) and not a.flags.writeable
        assert R.case(kind, 5, 1, 12, 17)[0] is a
    _, noise = R.reference('noise', 67, 1, 28, 28)
    assert noise.min() < 0.0 < noise.max() and np.abs(noise).max() < 0.2             # SSIM near 0, some values negative
    a, b, ma, mb = R.case('two_maps', 5, 1, 12, 17)
    assert (ma, mb) == (R.TANH, R.BYTES) and a.min() < 0.0 and b.max() > 100.0 and np.array_equal(b, np.round(b))
    a, b, _, _ = R.case('binary_dimmed', 5, 1, 12, 17)
    assert set(np.unique(a)) <= {0.0, 1.0} and np.array_equal(b, np.float32(0.7) * a)
    assert R.SHAPES == [(1, 1, 11, 11), (5, 1, 12, 17), (67, 1, 28, 28), (33, 3, 32, 32), (9, 1, 64, 64), (6, 3, 64, 64)]
    p = R.pass_values([0.01, 0.04], [0.5, 0.7])
    assert abs(p['dev rec psnr x'] - (20.0 - 10 * np.log10(0.04)) / 2) < 1e-12 and abs(p['dev rec ssim se x'] - 0.1 / np.sqrt(2)) < 1e-15
    assert abs(p['dev rec mse x'] - 0.025) < 1e-15 and abs(p['dev rec ssim x'] - 0.6) < 1e-15 and list(p) == KEYS


# ---- ABI -------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree(lib_built):
    from graphical_gan_amd import _lib, build
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = C.CDLL(lib_built)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        ret = 'size_t' if name.endswith('_workspace') else 'int'
        decl = re.search(r'\b%s\s+%s\(([^;]*)\);' % (ret, name), code)
        assert decl, name
        assert len(decl.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert _lib.SIGNATURES[name][0] is (C.c_size_t if ret == 'size_t' else C.c_int), name
    assert _lib.SIGNATURES['ggan_ssim_pairs'][1][6:10] == [C.c_float] * 4
    assert 'ssim_pairs.hip' in build.SOURCES and os.path.isfile(os.path.join(build.CSRC, 'ssim_pairs.hip'))
    assert _lib.load().ggan_version() == _lib.ABI_VERSION == 800            # new entry points only
    assert '#define GGAN_ABI_VERSION 800' in hdr


def test_workspace(lib_built):
    from graphical_gan_amd import _lib
    w = _lib.load().ggan_ssim_pairs_workspace
    for n, c, h, wd in ((1, 1, 11, 11), (10000, 3, 32, 32), (131072, 4, 64, 64), (5, 1, 12, 17), (3, 2, 64, 11)):
        assert w(n, c, h, wd) == 8 * n * c, (n, c, h, wd)                   # two floats per plane: linear in the planes, not in the pixels
    for bad in ((0, 1, 32, 32), (131073, 1, 32, 32), (5, 0, 32, 32), (5, 5, 32, 32), (5, 1, 10, 32), (5, 1, 32, 10), (5, 1, 65, 32),
                (5, 1, 32, 65), (-1, 1, 32, 32)):
        assert w(*bad) == 0, bad


def test_argument_errors_come_back_before_any_launch(lib_built):
    from graphical_gan_amd import _lib
    L = _lib.load()
    p = lambda v=4096: C.c_void_p(v)           # (never dereferenced: every case fails its checks first)

    def call(A=p(), B=p(), n=9, c=3, h=32, w=32, maps=(0.5, 0.5, 1.0, 0.0), mse=p(), ssim=p(), ws=p(), wsb=1 << 20):
        rc = L.ggan_ssim_pairs(A, B, n, c, h, w, maps[0], maps[1], maps[2], maps[3], mse, ssim, ws, wsb, None)
        return rc, (L.ggan_last_error() or b'').decode()
    for kw, word in ((dict(h=10), 'h, w'), (dict(w=65), 'h, w'), (dict(c=5), 'c <= 4'), (dict(n=0), 'n <= 131072'),
                     (dict(ssim=None), 'null'), (dict(mse=None), 'null'), (dict(wsb=L.ggan_ssim_pairs_workspace(9, 3, 32, 32) - 1), 'workspace'),
                     (dict(h=65), 'h, w'), (dict(w=10), 'h, w'), (dict(c=0), 'c <= 4'), (dict(n=131073), 'n <= 131072'), (dict(n=-3), 'n <= 131072'),
                     (dict(A=None), 'null'), (dict(B=None), 'null'), (dict(ws=None), 'null'), (dict(wsb=0), 'workspace'),
                     (dict(ws=p(4098)), 'aligned'), (dict(maps=(float('nan'), 0.0, 1.0, 0.0)), 'finite'),
                     (dict(maps=(0.5, 0.5, 1.0, float('inf'))), 'finite')):
        rc, msg = call(**kw)
        assert rc < 0 and 'ggan_ssim_pairs' in msg and word in msg, (kw, rc, msg)


def test_python_ops_refuse_what_they_cannot_do(lib_built):
    import torch
    from graphical_gan_amd import functional as F, _lib
    x, y = torch.zeros(7, 3 * 32 * 32), torch.zeros(7, 3 * 32 * 32)
    with pytest.raises(_lib.GganError):                              # no CPU path
        F.ssim_pairs(x, y, (3, 32, 32))
    with pytest.raises(_lib.GganError):
        F.ssim_pairs(x, x, (3, 32, 32), (0.5, 0.5))
    g = torch.zeros(7, 3 * 32 * 32, requires_grad=True)
    for call in (lambda: F.ssim_pairs(g, y, (3, 32, 32)), lambda: F.ssim_pairs(x, g, (3, 32, 32))):
        with pytest.raises(_lib.GganError, match='no backward'):
            call()
    for call in (lambda: F.ssim_pairs(x, y, (3, 32, 31)), lambda: F.ssim_pairs(x, y[:6], (3, 32, 32)), lambda: F.ssim_pairs(x, y, (3, 32)),
                 lambda: F.ssim_pairs(torch.zeros(7, 5 * 144), torch.zeros(7, 5 * 144), (5, 12, 12)),
                 lambda: F.ssim_pairs(torch.zeros(7, 100), torch.zeros(7, 100), (1, 10, 10)),
                 lambda: F.ssim_pairs(torch.zeros(2, 65 * 11), torch.zeros(2, 65 * 11), (1, 65, 11)),
                 lambda: F.ssim_pairs(torch.zeros(0, 121), torch.zeros(0, 121), (1, 11, 11)),
                 lambda: F.ssim_pairs(torch.zeros(121), torch.zeros(121), (1, 11, 11)),
                 lambda: F.ssim_pairs(x, y, (3, 32, 32), (0.5,)), lambda: F.ssim_pairs(x, y, (3, 32, 32), (0.5, float('nan'))),
                 lambda: F.ssim_pairs(x, y, (3, 32, 32), (1.0, 0.0), (float('inf'), 0.0)), lambda: F.ssim_pairs(x, y, (3, 32, 32), 0.5)):
        with pytest.raises(ValueError):
            call()


def test_psnr_from_mse_caps_at_100_db():
    import torch
    from graphical_gan_amd import functional as F
    mse = torch.tensor([0.0, 1e-12, 1e-10, 1e-4, 0.01, 0.25, 1.0], dtype=torch.float32)
    got = F.psnr_from_mse(mse)
    assert got.dtype == torch.float64 and tuple(got.shape) == (7,)
    want = R.psnr(mse.numpy())
    assert np.all(np.abs(got.numpy() - want) <= 1e-12) and got[0] == 100.0 and got[1] == 100.0 and np.all(np.isfinite(got.numpy()))
    assert abs(float(got[4]) - 20.0) < 1e-5 and abs(float(got[6])) == 0.0
    assert float(got.mean()) < 100.0                                   # (a perfect image does not poison a mean)


# ---- the pass's switches ---------------------------------------------------------------------------------------------------------------
def test_rec_settings_and_cadence(monkeypatch):
    from graphical_gan_amd import run
    every = IMAGE_SCRIPTS + SEQUENCE_SCRIPTS
    for v in SCORE_VARS:
        monkeypatch.delenv(v, raising=False)
    others = lambda s: (run.eval_settings(s), run.manifold_settings(s))
    base = {s: others(s) for s in every}
    for s in every:                                # the default is off
        assert run.score_settings(s) == {} and run.score_settings('/somewhere/%s.py' % s) == {}
    monkeypatch.setenv('GGAN_REC_EVERY', '20')
    for s in every:                                # all ten scripts, the state-space ones included (exactly the one key)
        assert run.score_settings(s) == {'REC_EVERY': 20} and run.score_settings('/somewhere/%s.py' % s) == {'REC_EVERY': 20}
    assert run.score_settings('no_such_script') == {}
    for s in every:                 # the other settings functions do not learn the variable, and the key is in no *_KEYS
        assert others(s) == base[s]
    assert 'REC_EVERY' not in run.EVAL_KEYS and 'REC_EVERY' not in run.MANIFOLD_KEYS
    for script in ('gan_inference_mnist', 'ssgan_inference_chairs'):
        S = dict(run.reference_block(script), **run.score_settings(script))
        assert run.eval_plan(S) is None and run.manifold_plan(S) is None
        assert [it for it in range(60) if 'rec' in run.scores_due(S, it)] == [19, 39, 59]
        assert not any(set(run.scores_due(S, it)) & {'mmd', 'prdc', 'knn', 'parzen'} for it in range(60))
        assert not any(run.scores_due(run.reference_block(script), it) for it in range(60))
    monkeypatch.delenv('GGAN_REC_EVERY')
    monkeypatch.setenv('GGAN_PARZEN_EVERY', '20')
    for s in every:
        assert 'REC_EVERY' not in run.score_settings(s)


def test_rec_constants_and_signatures():
    from graphical_gan_amd import evaluate
    assert evaluate.REC_MAX_ROWS == 10000 and list(evaluate.REC_KEYS) == KEYS
    assert list(inspect.signature(evaluate.Evaluator.rec_scores).parameters) == ['self', 'batches', 'return_rows']
    assert list(inspect.signature(evaluate.SequenceEvaluator.rec_scores).parameters) == ['self', 'batches', 'return_rows', 'per_frame']


def test_cli_refusals_come_with_their_reason_before_the_checkpoint_is_read(monkeypatch, capsys):
    from graphical_gan_amd import evaluate, engine, models_ssgan

    class Reached(Exception):
        pass

    def stop(*a, **k):
        raise Reached()
    monkeypatch.setattr(engine, 'Trainer', stop)            # (what main builds once no argument has been refused, before it reads the file)
    monkeypatch.setattr(models_ssgan, 'StateSpaceGAN', stop)
    monkeypatch.setattr(evaluate.lib, 'get_device', stop)
    seq = ['nowhere.npz', '--script', 'ssgan_inference_chairs']
    with pytest.raises(SystemExit):                         # the videos still need a place ...
        evaluate.main(seq)
    assert '--out-dir is required' in capsys.readouterr().err
    for flag, why in (('--mmd', 'no single code'), ('--prdc', 'no single code'), ('--knn', 'no single code'), ('--parzen', 'no single set of images')):
        with pytest.raises(SystemExit):                     # ... the other set-level passes are still refused for sequences, --rec or not ...
            evaluate.main(seq + ['--rec', flag])
        assert why in capsys.readouterr().err
    with pytest.raises(SystemExit):
        evaluate.main(['nowhere.npz', '--script', 'gan_inference_cifar10', '--rec', '--manifold', '--out-dir', 'x'])
    assert '--manifold' in capsys.readouterr().err
    for args in (seq + ['--rec'], seq + ['--rec', '--out-dir', 'x'], ['nowhere.npz', '--script', 'gan_inference_mnist', '--rec']):
        with pytest.raises(Reached):                        # ... and --rec itself refuses nothing, for any script, with or without --out-dir
            evaluate.main(args)
