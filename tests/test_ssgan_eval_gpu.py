"""-m gpu: the state-space scripts' video passes (evaluate.SequenceEvaluator; ssgan_inference_moving_mnist.py:568-618,
ssgan_inference_chairs.py:560-606) on the HIP path -- ggan_video_sheet_u8 against its host statement byte for byte, the three passes
against the float64 oracle (oracle/ssgan.py) on the same weights, data and noise, what disentangling means, training left bit-identical
by passes run in the middle of it, and the driver / checkpoint CLI files."""
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from test_ssgan_eval_cpu import read_gif

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('samples', 'train_data', 'reconstruction', 'disentangle')


def _fresh():
    from graphical_gan_amd import tflib as lib, optim
    optim.reset_optimizers()
    lib.delete_all_params()


# ---- 5. the kernel, exactly --------------------------------------------------------------------------------------------------------
def _large_grid(rows):
    nh = int(np.sqrt(rows))
    while rows % nh:
        nh -= 1
    return nh, rows // nh


def _host(gen, data, shape, a, b, d, interleave):
    """numpy float32 in the written order: q = trunc(((x + 1) * a) * b) / trunc(x * d), each product rounded once; sheet =
    large_image(q, size=(rows, LEN)); planes = the grey byte or 36 r6 + 6 g6 + b6, r6 = (5 r + 127) / 255"""
    from graphical_gan_amd.tflib.save_images import large_image
    C, H, W = shape
    a, b, d = np.float32(a), np.float32(b), np.float32(d)
    qg = qd = None
    if gen is not None:
        v = ((gen + np.float32(1)) * a) * b
        assert v.dtype == np.float32
        qg = np.clip(np.trunc(v), 0, 255).astype(np.uint8)
    if data is not None:
        v = data * d
        assert v.dtype == np.float32
        qd = np.clip(np.trunc(v), 0, 255).astype(np.uint8)
    if interleave:
        q = np.stack([qd, qg], 1).reshape((-1,) + qg.shape[1:])
    else:
        q = qg if qg is not None else qd
    rows, LEN = q.shape[:2]
    q = q.reshape(rows, LEN, C, H, W)
    sheet = large_image(q.reshape(rows * LEN, C, H, W), size=(rows, LEN))
    nh, nw = _large_grid(rows)
    planes = []
    for t in range(LEN):
        img = large_image(q[:, t], size=(nh, nw)).astype(np.int64)
        if C == 1:
            planes.append(img[:, :, 0])
        else:
            l6 = (5 * img + 127) // 255
            planes.append(36 * l6[:, :, 0] + 6 * l6[:, :, 1] + l6[:, :, 2])
    return sheet, np.stack(planes).astype(np.uint8)


def _edge_values(a, b):
    """generator outputs at and just beside -1, 1 and the inputs whose image sits on an integer boundary k"""
    f = np.float32
    vals = [f(-1), f(1), np.nextafter(f(-1), f(0)), np.nextafter(f(1), f(0)), f(0), np.nextafter(f(0), f(1)), np.nextafter(f(0), f(-1))]
    for k in (1, 2, 3, 64, 127, 128, 129, 200, 254, 255):
        x = f(k / (float(f(a)) * float(f(b))) - 1.0)
        vals += [x, np.nextafter(x, f(2)), np.nextafter(x, f(-2)), np.nextafter(np.nextafter(x, f(2)), f(2))]
    return np.asarray(vals, f)


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('maps', [(0.5, 255.99, 255.99), (255.99 / 2, 1.0, 1.0)], ids=['unit', 'bytes'])
@pytest.mark.parametrize('n,LEN,S', [(3, 5, 16), (5, 3, 16), (3, 2, 64)])
def test_video_sheet_kernel_is_exact(gpu, C, maps, n, LEN, S):
    """(3, 5, 16): 15 / 30 frames of 64 lane items against workgroups of 256 -- the last workgroup is partial"""
    import torch
    from graphical_gan_amd import functional as F
    from graphical_gan_amd import evaluate as E
    a, b, d = maps
    rng = np.random.default_rng(C * 100 + n)
    D = C * S * S
    gen = rng.uniform(-1, 1, size=(n, LEN, D)).astype(np.float32)
    ev = _edge_values(a, b)
    gen.reshape(-1)[:ev.size] = ev
    gen[-1, -1, -ev.size:] = ev
    if d == 1.0:
        data = rng.uniform(0, 256, size=(n, LEN, D)).astype(np.float32)
        data.reshape(-1)[:8] = [0, 255, 255.5, 1, np.nextafter(np.float32(1), np.float32(0)), 127.99999, 128, 254.99998]
    else:
        data = rng.random((n, LEN, D), dtype=np.float32)
        ks = np.asarray([k / 255.99 for k in (0, 1, 2, 127, 128, 254, 255)], np.float32)
        edge = np.concatenate([ks, np.nextafter(ks, np.float32(2)), np.nextafter(ks, np.float32(-1)), [np.float32(1)]]).astype(np.float32)
        data.reshape(-1)[:edge.size] = edge
    g, x = torch.as_tensor(gen, device=gpu), torch.as_tensor(data, device=gpu)
    for name, gg, dd, il in (('generated', gen, None, False), ('data', None, data, False), ('interleaved', gen, data, True)):
        sheet, planes = F.video_sheet_u8(g if gg is not None else None, x if dd is not None else None, (C, S, S), a, b, d, interleave=il)
        torch.cuda.synchronize()
        rows = 2 * n if il else n
        nh, nw = _large_grid(rows)
        assert tuple(sheet.shape) == (rows * S, LEN * S, C) and tuple(planes.shape) == (LEN, nh * S, nw * S)
        want_sheet, want_planes = _host(gg, dd, (C, S, S), a, b, d, il)
        assert np.array_equal(sheet.cpu().numpy(), want_sheet), name
        assert np.array_equal(planes.cpu().numpy(), want_planes), name
        hs, hp = E.host_sheet(gg, dd, (C, S, S), maps, il)            # the package's own host statement says the same
        assert np.array_equal(hs, want_sheet) and np.array_equal(hp, want_planes)


def test_video_sheet_is_capturable(gpu):
    import torch
    from graphical_gan_amd import functional as F
    g = torch.rand((4, 3, 3 * 16 * 16), device=gpu) * 2 - 1
    x = torch.rand((4, 3, 3 * 16 * 16), device=gpu)
    eager = F.video_sheet_u8(g, x, (3, 16, 16), interleave=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            out = F.video_sheet_u8(g, x, (3, 16, 16), interleave=True)
    torch.cuda.current_stream().wait_stream(s)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


# ---- 6. the passes against the oracle -------------------------------------------------------------------------------------------------
def _mk(gpu, pos_mode, op_dyn_mode, B=2, L=3, dim=4, channels=1, n_c=2, bn=False):
    """tests/test_ssgan_gpu.py::_mk (geometry, injected weights) -- with N_C = 2, so that N_VIS = B = 2 is a multiple of it
    (ssgan_inference_moving_mnist.py:56) and class 1 exists; bn: BN_FLAG with random scales / offsets on both sides"""
    from graphical_gan_amd import tflib as lib, optim
    from graphical_gan_amd.engine import Trainer
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    from oracle import ssgan as O
    kw = dict(batch_size=B, length=L, dim=dim, dim_op=16, dim_g=8, dim_l=4, pos_mode=pos_mode, op_dyn_mode=op_dyn_mode, channels=channels,
              n_c=n_c)
    ocfg = O.Cfg(**kw)
    P0 = O.init_params(ocfg, seed=0)
    rng = np.random.default_rng(5)
    for k in P0:
        if k.endswith('.b') or k.endswith('.Biases'):
            P0[k] = (0.1 * rng.standard_normal(P0[k].shape)).astype(np.float32)
    if bn:
        flat = 4 * 4 * 8 * dim
        shapes = {'Generator.BN1': (1, flat), 'Generator.BN2': (4 * dim,), 'Generator.BN3': (2 * dim,), 'Generator.BN4': (dim,)}
        for pre in ('Extractor', 'Extractor.G'):
            shapes.update({pre + '.BN2': (2 * dim,), pre + '.BN3': (4 * dim,), pre + '.BN4': (8 * dim,)})
        for k, s in sorted(shapes.items()):
            P0[k + '.scale'] = (1 + 0.1 * rng.standard_normal(s)).astype(np.float32)
            P0[k + '.offset'] = (0.1 * rng.standard_normal(s)).astype(np.float32)
    optim.reset_optimizers()
    lib.delete_all_params()
    cfg = SSConfig(dataset='chairs' if channels == 3 else 'moving_mnist', bn_g=bn, bn_e=bn, bn_d=bn, **kw)
    tr = Trainer(cfg, device=gpu, graph=False, inject_noise=True, model=StateSpaceGAN(cfg))
    tr.load_params(P0)
    return ocfg, P0, cfg, tr


def _oracle_passes(ocfg, P0, ev, feed, eps, bn, dtype=np.float64):
    """samples (:582-583), rec_x (:514-519) and dis_x (:609) composed from oracle/ssgan.py's nets; with bn, the same nets with
    Batchnorm after the layers the scripts put it (:171-204, :206-262: Linear -> BN1 -> relu, Deconv2..4 -> BN -> relu, Conv2..4 -> BN ->
    LeakyReLU), restated here from oracle.nets because oracle/ssgan.py builds the BN_FLAG = False graph only"""
    from oracle import ssgan as O, tape as tp, nets as N
    P = {k: tp.T(np.asarray(v, dtype)) for k, v in P0.items()}
    T = lambda t: tp.T(np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype))

    def generator(z_g, z_l, labels):
        if not bn:
            return O.Generator(ocfg, P, z_g, z_l, labels)
        out = tp.relu(N.Batchnorm(P, 'Generator.BN1', [0], N.Linear(P, 'Generator.Input', O._z_rows(ocfg, z_g, z_l, labels))))
        out = tp.reshape(out, (ocfg.B * ocfg.LEN, 8 * ocfg.dim, 4, 4))
        for nm in ('2', '3', '4'):
            out = tp.relu(N.Batchnorm(P, 'Generator.BN' + nm, [0, 2, 3], N.Deconv2D(P, 'Generator.' + nm, out)))
        return tp.reshape(tp.tanh(N.Deconv2D(P, 'Generator.5', out)), (ocfg.B, ocfg.LEN, ocfg.output_dim))

    def stack(pre, x):
        out = O._lrelu(N.Conv2D(P, pre + '.1', x))
        for i in (2, 3, 4):
            out = O._lrelu(N.Batchnorm(P, '%s.BN%d' % (pre, i), [0, 2, 3], N.Conv2D(P, '%s.%d' % (pre, i), out)))
        return out

    def extractors(real_x, real_y):
        if not bn:
            return O.Extractor(ocfg, P, real_x, real_y), O.G_Extractor(ocfg, P, real_x, real_y)
        B, L = ocfg.B, ocfg.LEN
        out = tp.reshape(stack('Extractor', tp.reshape(real_x, (B * L, ocfg.C, 64, 64))), (B * L, ocfg.flat))
        q_pre = tp.reshape(N.Linear(P, 'Extractor.Output', tp.concat([out, O.expand_labels(ocfg, real_y)], axis=1)), (B, L, ocfg.dim_l))
        out = tp.reshape(stack('Extractor.G', tp.reshape(real_x, (B, ocfg.C * L, 64, 64))), (B, ocfg.flat))
        return q_pre, N.Linear(P, 'Extractor.G.Output', tp.concat([out, real_y], axis=1))

    dt = dtype
    samples = generator(T(ev.fixed_noise_g), O.DynamicGenerator(ocfg, P, T(ev.pre_fixed_noise), T(eps)), T(ev.fixed_y))
    real_x = tp.T(dt(2) * (np.asarray(feed['real_x_unit'], dtype=dt) / dt(ocfg.x_div) - dt(.5)))
    real_y = tp.T(np.asarray(feed['real_y'], dt))
    q_pre, q_z_g = extractors(real_x, real_y)
    q_z_l = O.DynamicExtractor(ocfg, P, q_pre)
    rec_x = generator(q_z_g, q_z_l, real_y)
    dis_x = generator(T(ev.dis_g), q_z_l, T(ev.dis_y))
    return samples.v, rec_x.v, dis_x.v


@pytest.mark.parametrize('pos_mode,op_dyn_mode,channels,bn', [
    ('naive_mean_field', 'res', 1, False), ('gsp', 'res_w', 1, False), ('naive_mean_field', 'res_w', 3, False),
    ('naive_mean_field', 'res', 1, True)], ids=['nmf-res-mnist', 'gsp-resw-mnist', 'nmf-resw-chairs', 'bn-mnist'])
def test_passes_match_oracle(gpu, pos_mode, op_dyn_mode, channels, bn):
    """samples, rec_x, dis_x as floats within 1e-5 absolute of the float64 oracle (the bound tests/test_ssgan_gpu.py:68 applies to the
    same generator's output).  The oracle's own float32-vs-float64 gap is printed beside each figure."""
    from graphical_gan_amd.evaluate import SequenceEvaluator
    from oracle import ssgan as O
    ocfg, P0, cfg, tr = _mk(gpu, pos_mode, op_dyn_mode, channels=channels, n_c=0 if channels == 3 else 2, bn=bn)
    ev = SequenceEvaluator(tr, dict(BATCH_SIZE=2, N_VIS=2, SEED=1))
    feed = O.make_feed(ocfg, np.random.default_rng(3))
    batch = (feed['real_x_unit'], feed['real_y'])
    got = [ev.samples().cpu().numpy()]
    eps = ev.feed['epsilon'].cpu().numpy().copy()
    got += [ev.reconstructions(batch).cpu().numpy(), ev.disentangle(batch).cpu().numpy()]
    want = _oracle_passes(ocfg, P0, ev, feed, eps, bn)
    want32 = _oracle_passes(ocfg, P0, ev, feed, eps, bn, np.float32)
    errs = {}
    for name, g, w, w32 in zip(('samples', 'rec_x', 'dis_x'), got, want, want32):
        assert g.shape == w.shape == (2, 3, ocfg.output_dim)
        errs[name] = float(np.abs(g - w).max())
        print('%s: |hip - float64| = %.3g, oracle |float32 - float64| = %.3g' % (name, errs[name], float(np.abs(w32 - w).max())))
    assert max(errs.values()) <= 1e-5, errs
    # a second call draws a new epsilon (:137 inside :582); the fixed-data passes are functions of the data alone
    assert not np.array_equal(ev.samples().cpu().numpy(), got[0])
    assert not np.array_equal(ev.feed['epsilon'].cpu().numpy(), eps)
    assert np.array_equal(ev.reconstructions(batch).cpu().numpy(), got[1])
    # the Trainer's own feed and noise state were not the ones used
    assert tr.feed['rng_state'].data_ptr() != ev.feed['rng_state'].data_ptr()
    assert tr.feed['real_x_unit'].data_ptr() != ev.feed['real_x_unit'].data_ptr()


# ---- 7. what disentangling means --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('channels', [1, 3])
def test_disentangle_semantics(gpu, channels):
    import torch
    from graphical_gan_amd.evaluate import SequenceEvaluator
    from oracle import ssgan as O
    B = 4
    ocfg, P0, cfg, tr = _mk(gpu, 'gsp', 'res_w', B=B, channels=channels, n_c=0 if channels == 3 else 2)
    ev = SequenceEvaluator(tr, dict(BATCH_SIZE=B, N_VIS=B, SEED=2))
    feed = O.make_feed(ocfg, np.random.default_rng(8))
    x, y = feed['real_x_unit'], feed['real_y']
    base = ev.disentangle((x, y)).cpu().numpy()
    assert np.abs(base[0] - base[1]).max() > 1e-3                  # (different sequences give different rows)
    perm = np.array([2, 0, 3, 1])
    permuted = ev.disentangle((x[perm], y[perm])).cpu().numpy()
    # the rows follow their sequences (and, for moving-MNIST, their labels, which q_z_l reads); a kernel's row-to-tile mapping may
    # reorder sums, hence the tolerance of the oracle comparison rather than equality
    assert np.abs(permuted - base[perm]).max() <= 1e-5
    # fixed_noise_g is not an input
    ev.fixed_noise_g = torch.randn_like(ev.fixed_noise_g)
    assert np.array_equal(ev.disentangle((x, y)).cpu().numpy(), base)
    # B copies of one sequence: B identical rows
    same = ev.disentangle((np.repeat(x[:1], B, 0), np.repeat(y[:1], B, 0))).cpu().numpy()
    assert np.abs(same - same[0]).max() <= 1e-5
    assert np.abs(same[0] - base[0]).max() <= 1e-5                 # .. the row that sequence had in the mixed minibatch


# ---- 8. training is not disturbed -------------------------------------------------------------------------------------------------
def _train(S, cfg):
    from graphical_gan_amd import run, optim
    from graphical_gan_amd.models_ssgan import StateSpaceGAN
    _fresh()
    tr = run.train(S, cfg, model=StateSpaceGAN(cfg))
    w = tr.get_params()
    adam = {}
    for key, o in optim._optimizers.items():
        adam[key[0]] = (o.step.cpu().numpy().copy(), o.m.cpu().numpy().copy(), o.v.cpu().numpy().copy())
    return tr, w, adam


def _small(script, **over):
    from graphical_gan_amd import run
    kw = dict(BATCH_SIZE=4, LEN=3, DIM=4, DIM_LATENT_G=8, ITERS=6, LOG_EVERY=3, SYNTHETIC='force', SEED=3)
    if script == 'ssgan_inference_moving_mnist':
        kw['N_C'] = 2
    kw.update(over)
    S = run.reference_block(script, **kw)
    S['SCRIPT'] = script
    return S


@pytest.mark.parametrize('script,bn', [('ssgan_inference_moving_mnist', False), ('ssgan_inference_chairs', True)])
def test_training_bit_identical_with_video_passes(gpu, tmp_path, script, bn):
    from graphical_gan_amd import run
    S0 = _small(script, BN_FLAG=bn)
    assert S0.get('HIP_GRAPH', True) is True and not run.eval_plan(S0)
    tr0, w0, a0 = _train(dict(S0), run.config(S0))
    assert tr0.graph_enabled
    out = tmp_path / 'out'
    S1 = dict(S0, SAMPLE_EVERY=2, OUT_DIR=str(out))
    tr1, w1, a1 = _train(S1, run.config(S1))
    assert sorted(w0) == sorted(w1) and sorted(a0) == sorted(a1) and len(a0) == 2
    for k in w0:
        assert np.array_equal(w0[k], w1[k]), k
    for r in a0:
        for u, v in zip(a0[r], a1[r]):
            assert np.array_equal(u, v), r
    files = sorted(p.name for p in out.iterdir() if p.suffix in ('.png', '.gif'))
    assert files == sorted('%s_%d.%s' % (n, it, e) for n in NAMES for it in (1, 3, 5) for e in ('png', 'gif')), files


# ---- 9. the driver and the CLI ----------------------------------------------------------------------------------------------------
def read_png(path):
    b = open(path, 'rb').read()
    assert b[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(b):
        n, tag = struct.unpack('>I', b[pos:pos + 4])[0], b[pos + 4:pos + 8]
        body = b[pos + 8:pos + 8 + n]
        assert zlib.crc32(tag + body) & 0xffffffff == struct.unpack('>I', b[pos + 8 + n:pos + 12 + n])[0]
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    w, h, depth, ctype = hdr[:4]
    assert depth == 8 and ctype in (0, 2)
    ch = 1 if ctype == 0 else 3
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + w * ch)
    assert (raw[:, 0] == 0).all()                 # filter type None on every line
    return raw[:, 1:].reshape(h, w, ch)


@pytest.mark.parametrize('script', ['ssgan_inference_moving_mnist', 'ssgan_inference_chairs'])
def test_driver_writes_the_files_and_the_cli_repeats_them(gpu, tmp_path, script):
    from graphical_gan_amd import run, checkpoint
    out = tmp_path / 'out'
    S = _small(script, ITERS=4, SAMPLE_EVERY=2, OUT_DIR=str(out))
    cfg = run.config(S)
    tr, _, _ = _train(S, cfg)
    B, L, C, H = cfg.B, cfg.LEN, cfg.C, 64
    files = sorted(p.name for p in out.iterdir() if p.suffix in ('.png', '.gif'))
    assert files == sorted('%s_%d.%s' % (n, it, e) for n in NAMES for it in (1, 3) for e in ('png', 'gif')), files
    # the fixed minibatch: the first of the evaluation set, a function of the settings alone
    dev, _ = run.eval_sets(S, tr.model, gpu)
    x = dev[0][0].cpu().numpy().reshape(B, L, C, H, H)
    d = np.float32(1.0 if script.endswith('chairs') else 255.99)
    fixed = np.clip(np.trunc(x * d), 0, 255).astype(np.uint8)
    for it in (1, 3):
        for name in NAMES:
            rows = B if name in ('samples', 'train_data') else 2 * B
            img = read_png(str(out / ('%s_%d.png' % (name, it))))
            assert img.shape == (rows * H, L * H, C), (name, img.shape)
            rgb, planes, loops = read_gif(str(out / ('%s_%d.gif' % (name, it))))
            nh, nw = _large_grid(rows)
            assert planes.shape == (L, nh * H, nw * H) and loops == 0, (name, planes.shape)
            tiles = img.reshape(rows, H, L, H, C).transpose(0, 2, 4, 1, 3)          # [rows, LEN, C, H, W]
            if name in ('reconstruction', 'disentangle'):
                assert np.array_equal(tiles[0::2], fixed), name                      # even rows: the fixed minibatch
                assert tiles[1::2].std() > 0
            # the GIF shows the same bytes (exactly for grey, through the colour cube for RGB)
            cells = rgb.reshape(L, nh, H, nw, H, 3).transpose(1, 3, 0, 5, 2, 4).reshape(rows, L, 3, H, H)
            diff = np.abs(cells[:, :, :C].astype(np.int32) - tiles.astype(np.int32)).max()
            assert diff <= (0 if C == 1 else 26), (name, diff)
    # checkpoint -> the CLI in a fresh process writes the same reconstruction from it
    ckpt = str(tmp_path / 'params_4.npz')
    checkpoint.save(ckpt, tr)
    live = tmp_path / 'live'
    live.mkdir()
    from graphical_gan_amd.evaluate import SequenceEvaluator
    ev = SequenceEvaluator(tr, S)
    ev.set_fixed_data(dev[0])
    ev.save_videos(str(live), 'eval', train_data=dev[0])
    cli = tmp_path / 'cli'
    keys = ('BATCH_SIZE', 'LEN', 'DIM', 'DIM_LATENT_G', 'SYNTHETIC', 'SEED') + (('N_C',) if S['N_C'] else ())
    cmd = [sys.executable, '-m', 'graphical_gan_amd.evaluate', ckpt, '--script', script, '--out-dir', str(cli)]
    cmd += ['--set=%s=%s' % (k, S[k]) for k in keys]
    r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors='replace')[-2000:]
    assert sorted(p.name for p in cli.iterdir()) == sorted('%s_eval.%s' % (n, e) for n in NAMES for e in ('png', 'gif'))
    for name in NAMES:          # (fixed data and fixed noise depend on the settings seed alone; a fresh evaluator's first epsilon too)
        for e in ('png', 'gif'):
            assert (cli / ('%s_eval.%s' % (name, e))).read_bytes() == (live / ('%s_eval.%s' % (name, e))).read_bytes(), (name, e)
    # .. and they are the bytes the driver wrote after the last iteration, whose weights the checkpoint holds
    for name in ('reconstruction', 'disentangle'):
        for e in ('png', 'gif'):
            assert (cli / ('%s_eval.%s' % (name, e))).read_bytes() == (out / ('%s_3.%s' % (name, e))).read_bytes(), (name, e)
