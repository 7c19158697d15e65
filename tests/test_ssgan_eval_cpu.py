"""not-gpu: the host side of the state-space scripts' video passes (samples / train_data / reconstruction / disentangle,
ssgan_inference_moving_mnist.py:568-618): the GIF writer against a decoder of this file's own, the cadence settings, the C ABI of
ggan_video_sheet_u8 and its refusals, the evaluator's fixed inputs."""
import ctypes as C
import os
import re
import struct
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SSGAN = ('ssgan_inference_moving_mnist', 'ssgan_inference_chairs')


# ---- a GIF89a reader with a variable-width LZW decoder (shares nothing with the writer) ------------------------------------------
def _lzw(data, min_size, npix):
    clear, eoi = 1 << min_size, (1 << min_size) + 1
    table, width, prev = None, min_size + 1, None
    out = bytearray()
    acc = nbits = pos = 0
    while True:
        while nbits < width:
            acc |= data[pos] << nbits
            pos += 1
            nbits += 8
        code = acc & ((1 << width) - 1)
        acc >>= width
        nbits -= width
        if code == clear:
            table = [bytes([i]) for i in range(clear)] + [b'', b'']
            width, prev = min_size + 1, None
            continue
        if code == eoi:
            break
        if prev is None:
            entry = table[code]
        else:
            entry = table[code] if code < len(table) else prev + prev[:1]
            table.append(prev + entry[:1])
            if len(table) == (1 << width) and width < 12:
                width += 1
        out += entry
        prev = entry
    assert len(out) == npix, (len(out), npix)
    return bytes(out)


def read_gif(path):
    """-> (frames [n, h, w, 3] uint8 through the palette, index planes [n, h, w], loops: the NETSCAPE2.0 count or None)"""
    b = open(path, 'rb').read()
    assert b[:6] == b'GIF89a'
    w, h, flags = struct.unpack('<HHB', b[6:11])
    assert flags & 0x80
    ncol = 2 << (flags & 7)
    pal = np.frombuffer(b[13:13 + 3 * ncol], np.uint8).reshape(ncol, 3)
    pos, planes, loops = 13 + 3 * ncol, [], None

    def blocks(pos):
        data = bytearray()
        while b[pos]:
            data += b[pos + 1:pos + 1 + b[pos]]
            pos += 1 + b[pos]
        return bytes(data), pos + 1
    while b[pos] != 0x3B:
        if b[pos] == 0x21:
            label = b[pos + 1]
            data, pos = blocks(pos + 2)
            if label == 0xFF and data[:11] == b'NETSCAPE2.0':
                loops = struct.unpack('<H', data[12:14])[0]
        else:
            assert b[pos] == 0x2C
            x0, y0, fw, fh, fl = struct.unpack('<HHHHB', b[pos + 1:pos + 10])
            assert (x0, y0, fw, fh) == (0, 0, w, h) and not fl & 0xC0            # whole canvas, no local table, not interlaced
            min_size = b[pos + 10]
            data, pos = blocks(pos + 11)
            planes.append(np.frombuffer(_lzw(data + b'\0\0', min_size, w * h), np.uint8).reshape(h, w))
    planes = np.stack(planes)
    return pal[planes], planes, loops


def test_lzw_decoder_reads_a_compressing_stream():
    """the decoder above is a general one: a widely published 10 x 10 four-colour sample whose stream uses table entries and two code
    widths changes (3 -> 4 -> 5 -> 6 bits)"""
    data = bytes.fromhex('8C2D99872A1CDC33A00275EC95FAA8DE608C04914C01')
    px = _lzw(data + b'\0\0', 2, 100)
    want = ([1] * 5 + [2] * 5) * 3 + ([1] * 3 + [0] * 4 + [2] * 3) * 2 + ([2] * 3 + [0] * 4 + [1] * 3) * 2 + ([2] * 5 + [1] * 5) * 3
    assert list(px) == want


# ---- 1. save_gifs round trip -----------------------------------------------------------------------------------------------------
def test_save_gifs_grey_is_exact(tmp_path):
    from graphical_gan_amd.tflib import save_images as S
    rng = np.random.default_rng(0)
    x = rng.random((6, 5, 1, 16, 20), dtype=np.float32)
    x[0, 0, 0, 0, :4] = [0.0, 1.0, 0.5, 255 / 255.99]
    p = str(tmp_path / 'g.gif')
    S.save_gifs(x, p)
    rgb, planes, loops = read_gif(p)
    assert loops == 0                                            # the loop extension, for ever
    assert planes.shape == (5, 2 * 16, 3 * 20)                   # LEN frames; 6 samples tile as 2 x 3 (large_image's size=None rule)
    for t in range(5):
        want = S.large_image(x[:, t])[:, :, 0]
        assert np.array_equal(planes[t], want)
        assert np.array_equal(rgb[t], np.repeat(want[:, :, None], 3, axis=2))
    # bytes go through unchanged, and an explicit size is honoured
    xb = rng.integers(0, 256, size=(4, 3, 1, 8, 8)).astype(np.uint8)
    S.save_gifs(xb, p, size=(1, 4))
    _, planes, _ = read_gif(p)
    assert planes.shape == (3, 8, 32)
    assert all(np.array_equal(planes[t], S.large_image(xb[:, t], (1, 4))[:, :, 0]) for t in range(3))


def test_save_gifs_colour_cube(tmp_path):
    from graphical_gan_amd.tflib import save_images as S
    rng = np.random.default_rng(1)
    x = rng.integers(0, 256, size=(6, 4, 3, 16, 12)).astype(np.uint8)
    x[0, 0, :, 0, :6] = np.arange(6) * 51
    x[1, 0, 0, 0, :8] = [25, 26, 76, 77, 127, 128, 229, 230]     # either side of the cube's decision levels
    p = str(tmp_path / 'c.gif')
    S.save_gifs(x, p)
    rgb, planes, loops = read_gif(p)
    assert loops == 0 and rgb.shape == (4, 2 * 16, 3 * 12, 3)
    for t in range(4):
        want = S.large_image(x[:, t]).astype(np.int32)
        assert np.abs(rgb[t].astype(np.int32) - want).max() <= 26      # the cube's worst case: 25.5 levels per channel
        assert np.array_equal(planes[t], S.cube_index(want))
    # inputs already on cube levels come back exactly
    y = (rng.integers(0, 6, size=(4, 2, 3, 8, 8)) * 51).astype(np.uint8)
    S.save_gifs(y, p)
    rgb, _, _ = read_gif(p)
    assert all(np.array_equal(rgb[t], S.large_image(y[:, t])) for t in range(2))
    # floats in [0, 1] take large_image's 255.99 * x
    z = rng.random((2, 2, 3, 8, 8), dtype=np.float32)
    S.save_gifs(z, p)
    rgb, _, _ = read_gif(p)
    assert np.abs(rgb[0].astype(np.int32) - S.large_image(z[:, 0]).astype(np.int32)).max() <= 26


def test_write_gif_takes_ready_index_planes(tmp_path):
    """a frame longer than one clear-code run, a size that ends mid-run and mid-sub-block"""
    from graphical_gan_amd.tflib import save_images as S
    rng = np.random.default_rng(2)
    for h, w in ((1, 254), (1, 255), (3, 85), (37, 41), (64, 128)):
        planes = rng.integers(0, 256, size=(2, h, w)).astype(np.uint8)
        p = str(tmp_path / 'p.gif')
        S.write_gif(p, planes, S.grey_palette())
        _, got, _ = read_gif(p)
        assert np.array_equal(got, planes), (h, w)


# ---- 2. cadence ------------------------------------------------------------------------------------------------------------------
def test_eval_settings_of_the_sequence_scripts(monkeypatch):
    from graphical_gan_amd import run
    for k in run.EVAL_KEYS:
        monkeypatch.delenv('GGAN_' + k, raising=False)
    for name in SSGAN:
        S = run.eval_settings(os.path.join(ROOT, 'scripts', name + '.py'))
        assert S['SAMPLE_EVERY'] == 5000 and 'DEV_EVERY' not in S and 'ACCURACY_EVERY' not in S
        assert run.eval_plan(S) == {'SAMPLE_EVERY': 5000}
        src = open(os.path.join(ROOT, 'scripts', name + '.py')).read()
        assert re.search(r'^SETTINGS\.update\(run\.eval_settings\(__file__\)\)', src, re.M), name
    # the image names as they were
    assert run.eval_settings('gan_inference_cifar10') == dict(DEV_EVERY=100, SAMPLE_EVERY=5000, SCRIPT='gan_inference_cifar10')
    assert run.eval_settings('gmgan_inference_mnist.py') == dict(DEV_EVERY=100, SAMPLE_EVERY=5000, ACCURACY_EVERY=5000,
                                                                 SCRIPT='gmgan_inference_mnist')
    monkeypatch.setenv('GGAN_SAMPLE_EVERY', '7')
    monkeypatch.setenv('GGAN_DEV_EVERY', '3')
    for name in SSGAN:
        S = run.eval_settings(name)
        assert S['SAMPLE_EVERY'] == 7 and 'DEV_EVERY' not in S
    assert run.eval_settings('gan_inference_cifar10')['DEV_EVERY'] == 3


# ---- 3. the entry point ----------------------------------------------------------------------------------------------------------
def test_video_sheet_entry_point_is_declared_bound_and_refuses(lib_built):
    from graphical_gan_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'ggan.h')).read()
    assert int(re.search(r'#define GGAN_ABI_VERSION (\d+)', hdr).group(1)) == _lib.ABI_VERSION == 800
    name = 'ggan_video_sheet_u8'
    assert name in _lib.SIGNATURES and re.search(r'\bint %s\(' % name, hdr)
    assert hasattr(C.CDLL(_lib.LIB_PATH), name)
    L = _lib.load()
    fn = L.ggan_video_sheet_u8
    assert len(fn.argtypes) == 17
    p, n = C.c_void_p(64), C.c_void_p(0)
    err = lambda: L.ggan_last_error().decode()
    #          gen data sheet gif  n  rows LEN C  H   W  nh nw il   a    b       d
    assert fn(p, n, n, p, 2, 2, 3, 1, 16, 16, 1, 2, 0, .5, 255.99, 255.99, n) != 0 and 'null output' in err()
    assert fn(p, n, p, n, 2, 2, 3, 1, 16, 16, 1, 2, 0, .5, 255.99, 255.99, n) != 0 and 'null output' in err()
    for c in (0, 2, 4):
        assert fn(p, n, p, p, 2, 2, 3, c, 16, 16, 1, 2, 0, .5, 255.99, 255.99, n) != 0 and 'C must be' in err()
    assert fn(p, n, p, p, 2, 4, 3, 1, 16, 16, 2, 2, 1, .5, 255.99, 255.99, n) != 0 and 'data source' in err()
    assert fn(p, n, p, p, 2, 3, 3, 1, 16, 16, 1, 3, 0, .5, 255.99, 255.99, n) != 0 and 'rows' in err()
    assert fn(p, p, p, p, 2, 2, 3, 1, 16, 16, 1, 2, 1, .5, 255.99, 255.99, n) != 0 and 'rows' in err()       # interleaved: 2n rows
    assert fn(n, n, p, p, 2, 2, 3, 1, 16, 16, 1, 2, 0, .5, 255.99, 255.99, n) != 0                           # no source at all
    assert fn(p, n, p, p, 2, 2, 3, 1, 16, 18, 1, 2, 0, .5, 255.99, 255.99, n) != 0                           # W not a multiple of 4
    assert fn(p, n, p, p, 2, 2, 3, 1, 16, 16, 2, 2, 0, .5, 255.99, 255.99, n) != 0                           # nh * nw != rows
    assert fn(C.c_void_p(68), n, p, p, 2, 2, 3, 1, 16, 16, 1, 2, 0, .5, 255.99, 255.99, n) != 0 and 'misaligned' in err()


def test_sheet_grid_is_large_images_rule():
    from graphical_gan_amd import functional as F
    for n in list(range(1, 130)) + [800, 1550, 3100]:
        rows = int(np.sqrt(n))
        while n % rows:
            rows -= 1
        assert F.sheet_grid(n) == (rows, n // rows), n


# ---- 4. fixed inputs -------------------------------------------------------------------------------------------------------------
def _evaluator(dataset, seed=3, **kw):
    import torch
    from graphical_gan_amd.evaluate import SequenceEvaluator
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    chairs = dataset == 'chairs'
    cfg = SSConfig(batch_size=20, length=3, dim=4, dim_op=16, dim_g=8, dim_l=4, n_c=0 if chairs else 10, channels=3 if chairs else 1,
                   dataset=dataset, op_dyn_mode='res_w' if chairs else 'res', **kw)
    tr = types.SimpleNamespace(model=StateSpaceGAN(cfg), cfg=cfg, device=torch.device('cpu'))
    return SequenceEvaluator(tr, dict(BATCH_SIZE=20, N_VIS=20, SEED=seed)), cfg


@pytest.mark.parametrize('dataset', ['moving_mnist', 'chairs'])
def test_fixed_inputs(dataset):
    np.random.seed(11)
    before = np.random.get_state()
    ev, c = _evaluator(dataset)
    after = np.random.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    assert tuple(ev.pre_fixed_noise.shape) == (20, c.dim_l) and tuple(ev.fixed_noise_g.shape) == (20, c.dim_g)
    assert tuple(ev.dis_g.shape) == (20, c.dim_g) and tuple(ev.dis_y.shape) == (20, c.n_c) and tuple(ev.fixed_y.shape) == (20, c.n_c)
    g = ev.dis_g.numpy()
    assert (g == g[0]).all() and np.abs(g[0]).max() > 0
    if c.n_c:
        assert np.array_equal(ev.dis_y.numpy(), np.eye(10, dtype=np.float32)[np.ones(20, int)])
        assert np.array_equal(ev.fixed_y.numpy(), np.tile(np.eye(10, dtype=np.float32), (2, 1)))
    # the reference's order of draws from the evaluator's seed: pre_fixed_noise, fixed_noise_g, dis_g
    from graphical_gan_amd.evaluate import EVAL_SEED
    rng = np.random.RandomState(3 + EVAL_SEED)
    assert np.array_equal(ev.pre_fixed_noise.numpy(), rng.normal(size=(20, c.dim_l)).astype(np.float32))
    assert np.array_equal(ev.fixed_noise_g.numpy(), rng.normal(size=(20, c.dim_g)).astype(np.float32))
    assert np.array_equal(g[0], rng.normal(size=(1, c.dim_g)).astype(np.float32)[0])
    # the same settings draw the same tensors; another seed does not
    ev2, _ = _evaluator(dataset)
    for k in ('pre_fixed_noise', 'fixed_noise_g', 'dis_g', 'dis_y', 'fixed_y'):
        assert np.array_equal(getattr(ev, k).numpy(), getattr(ev2, k).numpy()), k
    ev3, _ = _evaluator(dataset, seed=4)
    assert not np.array_equal(ev.dis_g.numpy(), ev3.dis_g.numpy())
    assert ev.feed['rng_state'].tolist() == ev2.feed['rng_state'].tolist() != ev3.feed['rng_state'].tolist()


def test_n_vis_must_fit_the_classes():
    import torch
    from graphical_gan_amd.evaluate import SequenceEvaluator
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    cfg = SSConfig(batch_size=6, length=3, dim=4, dim_op=16, dim_g=8, dim_l=4)
    tr = types.SimpleNamespace(model=StateSpaceGAN(cfg), cfg=cfg, device=torch.device('cpu'))
    with pytest.raises(AssertionError):          # N_VIS % N_C (ssgan_inference_moving_mnist.py:56)
        SequenceEvaluator(tr, dict(BATCH_SIZE=6, N_VIS=6))


def test_eval_sets_learns_the_sequence_datasets_and_single_stream():
    from graphical_gan_amd import run
    from graphical_gan_amd.models_ssgan import SSConfig, StateSpaceGAN
    for script in SSGAN:
        S = run.reference_block(script, BATCH_SIZE=10, LEN=3, DIM=4, SYNTHETIC='force')
        m = StateSpaceGAN(run.config(S))
        np.random.seed(2)
        st = np.random.get_state()
        dev, test = run.eval_sets(S, m, 'cpu')
        assert np.array_equal(st[1], np.random.get_state()[1])
        assert test is None and tuple(dev[0][0].shape) == (10, 3, m.cfg.output_dim)
    m.fork_now = True
    with m.single_stream():
        assert m.fork_now is False
    assert m.fork_now is True


def test_host_sheet_pixel_maps():
    """the host statement of the kernel's arithmetic on the values the issue names: -1, 1 and k / 255.99 boundaries"""
    from graphical_gan_amd import evaluate as E
    assert E.pixel_maps('moving_mnist') == (0.5, 255.99, 255.99) and E.pixel_maps('chairs') == (255.99 / 2, 1.0, 1.0)
    x = np.array([-1.0, 1.0, 0.0, np.nextafter(np.float32(1), np.float32(0)), -0.5], np.float32)
    g = np.zeros((1, 1, 1, 4, 8), np.float32)
    g.reshape(-1)[:5] = x
    sheet, planes = E.host_sheet(g.reshape(1, 1, -1), None, (1, 4, 8), E.pixel_maps('moving_mnist'))
    assert list(sheet.reshape(-1)[:5]) == [0, 255, 127, 255, 63] and sheet.shape == (4, 8, 1) and planes.shape == (1, 4, 8)
    sheet, _ = E.host_sheet(g.reshape(1, 1, -1), None, (1, 4, 8), E.pixel_maps('chairs'))
    assert list(sheet.reshape(-1)[:5]) == [0, 255, 127, 255, 63]
