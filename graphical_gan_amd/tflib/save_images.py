"""Sample / reconstruction grid dump with the interface of tflib/save_images.py:53-87 (`save_images(X, save_path, size=None)`;
`large_image` returns the grid array).  Floats in [0,1] are mapped with 255.99*x as in the reference; the grid is nh x nw with
nh the largest divisor of the sample count not above its square root; [B,C,H,W], [B,H,W] and flattened [B,H*W] inputs.
The PNG is written with zlib directly (no scipy.misc / imageio in this image).

`save_gifs(x, save_path, size=None)` (tflib/save_images.py:47-51): x [num, LEN, C, H, W] -> an animated GIF of LEN frames, frame t =
large_image(x[:, t], size).  There is no imageio / PIL here either: `write_gif` writes GIF89a itself, looping (NETSCAPE2.0), 10 frames
per second (imageio's default), one global palette: the 256 greys for C = 1 (exact) or the 6x6x6 colour cube for C = 3 -- index
36 r6 + 6 g6 + b6 with r6 = (5 r + 127) / 255 in integers, level l shown as 51 l, no dither: the worst-case error is 25.5 levels per
channel.  The LZW stream is the "clear code before the table grows" form: every pixel is its own 9-bit code and a clear code goes out
after every 254 of them, so that a decoder's table never reaches the 512th entry and its code width never changes.  Any standard decoder
reads it; it does not compress (9/8 byte per pixel plus 1/255 for the sub-block lengths), which is what makes it a handful of numpy calls
instead of a per-pixel dictionary walk in Python.  At full size: moving-MNIST `samples` (16 frames of 320 x 640) 3.7 MB, chairs
`reconstruction` (31 frames of 640 x 640) 14.4 MB; the eight files of a firing take 0.13 s (moving-MNIST) / 0.26 s (chairs) of GIF
writing beside 0.38 / 2.1 s of zlib for the PNGs (docs/KERNELS.md).
`write_png` / `write_gif` take ready sheets / index planes (what ggan_video_sheet_u8 produces on the device) without re-tiling."""
import struct
import zlib

import numpy as np


def large_image(X, size=None):
    X = np.asarray(X)
    if np.issubdtype(X.dtype, np.floating):
        X = (255.99 * X).astype('uint8')
    n_samples = X.shape[0]
    if size is None:
        rows = int(np.sqrt(n_samples))
        while n_samples % rows != 0:
            rows -= 1
        nh, nw = rows, n_samples // rows
    else:
        nh, nw = size
        assert nh * nw == n_samples
    if X.ndim == 2:
        s = int(np.sqrt(X.shape[1]))
        X = X.reshape(X.shape[0], s, s)
    if X.ndim == 4:
        X = X.transpose(0, 2, 3, 1)          # BCHW -> BHWC
        h, w = X[0].shape[:2]
        img = np.zeros((h * nh, w * nw, X.shape[3]), dtype='uint8')
    elif X.ndim == 3:
        h, w = X[0].shape[:2]
        img = np.zeros((h * nh, w * nw), dtype='uint8')
    else:
        raise ValueError('unsupported sample array shape %r' % (X.shape,))
    for n, x in enumerate(X):
        j, i = n // nw, n % nw
        img[j * h:j * h + h, i * w:i * w + w] = x
    return img


def write_png(path, img):
    """8-bit greyscale [H,W] / [H,W,1] or RGB [H,W,3]"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    h, w = img.shape[:2]
    ctype = 0 if img.ndim == 2 else 2
    raw = b''.join(b'\x00' + img[r].tobytes() for r in range(h))

    def chunk(tag, data):
        c = struct.pack('>I', len(data)) + tag + data
        return c + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)

    with open(path, 'wb') as f:
        f.write(b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, ctype, 0, 0, 0)) +
                chunk(b'IDAT', zlib.compress(raw, 6)) + chunk(b'IEND', b''))


def save_images(X, save_path, size=None):
    write_png(save_path, large_image(X, size))


def cube_index(img):
    """RGB bytes [..., 3] -> the index into cube_palette(): 36 r6 + 6 g6 + b6, c6 = (5 c + 127) / 255 (the nearest of the levels 51 l)"""
    l6 = (5 * np.asarray(img).astype(np.int32) + 127) // 255
    return (36 * l6[..., 0] + 6 * l6[..., 1] + l6[..., 2]).astype(np.uint8)


def grey_palette():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def cube_palette():
    """256 RGB entries: the 216 colours of the 6x6x6 cube (levels 0, 51, .., 255) in index order, the rest black"""
    pal = np.zeros((256, 3), dtype=np.uint8)
    i = np.arange(216)
    pal[:216] = np.stack([i // 36, (i // 6) % 6, i % 6], 1) * 51
    return pal


_LZW_RUN = 254      # pixel codes between clear codes: the decoder's table stops at entry 511, the codes stay 9 bits wide


def _lzw_frame(idx):
    """palette indices [h, w] -> the frame's LZW bytes (minimum code size 8), packed into sub-blocks with the terminator"""
    px = np.ascontiguousarray(idx, dtype=np.uint8).reshape(-1).astype(np.uint16)
    n = px.size
    runs = -(-n // _LZW_RUN)
    codes = np.full((runs, _LZW_RUN + 1), 0xFFFF, dtype=np.uint16)     # 0xFFFF: the unused tail of the last run
    codes[:, 0] = 256                                                  # clear
    body = np.full(runs * _LZW_RUN, 0xFFFF, dtype=np.uint16)
    body[:n] = px
    codes[:, 1:] = body.reshape(runs, _LZW_RUN)
    codes = codes.reshape(-1)
    codes = np.concatenate([codes[codes != 0xFFFF], np.array([257], dtype=np.uint16)])      # .. end of information
    bits = ((codes[:, None] >> np.arange(9, dtype=np.uint16)) & 1).astype(np.uint8).reshape(-1)
    data = np.packbits(bits, bitorder='little')
    full = data.size // 255
    out = np.empty((full, 256), dtype=np.uint8)
    out[:, 0] = 255
    out[:, 1:] = data[:full * 255].reshape(full, 255)
    tail = data[full * 255:]
    return out.tobytes() + (bytes([tail.size]) + tail.tobytes() if tail.size else b'') + b'\x00'


def write_gif(path, planes, palette, delay_cs=10):
    """planes: uint8 palette indices [LEN, h, w]; palette: uint8 [256, 3].  GIF89a, one global colour table, looping for ever."""
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    assert planes.ndim == 3 and tuple(np.shape(palette)) == (256, 3), (planes.shape, np.shape(palette))
    n, h, w = planes.shape
    assert 0 < h < 65536 and 0 < w < 65536
    with open(path, 'wb') as f:
        f.write(b'GIF89a' + struct.pack('<HHBBB', w, h, 0xF7, 0, 0) + np.ascontiguousarray(palette, dtype=np.uint8).tobytes())
        f.write(b'\x21\xFF\x0BNETSCAPE2.0\x03\x01' + struct.pack('<H', 0) + b'\x00')
        for t in range(n):
            f.write(b'\x21\xF9\x04' + struct.pack('<BHB', 0, delay_cs, 0) + b'\x00')
            f.write(b'\x2C' + struct.pack('<HHHHB', 0, 0, w, h, 0) + b'\x08')
            f.write(_lzw_frame(planes[t]))
        f.write(b'\x3B')


def gif_planes(x, size=None):
    """x [num, LEN, C, H, W] (floats in [0, 1] or bytes) -> (palette indices [LEN, nh*H, nw*W], palette)"""
    x = np.asarray(x)
    assert x.ndim == 5 and x.shape[2] in (1, 3), x.shape
    frames = [large_image(x[:, t], size) for t in range(x.shape[1])]
    if x.shape[2] == 1:
        return np.stack([f[:, :, 0] for f in frames]), grey_palette()
    return np.stack([cube_index(f) for f in frames]), cube_palette()


def save_gifs(x, save_path, size=None):
    write_gif(save_path, *gif_planes(x, size))
