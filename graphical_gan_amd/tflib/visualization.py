"""tflib/visualization.py of the reference (scatter, :10-20: a seaborn lmplot of 2-D points coloured by class), without seaborn, pandas
or matplotlib: the points are rasterised on the host into a uint8 image and written by save_images.write_png.

The look: a white square canvas of SIZE x SIZE pixels over the data's bounding box plus a 5 % margin (one scale for both axes, the
box centred), a thin grey frame, one filled disc per point -- radius from mark_size as a scatter's area `s` in points^2 would give --,
one colour per class: ten distinct colours, a hue wheel beyond ten classes.  Later points are drawn over earlier ones."""
import colorsys
import os

import numpy as np

from .save_images import write_png

SIZE = 720
MARGIN = 0.05
PALETTE = ((31, 119, 180), (255, 127, 14), (44, 160, 44), (214, 39, 40), (148, 103, 189),
           (140, 86, 75), (227, 119, 194), (127, 127, 127), (188, 189, 34), (23, 190, 207))


def class_colours(n):
    """n RGB rows: the fixed ten-colour palette, or n hues around the wheel when there are more than ten classes"""
    if n <= len(PALETTE):
        return np.asarray(PALETTE[:max(n, 1)], np.uint8)
    return np.asarray([[int(round(255 * c)) for c in colorsys.hsv_to_rgb(k / float(n), 0.85, 0.85)] for k in range(n)], np.uint8)


def _radius(mark_size):
    """a marker of area mark_size points^2 (matplotlib's `s`) at 100 dpi: radius in pixels, at least one"""
    return max(1.0, float(np.sqrt(mark_size / np.pi)) * 100.0 / 72.0)


def rasterise(data, label, mark_size=2, n_classes=None, box=None):
    """data [n, 2], integer label [n] -> uint8 image [SIZE, SIZE, 3]; x to the right, y upwards.  box: (xmin, xmax, ymin, ymax) to
    draw in instead of the data's own bounding box."""
    data = np.asarray(data, np.float64).reshape(-1, 2)
    label = np.asarray(label).astype(np.int64).reshape(-1)
    assert len(label) == len(data), (data.shape, label.shape)
    n_classes = int(n_classes if n_classes is not None else (label.max() + 1 if len(label) else 1))
    colours = class_colours(n_classes)
    img = np.full((SIZE, SIZE, 3), 255, np.uint8)
    img[0, :], img[-1, :], img[:, 0], img[:, -1] = 200, 200, 200, 200
    if not len(data):
        return img
    x0, x1, y0, y1 = box if box is not None else (data[:, 0].min(), data[:, 0].max(), data[:, 1].min(), data[:, 1].max())
    span = max(x1 - x0, y1 - y0, 1e-12) * (1.0 + 2.0 * MARGIN)
    cx, cy = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    px = (data[:, 0] - cx) / span * (SIZE - 1) + 0.5 * (SIZE - 1)
    py = 0.5 * (SIZE - 1) - (data[:, 1] - cy) / span * (SIZE - 1)
    r = _radius(mark_size)
    k = int(np.ceil(r))
    ix, iy = np.rint(px).astype(np.int64), np.rint(py).astype(np.int64)
    rgb = colours[label % len(colours)]
    for dy in range(-k, k + 1):
        for dx in range(-k, k + 1):
            if dx * dx + dy * dy > r * r + 0.25:
                continue
            xx, yy = ix + dx, iy + dy
            ok = (xx >= 0) & (xx < SIZE) & (yy >= 0) & (yy < SIZE)
            img[yy[ok], xx[ok]] = rgb[ok]            # (a repeated pixel keeps the last point's colour: numpy assigns in order)
    return img


def scatter(data, label, dir, file_name, mus=None, mark_size=2):
    """the reference's signature: data [n, 2]; label [n] class numbers or one-hot rows [n, classes] (reduced by argmax); writes
    dir/file_name, and the points `mus` [m, 2], one class each, with 20 times the mark area into dir/mus_<file_name>."""
    label = np.asarray(label)
    if label.ndim == 2:
        label = np.argmax(label, axis=1)
    path = os.path.join(dir, file_name)
    write_png(path, rasterise(data, label, mark_size))
    if mus is not None:
        mus = np.asarray(mus)
        write_png(os.path.join(dir, 'mus_' + file_name), rasterise(mus, np.arange(mus.shape[0]), mark_size * 20))
    return path
