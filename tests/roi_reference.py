"""Host restatement (numpy) of what the reference's tissue-selection loop computes per window (RoiBuilder.py:156-169), for
the tests of `mil_amd.RoiSelector` / `mil_roi_stats`.  Nothing here imports Pillow: tests/test_cpu_roi_select.py compares every
piece with Pillow itself where it is installed, and the fixtures under tests/golden/ (make_roi_golden.py) come from Pillow.

  * `rgb2hsv_float`: Pillow's `rgb2hsv_row` (libImaging/Convert.c) with its number formats — float32 rc / gc / bc / h / s, the
    double expressions `h / 6.0 + 1.0`, `fmod(.., 1.0)`, `(int)(h * 255.0)`;
  * `hue_above`: the integer predicate the kernel uses for `h > hue_min`;
  * `window_stats`: the four integers `mil_roi_stats` returns for one window;
  * `imagestat_stddev` / `keep`: the statements of `ImageStat.Stat` (`sum`, `sum2`, `var`, `stddev`) and the reference's tests;
  * `sliding_window`, `select`: the reference's raster and its loop body over a slide.
"""
import math

import numpy as np

HUE_MIN, V_MIN, V_MAX, MIN_PASS, MIN_STDDEV = 120, 50, 210, 1000, 5


def rgb2hsv_float(rgb):
    """uint8 [...,3] RGB -> uint8 [...,3] HSV as `Image.convert('HSV')` computes it."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32 = np.float32
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    s = cr / np.where(grey, 1, maxc).astype(f32)
    rc, gc, bc = (maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr
    h = np.where(r == maxc, bc - gc,                                                           # float - float: float32
                 np.where(g == maxc, (2.0 + rc.astype(np.float64) - bc).astype(f32),             # 2.0 + float - float: double, stored as float
                          (4.0 + gc.astype(np.float64) - rc).astype(f32))).astype(f32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def hue_above(rgb, hue_min=HUE_MIN):
    """bool [...]: `h > hue_min` of Pillow's HSV, in integers (exact for hue_min = 120 on all 2^24 colours)."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    d = mx - mn
    num = np.where(r == mx, g - b, np.where(g == mx, 2 * d + (b - r), 4 * d + (r - g)))
    num = np.where(num < 0, num + 6 * d, num)
    return (d > 0) & (255 * num >= (hue_min + 1) * 6 * d)


def passes(rgb, hue_min=HUE_MIN, v_min=V_MIN, v_max=V_MAX):
    """bool [...]: the pixels RoiBuilder.py:163-165 keep (h > 120, v > 50, v < 210)."""
    v = np.asarray(rgb, dtype=np.uint8).max(axis=-1).astype(np.int64)
    return hue_above(rgb, hue_min) & (v > v_min) & (v < v_max)


def window_stats(win, hue_min=HUE_MIN, v_min=V_MIN, v_max=V_MAX):
    """int64 [4] of one uint8 [S,S,3] window: sum R, sum R^2, number of passing pixels, pixel count."""
    red = win[..., 0].astype(np.int64)
    return np.array([red.sum(), (red * red).sum(), passes(win, hue_min, v_min, v_max).sum(), red.size], dtype=np.int64)


def slide_stats(slide, coords, size, **kw):
    return np.stack([window_stats(slide[r:r + size, c:c + size], **kw) for r, c in coords]) if len(coords) else np.zeros((0, 4), np.int64)


def imagestat_stddev(sum_r, sum_r2, n):
    """`ImageStat.Stat(img).stddev[0]` from the integers: its `sum` and `sum2` are Python floats, `count` an int."""
    sum_, sum2 = float(sum_r), float(sum_r2)
    var = (sum2 - (sum_ ** 2.0) / n) / n
    return math.sqrt(var)


def keep(stats):
    """RoiBuilder.py:159 and :167 on one window's four integers."""
    s1, s2, n_pass, n = (int(v) for v in stats)
    return imagestat_stddev(s1, s2, n) > MIN_STDDEV and n_pass > MIN_PASS


def sliding_window(dimensions, step, padding=0):
    """RoiBuilder.py:104-114: (row, col) pairs, the column in the outer loop."""
    rows = range(padding, dimensions[0] - step - padding - 1, step)
    cols = range(padding, dimensions[1] - step - padding - 1, step)
    return [(row, col) for col in cols for row in rows]


def select(slide, size, padding=0):
    """The loop body of RoiBuilder.build() (:156-169) over a uint8 [H,W,3] slide: (list of kept windows, list of kept coords)."""
    data, coords = [], []
    for rc in sliding_window(slide.shape, size, padding):
        win = slide[rc[0]:rc[0] + size, rc[1]:rc[1] + size, :]
        if keep(window_stats(win)):
            data.append(win)
            coords.append(rc)
    return data, coords


def all_colours_image():
    """uint8 [4096,4096,3]: pixel v = y * 4096 + x has R = v & 255, G = (v >> 8) & 255, B = v >> 16 (every colour once)."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    return np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)
