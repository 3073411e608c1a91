"""Host restatement (numpy) of torchvision's ColorJitter on uint8 RGB images as its PIL backend computes it, for the tests of
`mil_amd.ColorJitter` / `mil_color_jitter_u8` (RoiBuilder.py:200).  Nothing here imports Pillow: tests/test_cpu_color_jitter.py
compares every piece with Pillow itself where it is installed, and tests/golden/jitter_chain.npz (make_jitter_golden.py) holds
Pillow's own bytes.

  * `blend`: `Image.blend(degenerate, image, factor)` (libImaging/Blend.c) — float32, a rounded multiply then a rounded add;
  * `grey`: `convert("L")`;
  * `contrast_mean`: `int(ImageStat.Stat(img.convert("L")).mean[0] + 0.5)` in integers;
  * `brightness` / `contrast` / `saturation`: `ImageEnhance.Brightness` / `.Contrast` / `.Color`;
  * `hsv2rgb`: Pillow's `hsv2rgb` (libImaging/Convert.c); `hue`: `adjust_hue` = HSV, h + shift mod 256, RGB;
  * `hue_shift`: the shift `adjust_hue` adds for a hue factor;
  * `jitter_batch` / `jitter_tile` / `jitter_tiles`: the chain on planar tiles in a given order.

Images are uint8 [...,3]; tiles are uint8 [3,R,R] planar, as `U8Tiles` holds them.
"""
import numpy as np

from roi_reference import rgb2hsv_float

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


def blend(d, x, a):
    """uint8 of `d + a * (x - d)` as ImagingBlend computes it: d, x integer arrays in 0..255, a the factor as float32."""
    a = np.float32(a)
    d, x = np.asarray(d).astype(np.int32), np.asarray(x).astype(np.int32)
    t = d.astype(np.float32) + a * (x - d).astype(np.float32)
    assert t.dtype == np.float32
    if 0.0 <= a <= 1.0:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def grey(rgb):
    rgb = np.asarray(rgb).astype(np.int64)
    return ((19595 * rgb[..., 0] + 38470 * rgb[..., 1] + 7471 * rgb[..., 2] + 0x8000) >> 16).astype(np.uint8)


def contrast_mean(rgb):
    lum = grey(rgb).astype(np.int64)
    n = lum.size
    return int((2 * int(lum.sum()) + n) // (2 * n))


def brightness(rgb, f):
    return blend(np.zeros_like(rgb), rgb, f)


def contrast(rgb, f):
    return blend(np.full_like(rgb, contrast_mean(rgb)), rgb, f)


def saturation(rgb, f):
    return blend(np.broadcast_to(grey(rgb)[..., None], np.shape(rgb)), rgb, f)


def hsv2rgb(hsv):
    """uint8 [...,3] HSV -> uint8 [...,3] RGB as `Image.convert('RGB')` of an HSV image computes it."""
    hsv = np.asarray(hsv, dtype=np.uint8)
    h, s, v = hsv[..., 0].astype(np.intp), hsv[..., 1].astype(np.intp), hsv[..., 2]
    # what depends on h and s alone, for their 256 values each (the same double expressions, evaluated once per value)
    hh = np.arange(256, dtype=np.float64) * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i).astype(np.float32).astype(np.float64)                               # [h]
    fs = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32).astype(np.float64)      # [s]
    one_p = 1.0 - fs                                                                 # [s]
    one_q = 1.0 - fs[None, :] * f[:, None]                                           # [h,s]
    one_t = 1.0 - fs[None, :] * (1.0 - f)[:, None]
    k = (i.astype(np.int64) % 6)[h]                                                  # h = 255: i = 6 -> case 0, f = 0

    def rnd(x):                                  # C's round(): half away from zero (all values here are >= 0)
        fl = np.floor(x)
        return np.clip(fl + (x - fl >= 0.5), 0, 255).astype(np.uint8)

    dv = v.astype(np.float64)
    p, q, t = rnd(dv * one_p[s]), rnd(dv * one_q[h, s]), rnd(dv * one_t[h, s])
    r = np.choose(k, [v, q, p, p, t, v])
    g = np.choose(k, [t, v, v, q, p, p])
    b = np.choose(k, [p, p, t, v, v, q])
    grey_px = hsv[..., 1] == 0
    return np.stack([np.where(grey_px, v, r), np.where(grey_px, v, g), np.where(grey_px, v, b)], axis=-1)


def hue_shift(hue_factor):
    """What `adjust_hue` adds to h: int(hue_factor * 255), truncated toward zero, mod 256 (-0.02 -> 251)."""
    return int(float(hue_factor) * 255) % 256


def hue(rgb, shift):
    hsv = rgb2hsv_float(rgb).copy()
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + int(shift)) % 256).astype(np.uint8)
    return hsv2rgb(hsv)


def contrast_batch(imgs, f):
    """`contrast` on every image of a uint8 [N,H,W,3] batch, each with its own mean."""
    lum = grey(imgs).astype(np.int64)
    n = lum.shape[1] * lum.shape[2]
    m = (2 * lum.sum(axis=(1, 2)) + n) // (2 * n)
    return blend(np.broadcast_to(m[:, None, None, None], imgs.shape), imgs, f)


def jitter_batch(tiles, order, factors, shift):
    """Planar uint8 [N,3,R,R] tiles, ALL through the ops of one `order` (codes 0..3, -1 = skip) with one set of factors (fb, fc,
    fs) and one hue shift, as ColorJitter.forward applies `fn_idx`; contrast takes each tile's own mean."""
    img = np.ascontiguousarray(np.moveaxis(np.asarray(tiles, dtype=np.uint8), 1, -1))
    for op in order:
        if op == BRIGHTNESS:
            img = brightness(img, factors[0])
        elif op == CONTRAST:
            img = contrast_batch(img, factors[1])
        elif op == SATURATION:
            img = saturation(img, factors[2])
        elif op == HUE:
            img = hue(img, shift)
        else:
            assert op == -1, op
    return np.ascontiguousarray(np.moveaxis(img, -1, 1))


def jitter_tile(tile, order, factors, shift):
    """One planar uint8 [3,R,R] tile."""
    return jitter_batch(np.asarray(tile)[None], order, factors, shift)[0]


def jitter_tiles(tiles, order, factors, shifts):
    """Planar uint8 [T,3,R,R] tiles, each with its own row of parameters."""
    return np.stack([jitter_tile(t, o, f, s) for t, o, f, s in zip(tiles, order, factors, shifts)]) if len(tiles) \
        else np.zeros_like(tiles)
