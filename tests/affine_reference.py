"""numpy restatement of the affine transform's byte contract (mil_affine_u8): Pillow's
`Image.transform(size, Image.AFFINE, m, Image.BILINEAR, fillcolor=fill)` on uint8 images, every channel separately, in IEEE
double with one rounded operation at a time (numpy fuses nothing), and of the two matrix helpers (`mil_amd.affine_matrix`:
torchvision's `_get_inverse_affine_matrix`; `mil_amd.quarter_turn_matrix`).  tests/test_cpu_affine.py pins it to Pillow itself
and to Pillow's recorded bytes; the GPU tests compare the kernel with it."""
import math

import numpy as np


def transform(src, m, out_hw=None, fill=0):
    """src uint8 [H,W,C] (or [H,W]), m six doubles (output -> input), out_hw = (oh, ow) (default: the source's), fill a byte or
    C bytes.  Returns uint8 [oh,ow,C] (or [oh,ow])."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    flat = src.ndim == 2
    p = src[..., None] if flat else src
    H, W, C = p.shape
    oh, ow = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    a0, a1, a2, a3, a4, a5 = (np.float64(v) for v in m)
    xs = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    ys = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        xin = (a0 * xs + a1 * ys) + a2
        yin = (a3 * xs + a4 * ys) + a5
        inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5), np.where(inside, yin, 0.5)
    xf, yf = xin - 0.5, yin - 0.5
    fx, fy = np.floor(xf), np.floor(yf)
    dx, dy = (xf - fx)[..., None], (yf - fy)[..., None]
    X, Y = fx.astype(np.int64), fy.astype(np.int64)
    x0, x1, y0 = np.clip(X, 0, W - 1), np.clip(X + 1, 0, W - 1), np.clip(Y, 0, H - 1)
    below = Y + 1 < H                                                   # Y >= -1: Y + 1 >= 0 always
    y1 = np.where(below, Y + 1, y0)
    pd = p.astype(np.float64)
    v1 = pd[y0, x0] + (pd[y0, x1] - pd[y0, x0]) * dx
    v2 = pd[y1, x0] + (pd[y1, x1] - pd[y1, x0]) * dx
    v2 = np.where(below[..., None], v2, v1)
    out = np.trunc(v1 + (v2 - v1) * dy).astype(np.uint8)
    f = np.broadcast_to(np.asarray(fill, dtype=np.uint8), (C,))
    out = np.where(inside[..., None], out, f[None, None, :])
    return out[..., 0] if flat else out


def transform_planar(tiles, matrices, out_hw=None, fill=0):
    """uint8 [n,3,h,w] with one matrix per tile -> uint8 [n,3,oh,ow]."""
    return np.stack([np.moveaxis(transform(np.moveaxis(t, 0, -1), m, out_hw, fill), -1, 0) for t, m in zip(tiles, matrices)]) \
        if len(tiles) else np.empty((0, 3) + tuple(out_hw if out_hw is not None else tiles.shape[2:]), np.uint8)


def slide_windows(slide, coords, matrices, size, fill=0):
    """The windows of `size` pixels at coords (row, col) of the slide [H,W,3], each transformed with its matrix in WINDOW
    coordinates while reading the whole slide: the origin is added to a2 (col) and a5 (row), one double addition each."""
    out = np.empty((len(coords), size, size, 3), np.uint8)
    for i, ((r, c), m) in enumerate(zip(coords, matrices)):
        mm = [np.float64(v) for v in m]
        mm[2] = mm[2] + np.float64(c)
        mm[5] = mm[5] + np.float64(r)
        out[i] = transform(slide, mm, (size, size), fill)
    return out


def affine_matrix(center, angle, translate, scale, shear):
    """torchvision's `_get_inverse_affine_matrix`, statement by statement."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def quarter_turn_matrix(k, size):
    """Derived from np.rot90: with N = size, rot90(img, 1)[i, j] = img[j, N-1-i], so output pixel (x, y) = (j, i) reads input
    (N-1-y, x): xin = N - (y + 0.5), yin = x + 0.5; the others by composing that map with itself."""
    n = float(size)
    return {0: [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 1: [0.0, -1.0, n, 1.0, 0.0, 0.0], 2: [-1.0, 0.0, n, 0.0, -1.0, n],
            3: [0.0, 1.0, 0.0, -1.0, 0.0, n]}[k % 4]
