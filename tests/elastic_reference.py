"""numpy restatement of the elastic deformation's byte contract (mil_affine_elastic_u8): the affine
transform of section 3.50 with one more term in the source coordinate, a uniform cubic B-spline of a per-tile control lattice
evaluated through separable tables.  IEEE double, one rounded operation at a time in the order the contract writes them (numpy
fuses nothing).  It imports nothing of the package; tests/test_cpu_elastic.py pins it to tests/affine_reference.py (zero
lattices), to Pillow's recorded bytes, to scipy and to its own recorded bytes; the GPU tests compare the kernel with it."""
import numpy as np


def tables(size, cells):
    """(idx int32 [size], w float64 [size,4]) of an axis of `size` output pixels divided into `cells` cells: output position x
    reads lattice entries idx[x] .. idx[x] + 3 with the weights w[x]."""
    size, cells = int(size), int(cells)
    assert size >= 1 and cells >= 1
    x = np.arange(size, dtype=np.float64)
    u = ((x + 0.5) * np.float64(cells)) / np.float64(size)
    i = np.minimum(np.floor(u), np.float64(cells - 1))
    t = u - i
    s = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    w0 = ((s * s) * s) / 6.0
    w1 = ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0
    w2 = (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0
    w3 = t3 / 6.0
    return i.astype(np.int32), np.stack([w0, w1, w2, w3], axis=1)


def field(ctrl, out_hw):
    """ctrl float64 [2,gy+3,gx+3] -> (dx, dy), two float64 [oh,ow]: the displacement of every output pixel."""
    c = np.asarray(ctrl, dtype=np.float64)
    assert c.ndim == 3 and c.shape[0] == 2 and c.shape[1] >= 4 and c.shape[2] >= 4
    oh, ow = int(out_hw[0]), int(out_hw[1])
    iy, wy = tables(oh, c.shape[1] - 3)
    ix, wx = tables(ow, c.shape[2] - 3)
    out = []
    for k in range(2):
        r = []
        for i in range(4):
            g = [c[k][(iy + j)[:, None], (ix + i)[None, :]] for j in range(4)]                    # [oh,ow] each
            r.append(((wy[:, 0:1] * g[0] + wy[:, 1:2] * g[1]) + wy[:, 2:3] * g[2]) + wy[:, 3:4] * g[3])
        out.append(((wx[None, :, 0] * r[0] + wx[None, :, 1] * r[1]) + wx[None, :, 2] * r[2]) + wx[None, :, 3] * r[3])
    return out[0], out[1]


def transform(src, m, ctrl, out_hw=None, fill=0):
    """src uint8 [H,W,C] (or [H,W]), m six doubles (output -> input), ctrl float64 [2,gy+3,gx+3] in source pixels, out_hw =
    (oh, ow) (default: the source's), fill a byte or C bytes.  Returns uint8 [oh,ow,C] (or [oh,ow])."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim in (2, 3)
    flat = src.ndim == 2
    p = src[..., None] if flat else src
    H, W, C = p.shape
    oh, ow = (H, W) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    ddx, ddy = field(ctrl, (oh, ow))
    a0, a1, a2, a3, a4, a5 = (np.float64(v) for v in m)
    xs = (np.arange(ow, dtype=np.float64) + 0.5)[None, :]
    ys = (np.arange(oh, dtype=np.float64) + 0.5)[:, None]
    with np.errstate(invalid="ignore", over="ignore"):
        xin = ((a0 * xs + a1 * ys) + a2) + ddx
        yin = ((a3 * xs + a4 * ys) + a5) + ddy
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


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def transform_planar(tiles, matrices, ctrl, out_hw=None, fill=0):
    """uint8 [n,3,h,w] with one matrix (None: the identity) and one lattice per tile -> uint8 [n,3,oh,ow]."""
    if matrices is None:
        matrices = [IDENTITY] * len(tiles)
    if not len(tiles):
        return np.empty((0, 3) + tuple(out_hw if out_hw is not None else tiles.shape[2:]), np.uint8)
    return np.stack([np.moveaxis(transform(np.moveaxis(t, 0, -1), m, c, out_hw, fill), -1, 0) for t, m, c in zip(tiles, matrices, ctrl)])


def transform_interleaved(rois, matrices, ctrl, fill=0):
    """uint8 [n,S,S,3] (the source of a window is the window) -> uint8 [n,S,S,3]."""
    if matrices is None:
        matrices = [IDENTITY] * len(rois)
    return np.stack([transform(r, m, c, None, fill) for r, m, c in zip(rois, matrices, ctrl)]) if len(rois) \
        else np.empty(rois.shape, np.uint8)


def slide_windows(slide, coords, matrices, ctrl, size, fill=0):
    """The windows of `size` pixels at coords (row, col) of the slide [H,W,3], each transformed with its matrix in WINDOW
    coordinates and deformed with its lattice while reading the whole slide: the origin is added to a2 (col) and a5 (row), one
    double addition each, before the displacement is."""
    if matrices is None:
        matrices = [IDENTITY] * len(coords)
    out = np.empty((len(coords), size, size, 3), np.uint8)
    for i, ((r, c), m, cl) in enumerate(zip(coords, matrices, ctrl)):
        mm = [np.float64(v) for v in m]
        mm[2] = mm[2] + np.float64(c)
        mm[5] = mm[5] + np.float64(r)
        out[i] = transform(slide, mm, cl, (size, size), fill)
    return out
