"""The arithmetic of `mil_map_quantile`, `mil_attr_render` and `mil_cam_overlay` restated in numpy,
operation by operation, so that any numpy gives the same bits.  Shared by tests/test_cpu_attr_render.py (held to
np.percentile, Pillow's and matplotlib's recorded tables) and tests/test_gpu_attr_render.py (the device is held to this)."""
import numpy as np

F32, F64 = np.float32, np.float64


def gray_of(x):
    """The ranked values of one group member: (|g0| + |g1|) + |g2| of a [3,...] gradient in fp32, a map as it is."""
    x = np.asarray(x, F32)
    return (np.abs(x[0]) + np.abs(x[1])) + np.abs(x[2])


def values_of(x, group="tile", raw=False):
    """[G, N] fp32: the values of every group of a gradient [T,3,H,W] (grayscale, or with raw every element) or a map [T,H,W]."""
    x = np.asarray(x, F32)
    if x.ndim == 4 and not raw:
        v = np.stack([gray_of(g) for g in x])
    else:
        v = x
    v = v.reshape(x.shape[0], -1)
    return v.reshape(1, -1) if group == "bag" else v


def ranks(n, q):
    """(lo, hi, t) of the q-th percentile of n values: numpy's linear method, vi = (n - 1) * (q / 100) in fp64."""
    qq = F64(q) / F64(100.0)
    vi = F64(n - 1) * qq
    lo = int(np.floor(vi))
    lo = min(lo, n - 1)
    hi = min(lo + 1, n - 1)
    return lo, hi, F64(vi - F64(lo))


def quantile_stats(values, q):
    """(stats [G,4] fp32 = min, max, s[lo], s[hi]; p [G] fp64) of values [G,N].  -0.0 counts as +0.0."""
    values = np.asarray(values, F32) + F32(0.0)
    g, n = values.shape
    lo, hi, t = ranks(n, q)
    stats, p = np.empty((g, 4), F32), np.empty(g, F64)
    for i in range(g):
        s = np.sort(values[i], kind="stable")
        a, b = F64(s[lo]), F64(s[hi])
        d = b - a
        p[i] = a + d * t if t < 0.5 else b - d * (F64(1.0) - t)
        stats[i] = (s[0], s[-1], s[lo], s[hi])
    return stats, p


def _per_tile(a, tiles):
    """Group statistics [G, ...] as one row per tile."""
    return a if a.shape[0] == tiles else np.repeat(a, tiles, axis=0)


def grayscale_bytes(x, q=99.0, group="tile"):
    """uint8 [T,H,W] of a gradient [T,3,H,W] or a map [T,H,W]."""
    x = np.asarray(x, F32)
    stats, p = quantile_stats(values_of(x, group), q)
    t = x.shape[0]
    stats, p = _per_tile(stats, t), _per_tile(p, t)
    out = np.zeros((t,) + x.shape[-2:], np.uint8)
    for i in range(t):
        gray = (gray_of(x[i]) if x.ndim == 4 else x[i]).astype(F64)
        mn = F64(stats[i, 0])
        den = p[i] - mn
        if den == 0:
            continue
        with np.errstate(all="ignore"):
            v = np.clip((gray - mn) / den, 0, 1)
            out[i] = np.nan_to_num(F64(255.0) * v, nan=0.0).astype(np.uint8)
    return out


def _hwc(a):
    return np.ascontiguousarray(a.transpose(1, 2, 0))


def colour_bytes(grad, group="tile"):
    """uint8 [T,H,W,3]: trunc(((g - min) / (max - min)) * 255) in fp32, min and max over the group."""
    grad = np.asarray(grad, F32)
    t = grad.shape[0]
    stats = _per_tile(quantile_stats(values_of(grad, group, raw=True), 100.0)[0], t)
    out = np.zeros((t,) + grad.shape[2:] + (3,), np.uint8)
    for i in range(t):
        mn, mx = stats[i, 0], stats[i, 1]
        span = F32(mx - mn)
        if span == 0:
            continue
        out[i] = _hwc((((grad[i] - mn) / span) * F32(255.0)).astype(np.uint8))
    return out


def pos_neg_bytes(grad, group="tile"):
    """(positive, negative) uint8 [T,H,W,3]: trunc((max(0, g) / max) * 255) and trunc((max(0, -g) / -min) * 255) in fp32."""
    grad = np.asarray(grad, F32)
    t = grad.shape[0]
    stats = _per_tile(quantile_stats(values_of(grad, group, raw=True), 100.0)[0], t)
    pos = np.zeros((t,) + grad.shape[2:] + (3,), np.uint8)
    neg = np.zeros_like(pos)
    for i in range(t):
        mn, mx = stats[i, 0], stats[i, 1]
        if mx > 0:
            pos[i] = _hwc(((np.maximum(F32(0), grad[i]) / mx) * F32(255.0)).astype(np.uint8))
        if -mn > 0:
            neg[i] = _hwc(((np.maximum(F32(0), -grad[i]) / -mn) * F32(255.0)).astype(np.uint8))
    return pos, neg


def composite(src, dst, alpha_byte):
    """Pillow's alpha_composite of a source with alpha `alpha_byte` over an opaque destination, per channel byte."""
    src, dst, a = np.asarray(src, np.uint32), np.asarray(dst, np.uint32), np.uint32(alpha_byte)
    tmp = np.uint32(64) * (src * a + dst * (np.uint32(255) - a)) + np.uint32(0x80 << 6)
    return ((((tmp >> 8) + tmp) >> 8) >> 6).astype(np.uint8)


def overlay_bytes(tiles_u8, map_u8, lut, alpha_byte):
    """(heat, on_image) uint8 [T,H,W,3] from planar uint8 tiles [T,3,H,W], map bytes [T,H,W] and a [256,3] table."""
    heat = np.asarray(lut, np.uint8)[np.asarray(map_u8)]
    dst = np.asarray(tiles_u8).transpose(0, 2, 3, 1)
    return heat, composite(heat, dst, alpha_byte)
