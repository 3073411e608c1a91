"""numpy restatement of what `mil_attr_mosaic` writes (include/mil_hip.h), for tests/test_cpu_attr_mosaic.py and
tests/test_gpu_attr_mosaic.py.  Written from the stated arithmetic, not from the kernel: plain loops over windows and owned
pixels, int64 sums.

Window t owns the n x n block whose top-left output pixel is out_pos[t]; for owned pixel (a, b) and channel c
  wy[k] = max(0, min((a+1)*Hm, (k+1)*n) - max(a*Hm, k*n))     wx[l] likewise with b and Wm
  v[c]  = (sum_k sum_l wy[k]*wx[l]*maps[t,k,l,c] + Hm*Wm//2) // (Hm*Wm)
  src   = lut[v] (one channel) or v (three);   heat = src
  a     = alpha, or (alpha*v + 127) // 255 with alpha_by_value
  on_tissue = (((tmp >> 8) + tmp) >> 8) >> 6,  tmp = 64*(src*a + dst*(255 - a)) + (0x80 << 6)
Pixels outside the canvas are dropped, every other pixel of a canvas keeps its value."""
import numpy as np


def weights(i, size, n):
    """int64 [size]: the overlap of output pixel i's footprint [i*size, (i+1)*size) with each map pixel's [k*n, (k+1)*n)."""
    k = np.arange(size, dtype=np.int64)
    return np.maximum(0, np.minimum((i + 1) * size, (k + 1) * n) - np.maximum(i * size, k * n))


def resample(m, n):
    """One map uint8 [Hm,Wm] or [Hm,Wm,C] to the n x n block, int64 [n,n] or [n,n,C]."""
    m = np.asarray(m).astype(np.int64)
    hm, wm = m.shape[:2]
    out = np.zeros((n, n) + m.shape[2:], dtype=np.int64)
    for a in range(n):
        wy = weights(a, hm, n)
        assert wy.sum() == hm
        for b in range(n):
            wx = weights(b, wm, n)
            total = 0
            for k in np.nonzero(wy)[0]:
                for l in np.nonzero(wx)[0]:
                    total = total + wy[k] * wx[l] * m[k, l]
            out[a, b] = (total + (hm * wm) // 2) // (hm * wm)
    return out


def composite(src, dst, a):
    """Pillow's alpha_composite of src with alpha a over the opaque dst (int64 arrays or scalars)."""
    tmp = 64 * (src * a + dst * (255 - a)) + (0x80 << 6)
    return (((tmp >> 8) + tmp) >> 8) >> 6


def render(heat, on_tissue, maps, out_pos, n, lut, alpha, alpha_by_value=False, values=None):
    """Fills the caller's canvases IN PLACE (uint8 [Ht,Wt,3] numpy arrays, either may be None) and returns them.  maps: uint8
    [T,Hm,Wm] (lut: uint8 [256,3]) or [T,Hm,Wm,3] (lut unused); out_pos: int [T,2].  values: `[resample(m, n) for m in maps]`
    where a caller renders the same maps more than once."""
    maps = np.asarray(maps)
    canvas = heat if heat is not None else on_tissue
    ht, wt = canvas.shape[:2]
    for t in range(len(maps)):
        v = resample(maps[t], n) if values is None else values[t]
        oy0, ox0 = (int(x) for x in out_pos[t])
        for a in range(n):
            for b in range(n):
                oy, ox = oy0 + a, ox0 + b
                if not (0 <= oy < ht and 0 <= ox < wt):
                    continue
                if maps.ndim == 3:
                    val = int(v[a, b])
                    src = np.asarray(lut)[val].astype(np.int64)
                    al = (alpha * val + 127) // 255 if alpha_by_value else alpha
                else:
                    src, al = v[a, b], alpha
                if heat is not None:
                    heat[oy, ox] = src
                if on_tissue is not None:
                    on_tissue[oy, ox] = composite(src, on_tissue[oy, ox].astype(np.int64), al)
    return heat, on_tissue
