"""numpy restatement of what `mil_heatmap_render` writes (include/mil_hip.h), for tests/test_gpu_heatmap.py.  Written from
the stated arithmetic, not from the kernel: int64 sums, one gather of all windows, one scatter per panel.

With n = S // D window t owns the n x n block at output pixel (row // D, col // D) in each of the five panels:
  box mean   m[c] = (sum over [aD,(a+1)D) x [bD,(b+1)D) + D*D//2) // (D*D)
  panel 0    m where jet_idx[0,t] < 0, else (m*(256-q0) + jet[i]*q0 + 128) >> 8
  panel 1    viridis[feat_idx[t, ((a-g)*8//(n-2g))*10 + (b-g)*10//(n-2g)]] for g <= a,b < n-g, g = inset // D (0 when n-2g < 1)
  panel 1+k  (255*(256-q1) + jet[i]*q1 + 128) >> 8 where i = jet_idx[k,t] >= 0
Every other pixel of the canvas keeps its value."""
import numpy as np


def box_mean(windows, D):
    """windows: uint8 [T,S,S,3] -> int64 [T,n,n,3]."""
    T, S = windows.shape[:2]
    n = S // D
    sums = windows.astype(np.int64).reshape(T, n, D, n, D, 3).sum(axis=(2, 4))
    return (sums + (D * D) // 2) // (D * D)


def render(canvas, slide, coords, S, D, jet_idx, feat_idx, jet, viridis, inset=16, q0=77, q1=230):
    """canvas: uint8 [5,Ht,Wt,3] (not modified); slide: uint8 [H,W,3]; coords: int [T,2] of (row, col); jet_idx: int [4,T];
    feat_idx: uint8 [T,80] or None; jet [105,3], viridis [256,3] uint8.  Returns the rendered copy of canvas."""
    out = np.array(canvas, copy=True)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 2)
    T = len(coords)
    if T == 0:
        return out
    assert S % D == 0
    n = S // D
    jet_idx = np.asarray(jet_idx, dtype=np.int64)
    jet, viridis = np.asarray(jet, dtype=np.int64), np.asarray(viridis, dtype=np.int64)
    span = np.arange(S)
    yy = coords[:, 0, None, None] + span[None, :, None]
    xx = coords[:, 1, None, None] + span[None, None, :]
    m = box_mean(slide[yy, xx], D)                                                   # [T,n,n,3]
    blk = np.arange(n)
    oy = (coords[:, 0] // D)[:, None, None] + blk[None, :, None]                     # [T,n,1]
    ox = (coords[:, 1] // D)[:, None, None] + blk[None, None, :]                     # [T,1,n]
    oy, ox = np.broadcast_to(oy, (T, n, n)), np.broadcast_to(ox, (T, n, n))

    i0 = jet_idx[0]
    blend = (m * (256 - q0) + jet[np.maximum(i0, 0)][:, None, None, :] * q0 + 128) >> 8
    out[0, oy, ox] = np.where((i0 < 0)[:, None, None, None], m, blend)
    for k in (1, 2, 3):
        ik = jet_idx[k]
        drawn = ik >= 0
        colour = (255 * (256 - q1) + jet[np.maximum(ik, 0)] * q1 + 128) >> 8         # [T,3]
        out[1 + k, oy[drawn], ox[drawn]] = np.broadcast_to(colour[drawn][:, None, None, :], (int(drawn.sum()), n, n, 3))
    if feat_idx is not None:
        g = inset // D
        if n - 2 * g < 1:
            g = 0
        w = n - 2 * g
        a = np.arange(w)
        cell = (a * 8 // w)[:, None] * 10 + (a * 10 // w)[None, :]                   # [w,w]
        codes = np.asarray(feat_idx)[:, cell]                                        # [T,w,w]
        out[1, oy[:, g:n - g, g:n - g], ox[:, g:n - g, g:n - g]] = viridis[codes]
    return out
