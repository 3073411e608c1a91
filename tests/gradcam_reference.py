"""numpy restatements of what `mil_grad_cam` computes (include/mil_hip.h), for tests/test_cpu_gradcam.py and
tests/test_gpu_gradcam.py.  Written from `gradcam.py:75-89` of the toolkit the reference vendors and from Pillow's resampling as
its sources state it, not from the kernel.  Pillow is not imported: the resize takes the coefficient tables as arguments
(`mil_resample_coeffs(..., MIL_FILTER_LANCZOS)`), and tests/golden/gradcam_lanczos.npz holds what Pillow itself returned.

  raw_map     fp64: w_k = mean over the pixels of grad[..., k]; raw = max(offset + sum_k w_k act_k, 0); only the c real channels
  raw_gate    the per-pixel forward error bound of the same sums in fp32, in any order
  quantise    fp32, exactly lines 85-87: cam = (cam - min) / (max - min); np.uint8(cam * 255); a constant tile gives zeros
  resize_u8   Pillow's two 8-bit passes: horizontal to uint8, then vertical to uint8, each from 1 << 21 with int32 sums, an
              arithmetic shift by 22 and a clamp; a pass whose sizes are equal is skipped"""
import numpy as np

PRECISION_BITS = 22


def raw_map(act, grad, c, offset):
    """act, grad: [n,h,w,cs] arrays of any float type (the values the kernel reads) -> float64 [n,h,w]."""
    a = np.asarray(act, dtype=np.float64)[..., :c]
    g = np.asarray(grad, dtype=np.float64)[..., :c]
    wk = g.mean(axis=(1, 2))
    return np.maximum(offset + np.einsum("nhwk,nk->nhw", a, wk), 0.0)


def raw_gate(act, grad, c, offset):
    """float64 [n,h,w]: 2 (h w + c + 2) 2^-24 (|offset| + sum_k mean|grad_k| |act_k|).  A sum of m fp32 terms in any order is
    within (m - 1) u of the exact one relative to the sum of magnitudes (u = 2^-24): h w terms and a division for w_k, then c
    products and the offset for the pixel; the factor 2 covers the second-order terms."""
    a = np.abs(np.asarray(act, dtype=np.float64)[..., :c])
    g = np.abs(np.asarray(grad, dtype=np.float64)[..., :c])
    n, h, w, _ = a.shape
    mag = abs(offset) + np.einsum("nhwk,nk->nhw", a, g.mean(axis=(1, 2)))
    return 2.0 * (h * w + c + 2) * 2.0 ** -24 * mag


def quantise(raw, value_range=None):
    """raw: float32 [n,h,w] -> uint8 [n,h,w].  value_range = (lo, hi): one range for every tile, raw clamped into it first."""
    raw = np.asarray(raw)
    assert raw.dtype == np.float32 and raw.ndim == 3
    out = np.zeros(raw.shape, dtype=np.uint8)
    for t, cam in enumerate(raw):
        if value_range is None:
            mn, mx = np.min(cam), np.max(cam)
        else:
            mn, mx = np.float32(value_range[0]), np.float32(value_range[1])
            cam = np.minimum(np.maximum(cam, mn), mx)
        if mx == mn:
            continue
        cam = (cam - mn) / (mx - mn)
        assert cam.dtype == np.float32
        out[t] = np.uint8(cam * 255)
    return out


def _pass(img, bounds, kk):
    """img: uint8 [..., n_in] resampled along its last axis to [..., n_out]."""
    bounds, kk = np.asarray(bounds, dtype=np.int64), np.asarray(kk, dtype=np.int64)
    n_out, ksize = kk.shape
    idx = bounds[:, :1] + np.arange(ksize)[None, :]                              # [n_out, ksize]
    valid = np.arange(ksize)[None, :] < bounds[:, 1:2]
    taps = img.astype(np.int64)[..., np.where(valid, idx, 0)]                       # [..., n_out, ksize]
    ss = (taps * np.where(valid, kk, 0)).sum(-1) + (1 << (PRECISION_BITS - 1))
    assert np.abs(ss).max() < 2 ** 31                                               # Pillow accumulates in int32
    return np.clip(ss >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_u8(q, ytab, xtab, H, W):
    """q: uint8 [n,h,w]; ytab / xtab = (bounds [out,2], kk [out,ksize]) for h -> H and w -> W -> uint8 [n,H,W]."""
    q = np.asarray(q)
    assert q.dtype == np.uint8 and q.ndim == 3
    n, h, w = q.shape
    if w != W:
        q = _pass(q, *xtab)
    if h != H:
        q = np.ascontiguousarray(_pass(q.transpose(0, 2, 1), *ytab).transpose(0, 2, 1))
    assert q.shape == (n, H, W)
    return q
