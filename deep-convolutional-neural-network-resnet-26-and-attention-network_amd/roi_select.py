"""Device-side tissue selection: the loop of the reference's `RoiBuilder.build()` (RoiBuilder.py:153-169) that cuts a
whole-slide image into `roi_size` windows (`sliding_window`, :104-114) and keeps those that look like tissue —
`ImageStat.Stat(roi).stddev[0] > 5` and more than 1000 pixels with `h > 120`, `50 < v < 210` in `roi.convert('HSV')`.

The slide stays on the GPU: one kernel (csrc/roi_select.hip, `mil_roi_stats`) reads every window once and returns four exact
integers per window (sum R, sum R^2, the number of passing pixels, the pixel count); the decision is taken from them on the
host with the statements Pillow executes, so it is the reference's bit for bit.  The kept windows are what
`TilePreprocessor.__call__` takes.  Reading slide files and the `.npy` caches stay with the caller.
"""
import math

import numpy as np
import torch

from . import _lib as L


class RoiSelector:
    """`roi_size`, `padding`: the reference's `params['roi_size']` / `params['padding']`; the other arguments are the
    constants of RoiBuilder.py:159-167."""

    def __init__(self, roi_size=1200, padding=0, min_stddev=5.0, hue_min=120, v_min=50, v_max=210, min_pass=1000):
        self.roi_size, self.padding = int(roi_size), int(padding)
        if self.roi_size < 1 or self.padding < 0:
            raise ValueError("roi_size must be positive and padding non-negative")
        self.min_stddev, self.min_pass = min_stddev, min_pass
        self.hue_min, self.v_min, self.v_max = int(hue_min), int(v_min), int(v_max)

    def raster(self, shape):
        """`sliding_window(shape, roi_size, padding)` (RoiBuilder.py:104-114) as a list of (row, col): the column is the
        outer loop, and the stop `dim - roi_size - padding - 1` leaves out a window that would end on the last pixel of
        an axis or on the one before it."""
        s, p = self.roi_size, self.padding
        rows, cols = range(p, shape[0] - s - p - 1, s), range(p, shape[1] - s - p - 1, s)
        return [(row, col) for col in cols for row in rows]

    def _windows(self, source, coords):
        """(contiguous source, int64 CPU byte offsets [n], row pitch in bytes, int64 CPU coords [n,2] or None)."""
        if not isinstance(source, torch.Tensor) or source.dtype != torch.uint8:
            raise ValueError(f"expected a uint8 tensor, got {getattr(source, 'dtype', type(source))}")
        s = self.roi_size
        if source.dim() == 3 and source.shape[2] == 3:
            h, w = int(source.shape[0]), int(source.shape[1])
            c = self.raster(source.shape) if coords is None else coords
            c = torch.as_tensor(np.asarray(c, dtype=np.int64).reshape(-1, 2))
            if c.numel() and (int(c.min()) < 0 or int(c[:, 0].max()) + s > h or int(c[:, 1].max()) + s > w):
                raise ValueError(f"a {s} x {s} window does not lie inside the {h} x {w} slide")
            off, pitch = (c[:, 0] * w + c[:, 1]) * 3, 3 * w
        elif source.dim() == 4 and source.shape[3] == 3 and coords is None:
            if source.shape[1] != s or source.shape[2] != s:
                raise ValueError(f"expected [n,{s},{s},3] ROIs, got {tuple(source.shape)}")
            c = None
            off, pitch = torch.arange(source.shape[0], dtype=torch.int64) * (3 * s * s), 3 * s
        else:
            raise ValueError("expected a slide [H,W,3] (with coords) or an ROI stack [n,S,S,3] (without), "
                             f"got {tuple(source.shape)}")
        if not source.is_cuda:
            raise RuntimeError("ROI selection runs on an AMD GPU only (no CPU fallback)")
        return source.contiguous(), off, pitch, c

    def stats(self, source, coords=None):
        """source: uint8 on the GPU, a slide [H,W,3] with coords (int [n,2] of (row, col); default `raster(source.shape)`)
        or an ROI stack [n,S,S,3] with coords=None.  Returns int64 [n,4] on the CPU: per window sum R, sum R^2, the number of
        pixels with h > hue_min and v_min < v < v_max (Pillow's HSV), and the pixel count."""
        src, off, pitch, _ = self._windows(source, coords)
        return self._stats(src, off, pitch)

    def _stats(self, src, off, pitch):
        n = int(off.numel())
        if n == 0:
            return torch.zeros((0, 4), dtype=torch.int64)
        out = torch.empty((n, 4), dtype=torch.int64, device=src.device)
        off_dev = off.to(src.device)
        L.check(L.lib().mil_roi_stats(src.data_ptr(), src.numel(), off_dev.data_ptr(), pitch, n, self.roi_size,
                                      self.hue_min, self.v_min, self.v_max, out.data_ptr(), L.stream_ptr()), "mil_roi_stats")
        return out.cpu()

    def keep(self, stats):
        """The reference's two tests (RoiBuilder.py:159, :167) on one window's integers, with Python floats and literally the
        statements `ImageStat.Stat` executes (`sum`, `sum2` are floats there, the count an int).  A variance that rounding
        makes negative counts as "no contrast"; the reference would raise in `math.sqrt` there."""
        s1, s2, n_pass, n = (int(v) for v in stats)
        sum_, sum2 = float(s1), float(s2)
        var = (sum2 - (sum_ ** 2.0) / n) / n
        if var < 0:
            return False
        return math.sqrt(var) > self.min_stddev and n_pass > self.min_pass

    def kept(self, source, coords=None):
        """`select()`'s second item — the `coor_cache`, int64 [T,2] numpy (row, col) of the kept windows (for an ROI stack their
        indices, [T]) — without building the ROI array: `TilePreprocessor.from_slide` reads the windows where they are."""
        src, off, pitch, c = self._windows(source, coords)
        st = self._stats(src, off, pitch)
        kept = [i for i in range(st.shape[0]) if self.keep(st[i].tolist())]
        return np.asarray(kept, dtype=np.int64) if c is None else c[kept].numpy().reshape(-1, 2)

    def select(self, source, coords=None):
        """(rois, kept_coords): the reference's `data_cache` array — uint8 [T,S,S,3] on the GPU, in raster order, ready for
        `TilePreprocessor.__call__` — and its `coor_cache`, int64 [T,2] numpy (row, col).  For an ROI stack the second item
        holds the indices of the kept ROIs, [T].  The reference evaluates the HSV count only when the contrast test
        passes; the conjunction is the same."""
        src, off, pitch, c = self._windows(source, coords)
        st = self._stats(src, off, pitch)
        kept = [i for i in range(st.shape[0]) if self.keep(st[i].tolist())]
        s = self.roi_size
        if c is None:
            return src[torch.as_tensor(kept, dtype=torch.int64, device=src.device)], np.asarray(kept, dtype=np.int64)
        rois = torch.empty((len(kept), s, s, 3), dtype=torch.uint8, device=src.device)
        for j, i in enumerate(kept):
            r, q = int(c[i, 0]), int(c[i, 1])
            rois[j].copy_(src[r:r + s, q:q + s])
        return rois, c[kept].numpy().reshape(-1, 2)
