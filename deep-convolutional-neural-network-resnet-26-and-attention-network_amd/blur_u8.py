"""Pillow's Gaussian blur on the device for uint8 tiles and maps: the defocus augmentation of the H&E studies (a scanner's focus
drifts between slides) on `U8Tiles` where they lie, and the smoothing the toolkit's users give `uint8` attribution maps before they
overlay them.  `img.filter(ImageFilter.GaussianBlur(s))` is not a Gaussian convolution: it is three passes of an extended box blur
along the rows, then three along the columns, in 32-bit fixed point, rounded to a byte after every pass — an integer contract, so the
kernel (csrc/blur_u8.hip, `mil_gaussian_blur_u8`) writes Pillow's bytes, bit for bit (include/mil_hip.h; the numpy restatement:
tests/blur_u8_reference.py).  `mil_pixel_blur` (feature_inv.gaussian_blur) stays what it is: an fp32 filter with scipy's taps.
"""
import math
import numbers

import torch

from . import ops
from .preprocess import U8Tiles


def _number(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool)


def checked_sigmas(sigma, n, name="sigma"):
    """(sigma_x, sigma_y), two float64 [n] host tensors, from what `gaussian_blur_u8` takes: a number, an (sx, sy) pair of
    numbers, or a per-item tensor [n] / [n,2].  Every value finite and in [0, 8]; anything else raises ValueError."""
    if _number(sigma):
        sigma = (sigma, sigma)
    if isinstance(sigma, (tuple, list)) and len(sigma) == 2 and all(_number(v) for v in sigma):
        cols = [torch.full((n,), float(v), dtype=torch.float64) for v in sigma]
    elif isinstance(sigma, torch.Tensor) and sigma.dtype != torch.bool and not sigma.is_complex():
        s = sigma.detach().cpu().to(torch.float64)
        if tuple(s.shape) == (n,):
            cols = [s, s]
        elif tuple(s.shape) == (n, 2):
            cols = [s[:, 0].contiguous(), s[:, 1].contiguous()]
        else:
            raise ValueError(f"{name} must be a number, an (sx, sy) pair or a tensor [{n}] / [{n},2], got shape {tuple(s.shape)}")
    else:
        raise ValueError(f"{name} must be a number, an (sx, sy) pair or a tensor [{n}] / [{n},2], got {sigma!r}")
    for c in cols:
        if c.numel() and (not bool(torch.isfinite(c).all()) or float(c.min()) < 0.0 or float(c.max()) > ops.BLUR_U8_MAX_SIGMA):
            raise ValueError(f"{name} must be finite and lie in [0, {ops.BLUR_U8_MAX_SIGMA:g}]")
    return cols[0], cols[1]


def gaussian_blur_u8(x, sigma, out=None):
    """`PIL.ImageFilter.GaussianBlur(sigma)` of every tile or map of x, bit for bit, in one launch.  x: `U8Tiles` on the GPU (the
    three bands of a tile share its sigma, as Pillow's `RGB` path does) or a uint8 map stack [T,H,W] on the GPU (Pillow's `L`).
    sigma: a number, an (sx, sy) pair — Pillow's tuple radius, x along the width — or a per-item tensor [T] / [T,2]; 0 on an
    axis leaves that axis alone, 0 on both makes the item a bit copy.  out: None, or a handle / tensor like x that does not overlap
    it (the blur is never in place).  Returns what it was given: new `U8Tiles` or a new tensor.  A CPU input raises RuntimeError;
    a wrong type or shape, or a sigma outside [0, 8], ValueError — all before any launch."""
    if isinstance(x, U8Tiles):
        u8, ppi = x.u8, 3
        if out is not None and not isinstance(out, U8Tiles):
            raise ValueError(f"out must be U8Tiles like x, got {type(out).__name__}")
        dst = None if out is None else out.u8
    elif isinstance(x, torch.Tensor) and x.dtype == torch.uint8 and x.dim() == 3:
        u8, ppi, dst = x, 1, out
    else:
        raise ValueError(f"x must be U8Tiles or a uint8 map stack [T,H,W], got {type(x).__name__} "
                         f"{getattr(x, 'dtype', '')} {tuple(getattr(x, 'shape', ()))}")
    sx, sy = checked_sigmas(sigma, u8.shape[0])
    res = ops.gaussian_blur_u8(u8, ops.box_blur_params(sx, sy), ppi, dst)
    if ppi == 1:
        return res
    return out if out is not None else U8Tiles(res)


def apply_blur(tiles, sigmas):
    """`U8Tiles` through `gaussian_blur_u8` with one sigma (or one (sx, sy) row) per tile; returns NEW `U8Tiles`.  Every refusal
    comes before a launch."""
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"the Gaussian blur works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
    if not isinstance(sigmas, torch.Tensor):
        try:
            sigmas = torch.as_tensor(sigmas, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"sigmas must be a tensor [{len(tiles)}] or [{len(tiles)},2], got {sigmas!r}") from None
    if sigmas.dim() == 0:
        raise ValueError(f"sigmas must be a tensor [{len(tiles)}] or [{len(tiles)},2], got a scalar")
    return gaussian_blur_u8(tiles, sigmas)


class GaussianBlurU8:
    """`GaussianBlurU8(sigma=(0.1, 2.0), p=0.5)` for `U8Tiles` on the GPU: each tile is blurred with probability p, with Pillow's
    `GaussianBlur(sigma)` and a sigma of its own.  sigma: a number (fixed) or a (lo, hi) range with 0 <= lo <= hi <= 8; p in
    [0, 1].  Bad values raise ValueError."""

    def __init__(self, sigma=(0.1, 2.0), p=0.5):
        if _number(sigma):
            sigma = (sigma, sigma)
        if not isinstance(sigma, (tuple, list)) or len(sigma) != 2 or not all(_number(v) and math.isfinite(v) for v in sigma):
            raise ValueError(f"sigma must be a number or a (lo, hi) pair of numbers, got {sigma!r}")
        lo, hi = float(sigma[0]), float(sigma[1])
        if not 0.0 <= lo <= hi <= ops.BLUR_U8_MAX_SIGMA:
            raise ValueError(f"sigma must satisfy 0 <= lo <= hi <= {ops.BLUR_U8_MAX_SIGMA:g}, got {(lo, hi)}")
        if not _number(p) or not 0.0 <= p <= 1.0:
            raise ValueError(f"p must be a probability in [0, 1], got {p!r}")
        self.sigma, self.p = (lo, hi), float(p)

    def draw_params(self, n, generator=None):
        """float64 [n] on the host: each tile's sigma, 0 meaning untouched.  The draw is this project's own: ONE
        `torch.rand((n, 2), dtype=float64)` u; tile i is blurred when u[i,0] < p, with sigma = lo + (hi - lo) u[i,1]."""
        if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
            raise ValueError(f"n must be an integer >= 0, got {n!r}")
        u = torch.rand((int(n), 2), dtype=torch.float64, generator=generator)
        lo, hi = self.sigma
        return torch.where(u[:, 0] < self.p, lo + (hi - lo) * u[:, 1], torch.zeros((), dtype=torch.float64))

    def apply(self, tiles, sigmas):
        """tiles: `U8Tiles` on the GPU; sigmas: `draw_params(len(tiles))` or injected float64 [n] (or [n,2]: (sx, sy) per tile).
        Returns NEW `U8Tiles`; a tile whose sigma is 0 is copied bit for bit.  CPU tiles raise RuntimeError; another handle, a
        wrong shape or a sigma outside [0, 8] ValueError — all before any launch."""
        return apply_blur(tiles, sigmas)

    def __call__(self, tiles, generator=None):
        if not isinstance(tiles, U8Tiles):
            raise ValueError(f"the Gaussian blur works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
        return apply_blur(tiles, self.draw_params(len(tiles), generator))
