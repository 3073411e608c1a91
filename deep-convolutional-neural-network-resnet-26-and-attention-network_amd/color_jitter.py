"""Colour jitter on the device: the augmentation the reference's train chain names and keeps commented out,
`transforms.ColorJitter(brightness=0.2, contrast=0.1, saturation=0.05, hue=0.02)` (RoiBuilder.py:200) — on the host several
Pillow passes per tile (RGB -> HSV -> RGB, ImageStat, three blends), here one kernel family (csrc/color_jitter.hip,
`mil_color_jitter_u8`) over the resized uint8 tiles where they lie: after Resize and the flips, before ToTensor, the position
of the line in the chain (flips commute with everything it does).  The bytes are Pillow's, as torchvision's PIL backend calls
it (ImageEnhance.Brightness / Contrast / Color, adjust_hue), bit for bit.
"""
import collections
import math
import numbers

import torch

from . import _lib as L
from .preprocess import U8Tiles

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

JitterParams = collections.namedtuple("JitterParams", ["order", "factors", "hue_shift"])
JitterParams.__doc__ = """Per tile, on the host: `order` int32 [n,4] (op codes 0 brightness, 1 contrast, 2 saturation, 3 hue in
the order they are applied, -1 = no op), `factors` float32 [n,3] (brightness, contrast, saturation), `hue_shift` int32 [n] in
0..255 (what adjust_hue adds to h: int(hue_factor * 255) mod 256)."""


def _range(value, name, center, bound, clip_first_on_zero):
    """torchvision's ColorJitter._check_input: (lo, hi), or None when the range collapses to the neutral value."""
    if isinstance(value, numbers.Number) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"if {name} is a single number, it must be non negative")
        lo, hi = center - float(value), center + float(value)
        if clip_first_on_zero:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2 and all(
            isinstance(v, numbers.Number) and not isinstance(v, bool) for v in value):
        lo, hi = float(value[0]), float(value[1])
    else:
        raise ValueError(f"{name} should be a single number or a (lo, hi) pair of numbers")
    if not (bound[0] <= lo <= hi <= bound[1]) or math.isinf(hi):
        raise ValueError(f"{name} values should lie in {bound} with lo <= hi, got {(lo, hi)}")
    return None if lo == hi == center else (lo, hi)


def hue_shift(hue_factor):
    """What adjust_hue adds to h for a hue factor: int(hue_factor * 255), truncated toward zero, mod 256 (-0.02 -> 251)."""
    return int(float(hue_factor) * 255) % 256


def checked_params(params, n):
    """`params` (a JitterParams or any (order, factors, hue_shift) triple) as contiguous host tensors for `n` tiles; raises
    ValueError for a wrong shape, an op code outside -1..3, a repeated op code, a factor that is not a finite number >= 0 or a
    shift outside 0..255."""
    try:
        order, factors, shift = params
    except (TypeError, ValueError):
        raise ValueError("jitter parameters are (order [n,4], factors [n,3], hue_shift [n])") from None
    order = torch.as_tensor(order).detach().cpu()
    factors = torch.as_tensor(factors).detach().cpu()
    shift = torch.as_tensor(shift).detach().cpu()
    if order.is_floating_point() or shift.is_floating_point() or order.dtype == torch.bool or shift.dtype == torch.bool:
        raise ValueError("order and hue_shift must be integers")
    if tuple(order.shape) != (n, 4) or tuple(factors.shape) != (n, 3) or tuple(shift.shape) != (n,):
        raise ValueError(f"expected order [{n},4], factors [{n},3] and hue_shift [{n}], got {tuple(order.shape)}, "
                         f"{tuple(factors.shape)}, {tuple(shift.shape)}")
    order, factors, shift = order.to(torch.int64), factors.to(torch.float32), shift.to(torch.int64)
    if n:
        if int(order.min()) < -1 or int(order.max()) > 3:
            raise ValueError("op codes must lie in -1..3")
        for op in range(4):
            if int((order == op).sum(dim=1).max()) > 1:
                raise ValueError(f"op code {op} is repeated in a tile's order")
        if int(shift.min()) < 0 or int(shift.max()) > 255:
            raise ValueError("hue shifts must lie in 0..255")
        if not bool(torch.isfinite(factors).all()) or float(factors.min()) < 0:
            raise ValueError("factors must be finite and non-negative")
    return JitterParams(order.to(torch.int32).contiguous(), factors.contiguous(), shift.to(torch.int32).contiguous())


def apply_jitter(tiles, params):
    """Jitters the `U8Tiles` in place with the per-tile `params` and returns the handle; every refusal comes before a launch."""
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"the colour jitter works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
    u8 = tiles.u8
    t, _, h, w = u8.shape
    if h != w:
        raise ValueError(f"expected square tiles, got {h} x {w}")
    p = checked_params(params, t)
    if not u8.is_cuda:
        raise RuntimeError("the colour jitter runs on an AMD GPU only (no CPU fallback)")
    if t and h > 4096:
        raise ValueError("tiles of more than 4096 x 4096 pixels are not supported")
    if t == 0:
        return tiles
    dev = u8.device
    order, factors, shift = (x.to(dev) for x in p)
    lsum = torch.empty(t, dtype=torch.int32, device=dev)
    L.check(L.lib().mil_color_jitter_u8(u8.data_ptr(), order.data_ptr(), factors.data_ptr(), shift.data_ptr(), lsum.data_ptr(),
                                        t, h, L.stream_ptr()), "mil_color_jitter_u8")
    return tiles


class ColorJitter:
    """torchvision's `ColorJitter(brightness=0, contrast=0, saturation=0, hue=0)` for `U8Tiles` on the GPU.  A number x means
    the range [max(0, 1 - x), 1 + x] of factors (hue: [-x, x], 0 <= x <= 0.5), a (lo, hi) pair is taken as given; a range that
    collapses to the neutral value switches the op off (torchvision's None).  Bad values raise ValueError."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        inf = float("inf")
        self.brightness = _range(brightness, "brightness", 1.0, (0.0, inf), True)
        self.contrast = _range(contrast, "contrast", 1.0, (0.0, inf), True)
        self.saturation = _range(saturation, "saturation", 1.0, (0.0, inf), True)
        self.hue = _range(hue, "hue", 0.0, (-0.5, 0.5), False)

    @property
    def ranges(self):
        """The four ranges by op code; None = switched off."""
        return (self.brightness, self.contrast, self.saturation, self.hue)

    def draw_params(self, n, generator=None):
        """`JitterParams` for n tiles, on the host.  The draw order is this project's own (as TilePreprocessor.draw_params'
        is), not torchvision's: one `torch.rand(n, 4)` whose per-row argsort is the tile's permutation of the four op codes
        (a switched-off op becomes -1 where it stands, so the active ops appear once each in a uniformly random order), then
        one `torch.rand(n, 4, dtype=float64)` u with factor = lo + (hi - lo) * u per op (brightness, contrast, saturation, hue
        factor) in double, the three factors cast to float32 as blend takes them and the hue factor turned into its shift.
        A switched-off op gets its neutral value (1.0, shift 0)."""
        order = torch.argsort(torch.rand((n, 4), generator=generator), dim=1).to(torch.int32)
        u = torch.rand((n, 4), dtype=torch.float64, generator=generator)
        vals = torch.empty((n, 4), dtype=torch.float64)
        for op, rng in enumerate(self.ranges):
            if rng is None:
                order[order == op] = -1
                vals[:, op] = 0.0 if op == HUE else 1.0
            else:
                vals[:, op] = rng[0] + (rng[1] - rng[0]) * u[:, op]
        shift = torch.remainder(torch.trunc(vals[:, HUE] * 255).to(torch.int64), 256).to(torch.int32)
        return JitterParams(order, vals[:, :3].to(torch.float32).contiguous(), shift)

    def apply(self, tiles, params):
        """tiles: `U8Tiles` on the GPU, params: `draw_params(len(tiles))` or injected ones.  Jitters in place and returns the
        handle.  CPU tiles raise RuntimeError; a shape mismatch, an op code outside -1..3, a repeated op code or a shift
        outside 0..255 ValueError — all before any launch."""
        return apply_jitter(tiles, params)

    def __call__(self, tiles, generator=None):
        return apply_jitter(tiles, self.draw_params(len(tiles), generator))
