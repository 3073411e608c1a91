"""Rotation and affine augmentation on the device: torchvision's `RandomAffine` / `RandomRotation` as its PIL backend computes
them — `img.transform(size, Image.AFFINE, matrix, Image.BILINEAR, fillcolor=fill)` with the matrix of
`_get_inverse_affine_matrix` — on `U8Tiles` (`RandomAffine.apply`) and, through `TilePreprocessor(..., affine=)` and
`SlideBag(affine=)`, on the windows of a resident slide, where a rotated window reads the tissue that really lies beside it
instead of black corners.  One kernel (csrc/affine.hip, `mil_affine_u8`); the bytes are Pillow's, bit for bit.  Bilinear only.
"""
import math
import numbers

import torch

from . import ops
from .preprocess import U8Tiles


def affine_matrix(center, angle, translate, scale, shear):
    """torchvision's `_get_inverse_affine_matrix(center, angle, translate, scale, shear)` in Python `math` doubles: the six
    entries a0..a5 of the map from OUTPUT to INPUT coordinates that `F.affine` hands to Pillow.  center = (cx, cy) (F.affine:
    (width * 0.5, height * 0.5)), angle in degrees, translate = (tx, ty) in pixels, scale > 0, shear = (sx, sy) in degrees
    (or one number: sx).  With rot, sx, sy in radians:

        a = cos(rot - sy) / cos(sy)                        b = -cos(rot - sy) * tan(sx) / cos(sy) - sin(rot)
        c = sin(rot - sy) / cos(sy)                        d = -sin(rot - sy) * tan(sx) / cos(sy) + cos(rot)
        m = [d, -b, 0, -c, a, 0], every entry / scale
        m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)      m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
        m[2] += cx                                         m[5] += cy

    the inverse of  T(center) T(translate) R(angle) Shear(sx, sy) Scale(scale) T(-center)."""
    cx, cy = (float(v) for v in center)
    tx, ty = (float(v) for v in translate)
    if isinstance(shear, numbers.Number):
        shear = (shear, 0.0)
    scale = float(scale)
    if not scale > 0.0:
        raise ValueError(f"scale must be positive, got {scale}")
    rot, sx, sy = math.radians(float(angle)), math.radians(float(shear[0])), math.radians(float(shear[1]))
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def quarter_turn_matrix(k, size):
    """The exact map (six integers as floats) that turns a size x size image by k * 90 degrees counter-clockwise, as
    `np.rot90(img, k)` does.  Integer entries put every input coordinate on a pixel centre: dx = dy = 0, the transform is a bit
    copy.  k is taken mod 4."""
    n = float(int(size))
    if n < 1:
        raise ValueError(f"size must be positive, got {size}")
    return [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0], [0.0, -1.0, n, 1.0, 0.0, 0.0],
            [-1.0, 0.0, n, 0.0, -1.0, n], [0.0, 1.0, 0.0, -1.0, 0.0, n]][int(k) % 4]


def compose(outer, inner):
    """The matrix of `inner` applied to the image first and `outer` second: as maps from output to input, p_in = inner(outer(p_out))."""
    a, q = inner, outer
    return [a[0] * q[0] + a[1] * q[3], a[0] * q[1] + a[1] * q[4], a[0] * q[2] + a[1] * q[5] + a[2],
            a[3] * q[0] + a[4] * q[3], a[3] * q[1] + a[4] * q[4], a[3] * q[2] + a[4] * q[5] + a[5]]


def _number(v):
    return isinstance(v, numbers.Number) and not isinstance(v, bool)


def _symmetric(value, name, lengths=(2,)):
    """torchvision's `_setup_angle` / shear check: a number x >= 0 means (-x, x), a sequence of an allowed length is taken as
    given."""
    if _number(value):
        if value < 0:
            raise ValueError(f"if {name} is a single number, it must be non negative")
        vals = (-float(value), float(value))
    elif isinstance(value, (tuple, list)) and len(value) in lengths and all(_number(v) for v in value):
        vals = tuple(float(v) for v in value)
    else:
        raise ValueError(f"{name} should be a number or a sequence of {' or '.join(map(str, lengths))} numbers")
    if not all(math.isfinite(v) for v in vals):
        raise ValueError(f"{name} must be finite, got {vals}")
    return vals


def _pair(value, name):
    if not isinstance(value, (tuple, list)) or len(value) != 2 or not all(_number(v) for v in value):
        raise ValueError(f"{name} should be a pair of numbers")
    return tuple(float(v) for v in value)


class RandomAffine:
    """torchvision's `RandomAffine(degrees, translate=None, scale=None, shear=None, fill=0)` (bilinear, PIL backend) for
    `U8Tiles` on the GPU; with translate, scale and shear left at None it is `RandomRotation(degrees)` about the centre without
    `expand`.  degrees, shear: a number x >= 0 means [-x, x], a pair is taken as given (shear: four numbers are the x and the y
    range); translate: (a, b) in [0, 1], the largest shifts as fractions of width and height; scale: (lo, hi), both positive.
    fill: a byte or three — (255, 255, 255) is the slide background of H&E.  quarter_turns=True composes a uniformly drawn
    multiple of 90 degrees (an exact integer matrix, `quarter_turn_matrix`) with the drawn map; with degrees=0 and the rest None
    that gives, with the two flips of `TilePreprocessor.draw_params`, all eight symmetries of the square exactly.  Bad values
    raise ValueError."""

    def __init__(self, degrees, translate=None, scale=None, shear=None, fill=0, quarter_turns=False):
        self.degrees = _symmetric(degrees, "degrees")
        self.translate = self.scale = self.shear = None
        if translate is not None:
            self.translate = _pair(translate, "translate")
            if not all(0.0 <= v <= 1.0 for v in self.translate):
                raise ValueError("translation values should be between 0 and 1")
        if scale is not None:
            self.scale = _pair(scale, "scale")
            if not all(v > 0.0 and math.isfinite(v) for v in self.scale):
                raise ValueError("scale values should be positive")
        if shear is not None:
            self.shear = _symmetric(shear, "shear", (2, 4))
        ops.affine_fill(fill)
        self.fill = fill
        self.quarter_turns = bool(quarter_turns)

    def draw_params(self, n, size, generator=None):
        """float64 [n,6] on the host: one matrix per tile of `size` pixels (a number, or (height, width)), in the tile's own
        coordinates, centre (width * 0.5, height * 0.5).  The draw order is this project's own (as
        `TilePreprocessor.draw_params`' and `ColorJitter.draw_params`' are), not torchvision's: ONE
        `torch.rand(n, 6, dtype=float64)` u — whatever is switched on — whose columns are angle, x translation, y translation,
        scale, x shear, y shear, each value lo + (hi - lo) * u in double; the translations range over [-a * width, a * width] and
        [-b * height, b * height] and are rounded to whole pixels as torchvision rounds them (Python's `round`: half to even);
        what is switched off gets its neutral value (0, 0, 1, 0).  Then, with quarter_turns, ONE
        `torch.randint(0, 4, (n,))` k: the tile is turned by k * 90 degrees after the drawn map (`compose`); that needs square
        tiles."""
        height, width = (int(size), int(size)) if _number(size) else (int(v) for v in size)
        if n < 0 or height < 1 or width < 1:
            raise ValueError(f"n must be >= 0 and size positive, got {n}, {size}")
        if self.quarter_turns and height != width:
            raise ValueError(f"quarter turns need square tiles, got {height} x {width}")
        u = torch.rand((n, 6), dtype=torch.float64, generator=generator).tolist()
        k = torch.randint(0, 4, (n,), generator=generator).tolist() if self.quarter_turns else None

        def pick(rng, v):
            return rng[0] + (rng[1] - rng[0]) * v

        center = (width * 0.5, height * 0.5)
        out = torch.empty((n, 6), dtype=torch.float64)
        for i in range(n):
            tx = ty = 0
            if self.translate is not None:
                mx, my = float(self.translate[0] * width), float(self.translate[1] * height)
                tx, ty = int(round(pick((-mx, mx), u[i][1]))), int(round(pick((-my, my), u[i][2])))
            sc = 1.0 if self.scale is None else pick(self.scale, u[i][3])
            sx = sy = 0.0
            if self.shear is not None:
                sx = pick(self.shear[:2], u[i][4])
                if len(self.shear) == 4:
                    sy = pick(self.shear[2:], u[i][5])
            m = affine_matrix(center, pick(self.degrees, u[i][0]), (tx, ty), sc, (sx, sy))
            if k is not None:
                m = compose(quarter_turn_matrix(k[i], width), m)
            out[i] = torch.tensor(m, dtype=torch.float64)
        return out

    def apply(self, tiles, matrices):
        """tiles: `U8Tiles` on the GPU, matrices: `draw_params(len(tiles), tiles.shape[2:])` or injected float64 [n,6].  Returns
        NEW `U8Tiles` of the same size (the transform cannot be done in place).  CPU tiles raise RuntimeError; another handle
        (`S2dTiles`, a tensor), a wrong shape or a non-finite entry ValueError — all before any launch."""
        return apply_affine(tiles, matrices, self.fill)

    def __call__(self, tiles, generator=None):
        if not isinstance(tiles, U8Tiles):
            raise ValueError(f"the affine transform works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
        return apply_affine(tiles, self.draw_params(len(tiles), tuple(tiles.shape[2:]), generator), self.fill)


def apply_affine(tiles, matrices, fill=0):
    """`U8Tiles` through `ops.affine_u8` with one matrix per tile; every refusal comes before a launch."""
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"the affine transform works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
    m = ops.affine_matrices(matrices, len(tiles))
    ops.affine_fill(fill)
    if not tiles.u8.is_cuda:
        raise RuntimeError("the affine transform runs on an AMD GPU only (no CPU fallback)")
    return U8Tiles(ops.affine_u8(tiles.u8, m, fill))
