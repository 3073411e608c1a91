"""Elastic deformation on the device, fused into the affine resampling: the morphology augmentation of the H&E literature
(random smooth displacement of every pixel) as ONE more term in the source coordinate that `mil_affine_u8` evaluates per output
pixel — a uniform cubic B-spline of a coarse per-tile control lattice, in source pixels — so a rotated and deformed tile or slide
window is interpolated once (csrc/affine.hip, `mil_affine_elastic_u8`; the byte contract and its numpy restatement:
include/mil_hip.h, tests/elastic_reference.py).  On `U8Tiles` through `ElasticDeform.apply`, on the windows of a resident slide
through `TilePreprocessor(..., elastic=)` and `SlideBag(elastic=)`, where a deformed window reads the tissue beside it.  A lattice
of zeros gives the affine transform's bytes, hence Pillow's.
"""
import math
import numbers

import torch

from . import ops
from .preprocess import U8Tiles


def _number(v):
    return isinstance(v, numbers.Number) and not isinstance(v, bool) and not isinstance(v, complex)


class ElasticDeform:
    """`ElasticDeform(magnitude, cells=4, clip=None, fill=0)` for `U8Tiles` on the GPU.  magnitude >= 0: the standard deviation,
    in pixels, of the control displacements; cells: the number of B-spline cells the tile is divided into, a positive integer or
    (gy, gx) — the lattice of a tile is [2, gy+3, gx+3]; clip: every control displacement is clamped to [-clip, clip] (default
    2 * magnitude); fill: a byte or three, for what leaves the source.  The B-spline weights are non-negative and sum to 1, so no
    pixel moves further than `clip` (plus rounding) in either direction.  Bad values raise ValueError."""

    def __init__(self, magnitude, cells=4, clip=None, fill=0):
        if not _number(magnitude) or not math.isfinite(magnitude) or magnitude < 0:
            raise ValueError(f"magnitude must be a finite number >= 0, got {magnitude!r}")
        self.magnitude = float(magnitude)
        if isinstance(cells, numbers.Integral) and not isinstance(cells, bool):
            cells = (cells, cells)
        if not isinstance(cells, (tuple, list)) or len(cells) != 2 or not all(
                isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 1 for v in cells):
            raise ValueError(f"cells must be a positive integer or a pair (gy, gx) of them, got {cells!r}")
        self.cells = (int(cells[0]), int(cells[1]))
        if clip is None:
            clip = 2.0 * self.magnitude
        if not _number(clip) or not math.isfinite(clip) or clip < 0:
            raise ValueError(f"clip must be a finite number >= 0, got {clip!r}")
        self.clip = float(clip)
        ops.affine_fill(fill)
        self.fill = fill

    def draw_params(self, n, size, generator=None):
        """float64 [n,2,gy+3,gx+3] on the host: one control lattice per tile of `size` pixels (a number, or (height, width)).
        ONE `torch.randn((n,2,gy+3,gx+3), dtype=float64)` draw, times `magnitude`, clamped to [-clip, clip]; the draw order is
        this project's own.  ValueError when `clip` exceeds 0.4 of the smaller cell side, min(height / gy, width / gx): control
        displacements below delta / 2.48 of the cell side delta are a SUFFICIENT condition for a 2-D cubic B-spline deformation
        not to fold (Choi & Lee, Injectivity conditions of 2D and 3D uniform cubic B-spline functions, 2000), and 0.4 < 1 / 2.48;
        the bound is that theorem's, not a measurement."""
        height, width = (int(size), int(size)) if _number(size) else (int(v) for v in size)
        if n < 0 or height < 1 or width < 1:
            raise ValueError(f"n must be >= 0 and size positive, got {n}, {size}")
        gy, gx = self.cells
        cell = min(height / gy, width / gx)
        if self.clip > 0.4 * cell:
            raise ValueError(f"clip {self.clip} exceeds 0.4 of the smaller cell side ({cell:g} pixels): the deformation could fold")
        z = torch.randn((n, 2, gy + 3, gx + 3), dtype=torch.float64, generator=generator)
        return (z * self.magnitude).clamp_(-self.clip, self.clip)

    def apply(self, tiles, ctrl, matrices=None):
        """tiles: `U8Tiles` on the GPU; ctrl: `draw_params(len(tiles), tiles.shape[2:])` or injected float64 [n,2,gy+3,gx+3];
        matrices: float64 [n,6] as `RandomAffine.draw_params` makes them, applied in the same resampling (None: the identity).
        Returns NEW `U8Tiles` of the same size.  CPU tiles raise RuntimeError; another handle (`S2dTiles`, a tensor), a wrong
        shape or a non-finite entry ValueError — all before any launch."""
        return apply_elastic(tiles, ctrl, matrices, self.fill)

    def __call__(self, tiles, generator=None):
        if not isinstance(tiles, U8Tiles):
            raise ValueError(f"the elastic deformation works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
        return apply_elastic(tiles, self.draw_params(len(tiles), tuple(tiles.shape[2:]), generator), None, self.fill)


def apply_elastic(tiles, ctrl, matrices=None, fill=0):
    """`U8Tiles` through `ops.elastic_u8` with one lattice (and one matrix) per tile; every refusal comes before a launch."""
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"the elastic deformation works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
    c = ops.elastic_lattice(ctrl, len(tiles))
    m = None if matrices is None else ops.affine_matrices(matrices, len(tiles))
    ops.affine_fill(fill)
    if not tiles.u8.is_cuda:
        raise RuntimeError("the elastic deformation runs on an AMD GPU only (no CPU fallback)")
    return U8Tiles(ops.elastic_u8(tiles.u8, m, c, fill))
