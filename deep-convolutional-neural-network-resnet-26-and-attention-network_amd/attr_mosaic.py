"""Slide mosaics of per-tile attribution maps, composited on the device.

`TileSaliency`, `TileGradCam`, `TileIntegratedGradients` and `TileSmoothGrad` compute what happens INSIDE the tiles and
`AttributionRenderer` turns it into bytes, one picture per tile; a pathologist reads the slide.  `AttributionMosaic` places
the pictures back where their windows lie: at thumbnail scale (`scale` slide pixels per output pixel) window (row, col) owns the
`roi_size // scale` square block of output pixels from (row // scale, col // scale) on — `AttentionMapRenderer`'s convention —
and one kernel (csrc/attr_mosaic.hip, `mil_attr_mosaic`) area-averages the window's map into that block, colours it and
composites it over the tissue thumbnail with Pillow's alpha_composite.  The arithmetic is integer (include/mil_hip.h states it,
tests/attr_mosaic_reference.py restates it in numpy), so the picture is reproducible bit for bit; only the thumbnail leaves HBM.
DESIGN.md section 3.42.
"""
import numpy as np
import torch

from . import ops
from .attr_render import colour_table
from .heatmap import AttentionMapRenderer, _owned_blocks_collide


class AttributionMosaic:
    """`roi_size`, `scale`: as for `AttentionMapRenderer` (scale divides roi_size).  `cmap`: one of `attr_render.CMAPS` or a
    uint8 [256,3] tensor, the colours of one-channel maps.  `alpha`: the opacity of the maps over the tissue, applied as the
    byte int(alpha * 255) as in `AttributionRenderer`; `alpha_by_value`: scale that byte by the map's value
    ((alpha_byte * v + 127) // 255), so that weak attribution lets the tissue show — one-channel maps only.

    maps: uint8 [T,Hm,Wm] (`AttributionRenderer.grayscale`, `TileGradCam.maps`; coloured through `cmap`) or uint8 [T,Hm,Wm,3]
    (`colour`, `pos_neg`, `overlay`'s heat; the colours themselves), contiguous, on the device, one per window and in the
    order of `coords`.  They must be maps of the whole window — tiles of the flat chain — of any size: Hm x Wm is resampled to
    the block, whatever the ratio.  Every argument is checked on the host before anything is launched."""

    def __init__(self, roi_size=1200, scale=16, cmap="jet", alpha=0.5, alpha_by_value=False):
        self._tissue = AttentionMapRenderer(roi_size, scale)
        self.roi_size, self.scale = self._tissue.roi_size, self._tissue.scale
        alpha = float(alpha)
        if not (0.0 <= alpha <= 1.0):
            raise ValueError(f"alpha must be in [0, 1], got {alpha}")
        if isinstance(cmap, torch.Tensor):
            if cmap.dtype != torch.uint8 or tuple(cmap.shape) != (256, 3):
                raise ValueError(f"cmap: a uint8 [256,3] tensor, got {cmap.dtype} {tuple(cmap.shape)}")
            table = cmap.detach().cpu().contiguous()
        else:
            table = colour_table(cmap)
        self.alpha, self.alpha_byte, self.alpha_by_value = alpha, int(alpha * 255), bool(alpha_by_value)
        self.table = table
        self._device_tables = {}

    def _lut(self, device):
        got = self._device_tables.get(device)
        if got is None:
            got = self._device_tables[device] = self.table.to(device)
        return got

    def _check_maps(self, maps, coords, device):
        """The refusals that concern the maps; `device`: where they must be (None: not known, the caller's next check refuses)."""
        if not isinstance(maps, torch.Tensor) or maps.dtype != torch.uint8:
            raise ValueError(f"maps must be a uint8 tensor, got {getattr(maps, 'dtype', type(maps).__name__)}: attribution tensors go "
                             "through AttributionRenderer.grayscale / colour first (normalisation is theirs)")
        if maps.dim() not in (3, 4) or (maps.dim() == 4 and maps.shape[3] != 3) or maps.shape[1] < 1 or maps.shape[2] < 1:
            raise ValueError(f"maps must be uint8 [T,Hm,Wm] or [T,Hm,Wm,3], got {tuple(maps.shape)}")
        if not maps.is_contiguous():
            raise ValueError("maps must be contiguous")
        if self.alpha_by_value and maps.dim() == 4:
            raise ValueError("alpha_by_value needs one-channel maps: a colour picture has no value to scale the alpha by")
        c = np.asarray(coords.cpu() if isinstance(coords, torch.Tensor) else coords)
        if c.size // 2 != maps.shape[0]:
            raise ValueError(f"{maps.shape[0]} maps for {c.size // 2} windows")
        if device is not None and maps.device != device:
            raise ValueError(f"maps are on {maps.device}, the slide or canvas on {device}")

    def render(self, slide, coords, maps):
        """slide: uint8 [H,W,3] on the GPU; coords: int [T,2] of (row, col), the kept windows; maps: see the class.  Returns
        uint8 [2, H//scale, W//scale, 3] on the slide's device: panel 0 the maps on white, panel 1 the maps over the tissue
        (the box mean of every window, `AttentionMapRenderer`'s panel 0 without rectangles); both white where no window lies."""
        self._check_maps(maps, coords, slide.device if isinstance(slide, torch.Tensor) else None)
        t = maps.shape[0]
        none = torch.full((4, t), -1, dtype=torch.int16)
        c = self._tissue._check(slide, coords, none, None, None)
        canvas = torch.full((5, slide.shape[0] // self.scale, slide.shape[1] // self.scale, 3), 255, dtype=torch.uint8, device=slide.device)
        self._tissue.render_into(canvas, slide, c, none)             # the tissue into panel 0, nothing else
        self._launch(canvas[1], canvas[0], c, maps)
        return canvas[:2].flip(0)

    def render_into(self, heat, on_tissue, coords, maps):
        """The lower call, on the caller's canvases: `heat` and `on_tissue`, uint8 [Ht,Wt,3], contiguous, on the maps' device,
        either may be None.  `heat` receives the coloured maps, `on_tissue` — which holds the tissue thumbnail — their
        composite over what it holds, in place; no pixel that a window does not own is touched.  Window (row, col) owns the
        block from (row // scale, col // scale) on, which must lie inside the canvas.  Returns (heat, on_tissue)."""
        canvas = heat if heat is not None else on_tissue
        self._check_maps(maps, coords, canvas.device if isinstance(canvas, torch.Tensor) else None)
        s, d = self.roi_size, self.scale
        if s % d != 0:
            raise ValueError(f"scale {d} does not divide roi_size {s}")
        if canvas is None:
            raise ValueError("neither heat nor on_tissue: nothing to draw on")
        for x in (heat, on_tissue):
            if x is not None and (not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or x.dim() != 3 or x.shape[2] != 3
                                  or x.shape != canvas.shape or not x.is_contiguous() or x.device != canvas.device):
                raise ValueError("expected contiguous uint8 canvases [Ht,Wt,3] of one shape on one device")
        c = np.asarray(coords.cpu() if isinstance(coords, torch.Tensor) else coords)
        if c.size and c.dtype.kind not in "iu":
            raise ValueError("coords must be integers")
        c = c.astype(np.int64).reshape(-1, 2)
        n, (ht, wt) = s // d, canvas.shape[:2]
        if c.size and (c.min() < 0 or (c[:, 0] // d).max() + n > ht or (c[:, 1] // d).max() + n > wt):
            raise ValueError(f"the {n} x {n} block of a window does not lie inside the {ht} x {wt} canvas")
        if _owned_blocks_collide(c[:, 0] // d, c[:, 1] // d, n):
            raise ValueError("two windows would own the same output pixel")
        if not canvas.is_cuda:
            raise RuntimeError("attribution mosaics are composited on an AMD GPU only (no CPU fallback)")
        self._launch(heat, on_tissue, c, maps)
        return heat, on_tissue

    def _launch(self, heat, on_tissue, c, maps):
        if len(c) == 0:
            return
        pos = torch.from_numpy(c // self.scale).to(torch.int32).contiguous().to(maps.device)
        ops.attr_mosaic(maps, pos, self.roi_size // self.scale, self._lut(maps.device) if maps.dim() == 3 else None, self.alpha_byte,
                        self.alpha_by_value, heat, on_tissue)
