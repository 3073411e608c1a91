"""Device-side tile finalisation: the reference's `RoiBuilder.img_finalize` / `img_finalize_flat`
(RoiBuilder.py:193-210, used by `get_train_data` :222-245 and `get_validation_data` :247-268) on cached uint8 ROIs that
stay resident in HBM, producing the fp32 [T,3,R,R] tile stack `Attention.forward` takes — instead of a per-tile
torchvision/Pillow chain on the host followed by an fp32 upload (the `Tensor.cuda()` time that dominated the reference's
profile).  The arithmetic is Pillow's bilinear resampling, bit-exact (see csrc/preprocess.hip).
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

AFFINE_CHUNK = 64       # windows per rotated stack of the `affine=` path: bounds the intermediate at AFFINE_CHUNK * 3 S^2 bytes


class S2dTiles:
    """A stack of tiles held as the bf16 space-to-depth tensor the stem kernels read, `xs [T, R/2, R/2, 16]` (channel =
    c*4 + dy*2 + dx of the 2x2 pixel block, 12 real): what `TilePreprocessor(..., out="s2d")` returns and what
    `Attention.forward` / `forward_bags` / `ResNet.forward` of both encoders (`encoder.ResNet`, `alt_resnet.ResNet`) accept in
    place of the fp32 `[T,3,R,R]` stack (bf16 compute mode).
    `shape` is the shape of the fp32 stack it stands for; indexing with a tensor / slice selects tiles."""

    def __init__(self, xs):
        if xs.dim() != 4 or xs.shape[3] != 16 or xs.dtype != torch.bfloat16:
            raise ValueError(f"expected a bf16 [T,H/2,W/2,16] space-to-depth tensor, got {tuple(xs.shape)} {xs.dtype}")
        self.xs = xs

    @property
    def shape(self):
        t, h2, w2, _ = self.xs.shape
        return torch.Size((t, 3, 2 * h2, 2 * w2))

    @property
    def device(self):
        return self.xs.device

    def dim(self):
        return 4

    def detach(self):
        return S2dTiles(self.xs.detach())

    def __len__(self):
        return self.xs.shape[0]

    def __getitem__(self, idx):
        return S2dTiles(self.xs[idx])

    @staticmethod
    def cat(parts):
        return S2dTiles(torch.cat([p.xs for p in parts], dim=0))


class U8Tiles:
    """A stack of tiles held as the 8-bit images they are: `u8 [T,3,H,W]` uint8, planar (the fp32 tensor's own indexing, one
    byte per element), standing for the fp32 stack `((u8.float() / 255) - 0.5) / 0.5` that ToTensor + Normalize(.5,.5) makes of
    them (RoiBuilder.py:193-210).  What `TilePreprocessor(..., out="u8")` returns and what `Attention.forward` / `forward_bags` /
    `forward_tile_parallel` / `ResNet.forward` of both encoders (`encoder.ResNet`, `alt_resnet.ResNet`) accept in place of the
    fp32 stack in EVERY compute mode: the decode is lossless,
    so outputs and gradients are bit for bit those of the fp32 tensor, at a quarter of its bytes.  A handle on the CPU is
    moved to the module's device as uint8.  Same surface as `S2dTiles`, plus `.float()`."""

    def __init__(self, u8):
        if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8:
            raise ValueError(f"expected a uint8 [T,3,H,W] tensor, got {getattr(u8, 'dtype', type(u8))}")
        if u8.dim() != 4 or u8.shape[1] != 3:
            raise ValueError(f"expected a uint8 [T,3,H,W] tensor, got {tuple(u8.shape)}")
        self.u8 = u8.contiguous()

    @property
    def shape(self):
        return self.u8.shape

    @property
    def device(self):
        return self.u8.device

    def dim(self):
        return 4

    def detach(self):
        return U8Tiles(self.u8.detach())

    def to(self, device):
        return U8Tiles(self.u8.to(device))

    _decode_tables = {}

    @staticmethod
    def decode_table(device):
        """The 256 fp32 values of the decode on `device`: computed once, on the host, and cached per device."""
        dev = torch.device(device)
        tab = U8Tiles._decode_tables.get(dev)
        if tab is None:
            tab = (((torch.arange(256, dtype=torch.uint8).float() / 255) - 0.5) / 0.5).to(dev)
            U8Tiles._decode_tables[dev] = tab
        return tab

    def float(self):
        """The fp32 [T,3,H,W] tensor the handle stands for: `((u8.float() / 255) - 0.5) / 0.5` as the CPU computes it (IEEE
        division — the definition of the decode).  The 256 values are computed once, on the host, and looked up on the
        handle's device: a GPU's own elementwise division need not round as the host's does."""
        return U8Tiles.decode_table(self.u8.device)[self.u8.to(torch.int32)]

    def __len__(self):
        return self.u8.shape[0]

    def __getitem__(self, idx):
        if not isinstance(idx, (torch.Tensor, slice)):
            raise TypeError("U8Tiles are indexed with a tensor or a slice (a selection of tiles)")
        return U8Tiles(self.u8[idx])

    @staticmethod
    def cat(parts):
        return U8Tiles(torch.cat([p.u8 for p in parts], dim=0))


class TilePreprocessor:
    """`update_resolution_and_buffer(resolution)` + the two transform chains for ROIs of `roi_size` pixels."""

    def __init__(self, roi_size, resolution, pad=100, device="cuda"):
        self.roi_size, self.resolution, self.pad = int(roi_size), int(resolution), int(pad)
        lib = L.lib()
        ks = ctypes.c_int(0)
        L.check(lib.mil_resize_plan(self.roi_size, self.resolution, ctypes.byref(ks)), "mil_resize_plan")
        self.ksize = ks.value
        self.bounds_host = np.zeros((self.resolution, 2), dtype=np.int32)
        kk = np.zeros((self.resolution, self.ksize), dtype=np.int32)
        L.check(lib.mil_resize_coeffs(self.roi_size, self.resolution, self.bounds_host.ctypes.data, kk.ctypes.data),
                "mil_resize_coeffs")
        self.kk_host = kk
        self.device = torch.device(device)
        self.bounds_dev = self.kk_dev = None

    def draw_params(self, n_tiles, generator=None):
        """Per tile (top, left, hflip, vflip) as the train chain draws them: RandomCrop offsets uniform in [0, 2*pad],
        each flip with probability 0.5 (RoiBuilder.py:197-201).  int32 [n_tiles, 4] on the host.  The draw order is this
        project's own (tops, lefts, hflips, vflips: four draws of n_tiles), as is that of the colour jitter's parameters
        (`ColorJitter.draw_params`: one draw of [n,4] for the op order, one of [n,4] for the factors), which `SlideBag`
        draws from the same generator after these."""
        p = torch.empty((n_tiles, 4), dtype=torch.int32)
        p[:, 0] = torch.randint(0, 2 * self.pad + 1, (n_tiles,), generator=generator)
        p[:, 1] = torch.randint(0, 2 * self.pad + 1, (n_tiles,), generator=generator)
        p[:, 2] = (torch.rand(n_tiles, generator=generator) < 0.5).to(torch.int32)
        p[:, 3] = (torch.rand(n_tiles, generator=generator) < 0.5).to(torch.int32)
        return p

    def _tables(self, dev):
        if self.bounds_dev is None or self.bounds_dev.device != dev:
            self.bounds_dev = torch.from_numpy(self.bounds_host).to(dev)
            self.kk_dev = torch.from_numpy(self.kk_host).to(dev)
        return self.bounds_dev, self.kk_dev

    def __call__(self, rois, params=None, out="nchw", jitter=None, *, stain=None, affine=None, affine_fill=0, elastic=None, blur=None):
        """rois: uint8 [T,S,S,3] on the GPU (the cached `data_cache` array).  params: int32 [T,4] from `draw_params`
        (train chain) or None (validation chain).  Returns fp32 [T,3,R,R] in [-1,1] (out="nchw": the reference's tensor), or
        — out="u8" — the same tiles as `U8Tiles` (the resized bytes, lossless: every compute mode, any resolution), or
        — out="s2d" — as `S2dTiles` (bf16 space-to-depth: the bf16 compute mode only).  With either handle the fp32 stack is
        never materialised.  jitter: `ColorJitter.draw_params(T)` (or injected `JitterParams`) — the resized bytes are colour-
        jittered (RoiBuilder.py:200) before they are returned (out="u8") or decoded with `U8Tiles.float()` (out="nchw":
        lossless, the values the fp32 chain makes of the jittered bytes); out="s2d" with a jitter raises ValueError.  stain: a
        `StainAffine` (one map, or one per tile) — the resized bytes go through it (`mil_stain_affine_u8`) BEFORE the colour
        jitter; out as with a jitter.  affine: float64 [T,6], one matrix per ROI in its own coordinates (`RandomAffine.draw_params(T,
        roi_size)`) — every ROI is first transformed as Pillow's `transform((S, S), AFFINE, m, BILINEAR, fillcolor=affine_fill)`
        does it (what lies outside the ROI becomes `affine_fill`, a byte or three), then goes through the chain above.  elastic:
        float64 [T,2,gy+3,gx+3], one control lattice per ROI in ROI pixels, before the resize (`ElasticDeform.draw_params(T,
        roi_size)`) — the ROI is deformed in the SAME resampling as `affine` (alone: with the identity matrix), one launch per
        stack of AFFINE_CHUNK (`mil_affine_elastic_u8`).  blur: float64 [T] (or [T,2]: (sx, sy)), one sigma per tile, 0 = untouched
        (`GaussianBlurU8.draw_params(T)`) — the LAST step of the chain, after the stain map and the colour jitter: the bytes are
        those of `GaussianBlurU8.apply` on what the same call returns without `blur=` (Pillow's `GaussianBlur`, bit for bit); out
        as with a jitter."""
        if blur is not None:
            t = rois.shape[0] if isinstance(rois, torch.Tensor) and rois.dim() == 4 else -1
            return self._blurred(out, blur, t, lambda: self(rois, params, "u8", jitter, stain=stain, affine=affine, affine_fill=affine_fill,
                                                            elastic=elastic))
        if jitter is not None or stain is not None:
            t = rois.shape[0] if isinstance(rois, torch.Tensor) and rois.dim() == 4 else -1      # -1: rois are refused below
            return self._jittered(out, jitter, t, lambda: self(rois, params, "u8", affine=affine, affine_fill=affine_fill, elastic=elastic),
                                  stain)
        if affine is not None or elastic is not None:
            if not isinstance(rois, torch.Tensor) or rois.dim() != 4:
                raise ValueError(f"expected uint8 [T,S,S,3] ROIs, got {tuple(getattr(rois, 'shape', ()))}")
            return self._transformed(rois, None, params, out, affine, affine_fill, elastic)
        self._check_out(out)
        if rois.dtype != torch.uint8 or rois.dim() != 4 or rois.shape[3] != 3 or rois.shape[1] != rois.shape[2]:
            raise ValueError(f"expected uint8 [T,S,S,3] ROIs, got {tuple(rois.shape)} {rois.dtype}")
        if rois.shape[1] != self.roi_size:
            raise ValueError(f"ROI size {rois.shape[1]} != {self.roi_size} this preprocessor was planned for")
        if not rois.is_cuda:
            raise RuntimeError("tile pre-processing runs on an AMD GPU only (no CPU fallback)")
        rois = rois.contiguous()
        t = rois.shape[0]
        b, k = self._tables(rois.device)
        params = self._params(params, t, rois.device)
        res, what = self._result(out, t, rois.device)
        fn = getattr(L.lib(), what)
        done = 0
        while done < t:                                      # grid.y limit: 65535 tiles per launch
            n = min(t - done, 65535)
            L.check(fn(rois[done:].data_ptr(), None if params is None else params[done:].data_ptr(),
                       self.bounds_host.ctypes.data, b.data_ptr(), k.data_ptr(), res[done:].data_ptr(),
                       n, self.roi_size, self.pad, self.resolution, L.stream_ptr()), what)
            done += n
        return S2dTiles(res) if out == "s2d" else U8Tiles(res) if out == "u8" else res

    def _jittered(self, out, jitter, t, make_u8, stain=None):
        """`make_u8()` (this preprocessor's U8Tiles of `t` tiles) mapped with `stain`, then jittered with `jitter` (either may
        be None), and returned as `out` asks; the parameters and `out` are checked before anything is launched."""
        from .color_jitter import apply_jitter, checked_params
        from .stain import apply_stain, checked_affine
        self._check_out(out)
        if out == "s2d":
            raise ValueError(f"the {'colour jitter' if jitter is not None else 'stain map'} works on the resized bytes: "
                             "use out='u8' (or 'nchw')")
        if stain is not None:
            checked_affine(stain, t if t >= 0 else 1)
        if jitter is not None and t >= 0:
            jitter = checked_params(jitter, t)
        tiles = make_u8()
        if stain is not None and len(tiles):
            apply_stain(tiles, stain)
        if jitter is not None:
            apply_jitter(tiles, jitter)
        return tiles if out == "u8" else tiles.float()

    def _blurred(self, out, blur, t, make_u8):
        """`make_u8()` (this preprocessor's U8Tiles of `t` tiles, every other step done) blurred with the per-tile sigmas `blur` and
        returned as `out` asks; the sigmas and `out` are checked before anything is launched."""
        from .blur_u8 import apply_blur, checked_sigmas
        self._check_out(out)
        if out == "s2d":
            raise ValueError("the Gaussian blur works on the resized bytes: use out='u8' (or 'nchw')")
        if not isinstance(blur, torch.Tensor) or blur.dim() not in (1, 2):
            raise ValueError(f"blur must be a tensor of per-tile sigmas [T] or [T,2], got {blur!r}")
        if t >= 0:
            checked_sigmas(blur, t, "blur")
        tiles = apply_blur(make_u8(), blur)
        return tiles if out == "u8" else tiles.float()

    def _transformed(self, source, coords, params, out, affine, fill, elastic=None):
        """The `affine=` / `elastic=` path of `__call__` (coords None) and `from_slide`: the windows transformed with
        `ops.affine_windows_u8` — with a lattice, `ops.elastic_windows_u8`: both transforms in one launch — in stacks of at most
        AFFINE_CHUNK, each handed to `__call__`; no array of T * S^2 pixels exists.  Everything is checked before the first
        launch."""
        from . import ops
        self._check_out(out)
        src, off, _ = source_windows(source, coords, self.roi_size)
        t = int(off.numel())
        m = None if affine is None else ops.affine_matrices(affine, t, "affine")
        lat = None if elastic is None else ops.elastic_lattice(elastic, t, "elastic")
        ops.affine_fill(fill)
        if not src.is_cuda:
            raise RuntimeError("tile pre-processing runs on an AMD GPU only (no CPU fallback)")
        params = self._params(params, t, src.device)
        if coords is not None:
            width = int(src.shape[1])
            coords = torch.stack([off // 3 // width, off // 3 % width], dim=1)                    # (row, col), int64
        parts = []
        for lo in range(0, t, AFFINE_CHUNK):
            hi = min(t, lo + AFFINE_CHUNK)
            if lat is not None:
                win = ops.elastic_windows_u8(src[lo:hi] if coords is None else src, None if coords is None else coords[lo:hi],
                                             None if m is None else m[lo:hi], lat[lo:hi], fill, self.roi_size)
            elif coords is None:
                win = ops.affine_windows_u8(src[lo:hi], None, m[lo:hi], fill)
            else:
                win = ops.affine_windows_u8(src, coords[lo:hi], m[lo:hi], fill, self.roi_size)
            parts.append(self(win, None if params is None else params[lo:hi], out))
        if not parts:
            res = self._result(out, 0, src.device)[0]
            return S2dTiles(res) if out == "s2d" else U8Tiles(res) if out == "u8" else res
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=0) if out == "nchw" else type(parts[0]).cat(parts)

    def _check_out(self, out):
        if out not in ("nchw", "s2d", "u8"):
            raise ValueError("out must be 'nchw', 's2d' or 'u8'")
        if out == "s2d" and self.resolution % 2:
            raise ValueError("the space-to-depth output needs an even resolution")

    def _params(self, params, t, dev):
        if params is None:
            return None
        params = torch.as_tensor(params, dtype=torch.int32)
        if tuple(params.shape) != (t, 4):
            raise ValueError("params must be int32 [T,4]")
        if t and (int(params[:, :2].min()) < 0 or int(params[:, :2].max()) > 2 * self.pad):
            raise ValueError("crop offsets must lie in [0, 2*pad]")
        return params.to(dev).contiguous()

    def _result(self, out, t, dev):
        """(the output tensor of `t` tiles, the name of the stack entry point that fills it)."""
        r = self.resolution
        if out == "s2d":
            return torch.empty((t, r // 2, r // 2, 16), dtype=torch.bfloat16, device=dev), "mil_tile_preprocess_s2d"
        if out == "u8":
            return torch.empty((t, 3, r, r), dtype=torch.uint8, device=dev), "mil_tile_preprocess_u8"
        return torch.empty((t, 3, r, r), dtype=torch.float32, device=dev), "mil_tile_preprocess"

    def from_slide(self, slide, coords, params=None, out="nchw", jitter=None, *, stain=None, affine=None, affine_fill=0, elastic=None,
                   blur=None):
        """The same chains on windows of a slide that stays where it is (`array_read_region`, RoiBuilder.py:117-124, then
        :193-210): slide uint8 [H,W,3] on the GPU (any contiguous view, whatever its alignment), coords int [T,2] of (row, col)
        of `roi_size` windows.  No [T,S,S,3] stack is made: the kernel reads the windows in place (mil_tile_preprocess_win*).
        params / out / the return value as in `__call__`, bit for bit what `__call__` returns for the same windows copied into a
        stack.  A window outside the slide raises ValueError, a slide on the CPU RuntimeError, both before any launch.  With
        coords=None `slide` is an ROI stack [n,S,S,3]: the same kernel at row pitch 3S.  jitter, stain: as in `__call__`.
        affine: float64 [T,6], one matrix per window in WINDOW coordinates (`RandomAffine.draw_params(T, roi_size)`).  Every
        window is first transformed — reading the SLIDE, so a rotated window shows the tissue beside it and only what lies
        outside the slide becomes `affine_fill` —, then goes through the chain: bit for bit
        `Image.fromarray(slide).transform((S, S), Image.AFFINE, m + origin, Image.BILINEAR, fillcolor=affine_fill)` followed by
        `__call__` on those windows (origin: col added to a2, row to a5).  The transformed windows are made AFFINE_CHUNK at a
        time.  elastic: float64 [T,2,gy+3,gx+3], one control lattice per window in window pixels (`ElasticDeform.draw_params(T,
        roi_size)`): the deformation is one more term of the same source coordinate, so with both `affine` and `elastic` a window
        is still resampled once, one launch per chunk, reading the slide.  blur: as in `__call__`, the last step."""
        if blur is not None:
            t = int(source_windows(slide, coords, self.roi_size)[1].numel())
            return self._blurred(out, blur, t,
                                 lambda: self.from_slide(slide, coords, params, "u8", jitter, stain=stain, affine=affine,
                                                         affine_fill=affine_fill, elastic=elastic))
        if jitter is not None or stain is not None:
            t = int(source_windows(slide, coords, self.roi_size)[1].numel())
            return self._jittered(out, jitter, t,
                                  lambda: self.from_slide(slide, coords, params, "u8", affine=affine, affine_fill=affine_fill,
                                                          elastic=elastic), stain)
        if affine is not None or elastic is not None:
            return self._transformed(slide, coords, params, out, affine, affine_fill, elastic)
        self._check_out(out)
        src, off, pitch = source_windows(slide, coords, self.roi_size)
        if not src.is_cuda:
            raise RuntimeError("tile pre-processing runs on an AMD GPU only (no CPU fallback)")
        t = int(off.numel())
        b, k = self._tables(src.device)
        params = self._params(params, t, src.device)
        res, what = self._result(out, t, src.device)
        what = what.replace("mil_tile_preprocess", "mil_tile_preprocess_win")
        fn = getattr(L.lib(), what)
        off_dev = off.to(src.device)
        done = 0
        while done < t:                                      # grid.y limit: 65535 windows per launch
            n = min(t - done, 65535)
            L.check(fn(src.data_ptr(), src.numel(), off_dev[done:].data_ptr(), pitch,
                       None if params is None else params[done:].data_ptr(), self.bounds_host.ctypes.data, b.data_ptr(),
                       k.data_ptr(), res[done:].data_ptr(), n, self.roi_size, self.pad, self.resolution, L.stream_ptr()), what)
            done += n
        return S2dTiles(res) if out == "s2d" else U8Tiles(res) if out == "u8" else res


def source_windows(source, coords, s):
    """The windows of `s` pixels of a source as mil_roi_stats / mil_tile_preprocess_win* address them: (contiguous source, int64
    CPU byte offsets [n] of each window's first pixel, row pitch in bytes).  source: uint8, a slide [H,W,3] with coords (int
    [n,2] of (row, col)) or an ROI stack [n,s,s,3] with coords=None.  Needs no device."""
    if not isinstance(source, torch.Tensor) or source.dtype != torch.uint8:
        raise ValueError(f"expected a uint8 tensor, got {getattr(source, 'dtype', type(source))}")
    if source.dim() == 3 and source.shape[2] == 3 and coords is not None:
        h, w = int(source.shape[0]), int(source.shape[1])
        c = coords.detach().cpu().numpy() if isinstance(coords, torch.Tensor) else np.asarray(coords)
        if c.size and c.dtype.kind not in "iu":
            raise ValueError("coords must be integers")
        c = torch.as_tensor(c.astype(np.int64).reshape(-1, 2))
        if c.numel() and (int(c.min()) < 0 or int(c[:, 0].max()) + s > h or int(c[:, 1].max()) + s > w):
            raise ValueError(f"a {s} x {s} window does not lie inside the {h} x {w} slide")
        return source.contiguous(), (c[:, 0] * w + c[:, 1]) * 3, 3 * w
    if source.dim() == 4 and source.shape[3] == 3 and coords is None:
        if source.shape[1] != s or source.shape[2] != s:
            raise ValueError(f"expected [n,{s},{s},3] ROIs, got {tuple(source.shape)}")
        return source.contiguous(), torch.arange(source.shape[0], dtype=torch.int64) * (3 * s * s), 3 * s
    raise ValueError(f"expected a slide [H,W,3] (with coords) or an ROI stack [n,S,S,3] (without), got {tuple(source.shape)}")
