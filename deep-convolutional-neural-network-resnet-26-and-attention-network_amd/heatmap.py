"""Attention heat maps rendered on the device from the resident slide: the data the reference's `visualize()` ->
`create_map()` (gbm/classify_combined.py:142-218) draws on its five tissue axes (`tissue_plots`, :185), as five uint8 RGB
panels at thumbnail scale.

create_map takes every kept ROI as pixels (`get_inference_data()`'s third item, [T,1200,1200,3]), `imshow`s each and adds one
coloured rectangle per tile and axis.  Here one kernel (csrc/heatmap.hip, `mil_heatmap_render`) reads every kept window once
where it lies in the slide, box-reduces it by `scale` and blends the attention colours; what leaves the device is
`[5, H//scale, W//scale, 3]` bytes:

  panel 0      the tissue under the mean map `A_ALL = (1/3)*(A[0]+A[1]+A[2])` as jet rectangles, alpha 0.3   (ax[0,0])
  panel 1      per tile, `Fterm` viewed 8 x 10 through imshow's defaults (viridis, per-image autoscale),
               inset by 16 slide pixels                                                                       (ax[0,1])
  panels 2-4   the maps `A[0..2]` as jet rectangles, alpha 0.9, on white                                      (ax[1,0..2])

The colour INDICES are computed on the host with the reference's own float32 statements (`attention_indices`,
`feature_indices`); the kernel's arithmetic is integer (include/mil_hip.h states it), so a picture is reproducible bit for bit.
matplotlib's vector rasterisation of the PDF is not reproduced, and the sixth axis (`M1`, three numbers) is
`visualize_terms`'s.
"""
import numpy as np
import torch

from . import _lib as L
from .train import _minmax_f32

# `cm.jet(np.linspace(0, 1, 105), bytes=True)[:, :3]` (`cmap_lin` of gbm/classify_combined.py:172 as bytes) and
# `cm.viridis(np.arange(256), bytes=True)[:, :3]` as matplotlib 3.10.8 returns them — carried as data: the package does not
# import matplotlib.  tests/golden/make_heatmap_golden.py records the same tables, tests/test_cpu_heatmap.py compares.
_JET105_HEX = (
    "00007f00008800009100009f0000a80000b60000bf0000cc0000d50000e30000ec0000fa0000ff0000ff0008ff0010ff001cff0024ff0030ff0038ff"
    "0044ff004cff0058ff0060ff006cff0074ff0080ff0088ff0090ff009cff00a4ff00b0ff00b8ff00c4ff00ccff00d8ff00e0fa05ecf10cf4ea15ffe1"
    "1cffda22ffd42cffca32ffc33cffba42ffb34cffaa53ffa35cff9a63ff936cff8973ff837cff7983ff7389ff6c93ff639aff5ca3ff53aaff4cb3ff42"
    "baff3cc3ff32caff2cd4ff22daff1ce4ff12eaff0cf1fc05faf000ffe900ffde00ffd700ffcb00ffc400ffb900ffb100ffa600ff9f00ff9400ff8c00"
    "ff8500ff7a00ff7300ff6700ff6000ff5500ff4d00ff4200ff3b00ff3000ff2800ff1d00ff1600fa0f00ec0300e30000d50000cc0000bf0000b60000"
    "a800009f00009100008800007f0000")
_VIRIDIS256_HEX = (
    "44015444025544035745055845065a45085b46095c460b5e460c5f460e61470f6247116347126547146647156747166947186a48196b481a6c481c6e"
    "481d6f481e70482071482172482273482374472575472676472777472878472a79472b7a472c7b462d7c462f7c46307d46317e45327f45347f453580"
    "453681443781443982433a83433b83433c84423d84423e854240854141864142864043874044873f45873f47883e48883e49893d4a893d4b893d4c89"
    "3c4d8a3c4e8a3b508a3b518a3a528b3a538b39548b39558b38568b38578c37588c37598c365a8c365b8c355c8c355d8c345e8d345f8d33608d33618d"
    "32628d32638d31648d31658d31668d30678d30688d2f698d2f6a8d2e6b8e2e6c8e2e6d8e2d6e8e2d6f8e2c708e2c718e2c728e2b738e2b748e2a758e"
    "2a768e2a778e29788e29798e287a8e287a8e287b8e277c8e277d8e277e8e267f8e26808e26818e25828e25838d24848d24858d24868d23878d23888d"
    "23898d22898d228a8d228b8d218c8d218d8c218e8c208f8c20908c20918c1f928c1f938b1f948b1f958b1f968b1e978a1e988a1e998a1e998a1e9a89"
    "1e9b891e9c891e9d881e9e881e9f881ea0871fa1871fa2861fa38620a48520a58521a68521a78422a78423a88323a98224aa8225ab8126ac8127ad80"
    "28ae7f29af7f2ab07e2bb17d2cb17d2eb27c2fb37b30b47a32b57a33b67935b77836b87738b97639b9763bba753dbb743ebc7340bd7242be7144be70"
    "45bf6f47c06e49c16d4bc26c4dc26b4fc36951c46853c56755c66657c66559c7645bc8625ec96160c96062ca5f64cb5d67cc5c69cc5b6bcd596dce58"
    "70ce5672cf5574d05477d05279d1517cd24f7ed24e81d34c83d34b86d44988d5478bd5468dd64490d64392d74195d73f97d83e9ad83c9dd93a9fd938"
    "a2da37a5da35a7db33aadb32addc30afdc2eb2dd2cb5dd2bb7dd29bade27bdde26bfdf24c2df22c5df21c7e01fcae01ecde01dcfe11cd2e11bd4e11a"
    "d7e219dae218dce218dfe318e1e318e4e318e7e419e9e419ece41aeee51bf1e51cf3e51ef6e61ff8e621fae622fde724")
JET105 = np.frombuffer(bytes.fromhex(_JET105_HEX), dtype=np.uint8).reshape(105, 3)
VIRIDIS256 = np.frombuffer(bytes.fromhex(_VIRIDIS256_HEX), dtype=np.uint8).reshape(256, 3)


def attention_indices(A1):
    """The index into `cmap_lin` of every rectangle create_map draws (gbm/classify_combined.py:178-202), int16 [4,T] on the
    CPU: row 0 for the mean map `A_ALL`, rows 1-3 for `A[0..2]`; -1 where it draws none (`if att_weights_norm[i] > 0.0`).
    `A1` is `visualize_terms(output)["A1"]`, [3,T].  The reference's statements run literally on float32 CPU tensors, so the
    rounding is theirs.  ValueError for a NaN and for an index above 104 (`int(nan)` / `cmap_lin[105]` raise upstream)."""
    A = torch.as_tensor(A1).detach().float().cpu()
    if A.dim() != 2 or A.shape[0] != 3:
        raise ValueError(f"A1 must be [3,T], got {tuple(A.shape)}")
    A_ALL = (1 / 3) * (A[0] + A[1] + A[2])
    att = torch.stack([100 * A_ALL, 100 * A[0], 100 * A[1], 100 * A[2]])
    if bool(torch.isnan(att).any()):
        raise ValueError("the attention map holds NaNs (a constant wROIs array normalises to 0/0)")
    drawn = att > 0.0
    if bool((drawn & (att >= 105.0)).any()):
        raise ValueError("an attention value above 1.05 has no colour: cmap_lin has 105 entries")
    idx = torch.where(drawn, att, torch.zeros_like(att)).to(torch.int64)          # int(.): truncation
    return torch.where(drawn, idx, torch.full_like(idx, -1)).to(torch.int16)


def feature_indices(Fterm):
    """The viridis index of every cell of `imshow(B[i])` (gbm/classify_combined.py:203; B[i] = Fterm[i] viewed 8 x 10), uint8
    [T,80] on the CPU: per tile `Normalize()` with autoscaling (`train._minmax_f32`), then matplotlib's `Colormap.__call__`
    on the float32 array — times 256 in float32, truncated, 256 mapped to 255.  A constant tile gives index 0.  ValueError
    for a NaN or an infinity."""
    F = torch.as_tensor(Fterm).detach().float().cpu()
    if F.dim() != 2 or F.shape[1] != 80:
        raise ValueError(f"Fterm must be [T,80], got {tuple(F.shape)}")
    if not bool(torch.isfinite(F).all()):
        raise ValueError("Fterm holds NaNs or infinities")
    out = np.zeros((F.shape[0], 80), dtype=np.uint8)
    for i in range(F.shape[0]):
        xa = _minmax_f32(F[i])
        xa *= 256
        xa[xa == 256] = 255
        out[i] = xa.astype(np.int64)
    return torch.from_numpy(out)


def _owned_blocks_collide(oy, ox, n):
    """Whether two of the n x n blocks with top-left corners (oy[i], ox[i]) share a pixel.  On the grid of n x n cells two
    corners in one cell always collide, and a block can only meet blocks whose corner lies in a neighbouring cell."""
    if len(oy) < 2:
        return False
    cy, cx = oy // n, ox // n + 1
    width = int(cx.max()) + 2
    key = cy * width + cx
    order = np.argsort(key, kind="stable")
    ks = key[order]
    if bool((ks[1:] == ks[:-1]).any()):
        return True
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        want = key + dy * width + dx
        at = np.minimum(np.searchsorted(ks, want), len(ks) - 1)
        j = order[at]
        hit = (ks[at] == want) & (np.abs(oy[j] - oy) < n) & (np.abs(ox[j] - ox) < n)
        if bool(hit.any()):
            return True
    return False


class AttentionMapRenderer:
    """`roi_size`: the reference's `params['roi_size']` (its hard-coded 1200 in create_map); `scale`: slide pixels per output
    pixel, a divisor of roi_size; `inset`: the 16 slide pixels by which create_map shrinks the feature image of a tile (:203);
    `alpha_tissue` / `alpha_map`: the rectangles' alpha on ax[0,0] / ax[1,0..2] (:192-201), applied in 1/256ths
    (`round(alpha * 256)`: 77 and 230)."""

    def __init__(self, roi_size=1200, scale=16, inset=16, alpha_tissue=0.3, alpha_map=0.9):
        self.roi_size, self.scale, self.inset = int(roi_size), int(scale), int(inset)
        if self.roi_size < 1 or self.scale < 1 or self.inset < 0:
            raise ValueError("roi_size and scale must be positive, inset non-negative")
        self.q_tissue, self.q_map = int(round(alpha_tissue * 256)), int(round(alpha_map * 256))
        if not (0 <= self.q_tissue <= 256 and 0 <= self.q_map <= 256):
            raise ValueError("an alpha lies in [0, 1]")
        self._luts = {}

    def _tables(self, device):
        if device not in self._luts:
            self._luts[device] = (torch.from_numpy(JET105.copy()).to(device), torch.from_numpy(VIRIDIS256.copy()).to(device))
        return self._luts[device]

    def render(self, slide, coords, A1, Fterm=None):
        """slide: uint8 [H,W,3] on the GPU; coords: int [T,2] of (row, col), the kept windows (`SlideBag.coords`, the
        reference's `raster`); A1: `visualize_terms(output)["A1"]`, [3,T]; Fterm: `output["Fterm"]`, [T,80], or None (panel
        1 then stays white).  Returns uint8 [5, H//scale, W//scale, 3] on the slide's device, white where no window lies;
        window (row, col) covers the output pixels from (row//scale, col//scale) on."""
        jet_idx = attention_indices(A1)
        feat_idx = None if Fterm is None else feature_indices(Fterm)
        c = self._check(slide, coords, jet_idx, feat_idx, None)
        canvas = torch.full((5, slide.shape[0] // self.scale, slide.shape[1] // self.scale, 3), 255, dtype=torch.uint8,
                            device=slide.device)
        return self._launch(canvas, slide, c, jet_idx, feat_idx)

    def _check(self, slide, coords, jet_idx, feat_idx, canvas):
        """Every refusal, on the host and before any launch; returns the coordinates as int64 numpy [T,2]."""
        s, d = self.roi_size, self.scale
        if s % d != 0:
            raise ValueError(f"scale {d} does not divide roi_size {s}")
        if not isinstance(slide, torch.Tensor) or slide.dtype != torch.uint8 or slide.dim() != 3 or slide.shape[2] != 3:
            raise ValueError(f"expected a uint8 [H,W,3] slide, got {getattr(slide, 'dtype', type(slide))} "
                             f"{tuple(getattr(slide, 'shape', ()))}")
        c = np.asarray(coords.cpu() if isinstance(coords, torch.Tensor) else coords)
        if c.size and c.dtype.kind not in "iu":
            raise ValueError("coords must be integers")
        c = c.astype(np.int64).reshape(-1, 2)
        t, (h, w) = len(c), slide.shape[:2]
        if not isinstance(jet_idx, torch.Tensor) or jet_idx.dtype != torch.int16 or tuple(jet_idx.shape) != (4, t):
            raise ValueError(f"expected int16 [4,{t}] jet indices (one column per window), got "
                             f"{getattr(jet_idx, 'dtype', type(jet_idx))} {tuple(getattr(jet_idx, 'shape', ()))}")
        if feat_idx is not None and (not isinstance(feat_idx, torch.Tensor) or feat_idx.dtype != torch.uint8
                                     or tuple(feat_idx.shape) != (t, 80)):
            raise ValueError(f"expected uint8 [{t},80] feature indices, got {getattr(feat_idx, 'dtype', type(feat_idx))} "
                             f"{tuple(getattr(feat_idx, 'shape', ()))}")
        if t and int(jet_idx.max()) > 104:
            raise ValueError("a jet index above 104")
        if c.size and (c.min() < 0 or c[:, 0].max() + s > h or c[:, 1].max() + s > w):
            raise ValueError(f"a {s} x {s} window does not lie inside the {h} x {w} slide")
        if _owned_blocks_collide(c[:, 0] // d, c[:, 1] // d, s // d):
            raise ValueError("two windows would own the same output pixel")
        if canvas is not None:
            want = (5, h // d, w // d, 3)
            if not isinstance(canvas, torch.Tensor) or canvas.dtype != torch.uint8 or tuple(canvas.shape) != want \
                    or not canvas.is_contiguous() or canvas.device != slide.device:
                raise ValueError(f"expected a contiguous uint8 canvas {want} on the slide's device")
        if not slide.is_cuda:
            raise RuntimeError("heat-map rendering runs on an AMD GPU only (no CPU fallback)")
        return c

    def render_into(self, canvas, slide, coords, jet_idx, feat_idx=None):
        """The lower call: writes the pixels the windows own into the caller's `canvas` (uint8 [5, H//scale, W//scale, 3],
        contiguous, on the slide's device) and touches no other.  jet_idx: int16 [4,T] (`attention_indices`; -1 = no
        rectangle); feat_idx: uint8 [T,80] (`feature_indices`) or None — panel 1 is then not written.  Returns canvas."""
        return self._launch(canvas, slide, self._check(slide, coords, jet_idx, feat_idx, canvas), jet_idx, feat_idx)

    def _launch(self, canvas, slide, c, jet_idx, feat_idx):
        t = len(c)
        if t == 0:
            return canvas
        src, dev = slide.contiguous(), slide.device
        h, w = int(src.shape[0]), int(src.shape[1])
        cc = torch.from_numpy(c)
        off = ((cc[:, 0] * w + cc[:, 1]) * 3).to(dev)
        pos = (cc // self.scale).to(torch.int32).contiguous().to(dev)
        jet, viridis = self._tables(dev)
        jidx = jet_idx.contiguous().to(dev)
        fidx = None if feat_idx is None else feat_idx.contiguous().to(dev)
        L.check(L.lib().mil_heatmap_render(src.data_ptr(), src.numel(), off.data_ptr(), 3 * w, t, self.roi_size, self.scale,
                                           pos.data_ptr(), jidx.data_ptr(), L.ptr(fidx), jet.data_ptr(), viridis.data_ptr(),
                                           self.inset, self.q_tissue, self.q_map, canvas.data_ptr(), canvas.shape[1],
                                           canvas.shape[2], L.stream_ptr()), "mil_heatmap_render")
        return canvas
