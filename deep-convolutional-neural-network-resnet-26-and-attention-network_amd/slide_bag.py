"""One slide's bag of tiles without a data cache: the device-side counterpart of the reference's `RoiBuilder` in state
VALID-READY (RoiBuilder.py:128-284).  The reference keeps two caches per slide, the kept coordinates (`coor_cache`) and the kept
ROIs themselves (`data_cache`, [T,1200,1200,3] uint8 — 10.8 GB at its 2500-tile cap), because every epoch re-reads the ROIs
from disk.  Here the slide is resident in HBM, `TilePreprocessor.from_slide` reads each window where it lies, and the only
thing a bag holds besides the slide is the coordinates: slide -> kept coordinates -> `U8Tiles` -> `Attention`, with nothing of
size T*S*S in between.  Reading slide files and `.npy` caches stays with the caller.
"""
import numpy as np
import torch

from .preprocess import TilePreprocessor
from .roi_select import RoiSelector


class SlideBag:
    """slide: uint8 [H,W,3] (on the GPU for everything but the host bookkeeping).  `roi_size`, `padding`: the reference's
    `params['roi_size']` / `params['padding']`; `pad`: its Pad(100); `max_tiles`: the hard limit of `get_train_data`
    (RoiBuilder.py:230).  `selector`: a `RoiSelector` of the same roi_size (default: the reference's constants).  `coords`:
    a loaded `coor_cache`, int [T,2] of (row, col) — `build()` then has nothing to do.  `color_jitter`: a `ColorJitter` —
    `get_train_data` then jitters its tiles (RoiBuilder.py:200); validation and inference data never are.
    `stain_normalizer`: a `StainNormalizer` — train, validation and inference tiles are mapped onto its target appearance with
    the bag's own fit, made once, at first use, on an evenly strided subset of at most 256 of its windows taken through the flat
    chain at the resolution of that moment, and kept as `stain_fit`.  `stain_jitter`: a `StainJitter` — train tiles only.  With
    both, normalisation and jitter are composed into one `StainAffine`: one launch, one rounding to bytes, before the colour
    jitter.  `affine`: a `RandomAffine` — every window of `get_train_data` is rotated / sheared / scaled / shifted about its
    centre BEFORE the train chain, reading the slide itself (the tissue beside the window, not a fill colour, fills the corners;
    only what lies outside the slide gets `affine.fill`); validation and inference data never are.  `elastic`: an `ElasticDeform`
    — every window of `get_train_data` is deformed with a drawn control lattice, in the same resampling as `affine` (one launch
    per chunk of windows; without an `affine` the fill is `elastic.fill`); validation and inference data never are.  `blur`: a
    `GaussianBlurU8` — every tile of `get_train_data` is blurred with a drawn sigma (0: left as it is), the LAST step of the train
    chain, after the stain map and the colour jitter; validation and inference data never are.

    Unlike the reference, a bag with no kept window returns an EMPTY stack [0,3,R,R] from the three `get_*` methods, not the
    `torch.zeros(20,3,128,128)` placeholder of RoiBuilder.py:236,257 (which has neither the bag's resolution nor any tile of
    it); the caller decides what to do with a slide without tissue."""

    def __init__(self, slide, roi_size=1200, padding=0, resolution=None, pad=100, max_tiles=2500, selector=None, coords=None,
                 color_jitter=None, *, stain_normalizer=None, stain_jitter=None, affine=None, elastic=None, blur=None):
        if not isinstance(slide, torch.Tensor) or slide.dtype != torch.uint8 or slide.dim() != 3 or slide.shape[2] != 3:
            raise ValueError(f"expected a uint8 [H,W,3] slide, got {getattr(slide, 'dtype', type(slide))} "
                             f"{tuple(getattr(slide, 'shape', ()))}")
        self.roi_size, self.padding, self.pad, self.max_tiles = int(roi_size), int(padding), int(pad), int(max_tiles)
        if self.roi_size < 1 or self.padding < 0 or self.pad < 0 or self.max_tiles < 1:
            raise ValueError("roi_size and max_tiles must be positive, padding and pad non-negative")
        self.selector = RoiSelector(self.roi_size, self.padding) if selector is None else selector
        if self.selector.roi_size != self.roi_size:
            raise ValueError(f"the selector cuts {self.selector.roi_size}-pixel windows, the bag {self.roi_size}-pixel ones")
        self.slide = slide
        self.color_jitter = color_jitter
        self.stain_normalizer, self.stain_jitter = stain_normalizer, stain_jitter
        self.affine = affine
        self.elastic = elastic
        self.blur = blur
        self.stain_fit = None                                # the bag's StainFit once a stain_normalizer made it
        self.coords = None                                   # coor_cache: int64 [T,2] numpy (row, col) once built
        if coords is not None:
            c = np.asarray(coords.cpu() if isinstance(coords, torch.Tensor) else coords)
            if c.size and c.dtype.kind not in "iu":
                raise ValueError("coords must be integers")
            c = c.astype(np.int64).reshape(-1, 2)
            s, (h, w) = self.roi_size, slide.shape[:2]
            if c.size and (c.min() < 0 or c[:, 0].max() + s > h or c[:, 1].max() + s > w):
                raise ValueError(f"a {s} x {s} window does not lie inside the {h} x {w} slide")
            self.coords = c
        self.resolution = self.prep = None
        if resolution is not None:
            self.update_resolution(resolution)

    @property
    def ntiles(self):
        """The number of kept windows; -1 before `build()`, as the reference's `params['ntiles']`."""
        return -1 if self.coords is None else len(self.coords)

    def build(self):
        """Runs the tissue selection over the slide's raster (RoiBuilder.py:153-169) unless `coords=` supplied its result."""
        if self.coords is None:
            self.coords = self.selector.kept(self.slide)
        return True

    def update_resolution(self, resolution):
        """`update_resolution_and_buffer` (RoiBuilder.py:182-212): the size of the tiles the `get_*` methods return."""
        self.resolution = int(resolution)
        self.prep = TilePreprocessor(self.roi_size, self.resolution, pad=self.pad, device=self.slide.device)

    def _ready(self):
        if self.coords is None or self.prep is None:
            raise RuntimeError("call build() and update_resolution() first "
                               f"(ntiles = {self.ntiles}, resolution = {self.resolution})")

    def choose(self, generator=None, choice=None):
        """The windows a training draw uses, as indices into `coords` (RoiBuilder.py:230-231): all of them, in order, when at
        most `max_tiles` were kept (returns None; `choice` is then not used); otherwise `max_tiles` distinct ones, drawn
        without replacement from `generator` or — `choice` — injected by the caller, in the order given."""
        n = self.ntiles
        if n < 0:
            raise RuntimeError("call build() first")
        if n <= self.max_tiles:
            return None
        if choice is None:
            return torch.randperm(n, generator=generator)[:self.max_tiles].numpy()
        idx = np.asarray(choice.cpu() if isinstance(choice, torch.Tensor) else choice).astype(np.int64).reshape(-1)
        if len(idx) != self.max_tiles or len(np.unique(idx)) != len(idx) or idx.min() < 0 or idx.max() >= n:
            raise ValueError(f"choice must hold {self.max_tiles} distinct indices below {n}")
        return idx

    def _stain(self, n, stain_jitter_params=None):
        """The `StainAffine` the bag applies to a stack of `n` of its tiles (None: none): the normaliser's map with the bag's
        fit — made here, once — followed by the stain jitter's per-tile maps, composed."""
        if n == 0 or (self.stain_normalizer is None and stain_jitter_params is None):
            return None
        aff = None
        if self.stain_normalizer is not None:
            if self.stain_fit is None:
                sub = self.coords[::-(-len(self.coords) // 256)]
                self.stain_fit = self.stain_normalizer.fit(self.prep.from_slide(self.slide, sub, None, "u8"))
            aff = self.stain_normalizer.affine(self.stain_fit)
        if stain_jitter_params is not None:
            jit = self.stain_jitter.affine(stain_jitter_params, n)
            aff = jit if aff is None else aff.then(jit)
        return aff

    def get_train_data(self, generator=None, choice=None, params=None, out="u8", jitter_params=None, *, stain_jitter_params=None,
                       affine_params=None, elastic_params=None, blur_params=None):
        """`get_train_data` (RoiBuilder.py:215-238): the cap of `choose`, then the train chain on the chosen windows with
        `draw_params(generator)` or the injected `params` [n,4].  A bag with a `color_jitter` then jitters the tiles with
        `color_jitter.draw_params(n, generator)` (drawn after the crop / flip parameters) or the injected `jitter_params`;
        a bag without one refuses `jitter_params`.  A bag with a `stain_jitter` draws `stain_jitter.draw_params(n, generator)`
        after those (or takes the injected `stain_jitter_params`); the stain map comes before the colour jitter.  A bag
        without one refuses `stain_jitter_params`.  A bag with an `affine` draws `affine.draw_params(n, roi_size, generator)`
        LAST, after every draw above (seeded sequences of bags without one do not move), or takes the injected `affine_params`
        (float64 [n,6], window coordinates); the windows are transformed before the train chain.  A bag without one refuses
        `affine_params`.  A bag with an `elastic` draws `elastic.draw_params(n, roi_size, generator)` after that, or
        takes the injected `elastic_params` (float64 [n,2,gy+3,gx+3], window pixels); a bag without one refuses
        `elastic_params`.  A bag with a `blur` draws `blur.draw_params(n, generator)` after that — the very last draw, so a
        bag without one consumes the random numbers it always did — or takes the injected `blur_params` (float64 [n] of sigmas, 0 =
        untouched); the blur is the last step of the chain.  A bag without one refuses `blur_params`."""
        self._ready()
        if blur_params is not None and self.blur is None:
            raise ValueError("blur_params given to a bag made without blur=")
        if elastic_params is not None and self.elastic is None:
            raise ValueError("elastic_params given to a bag made without elastic=")
        if affine_params is not None and self.affine is None:
            raise ValueError("affine_params given to a bag made without affine=")
        if jitter_params is not None and self.color_jitter is None:
            raise ValueError("jitter_params given to a bag made without color_jitter=")
        if stain_jitter_params is not None and self.stain_jitter is None:
            raise ValueError("stain_jitter_params given to a bag made without stain_jitter=")
        idx = self.choose(generator, choice)
        c = self.coords if idx is None else self.coords[idx]
        if params is None:
            params = self.prep.draw_params(len(c), generator)
        if self.color_jitter is not None and jitter_params is None:
            jitter_params = self.color_jitter.draw_params(len(c), generator)
        if self.stain_jitter is not None and stain_jitter_params is None and len(c):
            stain_jitter_params = self.stain_jitter.draw_params(len(c), generator)
        if self.affine is not None and affine_params is None:
            affine_params = self.affine.draw_params(len(c), self.roi_size, generator)
        if self.elastic is not None and elastic_params is None:
            elastic_params = self.elastic.draw_params(len(c), self.roi_size, generator)
        if self.blur is not None and blur_params is None:
            blur_params = self.blur.draw_params(len(c), generator)
        kw = {}                                              # only what the bag was made with: a plain bag makes the call it made
        if self.affine is not None or self.elastic is not None:
            kw.update(affine=affine_params, affine_fill=(self.elastic if self.affine is None else self.affine).fill)
        if self.elastic is not None:
            kw.update(elastic=elastic_params)
        if self.blur is not None:
            kw.update(blur=blur_params)
        return self.prep.from_slide(self.slide, c, params, out, jitter=jitter_params, stain=self._stain(len(c), stain_jitter_params), **kw)

    def get_validation_data(self, out="u8"):
        """`get_validation_data` (RoiBuilder.py:240-259): the flat chain on every kept window."""
        self._ready()
        return self.prep.from_slide(self.slide, self.coords, None, out, stain=self._stain(len(self.coords)))

    def get_inference_data(self, out="u8"):
        """`get_inference_data` (RoiBuilder.py:261-284): (tiles of the flat chain, their coordinates).  The reference's third
        item, the ROIs themselves (for `imshow` in its `visualize`), is `rois(indices)` for the ones that are drawn."""
        self._ready()
        return self.prep.from_slide(self.slide, self.coords, None, out, stain=self._stain(len(self.coords))), self.coords.copy()

    def attention_maps(self, output, scale, features=True, **renderer_args):
        """The five tissue panels of the reference's `visualize` -> `create_map` (gbm/classify_combined.py:142-218) for one
        forward's `output` dict over this bag's windows, uint8 [5, H//scale, W//scale, 3] on the slide's device
        (`AttentionMapRenderer.render`): `A1` of `visualize_terms(output)` colours the rectangles, `output["Fterm"]` the
        per-tile feature images (`features=False`: that panel stays white).  `renderer_args`: inset / alpha_tissue /
        alpha_map of `AttentionMapRenderer`.  The ROIs themselves are not materialised."""
        if self.coords is None:
            raise RuntimeError("call build() first")
        from .heatmap import AttentionMapRenderer
        from .train import visualize_terms
        renderer = AttentionMapRenderer(self.roi_size, scale, **renderer_args)
        return renderer.render(self.slide, self.coords, visualize_terms(output)["A1"], output["Fterm"] if features else None)

    def attribution_maps(self, maps, scale, **mosaic_args):
        """The slide mosaic of per-tile attribution maps over this bag's windows, uint8 [2, H//scale, W//scale, 3] on the
        slide's device (`AttributionMosaic.render`): panel 0 the maps on white, panel 1 the maps over the tissue.  maps: uint8
        [T,Hm,Wm] or [T,Hm,Wm,3], one per kept window in the order of `coords` — what `AttributionRenderer` or
        `TileGradCam.maps` made of the tiles of the FLAT chain (`get_inference_data` / `get_validation_data`).  Train tiles
        are cropped and flipped: their pixels do not lie where the window lies, and their maps do not belong here.
        `mosaic_args`: cmap / alpha / alpha_by_value of `AttributionMosaic`."""
        if self.coords is None:
            raise RuntimeError("call build() first")
        from .attr_mosaic import AttributionMosaic
        return AttributionMosaic(self.roi_size, scale, **mosaic_args).render(self.slide, self.coords, maps)

    def rois(self, indices):
        """The chosen kept windows as pixels, uint8 [n,S,S,3] on the slide's device — materialised on request only."""
        if self.coords is None:
            raise RuntimeError("call build() first")
        idx = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices).astype(np.int64).reshape(-1)
        s = self.roi_size
        out = torch.empty((len(idx), s, s, 3), dtype=torch.uint8, device=self.slide.device)
        for j, i in enumerate(idx):
            r, q = (int(v) for v in self.coords[i])
            out[j].copy_(self.slide[r:r + s, q:q + s])
        return out
