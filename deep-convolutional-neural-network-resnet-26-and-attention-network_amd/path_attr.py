"""Integrated gradients and SmoothGrad of a slide's tiles, accumulated on the device.

The two methods of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src) that average gradients:
`integrated_gradients.py` along a straight path from a baseline image to the tile, `smooth_grad.py` over noisy copies of the
tile.  With the stock model either is a Python loop around `x.requires_grad_()`.  Here a step is one launch that makes the
perturbed stack straight from the fp32 or uint8 tiles (`ops.path_point`: counter-based noise, torch's generator is not touched),
one pass of the hand-written encoder forward and of its data-gradient-only walk back (`attribution.bag_step`: no weight gradient
is launched), and the stem's data-gradient kernel adding `weight * gradient` into the running sum in its store epilogue
(`encoder_pixel_gradient(dx_acc=...)`): no per-step gradient tensor, no torch pass over it.  One
finishing launch (`ops.attr_finish`) turns the sum into attributions, maps and per-tile sums.  DESIGN.md section 3.40.
"""
import torch

from . import ops
from .attribution import bag_setup, bag_step, check_tiles, device_tiles, narrow_encoder
from .preprocess import U8Tiles

RULES = ("midpoint", "toolkit")
BASELINES = {"grey": 0.0, "white": 1.0, "black": -1.0}       # in normalised units: Normalize(.5, .5) maps [0, 1] to [-1, 1]
MAP_REDUCE = ("sum", "max")


def _wrap(tiles, x):
    """The device tensor `x` in the form the kernels take it."""
    return U8Tiles(x) if isinstance(tiles, U8Tiles) else x


class TileIntegratedGradients:
    """`TileIntegratedGradients(model, steps=32, rule="midpoint", baseline=0.0)` for a `mil_amd.Attention` with the narrow
    ResNet-26 (Sundararajan et al., "Axiomatic attribution for deep networks").  The bag is evaluated as the reference's
    `visualize()` evaluates a slide — eval mode: all tiles, no dropout — at every point base + alpha_k (tiles - base) of the path
    and the function differentiated is the bag's loss for `label`, with the sign of `TileSaliency.input_gradient`:

      gradients(tiles, label)     -> fp32 [T,3,H,W]: sum_k w_k d loss / d tiles at alpha_k (what the toolkit returns)
      attributions(tiles, label)  -> fp32 [T,3,H,W]: (tiles - baseline) * gradients
      maps(tiles, label, reduce)  -> fp32 [T,H,W]: |sum_c attributions| ("sum") or max_c |attributions| ("max")
      completeness(tiles, label)  -> two device scalars: (the sum of the attributions over the bag, loss(tiles) - loss(baseline
                                     bag)).  The axiom says they agree in the limit of many steps; on this model the sum is a
                                     cancellation of terms a thousand times the difference and converges slowly and not
                                     monotonically (DESIGN.md section 3.40 has a table): a diagnostic, not a test of the code

    baseline: a scalar, three per-channel values, or "grey" (0.0, the toolkit's implicit zero image), "white" (1.0, the slide
    background of H&E) or "black" (-1.0), in the normalised units of the tiles.
    rule="midpoint": alpha_k = (k + 1/2) / steps, k = 0..steps-1, weights 1/steps (the midpoint rule).  rule="toolkit":
    alpha_k = k / steps, k = 0..steps, weights 1/steps — the toolkit's own sum (integrated_gradients.py:32-37, 59-63), steps + 1
    points whose weights add up to (steps + 1) / steps.  The alphas are made in double precision and passed as fp32.

    `tiles`: an fp32 [T,3,H,W] stack or `U8Tiles` (decoded inside the kernels: bit for bit the results of `U8Tiles.float()`).
    A call leaves the model as it found it, as `TileSaliency` does: the `training` flag, every `.grad`, the torch RNG state and
    a `FlatParams` bucket are not touched."""

    def __init__(self, model, steps=32, rule="midpoint", baseline=0.0):
        narrow_encoder(model, "TileIntegratedGradients")
        if rule not in RULES:
            raise ValueError(f"rule must be one of {RULES}, got {rule!r}")
        if int(steps) != steps or steps < 1:
            raise ValueError(f"steps must be an integer >= 1, got {steps!r}")
        if isinstance(baseline, str):
            if baseline not in BASELINES:
                raise ValueError(f"baseline must be a number, three per-channel numbers or one of {tuple(BASELINES)}, got {baseline!r}")
            baseline = BASELINES[baseline]
        try:
            base = ops._base3(baseline)
        except TypeError:
            raise ValueError(f"baseline must be a number, three per-channel numbers or one of {tuple(BASELINES)}, got {baseline!r}") from None
        self.model, self.steps, self.rule, self.baseline = model, int(steps), rule, tuple(base)

    def path(self):
        """[(alpha_k, weight_k)] of the rule, in step order."""
        m = self.steps
        if self.rule == "midpoint":
            return [((k + 0.5) / m, 1.0 / m) for k in range(m)]
        return [(k / m, 1.0 / m) for k in range(m + 1)]

    def _accumulate(self, tiles, label):
        """(the path-averaged gradient, the device tensor behind the tiles) for the checked arguments."""
        model = self.model
        x = device_tiles(model, tiles)
        src = _wrap(tiles, x)
        setup = bag_setup(model, x.shape[0], label)
        acc = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        point = torch.empty_like(acc)
        for alpha, weight in self.path():
            # the encoder's backward is done with `point` before the next step overwrites it
            ops.path_point(src, alpha, self.baseline, out=point)
            bag_step(model, setup, point, dx_acc=(acc, weight))
        return acc, src

    def gradients(self, tiles, label):
        label = check_tiles(self.model, tiles, label, "path attribution")
        return self._accumulate(tiles, label)[0]

    def attributions(self, tiles, label):
        label = check_tiles(self.model, tiles, label, "path attribution")
        acc, src = self._accumulate(tiles, label)
        return ops.attr_finish(acc, src, self.baseline)[0]

    def maps(self, tiles, label, reduce="sum"):
        if reduce not in MAP_REDUCE:
            raise ValueError(f"reduce must be one of {MAP_REDUCE}, got {reduce!r}")
        label = check_tiles(self.model, tiles, label, "path attribution")
        acc, src = self._accumulate(tiles, label)
        return ops.attr_finish(acc, src, self.baseline, want_attr=False, want_map=True, map_mode=reduce)[1]

    def completeness(self, tiles, label):
        label = check_tiles(self.model, tiles, label, "path attribution")
        acc, src = self._accumulate(tiles, label)
        sums = ops.attr_finish(acc, src, self.baseline, want_attr=False, want_sums=True)[2]
        model = self.model
        setup = bag_setup(model, acc.shape[0], label)
        x = src.u8 if isinstance(src, U8Tiles) else src
        at_tiles = bag_step(model, setup, x, backward=False)[2]
        at_base = bag_step(model, setup, ops.path_point(src, 0.0, self.baseline), backward=False)[2]
        return sums.sum(), (at_tiles - at_base)[0]


class TileSmoothGrad:
    """`TileSmoothGrad(model, n=50, noise_level=0.15, seed=0)` (Smilkov et al., "SmoothGrad: removing noise by adding noise"):
    the mean of the gradients of the bag's loss for `label` at `n` noisy copies tiles + sigma * N(0, 1) of the tiles, with
    sigma = noise_level * (max - min) of the bag — the paper's definition; the range is taken on the device (`amin` / `amax`, no
    host synchronisation).  The toolkit's own `normal_(mean, sigma ** 2)` with sigma = multiplier / (max - min)
    (smooth_grad.py:31-37) divides where the paper multiplies and passes a variance for a standard deviation; it is not copied.

      gradients(tiles, label) -> fp32 [T,3,H,W]: the mean over sample = 0..n-1
      maps(tiles, label)      -> fp32 [T,H,W]: max_c |mean gradient|

    The noise of sample k is a function of (seed, k, element index) only (Philox4x32-10 + Box-Muller inside `ops.path_point`):
    the same seed gives the same bits, torch's generators are not drawn from.  Tiles, evaluation, sign and side effects as for
    `TileIntegratedGradients`."""

    def __init__(self, model, n=50, noise_level=0.15, seed=0):
        narrow_encoder(model, "TileSmoothGrad")
        if int(n) != n or n < 1:
            raise ValueError(f"n must be an integer >= 1, got {n!r}")
        if not float(noise_level) >= 0.0:
            raise ValueError(f"noise_level must be >= 0, got {noise_level!r}")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"seed must fit 64 bits, got {seed!r}")
        self.model, self.n, self.noise_level, self.seed = model, int(n), float(noise_level), int(seed)

    def _accumulate(self, tiles, label):
        model = self.model
        x = device_tiles(model, tiles)
        src = _wrap(tiles, x)
        setup = bag_setup(model, x.shape[0], label)
        rng = None
        if self.noise_level != 0.0:
            rng = torch.stack((x.amin(), x.amax()))
            if x.dtype == torch.uint8:                      # the decode is monotone: the range of the values is that of the codes
                rng = U8Tiles(rng.view(1, 1, 1, 2).expand(1, 3, 1, 2)).float()[0, 0, 0]
            rng = rng.to(torch.float32).contiguous()
        acc = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
        point = torch.empty_like(acc)
        for k in range(self.n):
            ops.path_point(src, 1.0, 0.0, noise_level=self.noise_level, value_range=rng, seed=self.seed, sample=k, out=point)
            bag_step(model, setup, point, dx_acc=(acc, 1.0 / self.n))
        return acc

    def gradients(self, tiles, label):
        label = check_tiles(self.model, tiles, label, "path attribution")
        return self._accumulate(tiles, label)

    def maps(self, tiles, label):
        label = check_tiles(self.model, tiles, label, "path attribution")
        return ops.attr_finish(self._accumulate(tiles, label), None, 0.0, want_attr=False, want_map=True, map_mode="grad_max")[1]
