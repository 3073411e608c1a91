"""Feature inversion and the pixel regularisers: an image optimised on the device until a stage sees in it what it saw in a tile.

`inverted_representation.py` of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src) is Mahendran &
Vedaldi's inverted representation: from noise, SGD with momentum on 1e-1 * ||f(x) - f(x0)||^2 / ||f(x0)||^2 plus an alpha norm
and a total-variation norm of the image, 201 steps of a Python loop around a hooked VGG, one image at a time.  Here the target is
the output of `layerN` of the tile encoder, a whole bag of tiles is inverted at once, and a step is the optional jittered copy
(`ops.pixel_shift`), the encoder's forward cut short at the stage (`encoder_forward(upto=)`), one launch pair that reads the
distance and writes the seed of the backward pass (`ops.stage_match`), the data-gradient-only walk to the pixels
(`encoder_pixel_gradient`), one launch that moves the gradient back through the jitter and adds the regularisers' gradients
(`ops.pixel_reg`) and one that takes the momentum step, projects and encodes (`ops.pixel_momentum_step`) — nothing synchronises
with the host.  `PixelRegularizer` also serves `FeatureVisualizer(regularizer=)`.  DESIGN.md section 3.46.

The regulariser that removes high-frequency patterns is a Gaussian blur, one launch of `ops.pixel_blur` (a separable filter with a
bit contract of its own, both passes in one kernel): of the image, every `blur_every` steps at the start of the step, or of the
gradient, in every step between `ops.pixel_reg` and the optimiser step.  The filter is never in place: the loops move between two
stacks allocated before they start, the jittered copy's where there is one.  `gaussian_blur` is the same launch for stacks and
attribution maps.  DESIGN.md section 3.47.
"""
from collections import namedtuple

import torch

from . import ops
from .attribution import check_tiles, compute_mode, device_tiles, model_device, narrow_encoder, stage_of
from .encoder import STAGE_WIDTHS, encoder_forward, encoder_pixel_gradient
from .preprocess import U8Tiles

WHAT = "feature inversion"

InversionResult = namedtuple("InversionResult", ["u8", "x", "trace", "terms"])
InversionResult.__doc__ = """What `FeatureInverter.invert` returns: `u8`, the final images as `U8Tiles`; `x`, the same images as the
fp32 [T,3,H,W] stack that was optimised; `trace` fp32 [steps, T], the weighted distance weight * ||f(x) - f(x0)||^2 / ||f(x0)||^2
of the image each step STARTED from; `terms` fp32 [steps, 2, T], that image's sum of x^alpha and its total variation."""


def _count(v, name, least=1):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or int(v) != v or v < least:
        raise ValueError(f"{name} must be an integer >= {least}, got {v!r}")
    return int(v)


def _sigma(v, name):
    """0.0 (off) or a sigma `ops.gauss_taps` takes."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or v < 0:
        raise ValueError(f"{name} must be a number >= 0 (0: off), got {v!r}")
    if v:
        try:
            ops.gauss_taps(v)
        except ValueError as e:
            raise ValueError(f"{name}: {e}") from None
    return float(v)


class PixelRegularizer:
    """`PixelRegularizer(alpha=6, alpha_weight=1e-7, tv_weight=1e-8, jitter=0, seed=0, *, blur_sigma=0.0, blur_every=4,
    grad_blur_sigma=0.0, blur_edge="reflect")` — what is added to an objective that is minimised over pixels:
    alpha_weight * sum x^alpha + tv_weight * TV(x), TV the toolkit's `total_variation_norm` with beta = 2;
    the defaults are the toolkit's (inverted_representation.py:74-84).  alpha: 2, 4, 6 or 8.  jitter: the largest shift in pixels
    of the cyclic jitter — every step evaluates the network on the image shifted by (dy, dx), each drawn from [-jitter, jitter],
    and the gradient is shifted back; 0: none.  `shifts(steps)` draws all of them at once from a CPU `torch.Generator` seeded
    with `seed`: the global generators are not touched and the shifts are the same on every machine.

    The two Gaussian blurs (`ops.pixel_blur`; sigma as `ops.gauss_taps` takes it, 0: off; blur_edge: "reflect", "replicate" or
    "wrap", the cyclic jitter's own rule):
      blur_sigma       image blur (Yosinski et al. 2015): at the START of step k, for k > 0 and k % blur_every == 0, the image is
                       replaced by its blurred copy, before the jittered copy and the forward.  A blur therefore never follows
                       the last optimiser step: the `u8` and `x` of a result stay the ones the step kernel encoded, and the trace
                       (and terms) of step k describe the blurred image, the one the step started from.  The blurred image is NOT
                       projected again: with project="u8" it is off the byte grid until the next optimiser step projects it.
      grad_blur_sigma  gradient blur: the gradient `gradient(...)` returns is blurred before the optimiser step, in every step.
    With both 0, the default, there is no new launch, no new allocation and every bit is as before.  The filter is never in
    place, so the loops move between two stacks (`blurred` returns them swapped) instead of copying back.  A value object: it
    holds no tensor."""

    def __init__(self, alpha=6, alpha_weight=1e-7, tv_weight=1e-8, jitter=0, seed=0, *, blur_sigma=0.0, blur_every=4, grad_blur_sigma=0.0,
                 blur_edge="reflect"):
        self.alpha, self.alpha_weight, self.tv_weight = ops.reg_weights(alpha, alpha_weight, tv_weight)
        self.jitter = _count(jitter, "jitter", 0)
        self.seed = _count(seed, "seed", 0)
        self.blur_sigma, self.grad_blur_sigma = _sigma(blur_sigma, "blur_sigma"), _sigma(grad_blur_sigma, "grad_blur_sigma")
        self.blur_every = _count(blur_every, "blur_every")
        self.blur_edge = ops.blur_edge(blur_edge)

    def __repr__(self):
        return (f"PixelRegularizer(alpha={self.alpha}, alpha_weight={self.alpha_weight}, tv_weight={self.tv_weight}, "
                f"jitter={self.jitter}, seed={self.seed}, blur_sigma={self.blur_sigma}, blur_every={self.blur_every}, "
                f"grad_blur_sigma={self.grad_blur_sigma}, blur_edge={self.blur_edge!r})")

    def shifts(self, steps):
        """[(dy, dx)] * steps: zeros without jitter, else `torch.randint(-jitter, jitter + 1, (steps, 2))` of a generator of
        their own."""
        if not self.jitter:
            return [(0, 0)] * steps
        gen = torch.Generator().manual_seed(self.seed)
        return [tuple(s) for s in torch.randint(-self.jitter, self.jitter + 1, (steps, 2), generator=gen).tolist()]

    def scratch(self, x):
        """(xs, out), the stacks a loop over x allocates before it starts, None where no option needs one.  xs holds the jittered
        copy during the forward and the backward walk and is dead otherwise: the image blur (at the start of a step) and the
        gradient blur (behind `ops.pixel_reg`) write into it, so with jitter the blurs cost no stack of their own and without
        it one.  out: the gradient moved back through the jitter.  A blur the images are too small for under "reflect" is refused
        here, before the first step, not at the step that would launch it."""
        for name in ("blur_sigma", "grad_blur_sigma"):
            sigma = getattr(self, name)
            if sigma and self.blur_edge == "reflect" and ops.gauss_taps(sigma)[0] > min(x.shape[-2:]) - 1:
                raise ValueError(f"{name}={sigma} with blur_edge='reflect' needs images of more than {ops.gauss_taps(sigma)[0]} pixels a side, "
                                 f"got {x.shape[-2]}x{x.shape[-1]}")
        xs =torch.empty_like(x) if self.jitter or self.blur_sigma or self.grad_blur_sigma else None
        return xs, torch.empty_like(x) if self.jitter else None

    def blurred(self, x, xs, k):
        """Step 0 of a regularised step k: (x, xs) — swapped, xs having received the blurred x, when step k starts with an image
        blur; as given otherwise."""
        if not self.blur_sigma or k == 0 or k % self.blur_every:
            return x, xs
        return ops.pixel_blur(x, xs, sigma=self.blur_sigma, edge=self.blur_edge), x

    def jittered(self, x, xs, shift):
        """Step 1 of a regularised step: the tensor the network reads — x itself without jitter, else its shifted copy in xs."""
        return ops.pixel_shift(x, xs, shift) if self.jitter else x

    def gradient(self, x, g, out, shift, terms=None, xs=None):
        """Step 5: g, the gradient with respect to `jittered(x)`, as the gradient of the regularised objective with respect to x.
        Without jitter it is written over g; with it, into `out`.  With a gradient blur its blurred copy, written into xs."""
        g = ops.pixel_reg(x, g, out if self.jitter else g, alpha=self.alpha, alpha_weight=self.alpha_weight, tv_weight=self.tv_weight,
                          shift=shift, terms=terms)
        return ops.pixel_blur(g, xs, sigma=self.grad_blur_sigma, edge=self.blur_edge) if self.grad_blur_sigma else g


def pixel_descent(x, steps, reg, gradient, step, want_terms=False):
    """The loop of the pixel optimisers (`FeatureInverter.invert`, `FeatureVisualizer.filters` / `dream` / `classes`): `steps`
    steps on the stack x, fp32 [T,3,H,W] on the device.  reg: a `PixelRegularizer`, whose protocol is followed here and nowhere
    else, or None — then no `pixel_shift`, `pixel_reg` or `pixel_blur` is launched and no scratch stack is allocated.
      gradient(xin, k) -> g    step k's objective on xin, the tensor the network reads (x, or its jittered copy), and its
                               gradient with respect to xin; called in the caller's grad mode
      step(x, g, k, u8_out)    the optimiser step on x in place, under `torch.no_grad()` like everything behind `gradient`;
                               u8_out: the byte buffer in the last step, which encodes into it, None before
    -> (x, u8, terms): the stack the last step wrote (a step that starts with an image blur swaps x with a scratch stack), its
    bytes, and with want_terms the regulariser's norms per step, fp32 [steps,2,T] (else None)."""
    u8 = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    terms = torch.empty((steps, 2, x.shape[0]), dtype=torch.float32, device=x.device) if want_terms else None
    if reg is not None:
        shifts, (xs, out) = reg.shifts(steps), reg.scratch(x)
    for k in range(steps):
        xin = x
        if reg is not None:
            x, xs = reg.blurred(x, xs, k)
            xin = reg.jittered(x, xs, shifts[k])
        g = gradient(xin, k)
        with torch.no_grad():
            if reg is not None:
                g = reg.gradient(x, g, out, shifts[k], None if terms is None else terms[k], xs)
            step(x, g, k, u8 if k == steps - 1 else None)
    return x, u8, terms


def gaussian_blur(x, sigma, edge="reflect", out=None):
    """The Gaussian blur of every plane of a stack [T,3,H,W] or of maps [T,H,W] (fp32, contiguous, on the device) in one launch:
    `scipy.ndimage.gaussian_filter(plane, sigma, truncate=4.0)` with the mode edge stands for ("reflect": scipy's "mirror",
    torch's `reflect` padding, radius <= min(H, W) - 1; "replicate": "nearest"; "wrap"), in fp32 with the fixed operation order
    of `ops.pixel_blur`.  sigma: about 0.125 <= sigma < 4.125 (`ops.gauss_taps`).  out: None or the caller's tensor, not
    overlapping x.  For example `renderer.grayscale(mil_amd.gaussian_blur(sal.maps(tiles, y), 2.0))`."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 3):
        raise ValueError(f"x must be an fp32 stack [T,3,H,W] or maps [T,H,W], got {tuple(getattr(x, 'shape', ()))}")
    return ops.pixel_blur(x, out, sigma=sigma, edge=edge)


def check_regularizer(regularizer, optional=False):
    if regularizer is None and optional:
        return None
    if not isinstance(regularizer, PixelRegularizer):
        raise ValueError(f"regularizer must be a mil_amd.PixelRegularizer{' or None' if optional else ''}, got {type(regularizer).__name__}")
    return regularizer


class FeatureInverter:
    """`FeatureInverter(model, lr=100.0, momentum=0.9, lr_decay=None, weight=0.1, regularizer=PixelRegularizer(), project="none")`
    — `model`: a `mil_amd.Attention` with the narrow ResNet-26, or that `ResNet` itself.

      invert(tiles, layer, steps=200, init_std=0.1, seed=0) -> InversionResult(u8, x, trace, terms)
          one image per tile, each optimised from `init_std * randn` (a CPU generator seeded with `seed`; the toolkit's
          `1e-1 * torch.randn`) so that `layer`'s output for it matches the output for the tile: SGD with momentum on
          weight * ||f(x) - f(tile)||^2 / ||f(tile)||^2 plus the regulariser.  `tiles`: an fp32 stack or `U8Tiles`, left untouched.
      distance(x, tiles, layer) -> fp32 [T]: that weighted distance, one truncated forward for x and one for the tiles.

    lr_decay=(every, factor) multiplies lr by `factor` after the steps 0, every, 2 every, ... — the toolkit's schedule, its decay
    after the very first step included.  The toolkit's own setting is lr=1e4, lr_decay=(40, 0.1) on a VGG; the default here, a
    constant lr=100, is NOT the toolkit's: on this encoder's golden weights at 64x64 the same loop on the fp32 CPU oracle with
    lr=1e4 and no decay is NaN within 12 steps, while lr=1e2 and lr=1e3 descend.  The target is the stage's output BEHIND its last
    LeakyReLU, as for `FeatureVisualizer`.  project: "none", "clamp" or "u8" (`ops.pixel_step`'s).  One forward of `tiles` and one
    `ops.stage_energy` per call; a step is six groups of launches (five without jitter) and nothing synchronises with the host;
    all three compute modes and every tile size the encoder takes.  A call leaves the model as it found it: the `training` flag,
    every `.grad`, the torch RNG states and a `FlatParams` bucket are not touched."""

    def __init__(self, model, lr=100.0, momentum=0.9, lr_decay=None, weight=0.1, regularizer=PixelRegularizer(), project="none"):
        self.net = narrow_encoder(model, "FeatureInverter", bare=True)
        if project not in ops.PIXEL_PROJECTIONS:
            raise ValueError(f"project must be one of {ops.PIXEL_PROJECTIONS}, got {project!r}")
        self.lr, _wd, self.momentum = ops.momentum_scalars(lr, momentum, 0.0)
        if lr_decay is not None:
            try:
                every, factor = lr_decay
                every, factor = _count(every, "lr_decay's every"), float(factor)
            except TypeError:
                raise ValueError(f"lr_decay must be None or (every, factor), got {lr_decay!r}") from None
            if not factor > 0.0 or factor == float("inf"):
                raise ValueError(f"lr_decay's factor must be a positive number, got {factor}")
            lr_decay = (every, factor)
        self.lr_decay = lr_decay
        self.weight = float(weight)
        if not self.weight > 0.0 or self.weight == float("inf"):
            raise ValueError(f"weight must be a positive number, got {weight!r}")
        self.regularizer = check_regularizer(regularizer)
        self.project = project

    def _target(self, tiles, stage, dtype):
        """The stage's output for the tiles, as the forward keeps it."""
        _feats, saved = encoder_forward(self.net, device_tiles(self.net, tiles, "FeatureInverter"), dtype, upto=stage)
        return saved["blocks"][-1][2]

    def invert(self, tiles, layer, steps=200, init_std=0.1, seed=0):
        stage = stage_of(layer)
        check_tiles(None, tiles, None, WHAT)
        steps, seed = _count(steps, "steps"), _count(seed, "seed", 0)
        init_std = float(init_std)
        if not init_std >= 0.0 or init_std == float("inf"):
            raise ValueError(f"init_std must be a number >= 0, got {init_std}")
        net, c = self.net, STAGE_WIDTHS[stage - 1]
        dev = model_device(net, "FeatureInverter")
        gen = torch.Generator().manual_seed(seed)
        x = (init_std * torch.randn(tuple(tiles.shape), generator=gen, dtype=torch.float32)).to(dev)
        trace = torch.empty((steps, x.shape[0]), dtype=torch.float32, device=dev)
        buf = torch.zeros_like(x)
        lr = self.lr
        with torch.no_grad(), compute_mode(net) as dtype:
            target = self._target(tiles, stage, dtype)
            energy = ops.stage_energy(target, c)

            def gradient(xin, k):
                _feats, saved = encoder_forward(net, xin, dtype, upto=stage)
                _loss, dz = ops.stage_match(saved["blocks"][-1][2], target, c, weight=self.weight, energy=energy, loss=trace[k])
                return encoder_pixel_gradient(net, saved, dtype, dz=dz, stage=stage)[0]

            def step(x, g, k, u8_out):
                nonlocal lr
                ops.pixel_momentum_step(x, g, buf, lr=lr, momentum=self.momentum, project=self.project, u8_out=u8_out)
                if self.lr_decay is not None and k % self.lr_decay[0] == 0:
                    lr *= self.lr_decay[1]
            x, u8, terms = pixel_descent(x, steps, self.regularizer, gradient, step, want_terms=True)
        return InversionResult(U8Tiles(u8), x, trace, terms)

    def distance(self, x, tiles, layer):
        stage = stage_of(layer)
        check_tiles(None, tiles, None, WHAT)
        check_tiles(None, x, None, WHAT)
        if tuple(x.shape) != tuple(tiles.shape):
            raise ValueError(f"x {tuple(x.shape)} and tiles {tuple(tiles.shape)} differ")
        c = STAGE_WIDTHS[stage - 1]
        with torch.no_grad(), compute_mode(self.net) as dtype:
            target = self._target(tiles, stage, dtype)
            return ops.stage_match(self._target(x, stage, dtype), target, c, weight=self.weight)[0]
