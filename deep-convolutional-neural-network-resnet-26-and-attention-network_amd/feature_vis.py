"""Activation maximisation: tiles optimised on the device so that a filter fires or a class is predicted.

The family of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src) that optimises the PIXELS:
`cnn_layer_visualization.py` — the one toolkit class the reference's driver imports by name (gbm/classify.py:30) — runs gradient
ascent on a random image so that one filter of one layer fires, `deep_dream.py` does the same from a real image, and
`generate_class_specific_samples.py` ascends a class score with the image re-quantised to bytes every step.  With the stock model
each is a Python loop of optimiser steps around a hooked forward, one image at a time.  Here a step is the encoder's forward cut
short at the stage (`encoder_forward(upto=)`), one launch that reads the objective and writes the seed of the backward pass
(`ops.stage_seed`), the data-gradient-only walk to the pixels (`encoder_pixel_gradient`: no weight-gradient launch) and one
launch that takes the optimiser step, projects the image and encodes it (`ops.pixel_step`); one tile carries one filter each, so
all channels of a stage are optimised in one batch.  DESIGN.md section 3.43.
"""
from collections import namedtuple

import torch

from . import ops
from .attribution import LAYERS, bag_evaluate, bag_setup, channel_list, check_tiles, compute_mode, device_tiles, model_device, narrow_encoder, stage_of  # noqa: F401
from .encoder import STAGE_WIDTHS, encoder_forward, encoder_pixel_gradient
from .feature_inv import _count, check_regularizer, pixel_descent
from .preprocess import U8Tiles

OPTIMIZERS = ops.PIXEL_RULES
WHAT = "feature visualisation"

FeatureVisResult = namedtuple("FeatureVisResult", ["u8", "x", "trace"])
FeatureVisResult.__doc__ = """What an optimisation returns: `u8`, the final images as `U8Tiles` (the toolkit's `recreate_image` at this
project's mean and std of 0.5); `x`, the same images as the fp32 [T,3,H,W] stack that was optimised; `trace` fp32 [steps, T], the
objective of the image each step STARTED from (the filter's mean activation; minus the bag's loss for `classes`)."""


def _size(size):
    try:
        h, w = (_count(v, "size") for v in size)
    except TypeError:
        raise ValueError(f"size must be (H, W), got {size!r}") from None
    return h, w


def _init_range(init):
    try:
        lo, hi = (int(v) for v in init)
    except (TypeError, ValueError):
        raise ValueError(f"init must be (lo, hi), a range of byte values, got {init!r}") from None
    if not 0 <= lo < hi <= 256:
        raise ValueError(f"init must satisfy 0 <= lo < hi <= 256, got {init!r}")
    return lo, hi


class FeatureVisualizer:
    """`FeatureVisualizer(model, optimizer="adam", lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, project="none")` —
    the defaults are the toolkit's `Adam([image], lr=0.1, weight_decay=1e-6)` (cnn_layer_visualization.py:45).  `model`: a
    `mil_amd.Attention` with the narrow ResNet-26, or that `ResNet` itself for the filter methods.

      filters(layer, channels=None, size=(256, 256), steps=30, init=(150, 180), seed=0)
          one tile per channel (None: every channel of the stage), each optimised from random bytes so that its channel of
          `layer`'s output has a large mean: `cnn_layer_visualization.py`.  The start bytes are `torch.randint(lo, hi)` of a CPU
          generator seeded with `seed` — the toolkit's `uniform(150, 180)`; the global generators are not drawn from and the
          bytes are the same on every machine.
      dream(tiles, layer, channels, steps=250)
          the same objective started from real tiles (an fp32 stack or `U8Tiles`, left untouched): `deep_dream.py`.  `channels`:
          an int or one per tile.
      classes(label, ntiles, size=(256, 256), steps=150, init=(0, 256), seed=0)
          a bag of `ntiles` >= 2 generated tiles that minimises the bag's loss for `label`, the head evaluated as
          `TileSaliency` evaluates it (eval mode).  `FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8")` with
          init=(0, 256) is `generate_class_specific_samples.py`: plain SGD at lr 6 on an image that is re-created as bytes and
          re-read every step (there the objective is minus the class logit, here the bag's loss).
      objective(tiles, layer, channels) -> fp32 [T]: the mean of each tile's channel, one truncated forward.

    The optimising methods return a `FeatureVisResult` (u8, x, trace).  The target is the stage's output BEHIND its last
    LeakyReLU — the tensor the forward keeps, and what a forward hook on the reference's `layerN` would see.  project: "none"
    (the layer visualisation), "clamp" (to [-1, 1]) or "u8" (the class-specific method's round trip through bytes).  A step is
    four groups of launches with no host synchronisation between them; all three compute modes and every tile size the encoder
    takes.  A call leaves the model as it found it, as `TileSaliency` does: the `training` flag, every `.grad`, the torch RNG
    states and a `FlatParams` bucket are not touched.

    regularizer (keyword only): None — every launch and every bit as without it — or a `mil_amd.PixelRegularizer`, which
    `filters`, `dream` and `classes` add to the objective they MINIMISE (minus the filter's mean; the bag's loss): every step
    then reads the network on the jittered copy of the image (`ops.pixel_shift`, with jitter) and sends the gradient through
    `ops.pixel_reg` before the optimiser step, as `mil_amd.FeatureInverter` does.  Its `blur_sigma` / `grad_blur_sigma` add one
    `ops.pixel_blur` launch at the start of every `blur_every`-th step (the image) or before every optimiser step (the gradient);
    the image then moves between two stacks, so the `x` of a result need not be the tensor the loop started from."""

    def __init__(self, model, optimizer="adam", lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, project="none", *, regularizer=None):
        net = narrow_encoder(model, "FeatureVisualizer", bare=True)
        self.regularizer = check_regularizer(regularizer, optional=True)
        if project not in ops.PIXEL_PROJECTIONS:
            raise ValueError(f"project must be one of {ops.PIXEL_PROJECTIONS}, got {project!r}")
        try:
            betas = tuple(float(b) for b in betas)
        except (TypeError, ValueError):
            raise ValueError(f"betas must be two numbers, got {betas!r}") from None
        if len(betas) != 2:
            raise ValueError(f"betas must be two numbers, got {betas!r}")
        ops.pixel_step_scalars(optimizer, lr, weight_decay, betas, eps, 1)
        self.model = model if model is not net else None       # the Attention model, where one was given
        self.net = net
        self.optimizer, self.lr, self.weight_decay, self.betas, self.eps = optimizer, float(lr), float(weight_decay), betas, float(eps)
        self.project = project

    # ---- pieces ------------------------------------------------------------------------------------------------------------
    def _device(self):
        return model_device(self.net, "FeatureVisualizer")

    def _start(self, ntiles, size, init, seed):
        """Random start bytes [ntiles,3,H,W] from a generator of their own, as the fp32 stack they decode to, on the device."""
        gen = torch.Generator().manual_seed(int(seed))
        u8 = torch.randint(init[0], init[1], (ntiles, 3, size[0], size[1]), generator=gen, dtype=torch.uint8)
        return U8Tiles(u8.to(self._device())).float()

    def _descend(self, x, steps, gradient):
        """`pixel_descent` with this visualiser's optimiser, projection and regulariser -> (x, u8)."""
        state = (torch.zeros_like(x), torch.zeros_like(x)) if self.optimizer == "adam" else None

        def step(x, g, k, u8_out):
            ops.pixel_step(x, g, state, rule=self.optimizer, lr=self.lr, weight_decay=self.weight_decay, betas=self.betas, eps=self.eps,
                           step=k + 1, project=self.project, u8_out=u8_out)
        return pixel_descent(x, steps, self.regularizer, gradient, step)[:2]

    def _ascend(self, x, stage, chans, steps):
        """`steps` steps on x (fp32 on the device, optimised in place) for channel chans[t] of stage `stage`."""
        net = self.net
        c = STAGE_WIDTHS[stage - 1]
        ch = torch.tensor(chans, dtype=torch.int32).to(x.device)
        trace = torch.empty((steps, x.shape[0]), dtype=torch.float32, device=x.device)
        with torch.no_grad(), compute_mode(net) as dtype:
            def gradient(xin, k):
                _feats, saved = encoder_forward(net, xin, dtype, upto=stage)
                _j, dz = ops.stage_seed(saved["blocks"][-1][2], ch, c, objective=trace[k])
                return encoder_pixel_gradient(net, saved, dtype, dz=dz, stage=stage)[0]
            x, u8 = self._descend(x, steps, gradient)
        return FeatureVisResult(U8Tiles(u8), x, trace)

    # ---- methods -----------------------------------------------------------------------------------------------------------
    def filters(self, layer, channels=None, size=(256, 256), steps=30, init=(150, 180), seed=0):
        stage = stage_of(layer)
        chans = channel_list(channels, STAGE_WIDTHS[stage - 1])
        size, steps, init = _size(size), _count(steps, "steps"), _init_range(init)
        return self._ascend(self._start(len(chans), size, init, seed), stage, chans, steps)

    def dream(self, tiles, layer, channels, steps=250):
        stage = stage_of(layer)
        check_tiles(None, tiles, None, WHAT)
        chans = channel_list(channels, STAGE_WIDTHS[stage - 1], tiles.shape[0])
        steps = _count(steps, "steps")
        dev = self._device()
        x = tiles.to(dev).float() if isinstance(tiles, U8Tiles) else tiles.detach().to(dev, torch.float32, copy=True).contiguous()
        return self._ascend(x, stage, chans, steps)

    def objective(self, tiles, layer, channels):
        stage = stage_of(layer)
        check_tiles(None, tiles, None, WHAT)
        chans = channel_list(channels, STAGE_WIDTHS[stage - 1], tiles.shape[0])
        x = device_tiles(self.net, tiles, "FeatureVisualizer")
        ch = torch.tensor(chans, dtype=torch.int32).to(x.device)
        with torch.no_grad(), compute_mode(self.net) as dtype:
            _feats, saved = encoder_forward(self.net, x, dtype, upto=stage)
            return ops.stage_seed(saved["blocks"][-1][2], ch, STAGE_WIDTHS[stage - 1])[0]

    def classes(self, label, ntiles, size=(256, 256), steps=150, init=(0, 256), seed=0):
        model = self.model
        if model is None:
            raise ValueError("classes() optimises the bag's loss: it needs the mil_amd.Attention model, not the bare encoder")
        if isinstance(label, bool) or not isinstance(label, int) or not 0 <= label < model.C:
            raise ValueError(f"label must be in [0, {model.C}), got {label!r}")
        ntiles = _count(ntiles, "ntiles", 2)
        size, steps, init = _size(size), _count(steps, "steps"), _init_range(init)
        x = self._start(ntiles, size, init, seed)
        setup = bag_setup(model, ntiles, int(label))
        weights = [w.detach() for w in model.head_weights()]      # hoisted out of the loop: the model does not change under it
        trace = torch.empty((steps, ntiles), dtype=torch.float32, device=x.device)
        with compute_mode(self.net) as dtype:
            def gradient(xin, k):
                saved, dH, loss = bag_evaluate(model, setup, xin, weights=weights)      # outside no_grad: the head is differentiated by autograd
                with torch.no_grad():
                    trace[k] = -loss
                    return encoder_pixel_gradient(self.net, saved, dtype, dfeats=dH)[0]
            x, u8 = self._descend(x, steps, gradient)
        return FeatureVisResult(U8Tiles(u8), x, trace)
