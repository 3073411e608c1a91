"""Pixel-level saliency of a slide's tiles: the gradient of the bag's loss with respect to the tiles, on the device.

The reference vendors a saliency toolkit (pytorch-cnn-visualizations-master/src: `vanilla_backprop.py`,
`grad_times_image.py`) and with its stock PyTorch model the gradient of a slide's class score with respect to the pixels is
one `x.requires_grad_()` away.  Here it is the data-gradient-only walk of the hand-written encoder chain (`attribution.bag_step`:
`encoder_pixel_gradient`, no weight gradient is launched) with the stem's data-gradient kernel (`ops.stem_dgrad`) at its end;
`AttentionMapRenderer` colours whole tiles, this resolves the pixels inside them.
"""
import torch

from .attribution import bag_setup, bag_step, check_tiles, device_tiles, narrow_encoder  # noqa: F401  (re-exported: the step's old home)
from .preprocess import U8Tiles

METHODS = ("gradient", "grad_x_input")


class TileSaliency:
    """`TileSaliency(model)` for a `mil_amd.Attention`.  The bag is evaluated as the reference's `visualize()` evaluates a
    slide — eval mode: all tiles, no dropout — for the class `label`:

      input_gradient(tiles, label) -> fp32 [T,3,H,W], d loss / d tiles (the normalised tiles; for `U8Tiles` the decoded values)
      maps(tiles, label, method)   -> fp32 [T,H,W]: "gradient" = max_c |dx| (Simonyan et al.; reduced inside the stem's
                                      data-gradient kernel, the three-channel gradient is never written), "grad_x_input" =
                                      |sum_c dx * x|

    `tiles`: an fp32 [T,3,H,W] stack or `U8Tiles` (what `SlideBag.get_inference_data()` hands over).  A call leaves the model
    as it found it: the `training` flag is not touched, no parameter's `.grad` is created or changed, the torch RNG is not
    drawn from and `direct_grad` accumulation is not triggered (the head's parameters enter detached, the encoder's gradients
    are dropped)."""

    def __init__(self, model):
        narrow_encoder(model, "TileSaliency")
        self.model = model

    def _check(self, tiles, label):
        return check_tiles(self.model, tiles, label, "saliency")

    def _backward(self, tiles, label, reduce):
        """(dx, sal, the tensor the encoder read) for the checked arguments."""
        x = device_tiles(self.model, tiles)
        dx, sal = bag_step(self.model, bag_setup(self.model, x.shape[0], label), x, dx_reduce=reduce)[:2]
        return dx, sal, x

    def input_gradient(self, tiles, label):
        label = self._check(tiles, label)
        return self._backward(tiles, label, None)[0]

    def maps(self, tiles, label, method="gradient"):
        if method not in METHODS:
            raise ValueError(f"method must be one of {METHODS}, got {method!r}")
        label = self._check(tiles, label)
        if method == "gradient":
            return self._backward(tiles, label, "max_abs")[1]
        dx, _sal, x = self._backward(tiles, label, None)
        if x.dtype == torch.uint8:
            x = U8Tiles(x).float()
        return (dx * x).sum(1).abs()
