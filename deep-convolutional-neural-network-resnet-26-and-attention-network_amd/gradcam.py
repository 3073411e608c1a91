"""Grad-CAM of a slide's tiles: which region of each tile drove the bag's class, at the resolution of a convolutional stage.

The other method of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src: `gradcam.py`).  With the
stock PyTorch model it takes a forward hook and a tensor hook on the target layer; here the stage's output is already kept by
the forward (`saved["blocks"]`), its gradient is the hand-written backward chain cut short (`encoder_stage_gradient`: for
`layer4` one pool-gradient launch, no convolution backward at all) and one kernel per bag turns the two into the toolkit's maps
(`ops.grad_cam`, csrc/grad_cam.hip).  `TileSaliency` resolves pixels through a whole encoder backward; this costs a forward.
"""
import torch

from . import ops
from .attribution import LAYERS, bag_evaluate, bag_setup, check_tiles, compute_mode, device_tiles, narrow_encoder, stage_of
from .encoder import STAGE_WIDTHS, encoder_stage_gradient

NORMALIZE = ("tile", "bag")


class TileGradCam:
    """`TileGradCam(model, layer="layer4")` for a `mil_amd.Attention` with the narrow ResNet-26.  The bag is evaluated as the
    reference's `visualize()` evaluates a slide — eval mode: all tiles, no dropout — for the class `label`:

      raw(tiles, label, offset=1.0)                   -> fp32 [T,h,w]: max(offset + sum_k w_k A_k, 0) at the stage's resolution,
                                                         w_k the tile's mean gradient of channel k (gradcam.py:75-84;
                                                         offset = 1.0 is the toolkit's `np.ones`)
      maps(tiles, label, offset=1.0, normalize="tile") -> uint8 [T,H,W]: min-max normalised, quantised and resized to the tile
                                                         with Pillow's LANCZOS filter, bit for bit what numpy and Pillow make of
                                                         `raw` (gradcam.py:85-89) — the toolkit's bytes before its final `/255`.
                                                         normalize="bag": one range for all tiles of the bag (their common
                                                         minimum and maximum, taken on the device) instead of each tile's own,
                                                         which keeps the tiles of a slide comparable

    The class evidence is MINUS the bag's loss for `label`: the head's backward kernel differentiates the loss only, so the
    gradient used is -d loss / d features.  The toolkit back-propagates the raw logit of the class; the two differ by the
    soft-max's derivative (and the head's other loss terms), and the sign is what the ReLU sees: a region that lowers the loss
    for `label` is positive evidence.
    Maps of non-square tiles are [H,W] (the toolkit's own `resize((shape[2], shape[3]))` swaps the two; not copied).

    `tiles`: what the encoder takes — an fp32 [T,3,H,W] stack, `U8Tiles`, or in the bf16 mode `S2dTiles`.  A call leaves the
    model as it found it: the `training` flag is not touched, no parameter's `.grad` is created or changed, the torch RNG is not
    drawn from and `direct_grad` accumulation is not triggered."""

    def __init__(self, model, layer="layer4"):
        narrow_encoder(model, "TileGradCam", lacks="stage-gradient path")
        self.model = model
        self.stage = stage_of(layer)
        self.layer = LAYERS[self.stage - 1]

    def _check(self, tiles, label):
        return check_tiles(self.model, tiles, label, "class activation map", s2d=True)

    def _stage_tensors(self, tiles, label):
        """(the stage's output, the gradient of minus the loss with respect to it, its real channels, the tiles' (H, W))."""
        model = self.model
        net = model.cnn.module
        x = device_tiles(model, tiles)
        first, blks = net.stages()[self.stage - 1]
        with compute_mode(net) as dtype:
            saved, dH, _loss = bag_evaluate(model, bag_setup(model, x.shape[0], label), x)
            with torch.no_grad():
                grad = encoder_stage_gradient(net, saved, -dH, dtype, self.stage)
        act = saved["blocks"][first + len(blks) - 1][2]
        return act, grad, STAGE_WIDTHS[self.stage - 1], saved["tile_hw"]

    def raw(self, tiles, label, offset=1.0):
        label = self._check(tiles, label)
        act, grad, c, hw = self._stage_tensors(tiles, label)
        return ops.grad_cam(act, grad, c, hw, offset=offset, want_map=False)[0]

    def maps(self, tiles, label, offset=1.0, normalize="tile"):
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
        label = self._check(tiles, label)
        return cam_bytes(*self._stage_tensors(tiles, label), offset, normalize)


def cam_bytes(act, grad, c, hw, offset, normalize):
    """The uint8 [T,H,W] maps of `TileGradCam.maps` from a stage's output and its gradient (`TileGuidedGradCam` makes its gate
    with the same launches)."""
    if normalize == "tile":
        return ops.grad_cam(act, grad, c, hw, offset=offset, want_raw=False)[1]
    raw = ops.grad_cam(act, grad, c, hw, offset=offset, want_map=False)[0]
    rng = torch.stack((raw.amin(), raw.amax()))
    return ops.grad_cam(act, grad, c, hw, offset=offset, value_range=rng, want_raw=False)[1]
