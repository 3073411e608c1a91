"""Guided backpropagation and guided Grad-CAM of a slide's tiles, on the device.

The three files of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src) that change the RULE of the
backward pass: `guided_backprop.py` hooks every activation so that it hands on `(out > 0) * clamp(grad, min=0)`
(guided_backprop.py:41-50), `layer_activation_with_guided_backprop.py` seeds the same pass from one filter of one layer, and
`guided_gradcam.py` multiplies its result by the Grad-CAM mask.  Here the LeakyReLU derivative lives in the store epilogues of the
data-gradient kernels, where no hook reaches it, so the rule is a second instantiation of those kernels
(`encoder_pixel_gradient(rule="guided")`: `ops.conv_dgrad_rule`, the guided forms of `ops.maxpool_bwd` and
`ops.avgpool_fc_bwd_data`) and the Grad-CAM product is a third epilogue of the stem's data-gradient kernel
(`ops.stem_dgrad(gate=)`).  LeakyReLU(0.1) is read as a ReLU: where the output is not positive nothing passes (the toolkit's
literal product with a negative output would flip signs).  DESIGN.md section 3.45.
"""
import torch

from . import ops
from .attribution import LAYERS, bag_evaluate, bag_setup, channel_list, check_tiles, compute_mode, device_tiles, narrow_encoder, stage_of
from .encoder import STAGE_WIDTHS, encoder_forward, encoder_pixel_gradient, encoder_stage_gradient
from .gradcam import NORMALIZE, cam_bytes

RULE = "guided"


class TileGuidedBackprop:
    """`TileGuidedBackprop(model)` for a `mil_amd.Attention` with the narrow ResNet-26.  The bag is evaluated as the reference's
    `visualize()` evaluates a slide — eval mode: all tiles, no dropout:

      gradients(tiles, label)          -> fp32 [T,3,H,W]: the class evidence carried back to the pixels with negative gradients
                                          zeroed at every activation.  The evidence is MINUS the bag's loss for `label`, as in
                                          `TileGradCam`: the seed is -d loss / d features, and here the sign decides what passes
      maps(tiles, label)               -> fp32 [T,H,W] = max_c |gradients|, reduced inside the stem's data-gradient kernel (the
                                          three-channel tensor is never written)
      filters(tiles, layer, channels)  -> fp32 [T,3,H,W]: the same rule seeded from one filter of one stage — the gradient of the
                                          filter's mean activation (`FeatureVisualizer`'s objective, ascending) behind the gate:
                                          (A > 0) / (h w) at the tile's channel of the stage output A, zero elsewhere.
                                          channels: an int, or one channel per tile.  The forward stops behind `layer`; no
                                          label, no head

    `tiles`: an fp32 [T,3,H,W] stack or `U8Tiles`.  Results feed `AttributionRenderer` and `SlideBag.attribution_maps` as any
    other attribution.  A call leaves the model as it found it: the `training` flag is not touched, no parameter's `.grad` is
    created or changed, the torch RNG is not drawn from and `direct_grad` accumulation is not triggered; no weight gradient is
    launched."""

    def __init__(self, model):
        narrow_encoder(model, "TileGuidedBackprop", lacks="guided data-gradient kernels")
        self.model = model

    def _walk(self, tiles, label, reduce):
        label = check_tiles(self.model, tiles, label, "guided gradient")
        model = self.model
        net = model.cnn.module
        x = device_tiles(model, tiles)
        with compute_mode(net) as dtype:
            saved, dH, _loss = bag_evaluate(model, bag_setup(model, x.shape[0], label), x)
            with torch.no_grad():
                return encoder_pixel_gradient(net, saved, dtype, dfeats=-dH, dx_reduce=reduce, rule=RULE)

    def gradients(self, tiles, label):
        return self._walk(tiles, label, None)[0]

    def maps(self, tiles, label):
        return self._walk(tiles, label, "max_abs")[1]

    def filters(self, tiles, layer, channels):
        stage = stage_of(layer)
        check_tiles(self.model, tiles, None, "guided gradient")
        c = STAGE_WIDTHS[stage - 1]
        chans = channel_list(channels, c, tiles.shape[0])
        net = self.model.cnn.module
        x = device_tiles(self.model, tiles)
        ch = torch.tensor(chans, dtype=torch.int32).to(x.device)
        with torch.no_grad(), compute_mode(net) as dtype:
            _feats, saved = encoder_forward(net, x, dtype, upto=stage)
            # slope 0: -(A > 0) / (h w) at the tile's channel — minus the gated seed of the ascending objective
            _obj, dz = ops.stage_seed(saved["blocks"][-1][2], ch, c, slope=0.0)
            return encoder_pixel_gradient(net, saved, dtype, dz=dz.neg_(), stage=stage, rule=RULE)[0]


class TileGuidedGradCam:
    """`TileGuidedGradCam(model, layer="layer4")`: guided backpropagation at the resolution of the pixels, weighted by the class
    activation map of `layer` (guided_gradcam.py:23-26):

      gradients(tiles, label, offset=1.0, normalize="tile") -> fp32 [T,3,H,W]
                 = TileGuidedBackprop.gradients * (TileGradCam.maps / 255) per pixel, bit for bit (the quotient an IEEE division)

    ONE forward serves both: the stage's gradient and `ops.grad_cam` give the uint8 map exactly as `TileGradCam.maps` makes it
    (offset, normalize: its arguments), then the guided walk runs on the same saved activations and the stem's data-gradient
    kernel multiplies by the map as it stores (`ops.stem_dgrad(gate=)`): no ungated gradient tensor is made.  `tiles` and the
    side-effect contract: `TileGuidedBackprop`'s."""

    def __init__(self, model, layer="layer4"):
        narrow_encoder(model, "TileGuidedGradCam", lacks="guided data-gradient kernels")
        self.model = model
        self.stage = stage_of(layer)
        self.layer = LAYERS[self.stage - 1]

    def gradients(self, tiles, label, offset=1.0, normalize="tile"):
        if normalize not in NORMALIZE:
            raise ValueError(f"normalize must be one of {NORMALIZE}, got {normalize!r}")
        label = check_tiles(self.model, tiles, label, "guided class activation gradient")
        model = self.model
        net = model.cnn.module
        x = device_tiles(model, tiles)
        first, blks = net.stages()[self.stage - 1]
        with compute_mode(net) as dtype:
            saved, dH, _loss = bag_evaluate(model, bag_setup(model, x.shape[0], label), x)
            with torch.no_grad():
                evidence = -dH
                grad = encoder_stage_gradient(net, saved, evidence, dtype, self.stage)
                act = saved["blocks"][first + len(blks) - 1][2]
                cam = cam_bytes(act, grad, STAGE_WIDTHS[self.stage - 1], saved["tile_hw"], offset, normalize)
                return encoder_pixel_gradient(net, saved, dtype, dfeats=evidence, rule=RULE, gate=cam)[0]
