"""Pixel-level saliency of a slide's tiles: the gradient of the bag's loss with respect to the tiles, on the device.

The reference vendors a saliency toolkit (pytorch-cnn-visualizations-master/src: `vanilla_backprop.py`,
`grad_times_image.py`) and with its stock PyTorch model the gradient of a slide's class score with respect to the pixels is
one `x.requires_grad_()` away.  Here it is one backward pass of the hand-written encoder chain with the stem's data-gradient
kernel (`ops.stem_dgrad`) at its end; `AttentionMapRenderer` colours whole tiles, this resolves the pixels inside them.
"""
import torch

from . import _lib as L
from .encoder import ResNet, encoder_backward, encoder_forward
from .head import BagLayout, head_apply
from .preprocess import S2dTiles, U8Tiles

METHODS = ("gradient", "grad_x_input")


def check_tiles(model, tiles, label, what):
    """The argument checks the pixel-level methods share (TileSaliency, TileIntegratedGradients, TileSmoothGrad), made before
    anything is launched; returns the label as an int."""
    if isinstance(tiles, S2dTiles):
        raise ValueError(f"S2dTiles hold bf16-rounded space-to-depth records: {what} takes the fp32 stack or U8Tiles")
    if not isinstance(tiles, (torch.Tensor, U8Tiles)):
        raise ValueError(f"tiles must be an fp32 [T,3,H,W] tensor or U8Tiles, got {type(tiles).__name__}")
    if tiles.dim() != 4 or tiles.shape[1] != 3:
        raise ValueError(f"expected [T,3,H,W] tiles, got {tuple(tiles.shape)}")
    if isinstance(tiles, torch.Tensor) and not tiles.is_floating_point():
        raise ValueError(f"a tensor of tiles must be floating point (wrap uint8 images in U8Tiles), got {tiles.dtype}")
    if tiles.shape[0] < 1:
        raise ValueError(f"an empty bag has no {what}")
    label = int(label)
    if not 0 <= label < model.C:
        raise ValueError(f"label must be in [0, {model.C}), got {label}")
    return label


def device_tiles(model, tiles):
    """The tensor the encoder reads for checked `tiles`, on the model's device: the bytes of `U8Tiles`, else detached fp32."""
    dev = model.weight_mask.device
    if dev.type != "cuda":
        raise RuntimeError("Attention runs on an AMD GPU only (module parameters are not on a CUDA/HIP device)")
    return tiles.u8.to(dev) if isinstance(tiles, U8Tiles) else tiles.detach().to(dev, torch.float32)


def bag_setup(model, ntiles, label):
    """What every evaluation of one bag of `ntiles` tiles for the class `label` shares: (layout, y, class weights)."""
    dev = model.weight_mask.device
    layout = BagLayout.cached([ntiles], dev)
    y = torch.tensor([label], dtype=torch.long, device=dev)
    cw = model.loss.weight
    if cw is not None:
        cw = torch.as_tensor(cw, dtype=torch.float32, device=dev).contiguous()
    return layout, y, cw


def bag_step(model, setup, x, *, dx_reduce=None, dx_acc=None, backward=True):
    """One eval-mode evaluation of the bag `x` (what `device_tiles` returned, or an fp32 stack made on the device) as the
    reference's `visualize()` evaluates a slide, and the gradient of its loss with respect to the tiles: (dx, sal, loss [1]).
    dx_reduce / dx_acc: `encoder_backward`'s.  backward=False: the loss alone.  The head's parameters enter detached and the
    encoder's gradients are dropped: no `.grad` is touched, no direct accumulation is triggered, no random number is drawn."""
    net = model.cnn.module
    layout, y, cw = setup
    mode = net.compute_dtype
    dtype = L.storage_dtype(mode)
    with L.f32_mma(L.mma_code(mode)):
        with torch.no_grad():
            feats, saved = encoder_forward(net, x, dtype)
        H = feats.detach().requires_grad_(backward)
        loss = head_apply(H, layout, y, None, cw, [w.detach() for w in model.head_weights()], None, direct=False)[0]
        if not backward:
            return None, None, loss.detach()
        (dH,) = torch.autograd.grad(loss.sum(), H)
        with torch.no_grad():
            _grads, dx, sal = encoder_backward(net, saved, dH, dtype, allow_direct=False, want_dx=True, dx_reduce=dx_reduce, dx_acc=dx_acc)
    return dx, sal, loss.detach()


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
        from .model import Attention
        if not isinstance(model, Attention):
            raise ValueError("TileSaliency takes a mil_amd.Attention model")
        if not isinstance(model.cnn.module, ResNet):
            raise ValueError("TileSaliency needs the narrow ResNet-26 encoder: the wide encoder (alt_resnet) has no stem data-gradient kernel")
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
