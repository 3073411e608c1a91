"""What the attribution classes share (TileSaliency, TileGradCam, TileIntegratedGradients, TileSmoothGrad, FeatureVisualizer):
the constructor, tile and channel checks, the move of the tiles to the device, and ONE evaluation of a bag for a label — the encoder's
forward, the head with its parameters detached, the gradient of the loss with respect to the features — which `bag_step`
continues to the pixels on the data-gradient-only walk (`encoder_pixel_gradient`).  DESIGN.md section 3.44.
"""
import contextlib

import torch

from . import _lib as L
from .encoder import ResNet, encoder_forward, encoder_pixel_gradient
from .head import BagLayout, head_apply
from .preprocess import S2dTiles, U8Tiles

LAYERS = ("layer1", "layer2", "layer3", "layer4")


def stage_of(layer):
    """1..4 for "layer1".."layer4" or the integer itself."""
    if isinstance(layer, str):
        if layer not in LAYERS:
            raise ValueError(f"layer must be one of {LAYERS} or 1..4, got {layer!r}")
        return LAYERS.index(layer) + 1
    if layer not in (1, 2, 3, 4) or isinstance(layer, bool):
        raise ValueError(f"layer must be one of {LAYERS} or 1..4, got {layer!r}")
    return int(layer)


def channel_list(channels, c, ntiles=None):
    """One channel in [0, c) per tile as a list of ints; None: all channels of the stage; an int: that channel for every tile."""
    if channels is None:
        if ntiles is not None:
            raise ValueError("channels: one per tile, or one int for all tiles")
        channels = range(c)
    elif isinstance(channels, int) and not isinstance(channels, bool):
        channels = [channels] * (1 if ntiles is None else ntiles)
    elif isinstance(channels, torch.Tensor):
        channels = channels.tolist()
    try:
        out = [int(k) for k in channels]
        exact = all(int(k) == k and not isinstance(k, bool) for k in channels)
    except (TypeError, ValueError):
        raise ValueError(f"channels must be integers, got {channels!r}") from None
    if not out or not exact:
        raise ValueError(f"channels must be a non-empty list of integers, got {list(channels)!r}")
    if ntiles is not None and len(out) != ntiles:
        raise ValueError(f"{len(out)} channels for {ntiles} tiles")
    bad = [k for k in out if not 0 <= k < c]
    if bad:
        raise ValueError(f"channels must lie in [0, {c}), got {bad}")
    return out


def narrow_encoder(model, who, bare=False, lacks="stem data-gradient kernel"):
    """The constructor check: `model` is a `mil_amd.Attention` — or, with `bare`, its encoder itself — with the narrow ResNet-26.
    Returns the encoder.  who: the class named in the message; lacks: what the wide encoder has not got for it."""
    from . import alt_resnet
    from .model import Attention
    if isinstance(model, Attention):
        net = model.cnn.module
    elif bare and isinstance(model, (ResNet, alt_resnet.ResNet)):
        net = model
    else:
        raise ValueError(f"{who} takes a mil_amd.Attention model" + (" or its narrow ResNet encoder" if bare else ""))
    if not isinstance(net, ResNet):
        raise ValueError(f"{who} needs the narrow ResNet-26 encoder: the wide encoder (alt_resnet) has no {lacks}")
    return net


def check_tiles(model, tiles, label, what, s2d=False):
    """The argument checks of the methods that take tiles, made before anything is launched; returns the label as an int (None
    with label=None, which skips the label's check: then `model` is not looked at).  what: the caller's word for its result;
    s2d: `S2dTiles` are taken as well, in the bf16 compute mode."""
    if isinstance(tiles, S2dTiles) and not s2d:
        raise ValueError(f"S2dTiles hold bf16-rounded space-to-depth records: {what} takes the fp32 stack or U8Tiles")
    if not isinstance(tiles, (torch.Tensor, U8Tiles, S2dTiles)):
        raise ValueError(f"tiles must be an fp32 [T,3,H,W] tensor{', U8Tiles or S2dTiles' if s2d else ' or U8Tiles'}, got {type(tiles).__name__}")
    if tiles.dim() != 4 or tiles.shape[1] != 3:
        raise ValueError(f"expected [T,3,H,W] tiles, got {tuple(tiles.shape)}")
    if isinstance(tiles, torch.Tensor) and not tiles.is_floating_point():
        raise ValueError(f"a tensor of tiles must be floating point (wrap uint8 images in U8Tiles), got {tiles.dtype}")
    if isinstance(tiles, S2dTiles) and model.cnn.module.compute_dtype != torch.bfloat16:
        raise ValueError("S2dTiles feed the bf16 compute mode only")
    if tiles.shape[0] < 1:
        raise ValueError(f"an empty bag has no {what}")
    if label is None:
        return None
    label = int(label)
    if not 0 <= label < model.C:
        raise ValueError(f"label must be in [0, {model.C}), got {label}")
    return label


def model_device(model, who="Attention"):
    """The device of an `Attention` model or of a bare encoder, which must be the GPU."""
    dev = (model.weight_mask if hasattr(model, "weight_mask") else model.conv1.weight).device
    if dev.type != "cuda":
        raise RuntimeError(f"{who} runs on an AMD GPU only (module parameters are not on a CUDA/HIP device)")
    return dev


def device_tiles(model, tiles, who="Attention"):
    """The tensor the encoder reads for checked `tiles`, on the model's device: the bytes of `U8Tiles`, the records of `S2dTiles`,
    else detached fp32."""
    dev = model_device(model, who)
    if isinstance(tiles, U8Tiles):
        return tiles.u8.to(dev)
    return tiles.xs.detach().to(dev) if isinstance(tiles, S2dTiles) else tiles.detach().to(dev, torch.float32)


@contextlib.contextmanager
def compute_mode(net):
    """Inside the block the kernels run in the encoder's compute mode; yields the storage dtype of its activations."""
    mode = net.compute_dtype
    with L.f32_mma(L.mma_code(mode)):
        yield L.storage_dtype(mode)


def bag_setup(model, ntiles, label):
    """What every evaluation of one bag of `ntiles` tiles for the class `label` shares: (layout, y, class weights)."""
    dev = model.weight_mask.device
    layout = BagLayout.cached([ntiles], dev)
    y = torch.tensor([label], dtype=torch.long, device=dev)
    cw = model.loss.weight
    if cw is not None:
        cw = torch.as_tensor(cw, dtype=torch.float32, device=dev).contiguous()
    return layout, y, cw


def bag_evaluate(model, setup, x, *, backward=True, weights=None):
    """One eval-mode evaluation of the bag `x` (what `device_tiles` returned, or an fp32 stack made on the device) as the
    reference's `visualize()` evaluates a slide: (the saved activations of `encoder_forward`, dH = d loss / d features [T,80],
    the detached loss [1]).  backward=False stops after the loss: dH is None.  To be called inside `compute_mode`.  The head's
    parameters enter detached (weights: `[w.detach() for w in model.head_weights()]`, for a caller that hoists them out of a
    loop): no `.grad` is touched, no direct accumulation is triggered, no random number is drawn."""
    layout, y, cw = setup
    net = model.cnn.module
    if weights is None:
        weights = [w.detach() for w in model.head_weights()]
    with torch.no_grad():
        feats, saved = encoder_forward(net, x, L.storage_dtype(net.compute_dtype))
    H = feats.detach().requires_grad_(backward)
    loss = head_apply(H, layout, y, None, cw, weights, None, direct=False)[0]
    dH = torch.autograd.grad(loss.sum(), H)[0] if backward else None
    return saved, dH, loss.detach()


def bag_step(model, setup, x, *, dx_reduce=None, dx_acc=None, backward=True):
    """`bag_evaluate` and the gradient of the loss with respect to the tiles: (dx, sal, loss [1]).  dx_reduce / dx_acc:
    `encoder_pixel_gradient`'s, the data-gradient-only walk — no weight gradient is launched, and dx is bit for bit that of
    `encoder_backward(want_dx=True)`.  backward=False: the loss alone."""
    net = model.cnn.module
    with compute_mode(net) as dtype:
        saved, dH, loss = bag_evaluate(model, setup, x, backward=backward)
        if not backward:
            return None, None, loss
        with torch.no_grad():
            dx, sal = encoder_pixel_gradient(net, saved, dtype, dfeats=dH, dx_reduce=dx_reduce, dx_acc=dx_acc)
    return dx, sal, loss
