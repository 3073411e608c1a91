"""Guided backpropagation through the ResNet-26 backbone, restated in torch: what the guided tests hold the kernels to.

The rule is the hook of the saliency toolkit the reference vendors (pytorch-cnn-visualizations-master/src/guided_backprop.py:41-50):
every activation hands on `(out > 0) * clamp(grad, min=0)` — with LeakyReLU(0.1) read as a ReLU.  The
toolkit itself cannot be imported here (its misc_functions.py needs torchvision), so the rule is restated.

`backbone` follows the contract of `oracle.mil_oracle.backbone(patterns=)`: the forward takes every LeakyReLU's branch from a
GIVEN activation pattern (that of the implementation under test), so an fp64 run differentiates the very linear piece the kernels
took; the backward of each LeakyReLU is the rule, gated by that same pattern — which IS `out > 0` of the run the pattern was
read from.  The stem's LeakyReLU runs at full resolution, before the pool: its gate sees the sum of the pooling windows'
contributions to a pixel, as the toolkit's hook does.  Test infrastructure only."""
import torch
import torch.nn.functional as F

from oracle import mil_oracle as orc


class GuidedLeaky(torch.autograd.Function):
    """y = v where `pos`, else LEAK * v.  Backward: (pos) * clamp(g, min=0) — guided_backprop.py:41-50 with `pos` = (out > 0);
    clamp=False leaves g unclamped: pos * g, the derivative of a ReLU on the given pattern."""

    @staticmethod
    def forward(ctx, v, pos, clamp=True):
        ctx.save_for_backward(pos)
        ctx.clamp = clamp
        return torch.where(pos, v, orc.LEAK * v)

    @staticmethod
    def backward(ctx, g):
        (pos,) = ctx.saved_tensors
        if ctx.clamp:
            g = torch.clamp(g, min=0)
        return pos.to(g.dtype) * g, None, None


def stem_full_pattern(pat, h, w):
    """(winner index [T,20,Hp*Wp] into the h*w stem map, bool [T,20,h,w]: the pixel won a window with a positive value) from
    `stem_tap` / `stem_pos`.  A pixel no window elected gets False: nothing reaches it in either pass."""
    tap, pos = pat["stem_tap"], pat["stem_pos"]
    n, c, hp, wp = tap.shape
    oy = torch.arange(hp).view(1, 1, hp, 1)
    ox = torch.arange(wp).view(1, 1, 1, wp)
    iy, ix = 2 * oy - 1 + tap // 3, 2 * ox - 1 + tap % 3
    assert int(iy.min()) >= 0 and int(iy.max()) < h and int(ix.min()) >= 0 and int(ix.max()) < w      # winners are real pixels
    idx = (iy * w + ix).reshape(n, c, hp * wp)
    full = torch.zeros(n, c, h * w, dtype=torch.bool)
    full.scatter_(2, idx, pos.reshape(n, c, hp * wp))
    return idx, full.view(n, c, h, w)


def backbone(sd, x, patterns, clamp=True, upto=None, prefix="cnn.module."):
    """gbm/model.py:50-61 on the pattern `patterns` with guided LeakyReLUs: [T,3,H,W] -> [T,80], or with upto = 1..4 the output
    of that stage [T,C,h,w].  Differentiate the result to get the guided gradient of the input."""
    pre = F.conv2d(x, sd[prefix + "conv1.weight"], sd[prefix + "conv1.bias"], stride=2, padding=3)
    n, c, h, w = pre.shape
    idx, pos_full = stem_full_pattern(patterns, h, w)
    stem = GuidedLeaky.apply(pre, pos_full, clamp)
    t = stem.reshape(n, c, h * w).gather(2, idx).view(patterns["stem_tap"].shape)       # the pool, at the given winners
    for li, _planes, stride in orc.STAGES:
        for b in range(orc.BLOCKS_PER_STAGE):
            p, name = f"{prefix}layer{li}.{b}.", f"layer{li}.{b}"
            s = stride if b == 0 else 1
            o = GuidedLeaky.apply(F.conv2d(t, sd[p + "conv1.weight"], sd[p + "conv1.bias"], stride=s, padding=1), patterns[name + ".o1"], clamp)
            o = F.conv2d(o, sd[p + "conv2.weight"], sd[p + "conv2.bias"], stride=1, padding=1)
            key = p + "downsample.0.weight"
            shortcut = F.conv2d(t, sd[key], None, stride=s) if key in sd else t
            t = GuidedLeaky.apply(o + shortcut, patterns[name], clamp)
        if upto == li:
            return t
    return t.mean(dim=(2, 3)) @ sd[prefix + "fc.weight"].t()


def oracle_patterns(sd, x):
    """The activation pattern of an un-patterned oracle forward, in the form `patterns` takes (what tests/test_oracle_golden.py
    builds): for the CPU tests, which have no implementation under test to read one from."""
    pre = F.conv2d(x, sd["cnn.module.conv1.weight"], sd["cnn.module.conv1.bias"], stride=2, padding=3)
    stem = F.leaky_relu(pre, orc.LEAK)
    h, w = stem.shape[2:]
    pool, idx = F.max_pool2d(stem, kernel_size=3, stride=2, padding=1, return_indices=True)
    hp, wp = pool.shape[2:]
    oy = torch.arange(hp).view(1, 1, hp, 1)
    ox = torch.arange(wp).view(1, 1, 1, wp)
    pat = {"stem_tap": (idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1)), "stem_pos": pool > 0}
    t = pool
    for li, _planes, stride in orc.STAGES:
        for b in range(orc.BLOCKS_PER_STAGE):
            p, name = f"cnn.module.layer{li}.{b}.", f"layer{li}.{b}"
            s = stride if b == 0 else 1
            o = F.leaky_relu(F.conv2d(t, sd[p + "conv1.weight"], sd[p + "conv1.bias"], stride=s, padding=1), orc.LEAK)
            pat[name + ".o1"] = o > 0
            o = F.conv2d(o, sd[p + "conv2.weight"], sd[p + "conv2.bias"], stride=1, padding=1)
            key = p + "downsample.0.weight"
            t = F.leaky_relu(o + (F.conv2d(t, sd[key], None, stride=s) if key in sd else t), orc.LEAK)
            pat[name] = t > 0
    return pat
