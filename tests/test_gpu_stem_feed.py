"""-m gpu: what each tile feed (fp32 tiles, `U8Tiles`, `S2dTiles`) leaves in the encoders' saved state for the backward, and when
an in-place change of the caller's tensor between forward and backward raises.

The other feed tests hold values (every feed bit-equal to the fp32 feed); this module holds the saving policy itself, which no
test stated directly.  `_narrow_expect` and `_wide_expect` are that policy written out by hand from the per-feed forwards as
they stood before they were folded into `ops.stem_forward` (`encoder._encoder_forward_from`, `_encoder_forward_from_u8`,
`alt_resnet._forward`); they are not derived from the code under test.  Each expectation is
(which of saved xs / x is set, whose storage it is, whether the caller's tensor is version-checked).

One deliberate reading: under `keep_s2d` the uint8 feed (every mode) and the fp32 feed in split precision record `x_src` too,
but it is the library's own clone, so writing to the caller's tensor cannot (and must not) raise.  "Raises" is therefore
asserted as "x_src is set AND is the caller's storage", and both halves are asserted separately."""
import functools
import itertools

import pytest
import torch

import mil_amd
from mil_amd import alt_resnet as alt, encoder, ops

pytestmark = pytest.mark.gpu

MODES = {"bf16": torch.bfloat16, "bf16x3": mil_amd.BF16X3, "f32": torch.float32}
FUSED_SHAPE = (3, 64, 64)               # has a fused stem kernel in bf16 and in split precision
CHAIN_SHAPE = (2, 30, 34)               # W % 4 != 0: stem_s2d* -> conv -> maxpool_fwd in every mode
NARROW = [(feed, mode, keep, fb, shape)
          for feed, mode in itertools.product(("f32", "u8", "s2d"), MODES) if feed != "s2d" or mode == "bf16"
          for keep in (False, True) for fb in (True, False) for shape in (FUSED_SHAPE, CHAIN_SHAPE)]
WIDE = [(feed, mode) for feed, mode in itertools.product(("f32", "u8", "s2d"), ("bf16", "bf16x3")) if feed != "s2d" or mode == "bf16"]
OWN, CALLER, CLONE = "own", "caller", "clone"


def _narrow_expect(feed, mode, keep, fb, shape):
    """(xs, x, x_src): None, or whose storage the saved tensor is — CALLER's, a CLONE of the caller's tensor (same dtype and
    shape, other storage) or the stem's OWN space-to-depth tensor."""
    fused = shape == FUSED_SHAPE and mode != "f32"        # exact fp32 has no fused stem; the un-hooked net fuses wherever it can
    split = mode == "bf16x3"
    if feed == "s2d":                   # xs is the caller's tensor, always version-checked
        return CALLER, None, CALLER
    if not fused:                       # the chain's own xs (fp32 in the fp32 modes); the tiles are not kept
        return OWN, None, None
    if feed == "f32":
        if split:                       # never an s2d copy: the tiles, or under keep_s2d an fp32 clone of them
            return (None, CLONE, CLONE) if keep else (None, CALLER, CALLER)
        if keep or not fb:              # the fused forward writes xs
            return OWN, None, None
        return None, CALLER, CALLER
    if not fb and not split:            # u8: xs rebuilt by stem_s2d_u8 for the un-fused backward
        return OWN, None, None
    return (None, CLONE, CLONE) if keep else (None, CALLER, CALLER)


def _wide_expect(feed):
    """(xs, x8, x_src)."""
    return {"f32": (OWN, None, None), "u8": (None, CALLER, CALLER), "s2d": (CALLER, None, CALLER)}[feed]


@functools.lru_cache(maxsize=None)
def _net(wide, mode):
    torch.manual_seed(7)
    cls = alt.ResNet(alt.BasicBlock, [1, 1, 1, 1], num_classes=80, compute_dtype=MODES[mode]) if wide else \
        encoder.ResNet(layers=(1, 1, 1, 1), num_classes=80, compute_dtype=MODES[mode])
    return cls.cuda()


def _feed(feed, shape):
    """(what the encoder is called with, the caller's tensor behind it)."""
    u8 = torch.randint(0, 256, (shape[0], 3) + shape[1:], dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
    if feed == "u8":
        return mil_amd.U8Tiles(u8), u8
    if feed == "s2d":
        xs = ops.stem_s2d_u8(u8, torch.bfloat16)
        return mil_amd.S2dTiles(xs), xs
    x = mil_amd.U8Tiles(u8).float()
    return x, x


def _whose(t, caller, stem_dtype):
    if t is None:
        return None
    if t.data_ptr() == caller.data_ptr():
        return CALLER
    if t.dtype == caller.dtype and t.shape == caller.shape:
        assert torch.equal(t, caller)
        return CLONE
    assert t.dim() == 4 and t.shape[3] == 16 and t.dtype == stem_dtype, (tuple(t.shape), t.dtype)
    return OWN


def _check(net, feed, shape, keys, want, stem_dtype):
    handle, caller = _feed(feed, shape)
    for p in net.parameters():
        p.grad = None
    feats = net(handle)
    saved = feats.grad_fn.saved
    got = tuple(_whose(saved[k], caller, stem_dtype) for k in keys)
    assert got == want, (got, want)
    checked = saved["x_src"] is not None and saved["x_src"].data_ptr() == caller.data_ptr()
    assert checked == (want[2] == CALLER)
    if checked:
        assert saved["x_version"] == caller._version
    caller.add_(1)                      # the caller's tensor changes between forward and backward
    if checked:
        with pytest.raises(RuntimeError, match="modified in place"):
            feats.sum().backward()
    else:
        feats.sum().backward()
        torch.cuda.synchronize()
        assert net.conv1.weight.grad is not None and bool(torch.isfinite(net.conv1.weight.grad).all())


@pytest.mark.parametrize("feed,mode,keep,fb,shape", NARROW,
                         ids=[f"{f}-{m}-keep{int(k)}-fb{int(b)}-{s[1]}x{s[2]}" for f, m, k, b, s in NARROW])
def test_narrow_encoder_saves_what_the_policy_says(feed, mode, keep, fb, shape):
    net = _net(False, mode)
    net.keep_s2d, net.fuse_backward = keep, fb
    try:
        _check(net, feed, shape, ("xs", "x", "x_src"), _narrow_expect(feed, mode, keep, fb, shape),
               torch.bfloat16 if mode == "bf16" else torch.float32)
    finally:
        net.keep_s2d, net.fuse_backward = False, True


@pytest.mark.parametrize("feed,mode", WIDE, ids=[f"{f}-{m}" for f, m in WIDE])
def test_wide_encoder_saves_what_the_policy_says(feed, mode):
    _check(_net(True, mode), feed, (2, 64, 64), ("xs", "x8", "x_src"), _wide_expect(feed),
           torch.bfloat16 if mode == "bf16" else torch.float32)
