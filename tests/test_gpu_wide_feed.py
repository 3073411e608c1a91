"""-m gpu: the wide encoder (`alt_resnet.ResNet`) fed by `U8Tiles` and `S2dTiles`, and the 64-channel fused stem forward from
bytes under it (`stem_fwd_fused_kernel<4, 4, false, false, true>`, csrc/stem_fused.hip).

Every comparison is against the wide encoder's own fp32 feed on the decoded tensor `U8Tiles(u8).float()`, which
tests/test_gpu_alt_resnet.py, test_gpu_wide_x3.py and test_gpu_alt_vjp.py hold to the reference goldens and to fp64.  The decode
is lossless and both feeds run the same arithmetic on the same values, so the comparisons are bit for bit (`torch.equal`) and
carry those guarantees over; no tolerance appears in this module.  The bytes are random uint8 from a seeded `torch.Generator`,
the weights the constructor's own under `torch.manual_seed`."""
import functools

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import alt_resnet as alt, ops

pytestmark = pytest.mark.gpu

MODES = [torch.bfloat16, torch.float32, mil_amd.BF16X3]
MODE_IDS = ["bf16", "f32", "bf16x3"]
# (n, H, W) of the kernel test: what the 8 x 16 pooled-pixel tile (64 input columns x 32 input rows) can get wrong
STEM_SHAPES = [
    (1, 16, 16),        # the image is smaller than one tile
    (3, 36, 44),        # partial tiles in both directions, odd pooled sizes 9 x 11
    (2, 96, 80),        # the wide golden's shape: three row tiles, two column tiles
    (2, 64, 136),       # three column tiles, the last partial
]
# name -> (layers, num_classes, (n, H, W)): the two configurations of the wide goldens, and a shape without a fused stem
CONFIGS = {
    "l1111_4x64x64": ((1, 1, 1, 1), 80, (4, 64, 64)),
    "l2222_2x96x80": ((2, 2, 2, 2), 80, (2, 96, 80)),
    "l1111_2x50x70": ((1, 1, 1, 1), 80, (2, 50, 70)),       # W % 4 != 0: stem_s2d(_u8) -> conv -> maxpool_fwd
}
FUSED = ["l1111_4x64x64", "l2222_2x96x80"]


def _bytes(n, h, w, seed):
    return torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def _make_net(layers, num_classes, mode, seed=1234):
    torch.manual_seed(seed)
    return alt.ResNet(alt.BasicBlock, list(layers), num_classes=num_classes, compute_dtype=mode).cuda()


def _step(net, feed):
    """Features and every parameter gradient of one forward + `feats.sum().backward()`."""
    for p in net.parameters():
        p.grad = None
    feats = net(feed)
    feats.sum().backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    assert all(g is not None for g in grads.values())
    return feats.detach().clone(), grads


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and list(a[1]) == list(b[1]) and all(torch.equal(_bits(g), _bits(b[1][k])) for k, g in a[1].items())


def _assert_same(got, want, what):
    assert got[0].shape == want[0].shape and torch.equal(_bits(got[0]), _bits(want[0])), (what, "features", float((got[0] - want[0]).abs().max()))
    assert list(got[1]) == list(want[1])
    for k, g in got[1].items():
        assert torch.equal(_bits(g), _bits(want[1][k])), (what, k, float((g - want[1][k]).abs().max()))


@functools.lru_cache(maxsize=None)
def _case(cfg, mi):
    """The net, the bytes and the fp32 feed's step for CONFIGS[cfg] in MODES[mi]: computed once, shared, never modified.  The
    fp32 feed runs twice: the tests compare bits, so it has to be bit-repeatable itself."""
    layers, nc, shape = CONFIGS[cfg]
    net = _make_net(layers, nc, MODES[mi])
    u8 = _bytes(*shape, seed=100 + 7 * len(cfg) + mi)
    x = mil_amd.U8Tiles(u8).float()
    assert x.dtype == torch.float32 and tuple(x.shape) == tuple(u8.shape)
    ref, again = _step(net, x), _step(net, x)
    return net, u8, ref, _same(ref, again)


def _reference(cfg, mi):
    net, u8, ref, repeatable = _case(cfg, mi)
    assert repeatable, f"the fp32 feed of {cfg} / {MODE_IDS[mi]} is not bit-repeatable on this device: there is nothing to compare a feed against"
    assert float(ref[0].abs().max()) > 0 and all(bool(torch.isfinite(g).all()) for g in ref[1].values())
    assert float(ref[1]["conv1.weight"].abs().max()) > 0
    return net, u8, ref


# ---- 3. the kernel: 64-channel fused stem forward from bytes (bf16) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stem_filter():
    """The constructor's own conv1 filter, packed as `alt_resnet._forward` packs it (bf16)."""
    net = _make_net((1, 1, 1, 1), 80, torch.bfloat16, seed=4321)
    return alt._packed_stem(net, torch.bfloat16)


@pytest.mark.parametrize("shape", STEM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem64_forward_u8_equals_the_fp32_feed(shape):
    wp, bp = _stem_filter()
    u8 = _bytes(*shape, seed=shape[1] + shape[2])
    got = ops.stem_fwd_fused_u8(u8, wp, bp, 64, slope=0.0)
    assert got is not None, "no fused 64-channel stem from bytes: a silent fallback would hide a missing kernel"
    want = ops.stem_fwd_fused(mil_amd.U8Tiles(u8).float(), wp, bp, 64, slope=0.0, keep_s2d=False)
    assert want is not None and want[0] is None
    torch.cuda.synchronize()
    (pool, widx), (pool_f, widx_f) = got, want[1:]
    n, h, w = shape
    hp, wo = (h // 2 - 1) // 2 + 1, (w // 2 - 1) // 2 + 1
    assert tuple(pool.shape) == tuple(widx.shape) == (n, hp, wo, 64) and pool.dtype == torch.bfloat16 and widx.dtype == torch.uint8
    assert torch.equal(_bits(pool), _bits(pool_f)), float((pool.float() - pool_f.float()).abs().max())
    assert torch.equal(widx, widx_f), int((widx != widx_f).sum())
    assert float(pool.float().abs().max()) > 0


def test_stem64_forward_u8_on_a_slice_of_the_stack():
    """`U8Tiles[idx]` hands the kernel a pointer into the stack: an image is 3 H W bytes, a multiple of 4 wherever W % 4 == 0."""
    wp, bp = _stem_filter()
    for shape in STEM_SHAPES:
        u8 = _bytes(shape[0] + 1, *shape[1:], seed=5)
        assert u8.data_ptr() % 4 == 0 and u8[1:].data_ptr() % 4 == 0, shape
    u8 = _bytes(3, 36, 44, seed=6)
    whole, part = ops.stem_fwd_fused_u8(u8, wp, bp, 64, slope=0.0), ops.stem_fwd_fused_u8(u8[1:], wp, bp, 64, slope=0.0)
    assert whole is not None and part is not None
    assert torch.equal(_bits(part[0]), _bits(whole[0][1:])) and torch.equal(part[1], whole[1][1:])


def test_stem64_forward_u8_refuses_what_it_cannot_do():
    wp, bp = _stem_filter()
    assert ops.stem_fwd_fused_u8(_bytes(2, 50, 70, seed=1), wp, bp, 64, slope=0.0) is None            # W % 4 != 0
    assert ops.stem_fwd_fused_u8(_bytes(2, 33, 64, seed=1), wp, bp, 64, slope=0.0) is None            # odd H
    from mil_amd import _lib as L
    with L.f32_mma(L.MIL_DT_F32S):                                                                    # split precision: as stem_fwd_fused
        assert ops.stem_fwd_fused_u8(_bytes(2, 64, 64, seed=1), wp, bp, 64, slope=0.0, dtype=torch.float32) is None
    assert ops.stem_fwd_fused_u8(_bytes(2, 64, 64, seed=1), wp, bp, 64, slope=0.0, dtype=torch.float32) is None   # exact fp32


# ---- 4. the encoder --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", range(3), ids=MODE_IDS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_wide_encoder_on_u8tiles_equals_the_fp32_feed(cfg, mi):
    net, u8, ref = _reference(cfg, mi)
    _assert_same(_step(net, mil_amd.U8Tiles(u8)), ref, "U8Tiles")
    host = mil_amd.U8Tiles(u8.cpu())                                  # a handle that still lives on the host: moved as uint8
    assert not host.u8.is_cuda
    _assert_same(_step(net, host), ref, "U8Tiles on the CPU")


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_wide_encoder_on_s2dtiles_equals_the_fp32_feed_bf16(cfg):
    net, u8, ref = _reference(cfg, 0)
    xs = ops.stem_s2d_u8(u8, torch.bfloat16)
    before = xs.clone()
    _assert_same(_step(net, mil_amd.S2dTiles(xs)), ref, "S2dTiles")
    assert torch.equal(_bits(xs), _bits(before))                      # the handle's own tensor is read, never written


@pytest.mark.parametrize("cfg", FUSED)
def test_wide_encoder_bf16_takes_the_fused_stem_for_both_handles(cfg, monkeypatch):
    """What the equalities above cannot see: that the fused kernels ran and that nothing made an fp32 stack."""
    net, u8, _ref = _reference(cfg, 0)
    calls = []

    def spy(name):
        real = getattr(ops, name)

        def wrapped(*a, **kw):
            out = real(*a, **kw)
            calls.append((name, out is not None))
            return out
        monkeypatch.setattr(ops, name, wrapped)
    for name in ("stem_fwd_fused", "stem_fwd_fused_u8", "stem_fwd_fused_xs", "stem_s2d", "stem_s2d_u8"):
        spy(name)
    _step(net, mil_amd.U8Tiles(u8))
    assert calls == [("stem_fwd_fused_u8", True), ("stem_s2d_u8", True)], calls      # forward fused; xs rebuilt for the backward only
    del calls[:]
    xs = mil_amd.S2dTiles(ops.stem_s2d_u8(u8, torch.bfloat16))
    del calls[:]
    _step(net, xs)
    assert calls == [("stem_fwd_fused_xs", True)], calls


@pytest.mark.parametrize("feed", ["u8-bf16", "u8-bf16x3", "s2d-bf16"])
def test_in_place_change_between_forward_and_backward_raises(feed):
    kind, mode = feed.split("-")
    net = _make_net((1, 1, 1, 1), 80, torch.bfloat16 if mode == "bf16" else mil_amd.BF16X3)
    u8 = _bytes(2, 64, 64, seed=9)
    if kind == "u8":
        handle, tensor = mil_amd.U8Tiles(u8), u8
    else:
        tensor = ops.stem_s2d_u8(u8, torch.bfloat16)
        handle = mil_amd.S2dTiles(tensor)
    feats = net(handle)
    tensor.add_(1)
    with pytest.raises(RuntimeError, match="modified in place"):
        feats.sum().backward()
    feats = net(handle)                                               # untouched until backward: fine
    feats.sum().backward()
    assert net.conv1.weight.grad is not None


def test_s2dtiles_are_refused_in_the_fp32_modes():
    xs = mil_amd.S2dTiles(ops.stem_s2d_u8(_bytes(2, 64, 64, seed=9), torch.bfloat16))
    for mode in (torch.float32, mil_amd.BF16X3):
        with pytest.raises(ValueError, match="bf16 compute mode only"):
            _make_net((1, 1, 1, 1), 80, mode)(xs)


# ---- 5. end to end: slide -> SlideBag -> wide encoder ------------------------------------------------------------------------------
@pytest.mark.parametrize("mi", range(3), ids=MODE_IDS)
def test_slide_bag_feeds_the_wide_encoder(mi):
    rng = np.random.default_rng(11)
    slide = torch.from_numpy(rng.integers(0, 256, (300, 410, 3), dtype=np.uint8)).cuda()
    coords = [(0, 0), (3, 141), (180, 290), (91, 7), (177, 155)]
    bag = mil_amd.SlideBag(slide, roi_size=120, resolution=32, pad=10, coords=coords)
    assert bag.build() and bag.ntiles == 5
    net = _make_net((1, 1, 1, 1), 80, MODES[mi])
    val = bag.get_validation_data()                                   # the default: out="u8"
    trn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    val_f = bag.get_validation_data(out="nchw")
    trn_f = bag.get_train_data(generator=torch.Generator().manual_seed(8), out="nchw")
    for what, h, x in (("validation", val, val_f), ("train", trn, trn_f)):
        assert isinstance(h, mil_amd.U8Tiles) and tuple(h.shape) == (5, 3, 32, 32) and x.dtype == torch.float32
        assert torch.equal(_bits(h.float()), _bits(x)), what
        with torch.no_grad():
            got, want = net(h), net(x)
        assert tuple(got.shape) == (5, 80) and torch.equal(_bits(got), _bits(want)), (what, float((got - want).abs().max()))
        assert float(want.abs().max()) > 0
    if mi == 0:                                                       # the third output form, bf16 mode
        xs = bag.get_validation_data(out="s2d")
        with torch.no_grad():
            assert torch.equal(_bits(net(xs)), _bits(net(val_f)))
