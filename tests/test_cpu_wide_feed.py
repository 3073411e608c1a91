"""No GPU needed: the host side of the wide encoder's uint8 / space-to-depth feed — what `mil_stem_fwd_fused_u8` answers for the
64-channel stem before any launch, and what `alt_resnet.ResNet.forward` refuses before any device call."""
import ctypes

import pytest
import torch

import mil_amd
from mil_amd import _lib as L

MIL_OK, MIL_ERR_ARG, MIL_ERR_UNSUPPORTED = 0, 1, 2


def _call(x, w, pool, widx, n_img, h, wd, cout_p, dtype):
    return mil_amd.lib().mil_stem_fwd_fused_u8(x, w, None, pool, widx, n_img, h, wd, cout_p, 0.0, dtype, None)


@pytest.fixture(scope="module")
def host_ptrs():
    """Four non-null, 4-byte aligned HOST pointers: none of the calls below may reach a launch (n_img = 0, or refused first)."""
    bufs = [(ctypes.c_uint32 * 16)() for _ in range(4)]
    ptrs = [ctypes.addressof(b) for b in bufs]
    assert all(p % 4 == 0 for p in ptrs)
    return bufs, ptrs


def test_stem_fwd_fused_u8_takes_the_64_channel_stem_in_bf16_only(host_ptrs):
    _bufs, (x, w, pool, widx) = host_ptrs
    assert _call(x, w, pool, widx, 0, 64, 64, 64, L.MIL_DT_BF16) == MIL_OK                 # MIL_ERR_UNSUPPORTED before this feed existed
    assert _call(x, w, pool, widx, 0, 64, 64, 24, L.MIL_DT_BF16) == MIL_OK                 # the 20-channel stem: as before
    assert _call(x, w, pool, widx, 0, 64, 64, 24, L.MIL_DT_F32S) == MIL_OK
    assert _call(x, w, pool, widx, 0, 64, 64, 64, L.MIL_DT_F32S) == MIL_ERR_UNSUPPORTED    # no fused 64-channel split-precision stem
    assert _call(x, w, pool, widx, 4, 64, 64, 64, L.MIL_DT_F32S) == MIL_ERR_UNSUPPORTED
    assert _call(x, w, pool, widx, 0, 64, 64, 64, L.MIL_DT_F32) == MIL_ERR_UNSUPPORTED
    assert _call(x, w, pool, widx, 0, 64, 64, 40, L.MIL_DT_BF16) == MIL_ERR_UNSUPPORTED


def test_stem_fwd_fused_u8_64_argument_and_shape_checks(host_ptrs):
    _bufs, (x, w, pool, widx) = host_ptrs
    for args in ((None, w, pool, widx), (x, None, pool, widx), (x, w, None, widx), (x, w, pool, None)):
        assert _call(*args, 4, 64, 64, 64, L.MIL_DT_BF16) == MIL_ERR_ARG
    assert _call(x, w, pool, widx, -1, 64, 64, 64, L.MIL_DT_BF16) == MIL_ERR_ARG
    assert _call(x, w, pool, widx, 4, 50, 70, 64, L.MIL_DT_BF16) == MIL_ERR_UNSUPPORTED    # W % 4 != 0
    assert _call(x, w, pool, widx, 4, 33, 64, 64, L.MIL_DT_BF16) == MIL_ERR_UNSUPPORTED    # odd H
    assert _call(x + 1, w, pool, widx, 4, 64, 64, 64, L.MIL_DT_BF16) == MIL_ERR_UNSUPPORTED  # x not 4-byte aligned


@pytest.mark.parametrize("mode", [torch.float32, mil_amd.BF16X3], ids=["f32", "bf16x3"])
def test_wide_encoder_refuses_s2dtiles_outside_bf16_mode(mode):
    """Raised by `ResNet.forward` itself, on the host: the parameters and the handle live on the CPU here."""
    from mil_amd import alt_resnet
    torch.manual_seed(0)
    net = alt_resnet.ResNet(layers=(1, 1, 1, 1), num_classes=8, compute_dtype=mode)
    xs = mil_amd.S2dTiles(torch.zeros((2, 16, 16, 16), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 compute mode only"):
        net(xs)
    with pytest.raises(ValueError, match="bf16 compute mode only"):
        net(xs.xs)                                                  # the bare tensor is told apart by its dtype, as in encoder.ResNet
    with pytest.raises(ValueError, match="must be the space-to-depth tensor"):
        net(torch.zeros((2, 3, 16, 12), dtype=torch.bfloat16))      # bf16, but not [T,H/2,W/2,16]
    with pytest.raises(ValueError, match="planar tile stack"):
        net(torch.zeros((2, 16, 16, 3), dtype=torch.uint8))         # uint8, but interleaved
