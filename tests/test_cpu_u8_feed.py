"""No GPU needed: the host side of the uint8 tile feed — the 256 values the kernels decode to (mil_u8_decode_table evaluates the
kernels' own decode expression, csrc/u8_feed.cuh, compiled for the host) and the `U8Tiles` handle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mil_amd
from oracle import preprocess_oracle as po


def _table():
    out = (ctypes.c_float * 256)()
    assert mil_amd.lib().mil_u8_decode_table(out) == 0
    return np.frombuffer(out, dtype=np.float32).copy()


def test_decode_table_is_the_reference_expression_bit_for_bit():
    tab = _table()
    want = ((torch.arange(256, dtype=torch.uint8).float() / 255) - 0.5) / 0.5
    assert np.array_equal(tab.view(np.uint32), want.numpy().view(np.uint32))
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, axis=2)            # an image holding every code
    orc = po.to_tensor_normalize(codes)
    assert orc.dtype == np.float32
    assert np.array_equal(orc[0].reshape(-1).view(np.uint32), tab.view(np.uint32))
    assert tab[0] == -1.0 and tab[255] == 1.0                                              # code 0 is NOT the conv's zero padding
    assert mil_amd.lib().mil_u8_decode_table(None) == 1


def test_decode_is_not_a_multiply():
    """Why the kernels carry a Newton-corrected decode: the cheap forms differ from the reference's division on many of the 256 codes."""
    u = np.arange(256, dtype=np.float32)
    tab = _table()
    mul = (u * np.float32(1.0 / 255.0) - np.float32(0.5)) * np.float32(2.0)
    assert int((mul != tab).sum()) > 50


def test_u8tiles_surface_and_errors():
    g = torch.Generator().manual_seed(3)
    u = torch.randint(0, 256, (7, 3, 10, 12), dtype=torch.uint8, generator=g)
    h = mil_amd.U8Tiles(u)
    assert tuple(h.shape) == (7, 3, 10, 12) and h.dim() == 4 and len(h) == 7 and h.device == u.device
    assert h.u8.dtype == torch.uint8 and h.u8.data_ptr() == u.data_ptr()                   # a handle, not a copy
    assert torch.equal(h[2:5].u8, u[2:5]) and tuple(h[2:5].shape) == (3, 3, 10, 12)
    idx = torch.tensor([6, 0, 3])
    assert torch.equal(h[idx].u8, u[idx])
    assert torch.equal(mil_amd.U8Tiles.cat([h[:2], h[5:]]).u8, torch.cat([u[:2], u[5:]]))
    d = h.detach()
    assert isinstance(d, mil_amd.U8Tiles) and d.u8.data_ptr() == u.data_ptr()
    f = h.float()
    assert f.dtype == torch.float32 and tuple(f.shape) == (7, 3, 10, 12)
    assert torch.equal(f, ((u.float() / 255) - 0.5) / 0.5)
    assert np.array_equal(f.numpy(), _table()[u.numpy()])                                  # the table IS the decode
    with pytest.raises(ValueError):
        mil_amd.U8Tiles(u.float())                                                         # wrong dtype
    with pytest.raises(ValueError):
        mil_amd.U8Tiles(u[0])                                                              # wrong rank
    with pytest.raises(ValueError):
        mil_amd.U8Tiles(torch.zeros((2, 4, 8, 8), dtype=torch.uint8))                      # wrong channel count
    with pytest.raises(ValueError):
        mil_amd.U8Tiles(u.permute(0, 2, 3, 1))                                             # interleaved [T,H,W,3] is not the layout
    # a non-contiguous planar view is taken as a contiguous copy
    assert mil_amd.U8Tiles(u[:, :, ::2]).u8.is_contiguous()
    assert mil_amd.U8Tiles is mil_amd.preprocess.U8Tiles and "U8Tiles" in mil_amd.__all__


def test_u8tiles_float_of_pillows_bytes_is_the_reference_tensor(golden_dir):
    z = np.load(os.path.join(golden_dir, "prep_s1200_r300_train.npz"))
    img = z["out_u8"]                                                                      # [T,300,300,3]: Pillow's own bytes
    h = mil_amd.U8Tiles(torch.from_numpy(img).permute(0, 3, 1, 2).contiguous())
    want = np.stack([po.to_tensor_normalize(t) for t in img])
    assert np.array_equal(h.float().numpy().view(np.uint32), want.view(np.uint32))


def test_new_entry_points_are_declared_and_bound():
    names = ("mil_u8_decode_table", "mil_tile_preprocess_u8", "mil_stem_s2d_u8", "mil_stem_fwd_fused_u8",
             "mil_stem_bwd_fused_u8_workspace", "mil_stem_bwd_fused_u8")
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mil_hip.h")).read()
    for n in names:
        assert n in mil_amd._lib.EXPORTS and hasattr(mil_amd.lib(), n) and ("int " + n + "(") in hdr, n
    assert mil_amd.lib().mil_abi_version() == 2
