"""CPU (-m "not gpu"): the colour jitter (mil_amd.ColorJitter / mil_color_jitter_u8, RoiBuilder.py:200) without a GPU — the numpy
restatement (tests/jitter_reference.py) against Pillow itself where Pillow is installed and against Pillow's recorded bytes
(tests/golden/jitter_chain.npz) everywhere, the constructor's ranges, the parameter draw, every refusal that must fire before a
launch, and the C entry's host-side status codes.  Every comparison is equality."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import _lib
from mil_amd import color_jitter as cj

import jitter_reference as jr
import roi_reference as rr

GROUPS = ("19", "32", "2", "1")


@functools.lru_cache(maxsize=None)
def _cube():
    c = rr.all_colours_image()
    c.setflags(write=False)
    return c


# ---- the restatement against Pillow ----------------------------------------------------------------------------------------------
def test_blend_equals_pillow_on_all_pairs():
    Image = pytest.importorskip("PIL.Image")
    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    im_d, im_x = Image.fromarray(d, "L"), Image.fromarray(x, "L")
    rng = np.random.default_rng(1)
    factors = [0.8, 1.2, 0.9, 1.1, 0.95, 1.05, 0.0, 0.5, 1.0, 2.0]
    factors += list(rng.uniform(0.8, 1.2, 100)) + list(rng.uniform(0.9, 1.1, 50)) + list(rng.uniform(0.0, 3.0, 50))
    for f in factors:
        f = float(np.float32(f))
        assert np.array_equal(jr.blend(d, x, f), np.asarray(Image.blend(im_d, im_x, f))), f


def test_grey_equals_pillow_on_all_colours():
    Image = pytest.importorskip("PIL.Image")
    assert np.array_equal(jr.grey(_cube()), np.asarray(Image.fromarray(_cube(), "RGB").convert("L")))


def test_hue_equals_pillow_on_all_colours():
    Image = pytest.importorskip("PIL.Image")
    hsv = np.asarray(Image.fromarray(_cube(), "RGB").convert("HSV"))
    assert np.array_equal(rr.rgb2hsv_float(_cube()), hsv)
    for shift in (0, 5, 128, 251):
        shifted = hsv.copy()
        shifted[..., 0] = ((hsv[..., 0].astype(np.int64) + shift) % 256).astype(np.uint8)
        want = np.asarray(Image.frombytes("HSV", (4096, 4096), shifted.tobytes()).convert("RGB"))
        for y in range(0, 4096, 1024):
            # jr.hue is rgb2hsv_float (equal on every colour, above), the shift and hsv2rgb: called as a whole at one shift
            got = jr.hue(_cube()[y:y + 1024], shift) if shift == 251 else jr.hsv2rgb(shifted[y:y + 1024])
            assert np.array_equal(got, want[y:y + 1024]), (shift, y)


def test_hsv2rgb_equals_pillow_on_all_triples():
    Image = pytest.importorskip("PIL.Image")
    want = np.asarray(Image.frombytes("HSV", (4096, 4096), _cube().tobytes()).convert("RGB"))
    for y in range(0, 4096, 1024):
        assert np.array_equal(jr.hsv2rgb(_cube()[y:y + 1024]), want[y:y + 1024]), y


def test_enhance_ops_and_contrast_mean_equal_pillow():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageStat
    rng = np.random.default_rng(2)
    for k in range(20):
        h, w = (int(v) for v in rng.integers(1, 40, 2))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        if k % 4 == 0:
            img = (img // 16 + 8 * k).astype(np.uint8)                  # a narrow band: means near a half-integer happen
        pim = Image.fromarray(img, "RGB")
        assert jr.contrast_mean(img) == int(ImageStat.Stat(pim.convert("L")).mean[0] + 0.5), k
        for f in (0.0, 0.5, 1.0, 2.0, 0.9, 1.1, float(np.float32(rng.uniform(0.8, 1.2)))):
            assert np.array_equal(jr.brightness(img, f), np.asarray(ImageEnhance.Brightness(pim).enhance(f))), (k, f)
            assert np.array_equal(jr.contrast(img, f), np.asarray(ImageEnhance.Contrast(pim).enhance(f))), (k, f)
            assert np.array_equal(jr.saturation(img, f), np.asarray(ImageEnhance.Color(pim).enhance(f))), (k, f)


# ---- the restatement against Pillow's recorded bytes (no Pillow needed) --------------------------------------------------------
def test_restatement_reproduces_the_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "jitter_chain.npz"))
    assert [z[f"in_{g}"].shape for g in GROUPS] == [(24, 3, 19, 19), (8, 3, 32, 32), (2, 3, 2, 2), (1, 3, 1, 1)]
    assert len({tuple(o) for o in z["order_19"]}) == 24 and (np.sort(z["order_19"], axis=1) == np.arange(4)).all()
    assert {0, 251} <= set(z["shift_19"].tolist()) | set(z["shift_32"].tolist())
    assert {0, 1, 2, 3} <= set((z["order_32"] == -1).sum(axis=1).tolist())                     # none, one, two, three ops off
    assert {0.0, 1.0, 2.0} <= set(z["factors_32"].ravel().tolist())
    for g in GROUPS:
        got = jr.jitter_tiles(z[f"in_{g}"], z[f"order_{g}"], z[f"factors_{g}"], z[f"shift_{g}"])
        assert got.dtype == np.uint8 and np.array_equal(got, z[f"out_{g}"]), g
        assert (z[f"out_{g}"] != z[f"in_{g}"]).any()
    assert jr.hue_shift(-0.02) == 251 and jr.hue_shift(0.02) == 5 and jr.hue_shift(0) == 0 and jr.hue_shift(0.5) == 127
    assert cj.hue_shift(-0.02) == 251 and cj.hue_shift(-0.5) == 129 and cj.hue_shift(0.003) == 0


# ---- the constructor ---------------------------------------------------------------------------------------------------------------
def test_ranges_and_switched_off_ops():
    j = mil_amd.ColorJitter(brightness=0.2, contrast=0.1, saturation=0.05, hue=0.02)          # RoiBuilder.py:200
    assert j.brightness == (0.8, 1.2) and j.contrast == (0.9, 1.1) and j.saturation == (0.95, 1.05) and j.hue == (-0.02, 0.02)
    assert mil_amd.ColorJitter().ranges == (None, None, None, None)
    assert mil_amd.ColorJitter(brightness=1.5).brightness == (0.0, 2.5)                       # max(0, 1 - x)
    j = mil_amd.ColorJitter(brightness=(0.5, 0.7), contrast=(1, 1), saturation=[1.0, 3.0], hue=(0, 0))
    assert j.ranges == ((0.5, 0.7), None, (1.0, 3.0), None)
    assert mil_amd.ColorJitter(hue=(-0.5, 0.5)).hue == (-0.5, 0.5) and mil_amd.ColorJitter(hue=(0.1, 0.1)).hue == (0.1, 0.1)
    assert "ColorJitter" in mil_amd.__all__


@pytest.mark.parametrize("kw", [dict(brightness=-0.1), dict(contrast=(1.2, 0.8)), dict(saturation=(-0.1, 1.0)), dict(hue=0.6),
                                dict(hue=(-0.6, 0.1)), dict(hue=-0.1), dict(brightness=(1.0,)), dict(contrast="0.1"),
                                dict(saturation=(0.9, 1.0, 1.1)), dict(brightness=float("inf")), dict(hue=None)])
def test_bad_constructor_values_raise(kw):
    with pytest.raises(ValueError):
        mil_amd.ColorJitter(**kw)


# ---- the draw ------------------------------------------------------------------------------------------------------------------------
def test_draw_params_shapes_ranges_and_reproducibility():
    j = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    p = j.draw_params(500, torch.Generator().manual_seed(5))
    assert isinstance(p, cj.JitterParams) and p._fields == ("order", "factors", "hue_shift")
    assert p.order.dtype == torch.int32 and tuple(p.order.shape) == (500, 4)
    assert p.factors.dtype == torch.float32 and tuple(p.factors.shape) == (500, 3)
    assert p.hue_shift.dtype == torch.int32 and tuple(p.hue_shift.shape) == (500,)
    assert not any(t.is_cuda for t in p)
    assert bool((p.order.sort(dim=1).values == torch.arange(4, dtype=torch.int32)).all())       # each op exactly once
    assert len({tuple(o) for o in p.order.tolist()}) == 24                                      # every order turns up
    lo, hi = torch.tensor([0.8, 0.9, 0.95]), torch.tensor([1.2, 1.1, 1.05])
    assert bool((p.factors >= lo).all()) and bool((p.factors <= hi).all())
    assert bool((p.factors.max(dim=0).values - p.factors.min(dim=0).values > 0.8 * (hi - lo)).all())
    assert set(p.hue_shift.tolist()) == {251, 252, 253, 254, 255, 0, 1, 2, 3, 4, 5}
    q = j.draw_params(500, torch.Generator().manual_seed(5))
    assert all(torch.equal(a, b) for a, b in zip(p, q))
    assert not torch.equal(p.factors, j.draw_params(500, torch.Generator().manual_seed(6)).factors)
    cj.checked_params(p, 500)                                                                   # what it draws, it accepts
    e = j.draw_params(0)
    assert tuple(e.order.shape) == (0, 4) and tuple(e.factors.shape) == (0, 3) and tuple(e.hue_shift.shape) == (0,)


def test_draw_params_with_switched_off_ops():
    j = mil_amd.ColorJitter(contrast=(0.5, 0.5), hue=(0.25, 0.25))
    p = j.draw_params(64, torch.Generator().manual_seed(7))
    assert bool(((p.order == 1).sum(dim=1) == 1).all()) and bool(((p.order == 3).sum(dim=1) == 1).all())
    assert bool(((p.order == -1).sum(dim=1) == 2).all()) and not bool((p.order == 0).any()) and not bool((p.order == 2).any())
    assert bool((p.factors[:, 1] == 0.5).all()) and bool((p.factors[:, 0] == 1).all()) and bool((p.factors[:, 2] == 1).all())
    assert bool((p.hue_shift == 63).all())
    assert {tuple(x for x in o if x >= 0) for o in p.order.tolist()} == {(1, 3), (3, 1)}
    off = mil_amd.ColorJitter().draw_params(3)
    assert bool((off.order == -1).all()) and bool((off.factors == 1).all()) and bool((off.hue_shift == 0).all())


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _params(n, order=(0, 1, 2, 3), factors=(1.1, 0.9, 1.0), shift=3):
    return cj.JitterParams(torch.tensor([order] * n, dtype=torch.int32), torch.tensor([factors] * n, dtype=torch.float32),
                           torch.tensor([shift] * n, dtype=torch.int32))


def test_apply_refuses_before_any_launch():
    j = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    tiles = mil_amd.U8Tiles(torch.zeros((2, 3, 8, 8), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        j.apply(tiles, _params(2))                                      # CPU tiles: no fallback
    for bad in (_params(3), _params(2, order=(0, 1, 2, 4)), _params(2, order=(0, 1, -2, 3)), _params(2, order=(0, 1, 1, -1)),
                _params(2, shift=256), _params(2, shift=-1), _params(2, factors=(1.0, float("nan"), 1.0)),
                _params(2, factors=(-0.5, 1.0, 1.0)), (torch.zeros((2, 4)), torch.ones((2, 3)), torch.zeros(2, dtype=torch.int32)),
                (torch.zeros((2, 3), dtype=torch.int32), torch.ones((2, 3)), torch.zeros(2, dtype=torch.int32)),
                (torch.zeros((2, 4), dtype=torch.int32), torch.ones((2, 4)), torch.zeros(2, dtype=torch.int32)), 5, None):
        with pytest.raises(ValueError):
            j.apply(tiles, bad)
    with pytest.raises(ValueError):
        j.apply(torch.zeros((2, 3, 8, 8), dtype=torch.uint8), _params(2))                       # a tensor, not the handle
    with pytest.raises(ValueError):
        j.apply(mil_amd.U8Tiles(torch.zeros((2, 3, 8, 6), dtype=torch.uint8)), _params(2))      # not square
    ok = cj.checked_params(_params(2, order=(-1, 3, -1, -1)), 2)                                # -1 may repeat
    assert ok.order.dtype == torch.int32 and ok.factors.dtype == torch.float32 and ok.hue_shift.dtype == torch.int32


def test_preprocessor_refuses_s2d_with_a_jitter_and_bad_params():
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    rois = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="out='u8'"):
        prep(rois, None, out="s2d", jitter=_params(2))
    with pytest.raises(ValueError, match="out='u8'"):
        prep.from_slide(slide, [(0, 0), (3, 5)], None, out="s2d", jitter=_params(2))
    for out in ("u8", "nchw"):
        with pytest.raises(ValueError):
            prep(rois, None, out=out, jitter=_params(3))                                        # one row per tile
        with pytest.raises(ValueError):
            prep.from_slide(slide, [(0, 0), (3, 5)], None, out=out, jitter=_params(2, order=(2, 2, 0, 1)))
        with pytest.raises(RuntimeError):
            prep(rois, None, out=out, jitter=_params(2))                                        # CPU ROIs: no fallback
    with pytest.raises(ValueError):
        prep(rois, None, out="nhwc", jitter=_params(2))
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=[(0, 0), (3, 5)])
    assert bag.color_jitter is None
    with pytest.raises(ValueError):
        bag.get_train_data(jitter_params=_params(2))                                            # a bag made without color_jitter=


# ---- the C entry's host-side checks ----------------------------------------------------------------------------------------------------
def test_entry_status_codes_need_no_gpu():
    assert "mil_color_jitter_u8" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(mil_amd.LIB_PATH), "mil_color_jitter_u8")
    f = mil_amd.lib().mil_color_jitter_u8
    buf = np.zeros(64, dtype=np.uint8)
    one = buf.ctypes.data
    for i in range(5):                                                   # any null pointer: MIL_ERR_ARG
        args = [one] * 5
        args[i] = None
        assert f(*args, 1, 2, None) == 1, i
    assert f(one, one, one, one, one, -1, 2, None) == 1
    assert f(one, one, one, one, one, 1, 0, None) == 1 and f(one, one, one, one, one, 1, -3, None) == 1
    assert f(one, one, one, one, one, 1, 5000, None) == 2 and f(one, one, one, one, one, 1, 4097, None) == 2
    assert f(one, one, one, one, one, 0, 5000, None) == 2               # the shape is refused whatever T is
    assert f(one, one, one, one, one, 0, 2, None) == 0 and f(one, one, one, one, one, 0, 4096, None) == 0
    assert mil_amd.lib().mil_abi_version() == 2
