"""CPU (-m "not gpu"): the from-slide tile pre-processing without a GPU — the three mil_tile_preprocess_win* entries refuse bad
arguments with a status code before any GPU call, and the host bookkeeping of `mil_amd.SlideBag` (argument checks, the
`coords=` round trip, the `max_tiles` cap with injected indices)."""
import ctypes

import numpy as np
import pytest
import torch

import mil_amd

ENTRIES = ("mil_tile_preprocess_win", "mil_tile_preprocess_win_u8", "mil_tile_preprocess_win_s2d")


@pytest.mark.parametrize("name", ENTRIES)
def test_win_entries_refuse_bad_arguments_without_a_gpu(name):
    from mil_amd import _lib
    assert name in _lib.EXPORTS and hasattr(ctypes.CDLL(mil_amd.LIB_PATH), name)
    f = getattr(mil_amd.lib(), name)
    s, r = 16, 8
    # host memory standing in for every pointer: a refused call dereferences none of them
    src = np.zeros(64 * 64 * 3 + 64, np.uint8)
    off, params = np.zeros(4, np.int64), np.zeros((4, 4), np.int32)
    bounds, kk, out = np.zeros((r, 2), np.int32), np.zeros((r, 8), np.int32), np.zeros(4 * 3 * r * r, np.float32)
    assert out.ctypes.data % 16 == 0 or name != "mil_tile_preprocess_win_s2d"
    good = [src.ctypes.data, src.size, off.ctypes.data, 3 * 64, params.ctypes.data, bounds.ctypes.data, bounds.ctypes.data,
            kk.ctypes.data, out.ctypes.data, 4, s, 4, r, None]

    def call(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*a)

    for i in (0, 2, 5, 6, 7, 8):                                  # base, win_off, bounds_host, bounds_dev, kk_dev, out
        assert call(**{f"a{i}": None}) == 1, i
    assert f(None, 0, None, 0, None, None, None, None, None, 1, s, 4, r, None) == 1
    assert call(a3=3 * s - 1) == 1 and call(a3=0) == 1 and call(a3=-192) == 1          # row_pitch < 3 S
    assert call(a1=-1) == 1                                       # base_bytes < 0
    assert call(a9=-1) == 1 and call(a10=0) == 1 and call(a12=0) == 1 and call(a11=-1) == 1       # T, S, R, pad
    assert mil_amd.lib().mil_abi_version() == 2


def _bag(**kw):
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8)
    coords = [(0, 0), (10, 20), (84, 104), (3, 7), (50, 50)]
    return mil_amd.SlideBag(slide, 16, 2, coords=coords, **kw), coords


def test_slide_bag_argument_checks():
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8)
    for bad in (slide.float(), slide[..., :2], slide[0], slide.numpy()):
        with pytest.raises(ValueError):
            mil_amd.SlideBag(bad, 16)
    for kw in ({"roi_size": 0}, {"padding": -1}, {"pad": -1}, {"max_tiles": 0}):
        with pytest.raises(ValueError):
            mil_amd.SlideBag(slide, **{"roi_size": 16, **kw})
    with pytest.raises(ValueError):
        mil_amd.SlideBag(slide, 16, selector=mil_amd.RoiSelector(roi_size=32))
    for bad in ([(85, 0)], [(0, 105)], [(-1, 0)], [(0.5, 1.0)]):
        with pytest.raises(ValueError):
            mil_amd.SlideBag(slide, 16, coords=bad)
    bag = mil_amd.SlideBag(slide, 16)
    assert bag.ntiles == -1 and bag.coords is None and bag.resolution is None
    with pytest.raises(RuntimeError):
        bag.get_validation_data()                                 # neither built nor given a resolution
    with pytest.raises(RuntimeError):
        bag.choose()
    with pytest.raises(RuntimeError):
        bag.rois([0])


def test_slide_bag_coords_round_trip_and_cap():
    bag, coords = _bag(max_tiles=3)
    assert bag.ntiles == 5 and bag.coords.dtype == np.int64 and np.array_equal(bag.coords, np.asarray(coords))
    assert bag.build() and bag.ntiles == 5                        # a loaded coor_cache: nothing to select (and no GPU needed)
    again = mil_amd.SlideBag(bag.slide, 16, 2, coords=torch.from_numpy(bag.coords))
    assert np.array_equal(again.coords, bag.coords) and again.choose() is None          # 5 <= 2500: every window, in order
    assert tuple(mil_amd.SlideBag(bag.slide, 16, coords=[]).coords.shape) == (0, 2)
    # the cap: injected indices are taken as given; a draw holds max_tiles distinct indices and follows the generator
    assert bag.choose(choice=[4, 0, 2]).tolist() == [4, 0, 2]
    assert bag.choose(choice=torch.tensor([1, 3, 2])).tolist() == [1, 3, 2]
    for bad in ([0, 1], [0, 1, 1], [0, 1, 5], [0, 1, -1], [0, 1, 2, 3]):
        with pytest.raises(ValueError):
            bag.choose(choice=bad)
    a = bag.choose(generator=torch.Generator().manual_seed(5))
    b = bag.choose(generator=torch.Generator().manual_seed(5))
    assert len(a) == 3 and len(set(a.tolist())) == 3 and set(a.tolist()) <= set(range(5)) and a.tolist() == b.tolist()
    assert np.array_equal(bag.rois([2, 0]).numpy(), np.zeros((2, 16, 16, 3), np.uint8))
    # the preprocessor is planned on the host; running it needs the GPU and says so
    bag.update_resolution(8)
    assert bag.resolution == 8 and bag.prep.roi_size == 16 and bag.prep.pad == 100
    with pytest.raises(RuntimeError):
        bag.get_validation_data()
    with pytest.raises(RuntimeError):
        bag.get_train_data(choice=[0, 1, 2])
