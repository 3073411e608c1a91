"""CPU (-m "not gpu"): tissue selection (mil_roi_stats / mil_amd.RoiSelector) without a GPU — the exported symbol and its
host-side refusals, the reference's raster (RoiBuilder.py:104-114), the host restatement tests/roi_reference.py against
Pillow itself (all 2^24 colours; skipped where Pillow is not installed) and against the Pillow-made fixtures (always)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import roi_reference as ref


def _all_colours():
    if not hasattr(_all_colours, "img"):
        _all_colours.img = ref.all_colours_image()
        _all_colours.img.setflags(write=False)
    return _all_colours.img


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_library_exports_mil_roi_stats():
    import mil_amd
    from mil_amd import _lib
    assert "mil_roi_stats" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(mil_amd.LIB_PATH), "mil_roi_stats")
    assert mil_amd.lib().mil_abi_version() == 2


def test_argument_and_range_errors_are_host_side():
    """Every refusal is decided before any GPU call: the status codes come back on a machine without a GPU (the pointers are
    never dereferenced — host buffers stand in for device memory)."""
    import mil_amd
    f = mil_amd.lib().mil_roi_stats
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    ok_args = dict(base=p, base_bytes=48, win_off=p, pitch=12, n=0, S=4, out=p)

    def call(**kw):
        a = dict(ok_args, **kw)
        return f(a["base"], a["base_bytes"], a["win_off"], a["pitch"], a["n"], a["S"], 120, 50, 210, a["out"], None)
    assert call() == 0                                           # n == 0: MIL_OK without a launch
    assert call(S=4096, pitch=3 * 4096) == 0
    assert call(base=None) == 1 and call(win_off=None) == 1 and call(out=None) == 1
    assert call(S=0) == 1 and call(S=-3) == 1
    assert call(pitch=11) == 1                                   # row_pitch < 3S
    assert call(n=-1) == 1
    assert call(S=4097, pitch=3 * 4097) == 2                     # MIL_ERR_UNSUPPORTED
    assert call(S=4097, pitch=11) == 2 and call(S=0, pitch=0, n=-1) == 1
    assert f(p, 48, p, 12, 0, 4, 256, 50, 210, p, None) == 1     # hue_min outside a byte


# ---- raster -------------------------------------------------------------------------------------------------------------------
def test_raster_is_the_references_sliding_window():
    import mil_amd
    sel = mil_amd.RoiSelector(roi_size=4)
    assert sel.raster((5, 5, 3)) == []                           # dim = S + 1: nothing
    assert sel.raster((6, 6, 3)) == [(0, 0)]                     # dim = S + 2: one window
    assert sel.raster((9, 9, 3)) == [(0, 0)] and sel.raster((10, 10, 3)) == [(0, 0), (4, 0), (0, 4), (4, 4)]
    assert sel.raster((10, 14, 3)) == [(0, 0), (4, 0), (0, 4), (4, 4), (0, 8), (4, 8)]        # (row, col), the column outer
    assert sel.raster((14, 6)) == [(0, 0), (4, 0), (8, 0)]
    pad = mil_amd.RoiSelector(roi_size=3, padding=1)
    assert pad.raster((12, 9, 3)) == [(1, 1), (4, 1)]
    assert pad.raster((12, 12, 3)) == [(1, 1), (4, 1), (1, 4), (4, 4)]
    assert mil_amd.RoiSelector(roi_size=3, padding=2).raster((9, 9, 3)) == [(2, 2)]
    for shape, s, p in (((61, 53, 3), 5, 0), ((160, 208, 3), 48, 7), ((100, 37, 3), 16, 3)):
        assert mil_amd.RoiSelector(s, p).raster(shape) == ref.sliding_window(shape, s, p)
    assert mil_amd.RoiSelector is mil_amd.roi_select.RoiSelector and "RoiSelector" in mil_amd.__all__


# ---- the host restatement against Pillow ----------------------------------------------------------------------------------------
def test_helper_equals_pillow_on_all_colours():
    Image = pytest.importorskip("PIL.Image")
    img = _all_colours()
    hsv = np.asarray(Image.fromarray(img).convert("HSV"))
    for y in range(0, 4096, 1024):                               # (in four parts: the float restatement's temporaries)
        assert np.array_equal(ref.rgb2hsv_float(img[y:y + 1024]), hsv[y:y + 1024])
    assert np.array_equal(ref.hue_above(img), hsv[..., 0] > 120)
    want = (hsv[..., 0] > 120) & (hsv[..., 2] > 50) & (hsv[..., 2] < 210)
    assert np.array_equal(ref.passes(img), want) and int(want.sum()) == 4786524


def test_helper_decision_equals_imagestat():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageStat
    rng = np.random.default_rng(3)
    wins = [rng.integers(0, 256, (48, 48, 3), dtype=np.uint8), rng.integers(100, 112, (48, 48, 3), dtype=np.uint8),
            np.full((48, 48, 3), 255, np.uint8), rng.integers(0, 256, (7, 5, 3), dtype=np.uint8)]
    half = np.full((48, 48, 3), 100, np.uint8)
    half[24:, :, 0] = 110                                        # variance exactly 25
    spoilt = half.copy()
    spoilt[0, 0, 0] = 90
    for w in wins + [half, spoilt]:
        st = ImageStat.Stat(Image.fromarray(w))
        s = ref.window_stats(w)
        assert (float(s[0]), float(s[1]), int(s[3])) == (st.sum[0], st.sum2[0], st.count[0])
        assert ref.imagestat_stddev(s[0], s[1], s[3]) == st.stddev[0]
        assert (ref.imagestat_stddev(s[0], s[1], s[3]) > 5) == (st.stddev[0] > 5)
    assert ref.imagestat_stddev(*ref.window_stats(half)[[0, 1, 3]]) == 5.0
    assert ref.imagestat_stddev(*ref.window_stats(spoilt)[[0, 1, 3]]) > 5.0


# ---- the fixtures (made by Pillow: tests/golden/make_roi_golden.py) --------------------------------------------------------------
def test_helper_reproduces_the_all_colours_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "roi_allcolours.npz"))
    img = _all_colours()
    coords = [tuple(int(v) for v in rc) for rc in z["coords"]]
    assert len(coords) == 256 and coords[1] == (256, 0) and coords[16] == (0, 256)
    got = ref.slide_stats(img, coords, 256)
    assert np.array_equal(got[:, :3], z["stats"]) and int(got[:, 2].sum()) == int(z["total"]) == 4786524
    assert int(ref.passes(img).sum()) == 4786524


def test_helper_reproduces_the_small_slide_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    slide = z["slide"]
    assert slide.shape == (160, 208, 3) and slide.dtype == np.uint8
    coords = ref.sliding_window(slide.shape, 48, 7)
    assert np.array_equal(np.array(coords), z["coords"]) and len(coords) == 12
    assert np.array_equal(ref.slide_stats(slide, coords, 48), z["stats"])
    data, kept = ref.select(slide, 48, 7)
    assert np.array_equal(np.array(kept).reshape(-1, 2), z["kept"]) and len(kept) == 4
    assert all(np.array_equal(d, slide[r:r + 48, c:c + 48]) for d, (r, c) in zip(data, kept))
    st = z["stats"]
    assert st[3, 2] == 1000 and st[4, 2] == 1001                 # the count threshold, from both sides
    assert ref.imagestat_stddev(st[5, 0], st[5, 1], st[5, 3]) == 5.0 < ref.imagestat_stddev(st[6, 0], st[6, 1], st[6, 3])


# ---- RoiSelector refuses before any launch --------------------------------------------------------------------------------------
def test_selector_refuses_cpu_tensors_and_wrong_inputs():
    import mil_amd
    sel = mil_amd.RoiSelector(roi_size=8)
    slide = torch.zeros((20, 30, 3), dtype=torch.uint8)
    for call in (sel.stats, sel.select):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(slide)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(torch.zeros((2, 8, 8, 3), dtype=torch.uint8))
        with pytest.raises(ValueError):
            call(slide.float())
        with pytest.raises(ValueError):
            call(slide.numpy())
        with pytest.raises(ValueError):
            call(torch.zeros((20, 30), dtype=torch.uint8))
        with pytest.raises(ValueError):
            call(torch.zeros((20, 30, 4), dtype=torch.uint8))
        with pytest.raises(ValueError):
            call(torch.zeros((2, 8, 9, 3), dtype=torch.uint8))   # an ROI stack of another size
        with pytest.raises(ValueError):
            call(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), coords=[(0, 0)])
        for bad in ([(13, 0)], [(0, 23)], [(-1, 0)], [(0, 0), (12, 23)]):
            with pytest.raises(ValueError, match="does not lie inside"):
                call(slide, coords=bad)
    with pytest.raises(ValueError):
        mil_amd.RoiSelector(roi_size=0)
    # the decision on the integers needs no GPU: the thresholds of the fixture
    assert sel.keep([241920, 25459200, 2304, 2304]) is False and sel.keep([241910, 25457300, 2304, 2304]) is True
    assert sel.keep([476000, 104000000, 1000, 2304]) is False and sel.keep([475900, 103960000, 1001, 2304]) is True
    assert sel.keep([255 * 2304, 255 * 255 * 2304, 2304, 2304]) is False
