"""-m gpu: tissue selection on the device (csrc/roi_select.hip through mil_amd.RoiSelector) — exact integers against fixtures
made by Pillow itself (tests/golden/make_roi_golden.py) and against the host restatement tests/roi_reference.py, which
tests/test_cpu_roi_select.py ties to Pillow.  Every comparison is equality."""
import os

import numpy as np
import pytest
import torch

import mil_amd
import roi_reference as ref

pytestmark = pytest.mark.gpu

H, W = 61, 53                                  # row pitch 159 bytes: a multiple of neither 4 nor 16
SIZES = (1, 5, 16, 37)


@pytest.fixture(scope="module")
def all_colours():
    img = ref.all_colours_image()
    img.setflags(write=False)
    return img, torch.from_numpy(img.copy()).cuda()


@pytest.fixture(scope="module")
def checker_slide():
    """61 x 53 slide whose pixels alternate, as on a chessboard, between colours that pass the HSV filter and colours that do
    not (random ones of either kind): about half the pixels pass, and the pixel in front of a window's row and the one behind
    it are of the other kind than the row's first and last — a head or tail pixel taken by mistake changes the result."""
    rng = np.random.default_rng(11)
    cand = rng.integers(0, 256, (H, W, 16, 3), dtype=np.uint8)
    cand[:, :, 14], cand[:, :, 15] = (150, 80, 180), (200, 210, 90)          # one certain colour of either kind
    want = ((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1).astype(bool)
    first = np.argmax(ref.passes(cand) == want[:, :, None], axis=2)
    slide = np.take_along_axis(cand, first[:, :, None, None], axis=2)[:, :, 0]
    assert np.array_equal(ref.passes(slide), want)
    slide.setflags(write=False)
    return slide


def _coords(s):
    """(0,0), the last row and column, every col mod 16 (so every col mod 4 and every 3*col mod 16), overlapping windows."""
    c = [(0, 0), (H - s, W - s), (H - s, 0), (0, W - s), (H - s, W - s - 1)]
    c += [(3, col) for col in range(16)] + [((7 * col) % (H - s + 1), col) for col in range(16)]
    assert all(r + s <= H and q + s <= W for r, q in c)
    assert {q % 4 for _, q in c} == set(range(4)) and {(3 * q) % 16 for _, q in c} == set(range(16))
    return c


# ---- 1. all colours ------------------------------------------------------------------------------------------------------------
def test_all_colours_as_256_windows_and_as_one(golden_dir, all_colours):
    z = np.load(os.path.join(golden_dir, "roi_allcolours.npz"))
    _, dev = all_colours
    got = mil_amd.RoiSelector(roi_size=256).stats(dev, coords=z["coords"])
    assert got.dtype == torch.int64 and tuple(got.shape) == (256, 4) and not got.is_cuda
    assert np.array_equal(got[:, :3].numpy(), z["stats"]) and bool((got[:, 3] == 256 * 256).all())
    one = mil_amd.RoiSelector(roi_size=4096).stats(dev, coords=[(0, 0)]).numpy()
    assert one.shape == (1, 4) and int(one[0, 2]) == 4786524 == int(z["total"]) and int(one[0, 3]) == 4096 * 4096
    assert np.array_equal(one[0, :3], z["stats"].sum(axis=0))


# ---- 2. alignment and edges, 4. the two source forms ----------------------------------------------------------------------------
@pytest.mark.parametrize("s", SIZES)
def test_unaligned_rows_heads_and_tails(checker_slide, s):
    coords = _coords(s)
    want = ref.slide_stats(checker_slide, coords, s)
    assert 0.3 < want[:, 2].sum() / want[:, 3].sum() < 0.7
    sel = mil_amd.RoiSelector(roi_size=s)
    dev = torch.from_numpy(checker_slide.copy()).cuda()
    got = sel.stats(dev, coords=coords).numpy()
    assert np.array_equal(got, want)
    # the same windows as a contiguous ROI stack: bitwise the same
    stack = np.stack([checker_slide[r:r + s, q:q + s] for r, q in coords])
    assert np.array_equal(sel.stats(torch.from_numpy(stack).cuda()).numpy(), got)
    # a source that does not start on a 16-byte boundary (a view 5 bytes into an allocation)
    buf = torch.full((H * W * 3 + 64,), 0xAB, dtype=torch.uint8).cuda()
    view = buf[5:5 + H * W * 3].view(H, W, 3)
    view.copy_(dev)
    assert view.data_ptr() % 16 == 5 and np.array_equal(sel.stats(view, coords=coords).numpy(), want)


def test_default_coords_are_the_raster(checker_slide):
    sel = mil_amd.RoiSelector(roi_size=16, padding=3)
    coords = ref.sliding_window(checker_slide.shape, 16, 3)
    assert len(coords) == 6
    got = sel.stats(torch.from_numpy(checker_slide.copy()).cuda()).numpy()
    assert np.array_equal(got, ref.slide_stats(checker_slide, coords, 16))


# ---- 3. accumulator range -------------------------------------------------------------------------------------------------------
def test_accumulators_do_not_overflow():
    white = np.full((1, 4096, 4096, 3), 255, np.uint8)
    got = mil_amd.RoiSelector(roi_size=4096).stats(torch.from_numpy(white).cuda()).numpy()
    assert np.array_equal(got[0], ref.window_stats(white[0])) and int(got[0, 1]) == 255 * 255 * 4096 * 4096
    rng = np.random.default_rng(2)
    rois = np.empty((3, 1200, 1200, 3), np.uint8)
    rois[0], rois[1], rois[2] = 255, (150, 80, 180), rng.integers(0, 256, (1200, 1200, 3), dtype=np.uint8)
    got = mil_amd.RoiSelector(roi_size=1200).stats(torch.from_numpy(rois).cuda()).numpy()
    want = np.stack([ref.window_stats(r) for r in rois])
    assert int(want[1, 2]) == 1440000 and int(want[0, 2]) == 0
    assert np.array_equal(got, want)


# ---- 5. launch chunking ---------------------------------------------------------------------------------------------------------
def test_more_windows_than_one_launch_and_none(checker_slide):
    rng = np.random.default_rng(9)
    n = 70000
    coords = np.stack([rng.integers(0, H, n), rng.integers(0, W, n)], axis=1)
    coords[:4] = [(0, 0), (H - 1, W - 1), (0, W - 1), (H - 1, 0)]
    red = checker_slide[..., 0].astype(np.int64)
    per_pixel = np.stack([red, red * red, ref.passes(checker_slide).astype(np.int64), np.ones_like(red)], axis=-1)
    assert np.array_equal(per_pixel[5, 7], ref.window_stats(checker_slide[5:6, 7:8]))
    sel = mil_amd.RoiSelector(roi_size=1)
    dev = torch.from_numpy(checker_slide.copy()).cuda()
    got = sel.stats(dev, coords=coords).numpy()
    assert got.shape == (n, 4) and np.array_equal(got, per_pixel[coords[:, 0], coords[:, 1]])
    empty = sel.stats(dev, coords=[])
    assert tuple(empty.shape) == (0, 4) and empty.dtype == torch.int64
    assert tuple(mil_amd.RoiSelector(roi_size=60).stats(dev).shape) == (0, 4)          # the raster of a slide that is too small


# ---- 6. select, 7. the chain into the tile pre-processing ------------------------------------------------------------------------
def test_select_keeps_what_the_reference_keeps(golden_dir):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    slide = z["slide"]
    sel = mil_amd.RoiSelector(roi_size=48, padding=7)
    dev = torch.from_numpy(slide).cuda()
    assert np.array_equal(sel.stats(dev).numpy(), z["stats"])
    rois, kept = sel.select(dev)
    assert kept.dtype == np.int64 and np.array_equal(kept, z["kept"])
    assert rois.is_cuda and rois.dtype == torch.uint8 and tuple(rois.shape) == (len(kept), 48, 48, 3)
    assert np.array_equal(rois.cpu().numpy(), np.stack([slide[r:r + 48, c:c + 48] for r, c in kept]))
    # an ROI stack selects by index
    sub, idx = sel.select(torch.from_numpy(np.stack([slide[r:r + 48, c:c + 48] for r, c in z["coords"]])).cuda())
    assert np.array_equal(z["coords"][idx], z["kept"]) and torch.equal(sub, rois)


def test_selected_rois_feed_the_tile_preprocessing(golden_dir):
    """The kept windows are the reference's data_cache: TilePreprocessor takes them as they are, and returns bitwise what it
    returns for the same windows sliced on the host and uploaded."""
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    slide = z["slide"]
    rois, kept = mil_amd.RoiSelector(roi_size=48, padding=7).select(torch.from_numpy(slide).cuda())
    prep = mil_amd.TilePreprocessor(48, 32)
    tiles = prep(rois, out="u8")
    host = np.stack([slide[r:r + 48, c:c + 48] for r, c in z["kept"]])
    want = prep(torch.from_numpy(host).cuda(), out="u8")
    assert len(kept) == 4 and tuple(tiles.shape) == (4, 3, 32, 32) and torch.equal(tiles.u8, want.u8)
