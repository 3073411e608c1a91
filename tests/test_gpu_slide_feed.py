"""-m gpu: tiles pre-processed straight from windows of a slide (mil_tile_preprocess_win* through
`TilePreprocessor.from_slide`, `RoiSelector.kept`, `SlideBag`).  Every comparison is equality of bytes or fp32 bits, against
two routes: (a) `oracle.preprocess_oracle.finalize_tile` on host slices `slide[r:r+s, c:c+s]` (pinned to Pillow by the goldens
of tests/test_gpu_preprocess.py) and (b) the existing stack entry `prep(stack)` on the same windows sliced on the host and
uploaded."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import mil_amd
from oracle import preprocess_oracle as po

pytestmark = pytest.mark.gpu

H, W = 61, 53                                  # row pitch 159 bytes: a multiple of neither 4 nor 16
PAD = 4
SIZES = [(5, 4), (16, 24), (37, 16), (16, 8)]  # (S, R); (16, 24) enlarges
FORMS = ("nchw", "u8", "s2d")


def _bits(x):
    """The result of any `out=` form as an integer tensor (equality of bytes / fp32 bits / bf16 bits)."""
    if isinstance(x, mil_amd.U8Tiles):
        return x.u8
    if isinstance(x, mil_amd.S2dTiles):
        return x.xs.view(torch.int16)
    return x.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _slide():
    """Bytes in 128..255: a neighbour's byte that leaks into a window, or into the zero padding, changes a result."""
    s = np.random.default_rng(3).integers(128, 256, (H, W, 3), dtype=np.uint8)
    s.setflags(write=False)
    return s


def _coords(s):
    """tests/test_gpu_roi_select.py:_coords — (0,0), the last row and column, every col mod 16, overlapping windows."""
    c = [(0, 0), (H - s, W - s), (H - s, 0), (0, W - s), (H - s, W - s - 1)]
    c += [(3, col) for col in range(16)] + [((7 * col) % (H - s + 1), col) for col in range(16)]
    assert all(r + s <= H and q + s <= W for r, q in c)
    assert {q % 4 for _, q in c} == set(range(4)) and {(3 * q) % 16 for _, q in c} == set(range(16))
    return c


def _combos(pad):
    """(top, left) over {0, pad, 2 pad}^2 with all four flip combinations: 36 rows."""
    return [(t, l, hf, vf) for t, l in itertools.product((0, pad, 2 * pad), repeat=2) for hf in (0, 1) for vf in (0, 1)]


@functools.lru_cache(maxsize=None)
def _case1(s, r):
    """Windows x parameter rows of case 1 and what route (b) returns for them, computed once and shared (read only)."""
    slide, coords, combos = _slide(), _coords(s), _combos(PAD)
    cross_c = [c for c in coords for _ in combos]
    cross_p = torch.tensor([p for _ in coords for p in combos], dtype=torch.int32)
    prep = mil_amd.TilePreprocessor(s, r, pad=PAD)
    stack = torch.from_numpy(np.stack([slide[y:y + s, x:x + s] for y, x in coords])).cuda()
    cross_stack = stack.repeat_interleave(len(combos), dim=0)
    want_flat = {f: _bits(prep(stack, out=f)).clone() for f in FORMS}
    want_train = {f: _bits(prep(cross_stack, cross_p, out=f)).clone() for f in FORMS}
    return prep, coords, cross_c, cross_p, want_flat, want_train


def _check_case1(dev, s, r):
    prep, coords, cross_c, cross_p, want_flat, want_train = _case1(s, r)
    for f in FORMS:                                                      # route (b), all three output forms
        assert torch.equal(_bits(prep.from_slide(dev, coords, out=f)), want_flat[f]), (f, "flat")
        assert torch.equal(_bits(prep.from_slide(dev, cross_c, cross_p, out=f)), want_train[f]), (f, "train")
    return prep, coords


@pytest.mark.parametrize("s,r", SIZES)
def test_unaligned_rows_heads_and_tails(s, r):
    slide = _slide()
    dev = torch.from_numpy(slide.copy()).cuda()
    prep, coords = _check_case1(dev, s, r)
    # route (a): every window through the flat chain and through one row of the train combinations (all 36 are used)
    combos = _combos(PAD)
    params = torch.tensor([combos[i % len(combos)] for i in range(len(coords))], dtype=torch.int32)
    assert len(coords) >= len(combos)
    flat = prep.from_slide(dev, coords).cpu().numpy()
    train = prep.from_slide(dev, coords, params).cpu().numpy()
    assert flat.dtype == np.float32 and flat.shape == (len(coords), 3, r, r)
    for i, (y, x) in enumerate(coords):
        roi = slide[y:y + s, x:x + s]
        assert np.array_equal(flat[i], po.finalize_tile(roi, r)), (i, y, x)
        assert np.array_equal(train[i], po.finalize_tile(roi, r, params[i].numpy(), pad=PAD)), (i, y, x, params[i].tolist())
    # the stack form of from_slide: the same kernel at pitch 3S
    stack = torch.from_numpy(np.stack([slide[y:y + s, x:x + s] for y, x in coords])).cuda()
    assert torch.equal(_bits(prep.from_slide(stack, None, params)), _bits(torch.from_numpy(train).cuda()))


@pytest.mark.parametrize("s,r", SIZES)
def test_source_not_16_byte_aligned(s, r):
    """The slide as a view 5 bytes into a buffer filled with 0xAB on both sides: identical results."""
    buf = torch.full((H * W * 3 + 64,), 0xAB, dtype=torch.uint8).cuda()
    view = buf[5:5 + H * W * 3].view(H, W, 3)
    view.copy_(torch.from_numpy(_slide().copy()))
    assert view.data_ptr() % 16 == 5
    _check_case1(view, s, r)


@pytest.mark.parametrize("r", [8, 24])
def test_aligned_fast_route(r):
    """Every row of every window on the source's 16-byte grid (pitch 192, columns at multiples of 16), neighbours non-zero,
    train chain at the extreme crop offsets."""
    s, pad = 16, 4
    slide = np.random.default_rng(4).integers(128, 256, (64, 64, 3), dtype=np.uint8)
    coords = [(y, x) for y in range(0, 64, 16) for x in range(0, 64, 16)]
    combos = [(t, l, hf, vf) for t in (0, 2 * pad) for l in (0, 2 * pad) for hf in (0, 1) for vf in (0, 1)]
    dev = torch.from_numpy(slide).cuda()
    assert dev.data_ptr() % 16 == 0
    prep = mil_amd.TilePreprocessor(s, r, pad=pad)
    cross_c = [c for c in coords for _ in combos]
    cross_p = torch.tensor([p for _ in coords for p in combos], dtype=torch.int32)
    stack = torch.from_numpy(np.stack([slide[y:y + s, x:x + s] for y, x in cross_c])).cuda()
    for f in FORMS:                                                      # route (b)
        assert torch.equal(_bits(prep.from_slide(dev, cross_c, cross_p, out=f)), _bits(prep(stack, cross_p, out=f))), f
        assert torch.equal(_bits(prep.from_slide(dev, coords, out=f)), _bits(prep(stack[::len(combos)].contiguous(), out=f))), f
    got = prep.from_slide(dev, cross_c, cross_p).cpu().numpy()
    flat = prep.from_slide(dev, coords).cpu().numpy()
    for i, (y, x) in enumerate(cross_c):                                 # route (a)
        assert np.array_equal(got[i], po.finalize_tile(slide[y:y + s, x:x + s], r, cross_p[i].numpy(), pad=pad)), (i, y, x)
    for i, (y, x) in enumerate(coords):
        assert np.array_equal(flat[i], po.finalize_tile(slide[y:y + s, x:x + s], r)), (i, y, x)


def test_production_size():
    """1200 x 1200 windows of a 2500 x 3700 slide (pitch 11100: a multiple of 4, not of 16) -> 300 x 300, both chains."""
    hh, ww, s, r = 2500, 3700, 1200, 300
    slide = np.random.default_rng(5).integers(0, 256, (hh, ww, 3), dtype=np.uint8)
    coords = [(0, 0), (hh - s, ww - s), (7, 1001)]
    params = torch.tensor([[0, 200, 1, 1], [200, 0, 0, 1], [37, 141, 1, 0]], dtype=torch.int32)
    dev = torch.from_numpy(slide).cuda()
    stack = torch.from_numpy(np.stack([slide[y:y + s, x:x + s] for y, x in coords])).cuda()
    prep = mil_amd.TilePreprocessor(s, r, pad=100)
    for f in ("u8", "nchw"):
        assert torch.equal(_bits(prep.from_slide(dev, coords, out=f)), _bits(prep(stack, out=f))), f
        assert torch.equal(_bits(prep.from_slide(dev, coords, params, out=f)), _bits(prep(stack, params, out=f))), f


def test_rows_longer_than_the_prefetched_path_takes():
    """A 1400-pixel window: rows of 4200 bytes are more than 256 granules, staged without the register prefetch."""
    hh, ww, s, r = 1403, 1411, 1400, 100
    slide = np.random.default_rng(8).integers(128, 256, (hh, ww, 3), dtype=np.uint8)
    coords = [(3, 11), (0, 0), (2, 6)]
    params = torch.tensor([[0, 200, 1, 0], [200, 0, 0, 1], [100, 100, 0, 0]], dtype=torch.int32)
    dev = torch.from_numpy(slide).cuda()
    stack = torch.from_numpy(np.stack([slide[y:y + s, x:x + s] for y, x in coords])).cuda()
    prep = mil_amd.TilePreprocessor(s, r, pad=100)
    assert torch.equal(prep.from_slide(dev, coords, out="u8").u8, prep(stack, out="u8").u8)
    assert torch.equal(prep.from_slide(dev, coords, params, out="u8").u8, prep(stack, params, out="u8").u8)
    assert torch.equal(prep.from_slide(stack, None, params, out="u8").u8, prep(stack, params, out="u8").u8)


def test_windows_beyond_4_gib():
    hh, ww, s, r = 36000, 40000, 64, 32
    if torch.cuda.mem_get_info()[0] < 6 * 1024 ** 3:
        pytest.skip("less than 6 GB of device memory free")
    dev = torch.zeros((hh, ww, 3), dtype=torch.uint8, device="cuda")
    assert dev.numel() > 1 << 32
    patch = np.random.default_rng(6).integers(128, 256, (s, s, 3), dtype=np.uint8)
    dev[hh - s:, ww - s:] = torch.from_numpy(patch).cuda()
    host_tail = np.zeros((2 * s, 2 * s, 3), np.uint8)                    # the slide's last 128 x 128 pixels
    host_tail[s:, s:] = patch
    coords = [(0, 0), (hh - s, ww - s), (hh - s - 1, ww - s - 5)]
    rois = [np.zeros((s, s, 3), np.uint8), patch, host_tail[s - 1:2 * s - 1, s - 5:2 * s - 5]]
    assert ((hh - s) * ww + ww - s) * 3 > 1 << 32
    prep = mil_amd.TilePreprocessor(s, r, pad=8)
    stack = torch.from_numpy(np.stack(rois)).cuda()
    params = torch.tensor([[16, 0, 0, 1], [0, 16, 1, 0], [3, 9, 1, 1]], dtype=torch.int32)
    got_flat, got_train = prep.from_slide(dev, coords, out="u8"), prep.from_slide(dev, coords, params, out="u8")
    del dev
    assert torch.equal(got_flat.u8, prep(stack, out="u8").u8)
    assert torch.equal(got_train.u8, prep(stack, params, out="u8").u8)
    assert int(got_flat.u8[1].max()) >= 128 and int(got_flat.u8[0].max()) == 0


def test_more_windows_than_one_launch_and_none():
    slide = _slide()
    rng = np.random.default_rng(9)
    n, s, r = 70000, 2, 2
    coords = np.stack([rng.integers(0, H - s + 1, n), rng.integers(0, W - s + 1, n)], axis=1)
    coords[:4] = [(0, 0), (H - s, W - s), (0, W - s), (H - s, 0)]
    yy = coords[:, 0, None, None] + np.arange(s)[None, :, None]
    xx = coords[:, 1, None, None] + np.arange(s)[None, None, :]
    stack = torch.from_numpy(slide[yy, xx]).cuda()
    assert tuple(stack.shape) == (n, s, s, 3) and np.array_equal(stack[n - 1].cpu().numpy(), slide[coords[-1, 0]:coords[-1, 0] + s, coords[-1, 1]:coords[-1, 1] + s])
    dev = torch.from_numpy(slide.copy()).cuda()
    prep = mil_amd.TilePreprocessor(s, r, pad=1)
    assert torch.equal(prep.from_slide(dev, coords, out="u8").u8, prep(stack, out="u8").u8)
    params = prep.draw_params(n, torch.Generator().manual_seed(1))
    assert torch.equal(prep.from_slide(dev, torch.from_numpy(coords), params).view(torch.int32), prep(stack, params).view(torch.int32))
    for f, shape, dtype in (("nchw", (0, 3, r, r), torch.float32), ("u8", (0, 3, r, r), torch.uint8), ("s2d", (0, 3, r, r), torch.bfloat16)):
        e = prep.from_slide(dev, [], out=f)
        assert tuple(e.shape) == shape and _bits(e).numel() == 0 and (e.xs if f == "s2d" else e.u8 if f == "u8" else e).dtype == dtype


def test_no_stack_is_made():
    """Eight 300 x 300 windows -> 64 x 64 bytes: the call's peak device allocation stays below half of the stack it would
    have had to gather (8 * 300 * 300 * 3 bytes)."""
    s, r, n = 300, 64, 8
    slide = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (700, 1300, 3), dtype=np.uint8)).cuda()
    coords = [(i * 50, i * 140 + 3) for i in range(n)]
    prep = mil_amd.TilePreprocessor(s, r)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    tiles = prep.from_slide(slide, coords, out="u8")
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    assert tuple(tiles.shape) == (n, 3, r, r)
    assert peak < n * s * s * 3 / 2, peak
    stack = torch.stack([slide[y:y + s, x:x + s] for y, x in coords])
    assert torch.equal(tiles.u8, prep(stack, out="u8").u8)


def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, **kw)


def test_slide_bag_end_to_end(golden_dir):
    z, dev, bag = _golden_bag(golden_dir)
    assert bag.ntiles == -1 and bag.build() and bag.ntiles == len(z["kept"]) == 4
    assert bag.coords.dtype == np.int64 and np.array_equal(bag.coords, z["kept"])
    sel = mil_amd.RoiSelector(roi_size=48, padding=7)
    assert np.array_equal(sel.kept(dev), z["kept"])
    rois, kept = sel.select(dev)
    stack_idx = sel.kept(torch.from_numpy(np.stack([z["slide"][r:r + 48, c:c + 48] for r, c in z["coords"]])).cuda())
    assert np.array_equal(z["coords"][stack_idx], z["kept"])
    prep = mil_amd.TilePreprocessor(48, 32)
    want = prep(rois, out="u8")
    got = bag.get_validation_data()
    assert isinstance(got, mil_amd.U8Tiles) and torch.equal(got.u8, want.u8)
    tiles, coords = bag.get_inference_data()
    assert torch.equal(tiles.u8, want.u8) and np.array_equal(coords, z["kept"])
    assert torch.equal(bag.get_validation_data(out="nchw").view(torch.int32), prep(rois).view(torch.int32))
    assert torch.equal(bag.rois([3, 1]), rois[torch.tensor([3, 1]).cuda()])
    net = mil_amd.Attention(3).eval()
    a, b = net(got, torch.tensor([1])), net(want, torch.tensor([1]))
    assert set(a) == set(b) and len(a) > 3
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a bag without tissue: an empty stack of the bag's resolution
    empty = mil_amd.SlideBag(torch.zeros((120, 130, 3), dtype=torch.uint8).cuda(), 48, 7, resolution=32)
    empty.build()
    assert empty.ntiles == 0 and tuple(empty.get_validation_data().shape) == (0, 3, 32, 32)
    assert tuple(empty.get_train_data(out="nchw").shape) == (0, 3, 32, 32)


def test_get_train_data_with_injected_choice_and_params(golden_dir):
    z, dev, bag = _golden_bag(golden_dir, pad=10, max_tiles=3)
    bag.build()
    choice = [2, 0, 3]
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1]], dtype=torch.int32)
    got = bag.get_train_data(choice=choice, params=params)
    want = bag.prep.from_slide(dev, z["kept"][choice], params, out="u8")
    assert len(got) == 3 and torch.equal(got.u8, want.u8)
    # route (a) on the injected draw
    for i, j in enumerate(choice):
        r, c = z["kept"][j]
        tile = po.finalize_tile(z["slide"][r:r + 48, c:c + 48], 32, params[i].numpy(), pad=10)
        assert np.array_equal(got.float()[i].cpu().numpy(), tile), i
    g = torch.Generator().manual_seed(3)
    idx = bag.choose(generator=g)
    assert len(idx) == 3 and len(set(idx.tolist())) == 3 and set(idx.tolist()) <= set(range(4))
    assert tuple(bag.get_train_data(generator=g).shape) == (3, 3, 32, 32)
    # at or below the cap every window is used, in order, and the same generator draws the same parameters
    full = mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, max_tiles=4, coords=z["kept"])
    assert full.build() and full.choose() is None
    p = full.prep.draw_params(4, torch.Generator().manual_seed(8))
    assert torch.equal(full.get_train_data(generator=torch.Generator().manual_seed(8)).u8, full.prep.from_slide(dev, z["kept"], p, out="u8").u8)


def test_errors_fire_before_any_launch():
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    dev = torch.from_numpy(_slide().copy()).cuda()
    for bad in ([(H - 15, 0)], [(0, W - 15)], [(-1, 0)], [(0, 0), (0, -1)]):
        with pytest.raises(ValueError):
            prep.from_slide(dev, bad)
    with pytest.raises(RuntimeError):
        prep.from_slide(torch.from_numpy(_slide().copy()), [(0, 0)])
    with pytest.raises(ValueError):
        prep.from_slide(dev.float(), [(0, 0)])
    with pytest.raises(ValueError):
        prep.from_slide(dev, [(0, 0), (1, 1)], torch.tensor([[0, 0, 0, 0], [9, 0, 0, 0]]))
    with pytest.raises(ValueError):
        prep.from_slide(dev, [(0, 0)], torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0]]))     # one row per window
    with pytest.raises(ValueError):
        prep.from_slide(dev, [(0, 0)], out="nhwc")
    with pytest.raises(ValueError):
        mil_amd.TilePreprocessor(16, 7).from_slide(dev, [(0, 0)], out="s2d")
    with pytest.raises(ValueError):
        prep.from_slide(dev, None)                                                     # a slide needs coords
    with pytest.raises(ValueError):
        prep.from_slide(torch.zeros((2, 15, 15, 3), dtype=torch.uint8).cuda(), None)   # a stack of another ROI size
    assert tuple(prep.from_slide(dev, [(H - 16, W - 16)]).shape) == (1, 3, 8, 8)        # the last window is inside
