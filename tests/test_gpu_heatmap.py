"""-m gpu: attention heat maps rendered from the resident slide (`mil_heatmap_render` through `AttentionMapRenderer` and
`SlideBag.attention_maps`).  Every comparison is equality with tests/heatmap_reference.py, the numpy restatement of the
arithmetic include/mil_hip.h states.  The canvas handed to the lower call is pre-filled with 0x5A, so a pixel the kernel
should have written and did not, or wrote and should not have, shows."""
import functools
import os

import numpy as np
import pytest
import torch

import heatmap_reference as ref
import mil_amd
from mil_amd import heatmap as hm

pytestmark = pytest.mark.gpu

H, W = 61, 53                                  # row pitch 159 bytes: a multiple of neither 4 nor 16
FILL = 0x5A
# the issue's sizes; (30, 15) in addition: the largest D of the one-add-per-pixel kernel next to (16, 16), the smallest of the
# two-bins-per-chunk kernel.  (37, 37) and (48, 16) have chunks that reach over both ends of a row.
SIZES = [(5, 1), (5, 5), (8, 4), (12, 3), (16, 16), (37, 37), (48, 16), (30, 15)]
JET_CODES = np.array([-1, 0, 1, 37, 100, 104], dtype=np.int16)


@functools.lru_cache(maxsize=None)
def _slide():
    s = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    s[:4, :4] = 255                                                # a saturated corner: the rounding at the top of the range
    s.setflags(write=False)
    return s


def _coords(s):
    """(0,0), the last row and column, and every column phase that fits: col = 0..15 where the slide is wide enough (every
    3*col % 16, asserted), else every column there is (S = 48 on 53 columns: the six phases 0, 3, .., 15 — the row pitch of
    159 = -1 mod 16 then walks each window through all sixteen alignments row by row)."""
    cols = list(range(min(16, W - s + 1)))
    c = [(0, 0), (H - s, W - s), (H - s, 0), (0, W - s), (H - s, max(W - s - 1, 0))]
    c += [(3, col) for col in cols] + [((7 * col) % (H - s + 1), col) for col in cols]
    c = list(dict.fromkeys(c))
    assert all(r + s <= H and q + s <= W for r, q in c)
    if W - s >= 15:
        assert {(3 * q) % 16 for _, q in c} == set(range(16))
    return c


def _groups(coords, s, d):
    """Greedy split into calls whose windows own disjoint output blocks (one window per call where they all collide)."""
    n, groups = s // d, []
    for r, q in coords:
        for g in groups:
            if all(abs(r // d - y // d) >= n or abs(q // d - x // d) >= n for y, x in g):
                g.append((r, q))
                break
        else:
            groups.append([(r, q)])
    return groups


def _indices(t, seed):
    rng = np.random.default_rng(seed)
    jet = torch.from_numpy(rng.choice(JET_CODES, size=(4, t)))
    feat = torch.from_numpy(rng.integers(0, 256, (t, 80), dtype=np.uint8))
    return jet, feat


def _check(renderer, dev, host, coords, jet, feat, s, d, inset=16):
    canvas = torch.full((5, host.shape[0] // d, host.shape[1] // d, 3), FILL, dtype=torch.uint8, device="cuda")
    got = renderer.render_into(canvas, dev, coords, jet, feat)
    assert got is canvas
    want = ref.render(np.full(tuple(canvas.shape), FILL, np.uint8), host, coords, s, d, jet.numpy(),
                      None if feat is None else feat.numpy(), hm.JET105, hm.VIRIDIS256, inset, renderer.q_tissue, renderer.q_map)
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"S={s} D={d} coords={coords[:4]}...: {len(bad)} bytes differ, first (panel,y,x,c)={bad[0].tolist()} "
                             f"got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def _alignment_case(dev, s, d):
    host, r = _slide(), mil_amd.AttentionMapRenderer(s, d)
    groups = _groups(_coords(s), s, d)
    assert sum(len(g) for g in groups) == len(_coords(s))
    assert s > H // 2 or max(len(g) for g in groups) > 1                    # several windows per call where they fit
    for i, g in enumerate(groups):
        jet, feat = _indices(len(g), 100 * s + i)
        _check(r, dev, host, g, jet, feat if i % 3 else None, s, d)


@pytest.mark.parametrize("s,d", SIZES)
def test_unaligned_rows_heads_and_tails(s, d):
    _alignment_case(torch.from_numpy(_slide().copy()).cuda(), s, d)


@pytest.mark.parametrize("s,d", SIZES)
def test_source_not_16_byte_aligned(s, d):
    """The slide as a view 5 bytes into a buffer filled with 0xAB on both sides: identical results."""
    buf = torch.full((H * W * 3 + 64,), 0xAB, dtype=torch.uint8).cuda()
    view = buf[5:5 + H * W * 3].view(H, W, 3)
    view.copy_(torch.from_numpy(_slide().copy()))
    assert view.data_ptr() % 16 == 5
    _alignment_case(view, s, d)


def test_range_one_pixel_from_a_whole_window():
    """D = 1200: 1.44 million pixels per output pixel — the 32-bit sums at their largest (3.7e8 on white)."""
    s = 1200
    r = mil_amd.AttentionMapRenderer(s, s)
    none = torch.full((4, 1), -1, dtype=torch.int16)
    white = torch.full((s, s, 3), 255, dtype=torch.uint8, device="cuda")
    canvas = torch.full((5, 1, 1, 3), FILL, dtype=torch.uint8, device="cuda")
    got = r.render_into(canvas, white, [(0, 0)], none).cpu().numpy()
    assert got[0].tolist() == [[[255, 255, 255]]] and (got[1:] == FILL).all()
    host = np.random.default_rng(12).integers(0, 256, (s, s, 3), dtype=np.uint8)
    host[:, :, 1] |= 0x80                                          # a channel with another mean
    mean = (host.astype(np.int64).sum(axis=(0, 1)) + s * s // 2) // (s * s)
    canvas.fill_(FILL)
    got = r.render_into(canvas, torch.from_numpy(host).cuda(), [(0, 0)], none).cpu().numpy()
    assert got[0, 0, 0].tolist() == mean.tolist() and mean[1] > mean[0] + 30
    _check(r, torch.from_numpy(host).cuda(), host, [(0, 0)], torch.tensor([[100], [0], [-1], [104]], dtype=torch.int16),
           torch.arange(80, dtype=torch.uint8).view(1, 80), s, s)


def test_range_scale_one_returns_the_window():
    s = 1200
    host = np.random.default_rng(13).integers(0, 256, (s + 3, s + 7, 3), dtype=np.uint8)
    r = mil_amd.AttentionMapRenderer(s, 1)
    canvas = torch.full((5, s + 3, s + 7, 3), FILL, dtype=torch.uint8, device="cuda")
    got = r.render_into(canvas, torch.from_numpy(host).cuda(), [(2, 5)], torch.full((4, 1), -1, dtype=torch.int16))
    want = np.full((5, s + 3, s + 7, 3), FILL, np.uint8)
    want[0, 2:2 + s, 5:5 + s] = host[2:2 + s, 5:5 + s]
    assert torch.equal(got.cpu(), torch.from_numpy(want))


@functools.lru_cache(maxsize=None)
def _raster_slide():
    s = np.random.default_rng(21).integers(0, 256, (203, 151, 3), dtype=np.uint8)
    s.setflags(write=False)
    return s


@pytest.mark.parametrize("scale,inset", [(16, 16), (16, 32), (4, 4), (4, 16), (4, 100), (2, 0)])
def test_raster_bag_all_five_panels(scale, inset):
    """A 203 x 151 slide, roi_size 48, padding 7 (window phase 7 % 16 != 0): six windows.  inset 16 at scale 16 leaves the
    centre pixel of a 3 x 3 block; inset 32 (scale 16) and 100 (scale 4) collapse to g = 0; scale 4 / 2 draw 12 / 24 pixel blocks
    (all 80 feature cells at (4, 4) and (2, 0))."""
    host = _raster_slide()
    dev = torch.from_numpy(host.copy()).cuda()
    coords = mil_amd.RoiSelector(48, 7).raster(host.shape)
    assert len(coords) == 6 and coords[0] == (7, 7)
    n = 48 // scale
    assert (n - 2 * (inset // scale) < 1) == ((scale, inset) in ((16, 32), (4, 100)))
    r = mil_amd.AttentionMapRenderer(48, scale, inset=inset)
    jet = torch.tensor([[-1, 0, 100, 104, 37, -1], [0, -1, 104, 100, -1, 5], [104, 100, -1, 0, 1, -1], [-1, -1, 0, 104, 100, 63]],
                       dtype=torch.int16)
    feat = torch.from_numpy(np.random.default_rng(22).integers(0, 256, (6, 80), dtype=np.uint8))
    feat[2] = 0                                                    # what a constant tile gives
    _check(r, dev, host, coords, jet, feat, 48, scale, inset)
    _check(r, dev, host, coords, jet, None, 48, scale, inset)
    # the public call: white canvas, indices from the reference's statements; twice, bit for bit
    a1 = torch.tensor([[0.0, 1e-6, 1.0, 1.045, 0.5, 0.0], [0.0, 0.3, 1.0, 0.999, 0.0, 0.017], [0.0, 0.0, 1.0, 0.2, 0.0, 0.62]])
    fterm = torch.randn(6, 80, generator=torch.Generator().manual_seed(23))
    fterm[4] = -1.25                                               # a constant tile
    idx, fidx = hm.attention_indices(a1), hm.feature_indices(fterm)
    assert {-1, 0, 100, 104} <= set(idx.flatten().tolist()) and fidx[4].tolist() == [0] * 80
    one = r.render(dev, coords, a1, fterm)
    two = r.render(dev, np.asarray(coords), a1.cuda(), fterm.cuda())
    assert one.dtype == torch.uint8 and tuple(one.shape) == (5, 203 // scale, 151 // scale, 3) and one.is_cuda
    assert torch.equal(one, two)
    want = ref.render(np.full(tuple(one.shape), 255, np.uint8), host, coords, 48, scale, idx.numpy(), fidx.numpy(), hm.JET105,
                      hm.VIRIDIS256, inset, 77, 230)
    assert np.array_equal(one.cpu().numpy(), want)
    assert (want[2:] != 255).any() and (want[1] != 255).any() and (want[:, -1] == 255).all()
    # other alphas reach the kernel
    r2 = mil_amd.AttentionMapRenderer(48, scale, inset=inset, alpha_tissue=1.0, alpha_map=0.0)
    assert (r2.q_tissue, r2.q_map) == (256, 0)
    _check(r2, dev, host, coords, jet, feat, 48, scale, inset)


def test_more_windows_than_one_launch_and_none():
    """70 000 distinct one-pixel windows (S = D = 1) of a 300 x 300 slide: two launches; T = 0: the canvas comes back untouched."""
    hh = ww = 300
    host = np.random.default_rng(31).integers(0, 256, (hh, ww, 3), dtype=np.uint8)
    rest = np.random.default_rng(32).permutation(np.arange(1, hh * ww - 1))[:69998]
    pick = np.concatenate([[0, hh * ww - 1], rest])                # the first and the last pixel of the slide among them
    coords = np.stack([pick // ww, pick % ww], axis=1)
    assert len(np.unique(pick)) == 70000
    jet, feat = _indices(70000, 33)
    dev = torch.from_numpy(host).cuda()
    r = mil_amd.AttentionMapRenderer(1, 1)
    _check(r, dev, host, coords, jet, feat, 1, 1)
    canvas = torch.full((5, hh, ww, 3), FILL, dtype=torch.uint8, device="cuda")
    out = r.render_into(canvas, dev, np.zeros((0, 2), dtype=np.int64), torch.zeros((4, 0), dtype=torch.int16))
    assert out is canvas and bool((out == FILL).all())
    assert bool((r.render(dev, [], torch.zeros(3, 0)) == 255).all())


def test_slide_bag_attention_maps_end_to_end(golden_dir):
    """slide -> tissue -> tiles -> model -> overlay: `attention_maps` equals `render` fed with the CPU copies of what
    `visualize_terms` and the forward return."""
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    bag = mil_amd.SlideBag(dev, 48, 7, resolution=32)
    with pytest.raises(RuntimeError):
        bag.attention_maps({}, 16)
    bag.build()
    tiles, coords = bag.get_inference_data()
    assert len(coords) == 4
    net = mil_amd.Attention(3).eval()
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()})
    with torch.no_grad():
        out = net(tiles, torch.tensor([1]))
    scale = 16
    got = bag.attention_maps(out, scale)
    hh, ww = z["slide"].shape[:2]
    assert got.dtype == torch.uint8 and tuple(got.shape) == (5, hh // scale, ww // scale, 3) and got.is_cuda
    a1 = mil_amd.visualize_terms(out)["A1"]
    fterm = out["Fterm"].detach().float().cpu()
    assert tuple(a1.shape) == (3, 4) and float(a1.min()) == 0.0 and float(a1.max()) == 1.0
    want = mil_amd.AttentionMapRenderer(48, scale).render(dev, coords, a1, fterm)
    assert torch.equal(got, want)
    host = ref.render(np.full(tuple(got.shape), 255, np.uint8), z["slide"], coords, 48, scale, hm.attention_indices(a1).numpy(),
                      hm.feature_indices(fterm).numpy(), hm.JET105, hm.VIRIDIS256)
    got = got.cpu().numpy()
    assert np.array_equal(got, host)
    owned = np.zeros((hh // scale, ww // scale), dtype=bool)
    for r, c in coords:
        owned[r // scale:r // scale + 3, c // scale:c // scale + 3] = True
    assert owned.sum() == 36 and (got[:, ~owned] == 255).all()                     # the background is white
    assert (got[0][owned] != 255).any() and (got[2:][:, owned] != 255).any()
    without = bag.attention_maps(out, scale, features=False).cpu().numpy()
    assert (without[1] == 255).all() and np.array_equal(without[[0, 2, 3, 4]], got[[0, 2, 3, 4]])
