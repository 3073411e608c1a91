"""-m gpu: the elastic deformation on the device (mil_affine_elastic_u8 through `ops.elastic_u8`, `ops.elastic_windows_u8`,
`ElasticDeform.apply`, `TilePreprocessor(..., elastic=)` and `SlideBag(elastic=)`).  Every comparison is equality of bytes (or of
fp32 bits): against the recorded fixture (tests/golden/elastic_u8.npz), against the numpy restatement tests/elastic_reference.py,
which tests/test_cpu_elastic.py pins to Pillow's bytes and to scipy, and — for lattices of zeros — against the affine kernel's
own output.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import ops
from mil_amd import preprocess as pp

import affine_reference as ar
import elastic_reference as er

pytestmark = pytest.mark.gpu


def _random_matrix(rng, h, w):
    return ar.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))),
                            rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


def _lattice(rng, n, gy, gx, sigma=1.5, clip=2.0):
    return np.clip(sigma * rng.standard_normal((n, 2, gy + 3, gx + 3)), -clip, clip)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bad_tiles(got, want):
    return np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1)).tolist()


def test_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "elastic_u8.npz"))
    for g in ("p17", "p33"):
        tin, m = z[g + "_in"], z[g + "_m"]
        tiles = tin[np.arange(len(m)) % len(tin)]
        fill = tuple(int(v) for v in z[g + "_fill"])
        got = ops.elastic_u8(_dev(tiles), torch.from_numpy(m), z[g + "_ctrl"], fill).cpu().numpy()
        assert got.shape == z[g + "_out"].shape and _bad_tiles(got, z[g + "_out"]) == [], g
    fill = tuple(int(v) for v in z["win_fill"])
    got = ops.elastic_windows_u8(_dev(z["slide"]), z["coords"], z["win_m"], z["win_ctrl"], fill, 24).cpu().numpy()
    assert _bad_tiles(got, z["win_out"]) == []


def test_zero_lattice_equals_the_affine_kernel():
    rng = np.random.default_rng(11)
    for h, w, oh, ow, gy, gx in ((1, 1, 1, 1, 1, 1), (17, 23, 17, 23, 3, 2), (23, 17, 9, 31, 2, 5), (40, 37, 40, 37, 4, 4)):
        n = 4
        tiles = _dev(rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8))
        ms = np.array([_random_matrix(rng, h, w) for _ in range(n)])
        want = ops.affine_u8(tiles, ms, (3, 250, 77), (oh, ow))
        for zero in (0.0, -0.0):
            got = ops.elastic_u8(tiles, ms, np.full((n, 2, gy + 3, gx + 3), zero), (3, 250, 77), (oh, ow))
            assert torch.equal(got, want), (h, w, zero)
    slide = _dev(rng.integers(0, 256, (70, 90, 3), dtype=np.uint8))
    coords = np.array([(0, 0), (0, 66), (46, 0), (46, 66), (20, 30)])
    ms = np.array([_random_matrix(rng, 24, 24) for _ in range(len(coords))])
    want = ops.affine_windows_u8(slide, coords, ms, (255, 255, 255), 24)
    for zero in (0.0, -0.0):
        got = ops.elastic_windows_u8(slide, coords, ms, np.full((len(coords), 2, 7, 7), zero), (255, 255, 255), 24)
        assert torch.equal(got, want), zero
    rois = _dev(rng.integers(0, 256, (3, 24, 24, 3), dtype=np.uint8))
    assert torch.equal(ops.elastic_windows_u8(rois, None, ms[:3], np.zeros((3, 2, 4, 4)), 9), ops.affine_windows_u8(rois, None, ms[:3], 9))


@pytest.mark.parametrize("h,w,oh,ow,cells", [(1, 1, 1, 1, (1, 1)), (1, 7, 7, 1, (2, 1)), (5, 3, 5, 3, (2, 2)), (17, 23, 17, 23, (3, 2)),
                                             (23, 17, 9, 31, (2, 5)), (33, 35, 33, 35, (4, 4)), (40, 37, 40, 37, (5, 5))])
def test_random_planar_cases_equal_the_restatement(h, w, oh, ow, cells):
    """The smallest tile; an output shape different from the input's; a partial last group (15 pixels); groups that cross a row
    end and a cell boundary (23 columns in 2 cells); several workgroups (33 * 35 > 1024 pixels)."""
    rng = np.random.default_rng(1000 * h + w)
    n = 6
    tiles = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    ms = np.array([_random_matrix(rng, h, w) for _ in range(n)])
    ms[0] = [1, 0, 0, 0, 1, 0]
    ctrl = _lattice(rng, n, *cells)
    fill = (3, 250, 77)
    got = ops.elastic_u8(_dev(tiles), ms, ctrl, fill, None if (oh, ow) == (h, w) else (oh, ow)).cpu().numpy()
    want = er.transform_planar(tiles, ms, ctrl, (oh, ow), fill)
    assert got.shape == (n, 3, oh, ow) and _bad_tiles(got, want) == []
    if (h, w) == (40, 37):                                              # matrices=None is the identity; the class goes the same way
        got = ops.elastic_u8(_dev(tiles), None, ctrl, fill).cpu().numpy()
        assert _bad_tiles(got, er.transform_planar(tiles, None, ctrl, None, fill)) == []
        handle = mil_amd.U8Tiles(_dev(tiles))
        out = mil_amd.ElasticDeform(1.5, cells=cells, clip=2.0, fill=fill).apply(handle, ctrl, ms)
        assert isinstance(out, mil_amd.U8Tiles) and out.u8.data_ptr() != handle.u8.data_ptr() and _bad_tiles(out.u8.cpu().numpy(), want) == []
        e = mil_amd.ElasticDeform(1.0, cells=cells, fill=fill)
        drawn = e(handle, torch.Generator().manual_seed(2))
        lat = e.draw_params(n, (h, w), torch.Generator().manual_seed(2))
        assert _bad_tiles(drawn.u8.cpu().numpy(), er.transform_planar(tiles, None, lat.numpy(), None, fill)) == []


@pytest.mark.parametrize("s", [1, 5, 24, 37])
def test_random_interleaved_cases_equal_the_restatement(s):
    """The ROI-stack form: the source of a window is the window, what lies outside it is fill."""
    rng = np.random.default_rng(s)
    n = 5
    rois = rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8)
    ms = np.array([_random_matrix(rng, s, s) for _ in range(n)])
    ctrl = _lattice(rng, n, min(s, 3), min(s, 4))
    got = ops.elastic_windows_u8(_dev(rois), None, ms, ctrl, (9, 8, 7)).cpu().numpy()
    assert _bad_tiles(got, er.transform_interleaved(rois, ms, ctrl, (9, 8, 7))) == []


def test_unaligned_slide_view_with_lattices_that_leave_the_slide():
    """A slide whose storage starts at an odd byte: windows in the four corners and inside, displaced by up to 8 pixels, so
    that in the corners source coordinates leave the slide and `fill` is taken."""
    rng = np.random.default_rng(4)
    slide = rng.integers(0, 255, (70, 90, 3), dtype=np.uint8)           # no byte 255: fill pixels can be counted
    buf = torch.empty(70 * 90 * 3 + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(70, 90, 3)
    view.copy_(_dev(slide))
    assert view.data_ptr() % 2 == 1
    s = 24
    coords = np.array([(0, 0), (0, 66), (46, 0), (46, 66), (20, 30), (23, 41), (11, 5)])
    ctrl = _lattice(rng, len(coords), 4, 4, 5.0, 8.0)
    got = ops.elastic_windows_u8(view, coords, None, ctrl, (255, 255, 255), s).cpu().numpy()
    want = er.slide_windows(slide, coords, None, ctrl, s, (255, 255, 255))
    assert _bad_tiles(got, want) == []
    filled = (want == 255).all(axis=-1).sum(axis=(1, 2))
    assert (filled[:4] > 0).all() and filled[4] == 0 and filled[5] == 0
    ms = np.array([_random_matrix(rng, s, s) for _ in range(len(coords))])
    got = ops.elastic_windows_u8(view, coords, ms, ctrl, (255, 255, 255), s).cpu().numpy()
    assert _bad_tiles(got, er.slide_windows(slide, coords, ms, ctrl, s, (255, 255, 255))) == []


def test_no_tiles_and_more_tiles_than_one_launch():
    e = ops.elastic_u8(torch.empty((0, 3, 8, 9), dtype=torch.uint8, device="cuda"), None, np.empty((0, 2, 4, 4)), 0, (4, 5))
    assert tuple(e.shape) == (0, 3, 4, 5)
    e = ops.elastic_windows_u8(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda"), None, None, np.empty((0, 2, 5, 5)), 0)
    assert tuple(e.shape) == (0, 8, 8, 3)
    h = mil_amd.U8Tiles(torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda"))
    assert len(mil_amd.ElasticDeform(0.2, cells=2)(h)) == 0
    # 65536 tiles of one pixel, every lattice its own constant: a displacement of a quarter pixel keeps the byte (both taps are
    # the one pixel), an x displacement of a whole pixel leaves the tile and gives the fill.  The second launch holds tile 65535,
    # whose lattice moves it out while tile 0's does not: it comes out right only if the lattice pointer advanced with the
    # matrices.
    t = 65536
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 255, (t, 3, 1, 1), dtype=np.uint8)         # no byte 255: the fill can be told apart
    leaves = rng.integers(0, 2, t).astype(bool)
    leaves[0], leaves[65534], leaves[65535] = False, False, True
    ctrl = np.zeros((t, 2, 4, 4))
    ctrl[:, 0] = np.where(leaves, 1.0, 0.25)[:, None, None]
    ctrl[:, 1] = np.where(rng.integers(0, 2, t) == 1, -0.25, 0.0)[:, None, None]
    got = ops.elastic_u8(_dev(tiles), None, ctrl, 255).cpu().numpy()
    want = tiles.copy()
    want[leaves] = 255
    assert _bad_tiles(got, want) == []
    assert (got[65535] == 255).all() and (got[65534] == tiles[65534]).all()
    assert _bad_tiles(got[:64], er.transform_planar(tiles[:64], None, ctrl[:64], None, 255)) == []


def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], **kw)


def _bits(x, out):
    return x.u8 if out == "u8" else x.xs.view(torch.int16) if out == "s2d" else x.view(torch.int32)


def test_from_slide_with_affine_and_elastic_equals_call_on_the_deformed_windows(golden_dir, monkeypatch):
    z, dev, bag = _golden_bag(golden_dir)
    slide, kept = z["slide"], z["kept"]
    prep, s = bag.prep, 48
    n = len(kept)
    assert n == 4
    aff = mil_amd.RandomAffine(180, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5, fill=(255, 255, 255))
    m = aff.draw_params(n, s, torch.Generator().manual_seed(3))
    c = mil_amd.ElasticDeform(2.0, cells=4).draw_params(n, s, torch.Generator().manual_seed(4))
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    deformed = er.slide_windows(slide, kept, m.numpy(), c.numpy(), s, (255, 255, 255))
    assert (deformed != ar.slide_windows(slide, kept, m.numpy(), s, (255, 255, 255))).any()
    launches = []
    real = ops.elastic_windows_u8
    monkeypatch.setattr(ops, "elastic_windows_u8", lambda *a, **k: launches.append(len(a[3])) or real(*a, **k))
    monkeypatch.setattr(ops, "affine_windows_u8", lambda *a, **k: pytest.fail("the affine launch of its own"))
    monkeypatch.setattr(pp, "AFFINE_CHUNK", 2)                          # two chunks: the seam is crossed
    for out in ("u8", "nchw", "s2d"):
        for p in (params, None):
            want = prep(_dev(deformed), p, out=out)
            launches.clear()
            got = prep.from_slide(dev, kept, p, out=out, affine=m, elastic=c, affine_fill=(255, 255, 255))
            assert launches == [2, 2]                                   # ONE launch per chunk for both transforms
            assert type(got) is type(want) and torch.equal(_bits(got, out), _bits(want, out)), (out, p is None)
        a, b = prep.from_slide(dev, kept, params, out=out, elastic=None), prep.from_slide(dev, kept, params, out=out)
        assert torch.equal(_bits(a, out), _bits(b, out)), out           # elastic=None is the call made before
    # an odd number of windows: the last chunk is short
    got = prep.from_slide(dev, kept[:3], params[:3], out="u8", affine=m[:3], elastic=c[:3], affine_fill=(255, 255, 255))
    assert torch.equal(got.u8, prep(_dev(deformed[:3]), params[:3], out="u8").u8)
    # elastic alone: the identity matrix
    alone = er.slide_windows(slide, kept, None, c.numpy(), s, 7)
    got = prep.from_slide(dev, kept, params, out="u8", elastic=c, affine_fill=7)
    assert torch.equal(got.u8, prep(_dev(alone), params, out="u8").u8)
    # the stack entry: the source of a window is the window itself
    plain = np.stack([slide[r:r + s, q:q + s] for r, q in kept])
    own = er.transform_interleaved(plain, m.numpy(), c.numpy(), 7)
    got = prep(_dev(plain), params, out="u8", affine=m, elastic=c, affine_fill=7)
    assert torch.equal(got.u8, prep(_dev(own), params, out="u8").u8) and not torch.equal(got.u8, prep(_dev(deformed), params, out="u8").u8)
    # with a colour jitter behind it: transform, chain, jitter
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    jp = jit.draw_params(n, torch.Generator().manual_seed(4))
    want = jit.apply(prep(_dev(deformed), params, out="u8"), jp)
    got = prep.from_slide(dev, kept, params, out="u8", jitter=jp, affine=m, elastic=c, affine_fill=(255, 255, 255))
    assert torch.equal(got.u8, want.u8)
    e = prep.from_slide(dev, kept[:0], None, out="u8", elastic=c[:0])
    assert isinstance(e, mil_amd.U8Tiles) and tuple(e.shape) == (0, 3, 32, 32)


def test_slide_bag_with_elastic(golden_dir):
    aff = mil_amd.RandomAffine(30, fill=(255, 255, 255))
    el = mil_amd.ElasticDeform(2.0, cells=4)
    z, dev, bag = _golden_bag(golden_dir, affine=aff, elastic=el)
    _, _, plain = _golden_bag(golden_dir)
    _, _, only = _golden_bag(golden_dir, elastic=mil_amd.ElasticDeform(2.0, cells=4, fill=9))
    kept = z["kept"]
    n = len(kept)
    assert bag.build() and plain.build() and only.build()
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    m = aff.draw_params(n, 48, torch.Generator().manual_seed(6))
    c = el.draw_params(n, 48, torch.Generator().manual_seed(7))
    train = bag.get_train_data(params=params, affine_params=m, elastic_params=c)
    deformed = er.slide_windows(z["slide"], kept, m.numpy(), c.numpy(), 48, (255, 255, 255))
    assert torch.equal(train.u8, bag.prep(_dev(deformed), params, out="u8").u8)
    assert not torch.equal(train.u8, plain.get_train_data(params=params).u8)                # train tiles are deformed
    assert torch.equal(bag.get_validation_data().u8, plain.get_validation_data().u8)        # validation and inference tiles are not
    assert torch.equal(bag.get_inference_data()[0].u8, plain.get_inference_data()[0].u8)
    assert torch.equal(only.get_validation_data().u8, plain.get_validation_data().u8)
    got = only.get_train_data(params=params, elastic_params=c)
    assert torch.equal(got.u8, bag.prep(_dev(er.slide_windows(z["slide"], kept, None, c.numpy(), 48, 9)), params, out="u8").u8)
    # drawn from the generator: the crop / flip parameters first, the affine's, the lattices last
    g = torch.Generator().manual_seed(8)
    p0 = bag.prep.draw_params(n, g)
    m0 = aff.draw_params(n, 48, g)
    c0 = el.draw_params(n, 48, g)
    drawn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    assert torch.equal(drawn.u8, bag.get_train_data(params=p0, affine_params=m0, elastic_params=c0).u8)
    # a seeded bag without elastic= gives the bytes it gave before: those of its own draws through the affine path alone
    _, _, old = _golden_bag(golden_dir, affine=aff)
    old.build()
    rotated = ar.slide_windows(z["slide"], kept, m0.numpy(), 48, (255, 255, 255))
    assert torch.equal(old.get_train_data(generator=torch.Generator().manual_seed(8)).u8, old.prep(_dev(rotated), p0, out="u8").u8)
    assert torch.equal(plain.get_train_data(generator=torch.Generator().manual_seed(8)).u8, plain.get_train_data(params=p0).u8)


def test_attention_forward_on_deformed_tiles():
    rng = np.random.default_rng(31)
    tiles = mil_amd.U8Tiles(_dev(rng.integers(0, 256, (8, 3, 64, 64), dtype=np.uint8)))
    out = mil_amd.ElasticDeform(1.5, cells=4, fill=(255, 255, 255))(tiles, torch.Generator().manual_seed(4))
    assert out.shape == tiles.shape and not torch.equal(out.u8, tiles.u8)
    torch.manual_seed(0)
    net = mil_amd.Attention(3).eval()
    res = net(out, torch.tensor([1]))
    assert len(res) > 3
    for k in res:
        assert bool(torch.isfinite(res[k]).all()), k
