"""-m gpu: the affine augmentation on the device (mil_affine_u8 through `ops.affine_u8`, `ops.affine_windows_u8`,
`RandomAffine.apply`, `TilePreprocessor(..., affine=)` and `SlideBag(affine=)`).  Every comparison is equality of bytes (or of
fp32 bits): against Pillow's recorded bytes (tests/golden/affine_u8.npz) and against the numpy restatement
tests/affine_reference.py, which tests/test_cpu_affine.py pins to Pillow.  No tolerance anywhere."""
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import ops
from mil_amd import preprocess as pp

import affine_reference as ar

pytestmark = pytest.mark.gpu


def _random_matrix(rng, h, w):
    return ar.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))),
                            rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bad_tiles(got, want):
    return np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1)).tolist()


def test_fixture_equals_pillows_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "affine_u8.npz"))
    for g in ("p17", "p33", "p64"):
        tin, m = z[g + "_in"], z[g + "_m"]
        tiles = tin[np.arange(len(m)) % len(tin)]
        fill = tuple(int(v) for v in z[g + "_fill"])
        got = ops.affine_u8(_dev(tiles), torch.from_numpy(m), fill).cpu().numpy()
        assert got.shape == z[g + "_out"].shape and _bad_tiles(got, z[g + "_out"]) == [], g
    fill = tuple(int(v) for v in z["win_fill"])
    got = ops.affine_windows_u8(_dev(z["slide"]), z["coords"], z["win_m"], fill, 24).cpu().numpy()
    assert _bad_tiles(got, z["win_out"]) == []


@pytest.mark.parametrize("h,w,oh,ow", [(1, 1, 1, 1), (1, 7, 7, 1), (5, 3, 5, 3), (17, 23, 17, 23), (23, 17, 9, 31), (33, 33, 33, 33),
                                       (40, 37, 40, 37), (31, 64, 33, 35)])
def test_random_planar_cases_equal_the_restatement(h, w, oh, ow):
    """Odd sizes (misaligned planes, a partial last group), several workgroups (33 * 35 > 1024), out_hw != the input size."""
    rng = np.random.default_rng(1000 * h + w)
    n = 6
    tiles = rng.integers(0, 256, (n, 3, h, w), dtype=np.uint8)
    ms = np.array([_random_matrix(rng, h, w) for _ in range(n)])
    ms[0] = [1, 0, 0, 0, 1, 0]
    fill = (3, 250, 77)
    got = ops.affine_u8(_dev(tiles), ms, fill, None if (oh, ow) == (h, w) else (oh, ow)).cpu().numpy()
    want = ar.transform_planar(tiles, ms, (oh, ow), fill)
    assert got.shape == (n, 3, oh, ow) and _bad_tiles(got, want) == []


@pytest.mark.parametrize("s", [1, 5, 24, 37])
def test_random_interleaved_cases_equal_the_restatement(s):
    """The ROI-stack form: the source of a window is the window, what lies outside it is fill."""
    rng = np.random.default_rng(s)
    n = 5
    rois = rng.integers(0, 256, (n, s, s, 3), dtype=np.uint8)
    ms = np.array([_random_matrix(rng, s, s) for _ in range(n)])
    got = ops.affine_windows_u8(_dev(rois), None, ms, (9, 8, 7)).cpu().numpy()
    want = np.stack([ar.transform(r, m, None, (9, 8, 7)) for r, m in zip(rois, ms)])
    assert _bad_tiles(got, want) == []


def test_quarter_turns_equal_rot90():
    rng = np.random.default_rng(3)
    for n in (1, 6, 33):
        tiles = _dev(rng.integers(0, 256, (4, 3, n, n), dtype=np.uint8))
        ms = torch.tensor([mil_amd.quarter_turn_matrix(k, n) for k in range(4)], dtype=torch.float64)
        got = ops.affine_u8(tiles, ms, 0)
        for k in range(4):
            assert torch.equal(got[k], torch.rot90(tiles[k], k, dims=(1, 2))), (n, k)
        rois = tiles.permute(0, 2, 3, 1).contiguous()
        got = ops.affine_windows_u8(rois, None, ms, 0)
        for k in range(4):
            assert torch.equal(got[k], torch.rot90(rois[k], k, dims=(0, 1))), (n, k)
    # the class: quarter turns alone are bit copies
    tiles = mil_amd.U8Tiles(_dev(rng.integers(0, 256, (16, 3, 20, 20), dtype=np.uint8)))
    a = mil_amd.RandomAffine(0, quarter_turns=True)
    m = a.draw_params(16, 20, torch.Generator().manual_seed(2))
    out = a.apply(tiles, m)
    assert isinstance(out, mil_amd.U8Tiles) and out.u8.data_ptr() != tiles.u8.data_ptr() and out.shape == tiles.shape
    turns = [[mil_amd.quarter_turn_matrix(k, 20) for k in range(4)].index(row) for row in m.tolist()]
    assert len(set(turns)) == 4
    for i, k in enumerate(turns):
        assert torch.equal(out.u8[i], torch.rot90(tiles.u8[i], k, dims=(1, 2))), i
    drawn = a(tiles, torch.Generator().manual_seed(2))
    assert torch.equal(drawn.u8, out.u8)


def test_unaligned_slide_view():
    """A slide whose storage starts at an odd byte, as `from_slide` allows: windows in the corners and inside."""
    rng = np.random.default_rng(4)
    slide = rng.integers(0, 256, (70, 90, 3), dtype=np.uint8)
    buf = torch.empty(70 * 90 * 3 + 1, dtype=torch.uint8, device="cuda")
    view = buf[1:].view(70, 90, 3)
    view.copy_(_dev(slide))
    assert view.data_ptr() % 2 == 1
    s = 24
    coords = np.array([(0, 0), (0, 66), (46, 0), (46, 66), (20, 30), (23, 41), (11, 5)])
    ms = np.array([_random_matrix(rng, s, s) for _ in range(len(coords))])
    got = ops.affine_windows_u8(view, coords, ms, (255, 255, 255), s).cpu().numpy()
    assert _bad_tiles(got, ar.slide_windows(slide, coords, ms, s, (255, 255, 255))) == []


def test_no_tiles_and_more_tiles_than_one_launch():
    e = ops.affine_u8(torch.empty((0, 3, 8, 9), dtype=torch.uint8, device="cuda"), torch.empty((0, 6), dtype=torch.float64), 0, (4, 5))
    assert tuple(e.shape) == (0, 3, 4, 5)
    e = ops.affine_windows_u8(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device="cuda"), None, np.empty((0, 6)), 0)
    assert tuple(e.shape) == (0, 8, 8, 3)
    h = mil_amd.U8Tiles(torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda"))
    assert len(mil_amd.RandomAffine(10)(h)) == 0
    # 65536 tiles of one pixel: the identity keeps the byte, a shift by one pixel gives the fill; the second launch holds tile 65535
    t = 65536
    rng = np.random.default_rng(5)
    tiles = rng.integers(0, 255, (t, 3, 1, 1), dtype=np.uint8)
    ms = np.tile(np.array([[1.0, 0, 0, 0, 1, 0]]), (t, 1))
    ms[1::2, 2] = 1.0
    got = ops.affine_u8(_dev(tiles), ms, 255).cpu().numpy()
    want = tiles.copy()
    want[1::2] = 255
    assert _bad_tiles(got, want) == []
    assert got[65535, 0, 0, 0] == 255 and (got[65534] == tiles[65534]).all()


def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], **kw)


def _bits(x, out):
    return x.u8 if out == "u8" else x.xs.view(torch.int16) if out == "s2d" else x.view(torch.int32)


def test_from_slide_with_affine_equals_call_on_the_rotated_windows(golden_dir, monkeypatch):
    z, dev, bag = _golden_bag(golden_dir)
    slide, kept = z["slide"], z["kept"]
    prep, s = bag.prep, 48
    n = len(kept)
    assert n == 4
    aff = mil_amd.RandomAffine(180, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5, fill=(255, 255, 255))
    m = aff.draw_params(n, s, torch.Generator().manual_seed(3))
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    rotated = ar.slide_windows(slide, kept, m.numpy(), s, (255, 255, 255))
    plain = np.stack([slide[r:r + s, c:c + s] for r, c in kept])
    assert (rotated != plain).any()
    monkeypatch.setattr(pp, "AFFINE_CHUNK", 2)                          # two chunks: the seam is crossed
    for out in ("u8", "nchw", "s2d"):
        for p in (params, None):
            want = prep(_dev(rotated), p, out=out)
            got = prep.from_slide(dev, kept, p, out=out, affine=m, affine_fill=(255, 255, 255))
            assert type(got) is type(want) and torch.equal(_bits(got, out), _bits(want, out)), (out, p is None)
        # affine=None is the call made before, bit for bit
        a, b = prep.from_slide(dev, kept, params, out=out, affine=None), prep.from_slide(dev, kept, params, out=out)
        assert torch.equal(_bits(a, out), _bits(b, out)) and torch.equal(_bits(a, out), _bits(prep(_dev(plain), params, out=out), out)), out
    # an odd number of windows: the last chunk is short
    got = prep.from_slide(dev, kept[:3], params[:3], out="u8", affine=m[:3], affine_fill=(255, 255, 255))
    assert torch.equal(got.u8, prep(_dev(rotated[:3]), params[:3], out="u8").u8)
    # the stack entry: the source of a window is the window itself
    own = np.stack([ar.transform(w, mm, None, 7) for w, mm in zip(plain, m.numpy())])
    got = prep(_dev(plain), params, out="u8", affine=m, affine_fill=7)
    assert torch.equal(got.u8, prep(_dev(own), params, out="u8").u8) and not torch.equal(got.u8, prep(_dev(rotated), params, out="u8").u8)
    # with a colour jitter behind it: transform, chain, jitter
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    jp = jit.draw_params(n, torch.Generator().manual_seed(4))
    want = jit.apply(prep(_dev(rotated), params, out="u8"), jp)
    got = prep.from_slide(dev, kept, params, out="u8", jitter=jp, affine=m, affine_fill=(255, 255, 255))
    assert torch.equal(got.u8, want.u8)
    e = prep.from_slide(dev, kept[:0], None, out="u8", affine=m[:0])
    assert isinstance(e, mil_amd.U8Tiles) and tuple(e.shape) == (0, 3, 32, 32)


def test_slide_bag_with_affine(golden_dir):
    aff = mil_amd.RandomAffine(30, fill=(255, 255, 255), quarter_turns=True)
    z, dev, bag = _golden_bag(golden_dir, affine=aff)
    _, _, plain = _golden_bag(golden_dir)
    kept = z["kept"]
    n = len(kept)
    assert bag.build() and plain.build()
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    m = aff.draw_params(n, 48, torch.Generator().manual_seed(6))
    train = bag.get_train_data(params=params, affine_params=m)
    rotated = ar.slide_windows(z["slide"], kept, m.numpy(), 48, (255, 255, 255))
    assert torch.equal(train.u8, bag.prep(_dev(rotated), params, out="u8").u8)
    assert not torch.equal(train.u8, plain.get_train_data(params=params).u8)                # train tiles change
    assert torch.equal(bag.get_train_data(params=params, affine_params=m).u8, train.u8)     # injected parameters reproduce a run
    assert torch.equal(bag.get_validation_data().u8, plain.get_validation_data().u8)        # validation and inference tiles do not
    assert torch.equal(bag.get_inference_data()[0].u8, plain.get_inference_data()[0].u8)
    # drawn from the generator: the crop / flip parameters first, the affine's last
    g = torch.Generator().manual_seed(8)
    p0 = bag.prep.draw_params(n, g)
    m0 = aff.draw_params(n, 48, g)
    drawn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    assert torch.equal(drawn.u8, bag.get_train_data(params=p0, affine_params=m0).u8)
    assert torch.equal(plain.get_train_data(generator=torch.Generator().manual_seed(8)).u8, plain.get_train_data(params=p0).u8)


def test_attention_forward_on_transformed_tiles():
    rng = np.random.default_rng(31)
    tiles = mil_amd.U8Tiles(_dev(rng.integers(0, 256, (8, 3, 64, 64), dtype=np.uint8)))
    out = mil_amd.RandomAffine(45, scale=(0.9, 1.1), fill=(255, 255, 255))(tiles, torch.Generator().manual_seed(4))
    assert out.shape == tiles.shape and not torch.equal(out.u8, tiles.u8)
    torch.manual_seed(0)
    net = mil_amd.Attention(3).eval()
    res = net(out, torch.tensor([1]))
    assert len(res) > 3
    for k in res:
        assert bool(torch.isfinite(res[k]).all()), k
