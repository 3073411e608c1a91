"""CPU (-m "not gpu"): the elastic deformation (mil_amd.ElasticDeform / mil_affine_elastic_u8) without a GPU — the numpy
restatement (tests/elastic_reference.py) against the affine restatement and Pillow's recorded bytes where the lattice is zero,
against scipy where the matrix is the identity, and against its own recorded bytes (tests/golden/elastic_u8.npz); the B-spline
tables and the convex-hull bound; the parameter draw; every refusal that must fire before a launch; the C entry's host-side
status codes.  Every comparison of bytes is equality except the scipy one, whose margin of one byte is stated there."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import _lib, ops

import affine_reference as ar
import elastic_reference as er

EPS = float(np.finfo(np.float64).eps)


def _random_matrix(rng, h, w):
    return ar.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))),
                            rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


# ---- a lattice of zeros is the affine transform ----------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (5, 3), (17, 23), (33, 33), (40, 37), (64, 64)])
def test_zero_lattice_equals_the_affine_restatement(h, w):
    rng = np.random.default_rng(100 * h + w)
    for k in range(4):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        m = _random_matrix(rng, h, w) if k else [1, 0, 0, 0, 1, 0]
        gy, gx = int(rng.integers(1, 6)), int(rng.integers(1, 6))
        want = ar.transform(img, m, None, (9, 8, 7))
        for zero in (0.0, -0.0):
            got = er.transform(img, m, np.full((2, gy + 3, gx + 3), zero), None, (9, 8, 7))
            assert np.array_equal(got, want), (h, w, k, zero)
    out_hw = (w + 2, h + 1)                                             # an output of another size
    m = _random_matrix(rng, h, w)
    assert np.array_equal(er.transform(img, m, np.zeros((2, 4, 5)), out_hw, 3), ar.transform(img, m, out_hw, 3))


def test_zero_lattice_equals_pillows_recorded_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "affine_u8.npz"))
    for g in ("p17", "p33", "p64"):
        tin, m = z[g + "_in"], z[g + "_m"]
        tiles = tin[np.arange(len(m)) % len(tin)]
        for zero in (0.0, -0.0):
            ctrl = np.full((len(m), 2, 7, 6), zero)
            assert np.array_equal(er.transform_planar(tiles, m, ctrl, None, z[g + "_fill"]), z[g + "_out"]), (g, zero)
    for zero in (0.0, -0.0):
        ctrl = np.full((len(z["coords"]), 2, 7, 7), zero)
        assert np.array_equal(er.slide_windows(z["slide"], z["coords"], z["win_m"], ctrl, 24, z["win_fill"]), z["win_out"])


# ---- the tables --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [1, 5, 17, 33, 37, 64, 300])
def test_table_properties_and_the_package_tables(size):
    for cells in range(1, 9):
        idx, w = er.tables(size, cells)
        assert idx.dtype == np.int32 and idx.shape == (size,) and w.dtype == np.float64 and w.shape == (size, 4)
        assert idx.min() >= 0 and idx.max() <= cells - 1 and (np.diff(idx) >= 0).all()
        assert np.isfinite(w).all() and (w >= 0).all()
        total = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        assert np.abs(total - 1.0).max() <= 2 * EPS, (size, cells, np.abs(total - 1.0).max())       # a few ulp of 1
        pidx, pw = ops.elastic_tables(size, cells)
        assert pidx.dtype == torch.int32 and pw.dtype == torch.float64 and not pidx.is_cuda and pw.is_contiguous()
        assert np.array_equal(pidx.numpy(), idx) and np.array_equal(pw.numpy().view(np.int64), w.view(np.int64))
    if size >= 8:                                                       # every cell is reached
        assert set(er.tables(size, 8)[0].tolist()) == set(range(8))
    for bad in ((0, 1), (4, 0), (4.0, 2), (4, True), ("4", 1)):
        with pytest.raises(ValueError):
            ops.elastic_tables(*bad)


def test_displacement_stays_inside_the_convex_hull_of_the_lattice():
    rng = np.random.default_rng(7)
    for k, (oh, ow, gy, gx) in enumerate([(1, 1, 1, 1), (5, 3, 1, 2), (17, 23, 3, 2), (33, 33, 4, 4), (40, 37, 5, 5), (64, 64, 4, 4),
                                          (64, 64, 8, 8), (300, 300, 8, 8)]):
        ctrl = np.clip(1.5 * rng.standard_normal((2, gy + 3, gx + 3)), -2.0, 2.0)
        dx, dy = er.field(ctrl, (oh, ow))
        assert dx.shape == (oh, ow) and max(np.abs(dx).max(), np.abs(dy).max()) <= 2.0, k
        # a saturated lattice: sixteen non-negative weights whose row and column sums are within 2 ulp of 1, added in seven
        # rounded operations per axis — the bound is clip * (1 + 2 eps)^2 * (1 + eps / 2)^14 < clip * (1 + 12 eps)
        dx, dy = er.field(np.full((2, gy + 3, gx + 3), 2.0), (oh, ow))
        assert np.abs(dx - 2.0).max() <= 24 * EPS and np.array_equal(dx, dy), k
        const = er.field(np.stack([np.full((gy + 3, gx + 3), -0.75), np.full((gy + 3, gx + 3), 1.25)]), (oh, ow))
        assert np.abs(const[0] + 0.75).max() <= 12 * EPS and np.abs(const[1] - 1.25).max() <= 12 * EPS


# ---- an outside check: scipy's linear interpolation at the displaced coordinates ---------------------------------------------------
@pytest.mark.parametrize("seed", range(8))
def test_identity_matrix_agrees_with_scipy_map_coordinates(seed):
    """With the identity matrix the source position of output pixel (x, y) is the index pair (y + dy, x + dx) (pixel centres
    are at index + 0.5 in the contract's coordinates).  scipy orders its roundings differently, so the floors may differ by one
    byte where the interpolated value lies within rounding of an integer; pixels at least 3 from every edge (|d| <= 2) read
    inside the image, where no edge rule of either side takes part."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    ctrl = np.clip(1.5 * rng.standard_normal((2, 7, 7)), -2.0, 2.0)
    got = er.transform(img, er.IDENTITY, ctrl, None, 0).astype(np.int64)
    dx, dy = er.field(ctrl, (64, 64))
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    want = np.stack([np.floor(ndimage.map_coordinates(img[..., c].astype(np.float64), [yy + dy, xx + dx], order=1))
                     for c in range(3)], axis=-1).astype(np.int64)
    inner = np.zeros((64, 64), bool)
    inner[3:-3, 3:-3] = True
    assert inner.mean() >= 0.80
    worst = int(np.abs(got - want)[inner].max())
    print(f"seed {seed}: worst |restatement - floor(scipy)| on {inner.mean():.1%} of the pixels = {worst}")
    assert worst <= 1
    assert (got != img)[inner].any()                                    # the lattice did move something


# ---- the restatement against its recorded bytes -----------------------------------------------------------------------------------
def test_restatement_reproduces_the_fixture(golden_dir):
    path = os.path.join(golden_dir, "elastic_u8.npz")
    assert os.path.getsize(path) < 100_000
    z = np.load(path)
    assert z["p17_in"].shape == (3, 3, 17, 23) and z["p17_ctrl"].shape == (3, 2, 6, 5)
    assert z["p33_in"].shape == (1, 3, 33, 33) and z["p33_ctrl"].shape == (3, 2, 7, 7)
    assert z["slide"].shape == (70, 90, 3) and z["coords"].shape == (4, 2) and z["win_out"].shape == (4, 24, 24, 3)
    for g in ("p17", "p33"):
        tin, m = z[g + "_in"], z[g + "_m"]
        tiles = tin[np.arange(len(m)) % len(tin)]
        assert np.array_equal(er.transform_planar(tiles, m, z[g + "_ctrl"], None, z[g + "_fill"]), z[g + "_out"]), g
    assert not z["p33_ctrl"][2].any()                                   # the zero lattice: the affine transform's bytes
    t33 = np.moveaxis(z["p33_in"][0], 0, -1)
    assert np.array_equal(np.moveaxis(z["p33_out"][2], 0, -1), ar.transform(t33, z["p33_m"][2], None, z["p33_fill"]))
    assert not np.array_equal(np.moveaxis(z["p33_out"][1], 0, -1), ar.transform(t33, z["p33_m"][1], None, z["p33_fill"]))
    assert np.array_equal(er.slide_windows(z["slide"], z["coords"], z["win_m"], z["win_ctrl"], 24, z["win_fill"]), z["win_out"])
    assert {(0, 0), (46, 66)} <= {tuple(c) for c in z["coords"].tolist()}
    filled = (z["win_out"] == 255).all(axis=-1).sum(axis=(1, 2))
    assert (filled[:2] > 0).all() and (filled[2:] == 0).all()           # the corners leave the slide, the inner windows do not


# ---- the constructor and the draw --------------------------------------------------------------------------------------------------
def test_constructor_values():
    e = mil_amd.ElasticDeform(1.5)
    assert e.magnitude == 1.5 and e.cells == (4, 4) and e.clip == 3.0 and e.fill == 0
    e = mil_amd.ElasticDeform(2, cells=(3, 2), clip=2.5, fill=(255, 255, 255))
    assert e.magnitude == 2.0 and e.cells == (3, 2) and e.clip == 2.5 and e.fill == (255, 255, 255)
    assert mil_amd.ElasticDeform(0).clip == 0.0
    assert "ElasticDeform" in mil_amd.__all__


@pytest.mark.parametrize("kw", [dict(magnitude=-1), dict(magnitude="1"), dict(magnitude=None), dict(magnitude=float("nan")),
                                dict(magnitude=float("inf")), dict(magnitude=True), dict(magnitude=1, cells=0), dict(magnitude=1, cells=2.5),
                                dict(magnitude=1, cells=(2, 3, 4)), dict(magnitude=1, cells=(2, -1)), dict(magnitude=1, cells="4"),
                                dict(magnitude=1, clip=-0.5), dict(magnitude=1, clip=float("nan")), dict(magnitude=1, clip="2"),
                                dict(magnitude=1, fill=256), dict(magnitude=1, fill=(1, 2)), dict(magnitude=1, fill=1.5)])
def test_bad_constructor_values_raise(kw):
    with pytest.raises(ValueError):
        mil_amd.ElasticDeform(**kw)


def test_draw_params_shape_clamp_order_and_fold_bound():
    e = mil_amd.ElasticDeform(1.5, cells=(3, 2), clip=2.0)
    p = e.draw_params(200, (24, 30), torch.Generator().manual_seed(5))
    assert p.dtype == torch.float64 and tuple(p.shape) == (200, 2, 6, 5) and not p.is_cuda and p.is_contiguous()
    assert float(p.abs().max()) == 2.0 and bool(torch.isfinite(p).all())                    # some entries reach the clamp
    assert torch.equal(p, e.draw_params(200, (24, 30), torch.Generator().manual_seed(5)))
    assert not torch.equal(p, e.draw_params(200, (24, 30), torch.Generator().manual_seed(6)))
    assert tuple(e.draw_params(0, 24).shape) == (0, 2, 6, 5)
    g = torch.Generator().manual_seed(5)                                # the documented draw: ONE randn, nothing else
    want = (torch.randn((200, 2, 6, 5), dtype=torch.float64, generator=g) * 1.5).clamp(-2.0, 2.0)
    g2 = torch.Generator().manual_seed(5)
    assert torch.equal(e.draw_params(200, (24, 30), g2), want) and torch.equal(g2.get_state(), g.get_state())
    # the default clip is twice the magnitude
    q = mil_amd.ElasticDeform(1.0).draw_params(500, 64, torch.Generator().manual_seed(1))
    assert 1.9 < float(q.abs().max()) <= 2.0
    # clip against 0.4 of the smaller cell side: 24 / 3 = 8 rows, 30 / 2 = 15 columns -> 3.2 pixels
    mil_amd.ElasticDeform(1, cells=(3, 2), clip=3.2).draw_params(1, (24, 30))
    with pytest.raises(ValueError, match="fold"):
        mil_amd.ElasticDeform(1, cells=(3, 2), clip=3.3).draw_params(1, (24, 30))
    with pytest.raises(ValueError, match="fold"):
        mil_amd.ElasticDeform(2, cells=8).draw_params(1, 64)            # clip 4 > 0.4 * 8
    for bad in ((-1, 24), (1, 0), (1, (24, 0))):
        with pytest.raises(ValueError):
            e.draw_params(*bad)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _eye(n):
    return torch.tensor([[1.0, 0, 0, 0, 1.0, 0]] * n, dtype=torch.float64)


def _lat(n, gy=4, gx=4):
    return torch.zeros((n, 2, gy + 3, gx + 3), dtype=torch.float64)


def _bad_lattices(n):
    nan, inf = _lat(n), _lat(n)
    nan[n - 1, 1, 2, 3] = float("nan")
    inf[0, 0, 0, 0] = float("-inf")
    return (_lat(n + 1), torch.zeros((n, 3, 7, 7), dtype=torch.float64), torch.zeros((n, 2, 3, 7), dtype=torch.float64),
            torch.zeros((n, 2, 7, 3), dtype=torch.float64), torch.zeros((n, 2, 7), dtype=torch.float64), nan, inf, None, "c",
            torch.zeros((n, 2, 7, 7), dtype=torch.bool), torch.zeros((n, 2, 7, 7), dtype=torch.complex64))


def test_elastic_lattice():
    c = ops.elastic_lattice(np.ones((2, 2, 4, 9), np.float32), 2)
    assert c.dtype == torch.float64 and tuple(c.shape) == (2, 2, 4, 9) and c.is_contiguous() and not c.is_cuda
    assert tuple(ops.elastic_lattice(torch.zeros((3, 2, 5, 5), dtype=torch.int32), 3).shape) == (3, 2, 5, 5)
    assert tuple(ops.elastic_lattice(np.zeros((0, 2, 4, 4)), 0).shape) == (0, 2, 4, 4)
    for bad in _bad_lattices(2):
        with pytest.raises(ValueError):
            ops.elastic_lattice(bad, 2)


def test_apply_and_ops_refuse_before_any_launch():
    e = mil_amd.ElasticDeform(1.0)
    tiles = mil_amd.U8Tiles(torch.zeros((2, 3, 32, 24), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        e.apply(tiles, _lat(2))                                         # CPU tiles: no fallback
    with pytest.raises(RuntimeError):
        e.apply(tiles, _lat(2), _eye(2))
    with pytest.raises(RuntimeError):
        e(tiles)
    for bad in _bad_lattices(2):
        with pytest.raises(ValueError):
            e.apply(tiles, bad)
    nan = _eye(2)
    nan[1, 2] = float("nan")
    for bad in (_eye(3), nan, torch.zeros((2, 5), dtype=torch.float64), "m"):
        with pytest.raises(ValueError):
            e.apply(tiles, _lat(2), bad)
    with pytest.raises(ValueError):
        e.apply(torch.zeros((2, 3, 8, 8), dtype=torch.uint8), _lat(2))  # a tensor, not the handle
    s2d = mil_amd.S2dTiles(torch.zeros((2, 4, 4, 16), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="U8Tiles"):
        e.apply(s2d, _lat(2))
    with pytest.raises(ValueError, match="U8Tiles"):
        e(s2d)
    with pytest.raises(ValueError, match="fold"):
        mil_amd.ElasticDeform(4.0, cells=8)(mil_amd.U8Tiles(torch.zeros((1, 3, 16, 16), dtype=torch.uint8)))
    u8 = torch.zeros((2, 3, 8, 6), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.elastic_u8(u8, None, _lat(2))                               # the launcher itself: not on the GPU
    with pytest.raises(ValueError):
        ops.elastic_u8(u8.float(), None, _lat(2))
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.elastic_windows_u8(slide, [(0, 0), (3, 5)], _eye(2), _lat(2), 0, 16)
    with pytest.raises(RuntimeError):
        ops.elastic_windows_u8(slide, [(0, 0), (3, 5)], None, _lat(2), 0, 16)
    for args in ((slide, [(0, 0), (30, 5)], _eye(2), _lat(2), 0, 16), (slide, [(0, 0)], _eye(2), _lat(1), 0, 16),
                 (slide, [(0, 0)], _eye(1), _lat(2), 0, 16), (slide, [(0, 0)], _eye(1), _lat(1), 300, 16),
                 (slide, [(0, 0)], _eye(1), _lat(1), 0, None), (slide, [(0, 0)], nan[1:], _lat(1), 0, 16),
                 (slide[None], None, _eye(2), _lat(2), 0), (slide, [(0, 0)], None, _bad_lattices(1)[5], 0, 16)):
        with pytest.raises(ValueError):
            ops.elastic_windows_u8(*args)


def test_preprocessor_and_bag_refuse_before_any_launch():
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    rois = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    coords = [(0, 0), (3, 5)]
    for out in ("u8", "nchw", "s2d"):
        for aff in (None, _eye(2)):
            with pytest.raises(RuntimeError):
                prep(rois, None, out=out, affine=aff, elastic=_lat(2))  # CPU ROIs: no fallback
            with pytest.raises(RuntimeError):
                prep.from_slide(slide, coords, None, out=out, affine=aff, elastic=_lat(2))
            for bad in _bad_lattices(2)[:7]:
                with pytest.raises(ValueError):
                    prep(rois, None, out=out, affine=aff, elastic=bad)
                with pytest.raises(ValueError):
                    prep.from_slide(slide, coords, None, out=out, affine=aff, elastic=bad)
    with pytest.raises(ValueError):
        prep.from_slide(slide, coords, None, out="u8", affine=_eye(3), elastic=_lat(2))
    with pytest.raises(ValueError):
        prep.from_slide(slide, coords, None, out="u8", elastic=_lat(2), affine_fill=(1, 2))
    with pytest.raises(ValueError):
        prep.from_slide(slide, [(0, 0), (30, 5)], None, out="u8", elastic=_lat(2))              # a window outside the slide
    with pytest.raises(ValueError):
        prep(torch.zeros((2, 12, 12, 3), dtype=torch.uint8), None, out="u8", elastic=_lat(2))   # not the planned ROI size
    with pytest.raises(ValueError):
        prep(rois, None, out="nhwc", elastic=_lat(2))
    with pytest.raises(ValueError):
        prep(rois, None, out="u8", elastic=_lat(2), jitter="j")
    with pytest.raises(TypeError):
        prep.from_slide(slide, coords, None, "u8", None, None, None, 0, _lat(2))                # keyword-only
    with pytest.raises(TypeError):
        prep(rois, None, "u8", None, None, None, 0, _lat(2))
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords)
    assert bag.elastic is None
    with pytest.raises(ValueError, match="elastic="):
        bag.get_train_data(elastic_params=_lat(2))                      # a bag made without elastic=
    with pytest.raises(TypeError):
        mil_amd.SlideBag(slide, 16, 0, 8, 4, 2500, None, coords, None, None, None, None, mil_amd.ElasticDeform(1))
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, elastic=mil_amd.ElasticDeform(0.5))
    with pytest.raises(RuntimeError):
        bag.get_train_data()                                            # a CPU slide: no fallback
    with pytest.raises(ValueError):
        bag.get_train_data(elastic_params=_lat(3))


class _Recorder:
    """Stands in for a TilePreprocessor: records what the bag hands it, draws as the real one does, launches nothing."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def draw_params(self, n, generator=None):
        return self.real.draw_params(n, generator)

    def from_slide(self, *args, **kw):
        self.calls.append((args, kw))
        return "tiles"


def test_bag_draws_the_lattices_last_and_bags_without_elastic_do_not_move():
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    coords = [(0, 0), (3, 5), (20, 20)]
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    aff = mil_amd.RandomAffine(20, fill=(255, 255, 255))
    el = mil_amd.ElasticDeform(0.5, cells=2, fill=7)
    g0 = torch.Generator().manual_seed(77)
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    want = (prep.draw_params(3, g0), jit.draw_params(3, g0), aff.draw_params(3, 16, g0))
    state_before = g0.get_state()

    old = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, color_jitter=jit, affine=aff)
    old.prep = rec = _Recorder(old.prep)
    g1 = torch.Generator().manual_seed(77)
    assert old.get_train_data(generator=g1) == "tiles"
    assert torch.equal(g1.get_state(), state_before)                    # a bag without elastic= draws what it drew before
    (args, kw), = rec.calls
    assert torch.equal(kw["affine"], want[2]) and kw["affine_fill"] == (255, 255, 255) and "elastic" not in kw

    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, color_jitter=jit, affine=aff, elastic=el)
    bag.prep = rec = _Recorder(bag.prep)
    g2 = torch.Generator().manual_seed(77)
    bag.get_train_data(generator=g2)
    (args, kw), = rec.calls
    assert torch.equal(args[2], want[0]) and torch.equal(kw["affine"], want[2]) and kw["affine_fill"] == (255, 255, 255)
    assert torch.equal(kw["elastic"], el.draw_params(3, 16, g0)) and torch.equal(g2.get_state(), g0.get_state())   # the last draw
    rec.calls.clear()
    inj = _lat(3, 2, 2)
    bag.get_train_data(generator=torch.Generator().manual_seed(77), elastic_params=inj)
    assert rec.calls[0][1]["elastic"] is inj
    rec.calls.clear()
    bag.get_validation_data()
    bag.get_inference_data()
    assert all("elastic" not in kw and "affine" not in kw for _, kw in rec.calls) and len(rec.calls) == 2           # never deformed

    alone = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, elastic=el)      # no affine: the deform's own fill
    alone.prep = rec = _Recorder(alone.prep)
    g3 = torch.Generator().manual_seed(3)
    alone.get_train_data(generator=g3)
    g4 = torch.Generator().manual_seed(3)
    prep.draw_params(3, g4)
    (args, kw), = rec.calls
    assert kw["affine"] is None and kw["affine_fill"] == 7 and torch.equal(kw["elastic"], el.draw_params(3, 16, g4))
    with pytest.raises(ValueError, match="affine="):
        alone.get_train_data(affine_params=_eye(3))


# ---- the C entry's host-side checks ----------------------------------------------------------------------------------------------------
def test_entry_status_codes_need_no_gpu():
    assert "mil_affine_elastic_u8" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(mil_amd.LIB_PATH), "mil_affine_elastic_u8")
    f = mil_amd.lib().mil_affine_elastic_u8
    buf = np.zeros(64, dtype=np.float64)
    one = buf.ctypes.data

    def call(src=one, st=(48, 4, 1, 16), wh=(4, 4), dst=one, ds=(1, 16), out=(4, 4), mat=one, n=1, ctrl=one, lat=(4, 4), iy=one, wy=one,
             ix=one, wx=one):
        return f(src, *st, *wh, dst, *ds, *out, mat, 0, n, ctrl, *lat, iy, wy, ix, wx, None)

    assert call(src=None) == 1 and call(dst=None) == 1 and call(mat=None) == 1
    assert call(ctrl=None) == 1 and call(iy=None) == 1 and call(wy=None) == 1 and call(ix=None) == 1 and call(wx=None) == 1
    assert call(n=-1) == 1
    for bad in ((3, 4), (4, 3), (0, 7), (7, -1)):
        assert call(lat=bad) == 1 and call(lat=bad, n=0) == 1
    for bad in ((0, 4), (4, 0), (-3, 4)):
        assert call(wh=bad) == 1 and call(out=bad) == 1
    assert call(st=(-1, 4, 1, 16)) == 1 and call(st=(48, 0, 1, 16)) == 1 and call(st=(48, 4, 0, 16)) == 1 and call(st=(48, 4, 1, 0)) == 1
    assert call(ds=(0, 16)) == 1 and call(ds=(1, 0)) == 1
    assert call(out=(65536, 65536)) == 2 and call(out=(65536, 65536), n=0) == 2         # the shape is refused whatever n is
    assert call(n=0) == 0 and call(n=0, st=(0, 12, 3, 1), ds=(3, 1), lat=(11, 4)) == 0  # n == 0: success without a launch
    assert mil_amd.lib().mil_abi_version() == 2
