"""CPU (-m "not gpu"): the affine augmentation (mil_amd.RandomAffine / mil_affine_u8) without a GPU — the numpy restatement
(tests/affine_reference.py) against Pillow itself where Pillow is installed and against Pillow's recorded bytes
(tests/golden/affine_u8.npz) everywhere, the matrix helpers, the constructor's ranges, the parameter draw, every refusal that
must fire before a launch, and the C entry's host-side status codes.  Every comparison of bytes is equality."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import _lib, ops
from mil_amd import affine as af

import affine_reference as ar


def _pillow(img, m, out_hw, fill):
    from PIL import Image
    oh, ow = out_hw
    mode = "L" if img.ndim == 2 else "RGB"
    fc = int(fill) if img.ndim == 2 else tuple(int(v) for v in np.broadcast_to(fill, (3,)))
    return np.asarray(Image.fromarray(np.ascontiguousarray(img), mode).transform(
        (ow, oh), Image.AFFINE, tuple(float(v) for v in m), Image.BILINEAR, fillcolor=fc))


def _random_matrix(rng, h, w):
    return ar.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-4, 5)), int(rng.integers(-4, 5))),
                            rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


# ---- the restatement against Pillow ----------------------------------------------------------------------------------------------
def test_restatement_equals_pillow_on_random_cases():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(50)
    sizes = [(1, 1, 1, 1), (1, 1, 5, 7), (1, 9, 1, 9), (7, 1, 3, 1), (1, 40, 40, 1), (40, 40, 40, 40)]
    for k in range(300):
        h, w, oh, ow = sizes[k] if k < len(sizes) else (int(v) for v in rng.integers(1, 41, 4))
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        fill = tuple(int(v) for v in rng.integers(0, 256, 3))
        m = _random_matrix(rng, h, w)
        if k % 7 == 0:                                                  # right angles through the trigonometric formula
            m = ar.affine_matrix((w * 0.5, h * 0.5), float(rng.choice([0, 90, 180, 270, -90])), (0, 0), 1.0, (0.0, 0.0))
        assert np.array_equal(ar.transform(img, m, (oh, ow), fill), _pillow(img, m, (oh, ow), fill)), (k, h, w, oh, ow, m)
    grey = rng.integers(0, 256, (13, 9), dtype=np.uint8)                # a single channel takes the same arithmetic
    m = _random_matrix(rng, 13, 9)
    assert np.array_equal(ar.transform(grey, m, (11, 10), 7), _pillow(grey, m, (11, 10), 7))


def test_quarter_turns_identity_and_outside_equal_pillow_and_rot90():
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(51)
    for n in (1, 2, 17, 32):
        img = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
        for k in range(4):
            m = ar.quarter_turn_matrix(k, n)
            want = np.rot90(img, k)
            assert np.array_equal(_pillow(img, m, (n, n), 9), want), (n, k)
            assert np.array_equal(ar.transform(img, m, None, 9), want), (n, k)
    img = rng.integers(0, 256, (11, 14, 3), dtype=np.uint8)
    assert np.array_equal(ar.transform(img, [1, 0, 0, 0, 1, 0]), img) and np.array_equal(_pillow(img, [1, 0, 0, 0, 1, 0], (11, 14), 0), img)
    for m in ([1, 0, 14, 0, 1, 0], [1, 0, 0, 0, 1, -11], [0.5, 0, -30, 0, 0.5, 3], [1, 0, 0, 0, 1, 1e300]):
        want = np.broadcast_to(np.array([4, 5, 6], np.uint8), (11, 14, 3))
        assert np.array_equal(ar.transform(img, m, None, (4, 5, 6)), want) and np.array_equal(_pillow(img, m, (11, 14), (4, 5, 6)), want)


def test_whole_slide_windows_equal_pillow():
    """A rotated window reads the slide, not itself: the four corner windows hit the clip, the Y+1 row rule and the fill; the
    inner ones read their real neighbourhood and get no fill."""
    pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(52)
    slide = rng.integers(0, 255, (70, 90, 3), dtype=np.uint8)           # no byte 255: fill pixels can be counted
    s = 24
    coords = [(0, 0), (0, 90 - s), (70 - s, 0), (70 - s, 90 - s), (20, 30), (23, 41), (46, 0), (0, 33)]
    ms = [ar.affine_matrix((s * 0.5, s * 0.5), a, (0, 0), sc, (sh, 0.0))
          for a, sc, sh in [(45, 1, 0), (-30, 1, 0), (17.5, 0.8, 5), (200, 1, 0), (45, 1, 0), (-8, 0.8, -10), (90, 1, 0), (3, 2, 0)]]
    got = ar.slide_windows(slide, coords, ms, s, (255, 255, 255))
    for i, ((r, c), m) in enumerate(zip(coords, ms)):
        mm = list(m)
        mm[2], mm[5] = mm[2] + float(c), mm[5] + float(r)
        assert np.array_equal(got[i], _pillow(slide, mm, (s, s), (255, 255, 255))), i
    filled = (got == 255).all(axis=-1).sum(axis=(1, 2))
    assert (filled[:4] > 0).all() and filled[4] == 0 and filled[5] == 0
    own = ar.transform(slide[20:44, 30:54], ms[4], None, (255, 255, 255))                   # the window alone has white corners
    assert (own == 255).all(axis=-1).sum() > 0 and not np.array_equal(own, got[4])


# ---- the restatement against Pillow's recorded bytes (no Pillow needed) --------------------------------------------------------
def test_restatement_reproduces_the_fixture(golden_dir):
    path = os.path.join(golden_dir, "affine_u8.npz")
    assert os.path.getsize(path) < 100_000
    z = np.load(path)
    assert z["p17_in"].shape == (3, 3, 17, 23) and z["p33_in"].shape == (1, 3, 33, 33) and z["p64_in"].shape == (1, 3, 64, 64)
    assert z["slide"].shape == (70, 90, 3) and z["coords"].shape == (6, 2) and z["win_out"].shape == (6, 24, 24, 3)
    for g in ("p17", "p33", "p64"):
        tin, m = z[g + "_in"], z[g + "_m"]
        tiles = tin[np.arange(len(m)) % len(tin)]
        assert np.array_equal(ar.transform_planar(tiles, m, None, z[g + "_fill"]), z[g + "_out"]), g
    for k in range(4):                                                  # the quarter turns are bit copies
        assert np.array_equal(z["p33_out"][k], np.rot90(z["p33_in"][0], k, axes=(1, 2))), k
    assert (z["p33_out"][4] == z["p33_fill"][:, None, None]).all()      # wholly outside
    assert np.array_equal(ar.slide_windows(z["slide"], z["coords"], z["win_m"], 24, z["win_fill"]), z["win_out"])
    corners = {(0, 0), (0, 66), (46, 0), (46, 66)}
    assert corners <= {tuple(c) for c in z["coords"].tolist()}


# ---- the matrix helpers --------------------------------------------------------------------------------------------------------------
def test_affine_matrix_hand_computed_cases():
    assert mil_amd.affine_matrix((12, 12), 0, (0, 0), 1.0, (0, 0)) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert mil_amd.affine_matrix((5, 7), 0, (3, -2), 1.0, (0, 0)) == [1.0, 0.0, -3.0, 0.0, 1.0, 2.0]       # output -> input: minus
    assert mil_amd.affine_matrix((4, 4), 0, (0, 0), 2.0, 0.0) == [0.5, 0.0, 2.0, 0.0, 0.5, 2.0]            # 0.5 p + (c - 0.5 c)
    m = mil_amd.affine_matrix((10, 6), 90, (0, 0), 1.0, (0, 0))         # a rotation about (10, 6): the centre is a fixed point
    c, s = math.cos(math.radians(90)), math.sin(math.radians(90))
    assert m[:2] == [c, s] and m[3:5] == [-s, c]
    assert abs(m[0] * 10 + m[1] * 6 + m[2] - 10) < 1e-12 and abs(m[3] * 10 + m[4] * 6 + m[5] - 6) < 1e-12
    m = mil_amd.affine_matrix((8, 8), 30, (0, 0), 1.0, (0, 0))
    c, s = math.cos(math.radians(30)), math.sin(math.radians(30))
    assert np.allclose(m, [c, s, 8 - 8 * c - 8 * s, -s, c, 8 + 8 * s - 8 * c], rtol=0, atol=1e-14)
    rng = np.random.default_rng(53)
    for _ in range(50):                                                 # the package's formula is the restatement's, bit for bit
        args = ((rng.uniform(1, 40), rng.uniform(1, 40)), rng.uniform(-360, 360), (int(rng.integers(-9, 10)), int(rng.integers(-9, 10))),
                rng.uniform(0.3, 3.0), (rng.uniform(-30, 30), rng.uniform(-30, 30)))
        assert mil_amd.affine_matrix(*args) == ar.affine_matrix(*args)
    with pytest.raises(ValueError):
        mil_amd.affine_matrix((1, 1), 0, (0, 0), 0.0, (0, 0))


def test_quarter_turn_matrices_are_integers():
    for n in (1, 24, 1200):
        for k in range(-1, 6):
            m = mil_amd.quarter_turn_matrix(k, n)
            assert m == ar.quarter_turn_matrix(k, n) and all(float(v).is_integer() for v in m)
    q = mil_amd.quarter_turn_matrix(1, 24)
    m = q
    for _ in range(3):                                                  # four quarter turns are the identity
        m = af.compose(q, m)
    assert m == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert af.compose(q, q) == mil_amd.quarter_turn_matrix(2, 24)
    with pytest.raises(ValueError):
        mil_amd.quarter_turn_matrix(1, 0)


# ---- the constructor and the draw --------------------------------------------------------------------------------------------------
def test_ranges():
    a = mil_amd.RandomAffine(15)
    assert a.degrees == (-15.0, 15.0) and a.translate is None and a.scale is None and a.shear is None and a.fill == 0
    a = mil_amd.RandomAffine((10, 20), translate=(0.1, 0.2), scale=(0.8, 1.25), shear=5, fill=(255, 255, 255), quarter_turns=True)
    assert a.degrees == (10.0, 20.0) and a.translate == (0.1, 0.2) and a.scale == (0.8, 1.25) and a.shear == (-5.0, 5.0)
    assert a.fill == (255, 255, 255) and a.quarter_turns is True
    assert mil_amd.RandomAffine(0, shear=(1, 2, 3, 4)).shear == (1.0, 2.0, 3.0, 4.0)
    assert {"RandomAffine", "affine_matrix", "quarter_turn_matrix"} <= set(mil_amd.__all__)


@pytest.mark.parametrize("kw", [dict(degrees=-1), dict(degrees=(1, 2, 3)), dict(degrees="10"), dict(degrees=None), dict(degrees=float("nan")),
                                dict(degrees=0, translate=0.1), dict(degrees=0, translate=(0.1, 1.5)), dict(degrees=0, translate=(-0.1, 0)),
                                dict(degrees=0, scale=(0, 1)), dict(degrees=0, scale=1.0), dict(degrees=0, scale=(-1, 1)),
                                dict(degrees=0, shear=-2), dict(degrees=0, shear=(1, 2, 3)), dict(degrees=0, fill=256),
                                dict(degrees=0, fill=(1, 2)), dict(degrees=0, fill=1.5), dict(degrees=0, fill=(0, 0, -1))])
def test_bad_constructor_values_raise(kw):
    with pytest.raises(ValueError):
        mil_amd.RandomAffine(**kw)


def test_draw_params_shapes_ranges_order_and_reproducibility():
    a = mil_amd.RandomAffine(30, translate=(0.1, 0.2), scale=(0.8, 1.25), shear=(-5, 5, -3, 3))
    p = a.draw_params(200, 24, torch.Generator().manual_seed(5))
    assert p.dtype == torch.float64 and tuple(p.shape) == (200, 6) and not p.is_cuda and bool(torch.isfinite(p).all())
    assert torch.equal(p, a.draw_params(200, 24, torch.Generator().manual_seed(5)))
    assert not torch.equal(p, a.draw_params(200, 24, torch.Generator().manual_seed(6)))
    assert tuple(a.draw_params(0, 24).shape) == (0, 6)
    # the documented order: one rand(n, 6) in float64 — angle, tx, ty, scale, shear x, shear y —, then (quarter turns) one randint
    g = torch.Generator().manual_seed(5)
    u = torch.rand((200, 6), dtype=torch.float64, generator=g).tolist()
    state = g.get_state()
    mx, my = 0.1 * 24, 0.2 * 24
    for i in (0, 7, 199):
        tx, ty = int(round(-mx + (mx + mx) * u[i][1])), int(round(-my + (my + my) * u[i][2]))
        want = ar.affine_matrix((12.0, 12.0), -30.0 + 60.0 * u[i][0], (tx, ty), 0.8 + (1.25 - 0.8) * u[i][3],
                                (-5.0 + 10.0 * u[i][4], -3.0 + 6.0 * u[i][5]))
        assert p[i].tolist() == want, i
    g2 = torch.Generator().manual_seed(5)
    a.draw_params(200, 24, g2)
    assert torch.equal(g2.get_state(), state)                           # nothing else is drawn
    # whole-pixel translations: with nothing else switched on the matrix is the identity shifted by integers
    t = mil_amd.RandomAffine(0, translate=(0.5, 0.5)).draw_params(100, (10, 20), torch.Generator().manual_seed(1))
    assert bool((t[:, [0, 4]] == 1).all()) and bool((t[:, [1, 3]] == 0).all()) and bool((t[:, [2, 5]] == t[:, [2, 5]].round()).all())
    assert float(t[:, 2].abs().max()) <= 10 and float(t[:, 5].abs().max()) <= 5 and len(set(t[:, 2].tolist())) > 5
    # a rectangle's centre
    r = mil_amd.RandomAffine((90, 90)).draw_params(1, (10, 20))[0].tolist()
    assert r == ar.affine_matrix((10.0, 5.0), 90.0, (0, 0), 1.0, (0.0, 0.0))


def test_quarter_turns_alone_give_the_integer_matrices():
    a = mil_amd.RandomAffine(0, quarter_turns=True)
    g = torch.Generator().manual_seed(9)
    p = a.draw_params(64, 24, g)
    g2 = torch.Generator().manual_seed(9)
    torch.rand((64, 6), dtype=torch.float64, generator=g2)
    k = torch.randint(0, 4, (64,), generator=g2).tolist()
    assert torch.equal(g.get_state(), g2.get_state()) and set(k) == {0, 1, 2, 3}
    for i in range(64):
        assert p[i].tolist() == ar.quarter_turn_matrix(k[i], 24), i     # exactly; -0.0 == 0.0
    assert bool((p == p.round()).all())
    with pytest.raises(ValueError):
        a.draw_params(2, (24, 25))
    # composed with a drawn rotation: the quarter turn comes after it
    b = mil_amd.RandomAffine((10, 10), quarter_turns=True).draw_params(8, 24, torch.Generator().manual_seed(9))
    base = ar.affine_matrix((12.0, 12.0), 10.0, (0, 0), 1.0, (0.0, 0.0))
    g3 = torch.Generator().manual_seed(9)
    torch.rand((8, 6), dtype=torch.float64, generator=g3)
    k = torch.randint(0, 4, (8,), generator=g3).tolist()
    for i in range(8):
        assert b[i].tolist() == af.compose(ar.quarter_turn_matrix(k[i], 24), base)


# ---- refusals before any launch ------------------------------------------------------------------------------------------------------
def _eye(n):
    return torch.tensor([[1.0, 0, 0, 0, 1.0, 0]] * n, dtype=torch.float64)


def test_apply_and_ops_refuse_before_any_launch():
    a = mil_amd.RandomAffine(10)
    tiles = mil_amd.U8Tiles(torch.zeros((2, 3, 8, 6), dtype=torch.uint8))
    with pytest.raises(RuntimeError):
        a.apply(tiles, _eye(2))                                         # CPU tiles: no fallback
    with pytest.raises(RuntimeError):
        a(tiles)
    nan = _eye(2)
    nan[1, 2] = float("nan")
    inf = _eye(2)
    inf[0, 0] = float("inf")
    for bad in (_eye(3), torch.zeros((2, 5), dtype=torch.float64), torch.zeros(12, dtype=torch.float64), nan, inf, None, "m",
                torch.zeros((2, 6), dtype=torch.bool)):
        with pytest.raises(ValueError):
            a.apply(tiles, bad)
    with pytest.raises(ValueError):
        a.apply(torch.zeros((2, 3, 8, 8), dtype=torch.uint8), _eye(2))  # a tensor, not the handle
    s2d = mil_amd.S2dTiles(torch.zeros((2, 4, 4, 16), dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="U8Tiles"):
        a.apply(s2d, _eye(2))
    with pytest.raises(ValueError, match="U8Tiles"):
        a(s2d)
    u8 = torch.zeros((2, 3, 8, 6), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.affine_u8(u8, _eye(2))                                      # the launcher itself: not on the GPU
    with pytest.raises(ValueError):
        ops.affine_u8(u8.float(), _eye(2))
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.affine_windows_u8(slide, [(0, 0), (3, 5)], _eye(2), 0, 16)
    for args in ((slide, [(0, 0), (30, 5)], _eye(2), 0, 16), (slide, [(0, 0)], _eye(2), 0, 16), (slide, [(0, 0)], _eye(1), 300, 16),
                 (slide, [(0, 0)], _eye(1), 0, None), (slide, [(0, 0)], nan[1:], 0, 16), (slide[None], None, _eye(2), 0)):
        with pytest.raises(ValueError):
            ops.affine_windows_u8(*args)
    assert ops.affine_fill(7) == 7 | 7 << 8 | 7 << 16 and ops.affine_fill((1, 2, 3)) == 1 | 2 << 8 | 3 << 16


def test_preprocessor_and_bag_refuse_before_any_launch():
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    rois = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    coords = [(0, 0), (3, 5)]
    nan = _eye(2)
    nan[0, 5] = float("nan")
    for out in ("u8", "nchw", "s2d"):
        with pytest.raises(RuntimeError):
            prep(rois, None, out=out, affine=_eye(2))                   # CPU ROIs: no fallback
        with pytest.raises(RuntimeError):
            prep.from_slide(slide, coords, None, out=out, affine=_eye(2))
        for bad in (_eye(3), nan, torch.zeros((2, 4), dtype=torch.float64)):
            with pytest.raises(ValueError):
                prep(rois, None, out=out, affine=bad)
            with pytest.raises(ValueError):
                prep.from_slide(slide, coords, None, out=out, affine=bad)
    with pytest.raises(ValueError):
        prep.from_slide(slide, coords, None, out="u8", affine=_eye(2), affine_fill=(1, 2))
    with pytest.raises(ValueError):
        prep.from_slide(slide, [(0, 0), (30, 5)], None, out="u8", affine=_eye(2))              # a window outside the slide
    with pytest.raises(ValueError):
        prep(torch.zeros((2, 12, 12, 3), dtype=torch.uint8), None, out="u8", affine=_eye(2))   # not the planned ROI size
    with pytest.raises(ValueError):
        prep(rois, None, out="nhwc", affine=_eye(2))
    with pytest.raises(TypeError):
        prep.from_slide(slide, coords, None, "u8", None, None, _eye(2))                       # keyword-only
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords)
    assert bag.affine is None
    with pytest.raises(ValueError, match="affine="):
        bag.get_train_data(affine_params=_eye(2))                       # a bag made without affine=
    with pytest.raises(TypeError):
        mil_amd.SlideBag(slide, 16, 0, 8, 4, 2500, None, coords, None, mil_amd.RandomAffine(5))


class _Recorder:
    """Stands in for a TilePreprocessor: records what the bag hands it, draws as the real one does, launches nothing."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def draw_params(self, n, generator=None):
        return self.real.draw_params(n, generator)

    def from_slide(self, *args, **kw):
        self.calls.append((args, kw))
        return "tiles"


def test_bag_without_affine_consumes_the_generator_as_before():
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    coords = [(0, 0), (3, 5), (20, 20)]
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    sj = mil_amd.StainJitter(0.05, 0.01)
    # what a bag drew before this feature: crop / flip parameters, the colour jitter's, the stain jitter's — nothing after
    g0 = torch.Generator().manual_seed(77)
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    want = (prep.draw_params(3, g0), jit.draw_params(3, g0), sj.draw_params(3, g0))
    state_before = g0.get_state()

    plain = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, color_jitter=jit, stain_jitter=sj)
    plain.prep = rec = _Recorder(plain.prep)
    g1 = torch.Generator().manual_seed(77)
    assert plain.get_train_data(generator=g1) == "tiles"
    assert torch.equal(g1.get_state(), state_before)
    (args, kw), = rec.calls
    assert torch.equal(args[2], want[0]) and all(torch.equal(x, y) for x, y in zip(kw["jitter"], want[1]))
    assert "affine" not in kw and "affine_fill" not in kw               # the call is the one made before

    aff = mil_amd.RandomAffine(20, fill=(255, 255, 255), quarter_turns=True)
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=coords, color_jitter=jit, stain_jitter=sj, affine=aff)
    bag.prep = rec = _Recorder(bag.prep)
    g2 = torch.Generator().manual_seed(77)
    bag.get_train_data(generator=g2)
    (args, kw), = rec.calls
    assert torch.equal(args[2], want[0]) and all(torch.equal(x, y) for x, y in zip(kw["jitter"], want[1]))     # the same draws first
    assert torch.equal(kw["affine"], aff.draw_params(3, 16, g0)) and kw["affine_fill"] == (255, 255, 255)     # then the affine's
    assert torch.equal(g2.get_state(), g0.get_state())
    rec.calls.clear()
    inj = _eye(3)
    bag.get_train_data(generator=torch.Generator().manual_seed(77), affine_params=inj)
    assert rec.calls[0][1]["affine"] is inj
    rec.calls.clear()
    bag.get_validation_data()
    bag.get_inference_data()
    assert all("affine" not in kw for _, kw in rec.calls) and len(rec.calls) == 2                              # never transformed


# ---- the C entry's host-side checks ----------------------------------------------------------------------------------------------------
def test_entry_status_codes_need_no_gpu():
    assert "mil_affine_u8" in _lib.EXPORTS
    assert hasattr(ctypes.CDLL(mil_amd.LIB_PATH), "mil_affine_u8")
    f = mil_amd.lib().mil_affine_u8
    buf = np.zeros(64, dtype=np.float64)
    one = buf.ctypes.data

    def call(src=one, st=(48, 4, 1, 16), wh=(4, 4), dst=one, ds=(1, 16), out=(4, 4), mat=one, n=1):
        return f(src, *st, *wh, dst, *ds, *out, mat, 0, n, None)

    assert call(src=None) == 1 and call(dst=None) == 1 and call(mat=None) == 1
    assert call(n=-1) == 1
    for bad in ((0, 4), (4, 0), (-3, 4)):
        assert call(wh=bad) == 1 and call(out=bad) == 1
    assert call(st=(-1, 4, 1, 16)) == 1 and call(st=(48, 0, 1, 16)) == 1 and call(st=(48, 4, 0, 16)) == 1 and call(st=(48, 4, 1, 0)) == 1
    assert call(ds=(0, 16)) == 1 and call(ds=(1, 0)) == 1
    assert call(out=(65536, 65536)) == 2 and call(out=(65536, 65536), n=0) == 2         # the shape is refused whatever n is
    assert call(n=0) == 0 and call(n=0, st=(0, 12, 3, 1), ds=(3, 1)) == 0               # n == 0: success without a launch
    assert mil_amd.lib().mil_abi_version() == 2
