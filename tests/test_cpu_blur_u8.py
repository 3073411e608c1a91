"""CPU (-m "not gpu"): Pillow's Gaussian blur for uint8 tiles without a GPU — the numpy restatement of `mil_gaussian_blur_u8` against
Pillow itself (live, where Pillow imports) and against the bytes Pillow wrote into tests/golden/gaussian_blur_u8.npz, the six integers
`ops.box_blur_params` makes of a sigma, `GaussianBlurU8.draw_params`, every refusal of the host layer (they fire before anything is
launched), and the status codes of the entry point."""
import ctypes
import os

import numpy as np
import pytest
import torch

import blur_u8_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AWKWARD = [0.05, 0.3, 0.6, 1.0, 1.4, 2.0, 4.0, 8.0]


def test_the_restatement_is_pillows_gaussian_blur_bit_for_bit():
    """330 random (size, sigma) pairs: heights and widths 1..80 (the first 80 cases walk the sizes 1..80 so that every one is
    met, planes narrower than the box included), sigmas up to 8 with the awkward ones (0.3, 0.6, 1.0, 1.4: a box radius about to
    change) among them, `L` and `RGB`, and every third case Pillow's (sx, sy) tuple radius, which runs the two axes with
    independent radii."""
    PIL = pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    rng = np.random.default_rng(20261021)
    n = 0
    for i in range(330):
        h, w = (i + 1, 81 - (i + 1)) if i < 80 else (int(rng.integers(1, 81)), int(rng.integers(1, 81)))
        s = float(AWKWARD[i % 8]) if i % 2 else float(rng.uniform(0.0, 8.0))
        sigma = (s, float(rng.choice([0.0, 0.3, 8.0, rng.uniform(0.0, 8.0)]))) if i % 3 == 2 else s
        img = rng.integers(0, 256, (h, w, 3) if i % 2 else (h, w), dtype=np.uint8)
        if i % 5 == 0:
            img[: h // 2] = 255 * (i % 2)                       # a flat region: saturation
        want = np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur(sigma)))
        got = ref.blur_image(img, sigma)
        assert np.array_equal(got, want), (PIL.__version__, h, w, sigma, int(np.abs(got.astype(int) - want).max()))
        n += 1
    assert n >= 300


def test_the_tuple_radius_blurs_the_two_axes_independently():
    """(sx, 0) blurs along the width only, (0, sy) along the height only, and (sx, sy) is the one after the other: what the
    restatement says, and — where Pillow imports — what Pillow does."""
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (23, 31), dtype=np.uint8)
    a = ref.blur_image(img, (2.0, 0.0))
    assert np.array_equal(ref.blur_image(a, (0.0, 3.0)), ref.blur_image(img, (2.0, 3.0)))
    col = np.repeat(rng.integers(0, 256, (23, 1), dtype=np.uint8), 31, axis=1)          # constant along the width
    assert np.array_equal(ref.blur_image(col, (5.0, 0.0)), col) and not np.array_equal(ref.blur_image(col, (0.0, 5.0)), col)
    pytest.importorskip("PIL")
    from PIL import Image, ImageFilter
    assert np.array_equal(np.asarray(Image.fromarray(img).filter(ImageFilter.GaussianBlur((2.0, 0.0)))), a)
    assert np.array_equal(np.asarray(Image.fromarray(col).filter(ImageFilter.GaussianBlur((5.0, 0.0)))), col)


def test_the_restatement_equals_pillows_recorded_bytes(golden_dir):
    path = os.path.join(golden_dir, "gaussian_blur_u8.npz")
    assert os.path.getsize(path) < 64 * 1024
    z = np.load(path)
    seen, shapes = set(), set()
    for name in ("rgb_70x67", "rgb_33x47", "l_64x64", "l_5x3"):
        img, sigmas, want = z[name + "_in"], z[name + "_sigmas"], z[name + "_out"]
        assert img.dtype == np.uint8 and want.shape == (len(sigmas),) + img.shape
        shapes.add(img.shape)
        assert (img == 0).any() and (img == 255).any()
        for s, w in zip(sigmas, want):
            assert np.array_equal(ref.blur_image(img, (float(s[0]), float(s[1]))), w), (name, s)
            seen.update(float(v) for v in s)
    assert shapes == {(70, 67, 3), (33, 47, 3), (64, 64), (5, 3)}
    assert {0.3, 1.0, 1.4, 4.0, 8.0} <= seen
    assert any(s[0] != s[1] for name in ("rgb_33x47", "l_64x64") for s in z[name + "_sigmas"])       # an anisotropic case


def test_box_blur_params_identities():
    import mil_amd
    from mil_amd import _lib, ops
    assert _lib.BLUR_U8_MAX_BOX == ref.MAX_BOX == 7 and ops.BLUR_U8_MAX_SIGMA == 8.0
    ident = [0, 1 << 24, 0]
    assert ops.box_blur_params(0.0).tolist() == [ident + ident]
    assert ops.box_blur_params(8.0).tolist() == [[7, 1052688, 493448] * 2]                  # sigma 8: l = 7
    sweep = sorted(set(AWKWARD + [0.0, 1e-3, 7.999] + np.linspace(0.0, 8.0, 161).tolist()))
    p = ops.box_blur_params(sweep)
    assert p.dtype == torch.int32 and tuple(p.shape) == (len(sweep), 6) and not p.is_cuda
    assert torch.equal(p[:, :3], p[:, 3:])
    assert np.array_equal(p.numpy(), ref.params_array(sweep))
    r, ww, fw = (p[:, k].to(torch.int64) for k in range(3))
    assert int(r.min()) == 0 and int(r.max()) == 7 and bool((r[1:] >= r[:-1]).all())
    assert int(ww.min()) > 0 and int(fw.min()) >= 0
    total = (2 * r + 1) * ww + 2 * fw
    assert int(total.max()) <= 1 << 24 and int(total.min()) >= (1 << 24) - 1                 # fw is a floor of a half
    assert bool((ww[1:] < (1 << 24)).all())                                                   # only sigma 0 is the identity here
    # the two axes are independent; a single number beside n is repeated
    q = ops.box_blur_params([0.0, 0.3], [4.0, 0.0])
    assert q.tolist() == [ident + list(ref.box_params(4.0)), list(ref.box_params(0.3)) + ident]
    assert ops.box_blur_params([1.0, 2.0], 3.0).tolist() == [list(ref.item_params(1.0, 3.0)), list(ref.item_params(2.0, 3.0))]
    assert tuple(ops.box_blur_params([]).shape) == (0, 6)
    assert ops.box_blur_params(torch.tensor([1.4])).tolist() == [list(ref.item_params(1.4))]
    for bad in (-0.1, 8.001, float("nan"), float("inf"), "1", None, True, [[1.0]], [1.0, -1.0]):
        with pytest.raises(ValueError, match="sigma"):
            ops.box_blur_params(bad)
    with pytest.raises(ValueError, match="sigma"):
        ops.box_blur_params([1.0, 2.0], [1.0, 2.0, 3.0])
    assert "GaussianBlurU8" in mil_amd.__all__ and "gaussian_blur_u8" in mil_amd.__all__


def test_draw_params():
    import mil_amd
    blur = mil_amd.GaussianBlurU8()
    assert blur.sigma == (0.1, 2.0) and blur.p == 0.5
    a = blur.draw_params(1000, torch.Generator().manual_seed(3))
    b = blur.draw_params(1000, torch.Generator().manual_seed(3))
    assert a.dtype == torch.float64 and tuple(a.shape) == (1000,) and torch.equal(a, b)
    # the draw itself: one rand(n, 2) in float64
    u = torch.rand((1000, 2), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    assert torch.equal(a, torch.where(u[:, 0] < 0.5, 0.1 + 1.9 * u[:, 1], torch.zeros((), dtype=torch.float64)))
    on = a[a > 0]
    assert 400 < len(on) < 600 and float(on.min()) >= 0.1 and float(on.max()) <= 2.0
    assert not bool(mil_amd.GaussianBlurU8((0.5, 8.0), p=0).draw_params(200).any())
    full = mil_amd.GaussianBlurU8((0.5, 8.0), p=1).draw_params(200)
    assert float(full.min()) >= 0.5 and float(full.max()) <= 8.0
    fixed = mil_amd.GaussianBlurU8(1.5, p=1.0).draw_params(7)
    assert fixed.tolist() == [1.5] * 7 and mil_amd.GaussianBlurU8(1.5).sigma == (1.5, 1.5)
    assert tuple(blur.draw_params(0).shape) == (0,)
    for kw in (dict(sigma=-1.0), dict(sigma=(2.0, 1.0)), dict(sigma=(0.0, 8.5)), dict(sigma=(1.0,)), dict(sigma="1"), dict(sigma=None),
               dict(sigma=float("nan")), dict(sigma=(0.1, float("inf"))), dict(sigma=True), dict(p=-0.1), dict(p=1.5), dict(p="x"),
               dict(p=None), dict(p=float("nan"))):
        with pytest.raises(ValueError):
            mil_amd.GaussianBlurU8(**kw)
            pytest.fail(f"{kw} was accepted")
    for n in (-1, 1.5, None, True):
        with pytest.raises(ValueError):
            blur.draw_params(n)


def _bag(**kw):
    import mil_amd
    slide = torch.zeros((64, 80, 3), dtype=torch.uint8)
    return mil_amd.SlideBag(slide, roi_size=16, resolution=8, pad=2, coords=[[0, 0], [5, 7], [40, 60]], **kw)


def test_a_bag_without_blur_draws_the_stream_it_always_drew():
    """On CPU tensors `get_train_data` draws its parameters and is then refused by the device check: the state the generator is
    left in is that of the existing draw functions — with a blur, of those and ONE more draw, the last."""
    import mil_amd
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    aff = mil_amd.RandomAffine(30)
    el = mil_amd.ElasticDeform(1.0, cells=2)
    blur = mil_amd.GaussianBlurU8()

    def after(bag):
        g = torch.Generator().manual_seed(11)
        with pytest.raises(RuntimeError, match="GPU"):
            bag.get_train_data(generator=g)
        return g.get_state()

    def expected(with_blur):
        g = torch.Generator().manual_seed(11)
        prep = mil_amd.TilePreprocessor(16, 8, pad=2, device="cpu")
        prep.draw_params(3, g)
        jit.draw_params(3, g)
        aff.draw_params(3, 16, g)
        el.draw_params(3, 16, g)
        if with_blur:
            blur.draw_params(3, g)
        return g.get_state()

    old = after(_bag(color_jitter=jit, affine=aff, elastic=el))
    new = after(_bag(color_jitter=jit, affine=aff, elastic=el, blur=blur))
    assert torch.equal(old, expected(False)) and torch.equal(new, expected(True)) and not torch.equal(old, new)
    # injected sigmas draw nothing
    g = torch.Generator().manual_seed(11)
    with pytest.raises(RuntimeError, match="GPU"):
        _bag(color_jitter=jit, affine=aff, elastic=el, blur=blur).get_train_data(generator=g, blur_params=torch.zeros(3, dtype=torch.float64))
    assert torch.equal(g.get_state(), old)


def test_refusals_come_before_any_launch():
    import mil_amd
    from mil_amd import ops
    tiles = mil_amd.U8Tiles(torch.zeros((3, 3, 9, 12), dtype=torch.uint8))
    maps = torch.zeros((3, 9, 12), dtype=torch.uint8)
    blur = mil_amd.GaussianBlurU8()
    # a well-formed call on the CPU reaches the device check
    for call in (lambda: mil_amd.gaussian_blur_u8(tiles, 1.0), lambda: mil_amd.gaussian_blur_u8(maps, (1.0, 0.0)),
                 lambda: mil_amd.gaussian_blur_u8(maps, torch.tensor([0.0, 1.0, 8.0])),
                 lambda: mil_amd.gaussian_blur_u8(tiles, torch.ones(3, 2), out=mil_amd.U8Tiles(torch.zeros_like(tiles.u8))),
                 lambda: blur.apply(tiles, torch.zeros(3, dtype=torch.float64)), lambda: blur(tiles),
                 lambda: ops.gaussian_blur_u8(maps, ops.box_blur_params([1.0] * 3), 1)):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    for sigma in (-1.0, 8.5, float("nan"), "1", None, True, (1.0, 2.0, 3.0), (1.0, -2.0), torch.ones(4), torch.ones(3, 3), torch.ones(2, 2),
                  torch.tensor([1.0, 2.0, 9.0]), torch.tensor([1.0, float("inf"), 1.0])):
        with pytest.raises(ValueError, match="sigma"):
            mil_amd.gaussian_blur_u8(tiles, sigma)
    for x in (tiles.u8, tiles.u8.float(), maps.float(), torch.zeros(9, 12, dtype=torch.uint8), None, mil_amd.S2dTiles(torch.zeros(1, 4, 4, 16, dtype=torch.bfloat16))):
        with pytest.raises(ValueError, match="U8Tiles"):
            mil_amd.gaussian_blur_u8(x, 1.0)
    with pytest.raises(ValueError, match="out must"):
        mil_amd.gaussian_blur_u8(tiles, 1.0, out=torch.zeros_like(tiles.u8))
    with pytest.raises(ValueError, match="out must"):
        mil_amd.gaussian_blur_u8(maps, 1.0, out=torch.zeros(3, 9, 11, dtype=torch.uint8))
    with pytest.raises(ValueError, match="overlaps"):
        mil_amd.gaussian_blur_u8(maps, 1.0, out=maps)
    flat = torch.zeros(2 * maps.numel(), dtype=torch.uint8)
    a, b = flat[:maps.numel()].view(maps.shape), flat[maps.numel() - 1:2 * maps.numel() - 1].view(maps.shape)
    with pytest.raises(ValueError, match="overlaps"):
        mil_amd.gaussian_blur_u8(a, 1.0, out=b)
    for sig in (torch.zeros(2), torch.zeros(3, 3), 1.0, None, torch.tensor([0.0, 9.0, 0.0])):
        with pytest.raises(ValueError, match="sigma"):
            blur.apply(tiles, sig)
    for handle in (tiles.u8, maps, None):
        with pytest.raises(ValueError, match="U8Tiles"):
            blur.apply(handle, torch.zeros(3))
        with pytest.raises(ValueError, match="U8Tiles"):
            blur(handle)
    # ops: the parameter ranges the entry point leaves to its caller, and the shapes
    good = ops.box_blur_params([1.0] * 3)
    for row in ([8, 1, 0, 0, 1 << 24, 0], [-1, 1, 0, 0, 1 << 24, 0], [0, 1 << 24, 0, 0, 1 << 24, 1], [0, -1, 0, 0, 1, 0], [1, 1 << 23, 0, 0, 1, 0],
                [0, 1, 0, 7, 1 << 21, 0]):
        bad = good.clone()
        bad[1] = torch.tensor(row, dtype=torch.int32)
        with pytest.raises(ValueError, match="params"):
            ops.gaussian_blur_u8(maps, bad, 1)
    for bad in (good[:2], good[:, :5], good.float(), good.tolist(), None):
        with pytest.raises(ValueError, match="params"):
            ops.gaussian_blur_u8(maps, bad, 1)
    with pytest.raises(ValueError, match="multiple"):
        ops.gaussian_blur_u8(maps[:2], good[:1], 3)
    for ppi in (0, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="planes_per_item"):
            ops.gaussian_blur_u8(maps, good, ppi)
    for x in (maps.float(), torch.zeros(12, dtype=torch.uint8), None):
        with pytest.raises(ValueError, match="u8 must"):
            ops.gaussian_blur_u8(x, good, 1)
    with pytest.raises(ValueError, match="contiguous"):
        ops.gaussian_blur_u8(maps.transpose(1, 2), good, 1)
    with pytest.raises(ValueError, match="planes of"):
        ops.gaussian_blur_u8(torch.zeros(3, 0, 4, dtype=torch.uint8), good, 1)


def test_the_preprocessor_and_the_bag_refuse_before_any_launch():
    import mil_amd
    bag = _bag()
    slide, prep, coords = bag.slide, bag.prep, bag.coords
    sig = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    rois = torch.zeros((3, 16, 16, 3), dtype=torch.uint8)
    with pytest.raises(TypeError):                                               # keyword only
        prep.from_slide(slide, coords, None, "u8", None, None, None, 0, None, sig)
    for out in ("u8", "nchw"):
        with pytest.raises(RuntimeError, match="GPU"):                           # well formed: as far as the device check
            prep.from_slide(slide, coords, None, out, blur=sig)
        with pytest.raises(RuntimeError, match="GPU"):
            prep(rois, None, out, blur=sig)
    with pytest.raises(ValueError, match="resized bytes"):
        prep.from_slide(slide, coords, None, "s2d", blur=sig)
    with pytest.raises(ValueError, match="resized bytes"):
        prep(rois, None, "s2d", blur=sig)
    with pytest.raises(ValueError, match="out must"):
        prep.from_slide(slide, coords, None, "hwc", blur=sig)
    for bad in (sig[:2], torch.zeros(3, 3), torch.tensor([0.0, 9.0, 1.0]), torch.tensor([0.0, -1.0, 1.0]), 1.0, [0.0, 1.0, 2.0], "x"):
        with pytest.raises(ValueError, match="blur"):
            prep.from_slide(slide, coords, None, "u8", blur=bad)
        with pytest.raises(ValueError, match="blur"):
            prep(rois, None, "u8", blur=bad)
    # the bag: blur_params only where blur= was given; validation and inference data have no such argument
    with pytest.raises(ValueError, match="blur_params given to a bag made without blur="):
        bag.get_train_data(blur_params=sig)
    with pytest.raises(TypeError):
        bag.get_validation_data(blur_params=sig)
    blurred = _bag(blur=mil_amd.GaussianBlurU8())
    with pytest.raises(ValueError, match="blur"):
        blurred.get_train_data(blur_params=sig[:2])
    with pytest.raises(RuntimeError, match="GPU"):
        blurred.get_train_data(blur_params=sig)
    assert _bag().blur is None and blurred.blur is not None


def test_the_entry_point_is_declared_bound_and_returns_status_codes_without_a_gpu():
    import mil_amd
    from mil_amd import _lib
    header = open(os.path.join(ROOT, "include", "mil_hip.h")).read()
    assert ("int mil_gaussian_blur_u8(const uint8_t* in, uint8_t* out, const int32_t* params, int planes, int planes_per_item, int H, int W, "
            "void* stream);") in header
    assert "#define MIL_BLUR_U8_MAX_BOX 7" in header and "WHO CHECKS WHAT" in header
    assert "mil_gaussian_blur_u8" in _lib.EXPORTS
    src = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "Makefile")).read()
    assert " blur_u8.hip " in src
    f = mil_amd.lib().mil_gaussian_blur_u8
    vp = ctypes.c_void_p
    # six planes of 8x8 (384 bytes)
    x, out, p = vp(4096), vp(4096 + 384), vp(1 << 20)
    assert f(None, out, p, 6, 3, 8, 8, None) == 1
    assert f(x, None, p, 6, 3, 8, 8, None) == 1
    assert f(x, out, None, 6, 3, 8, 8, None) == 1
    assert f(x, x, p, 6, 3, 8, 8, None) == 1                                     # never in place
    assert f(x, vp(4096 + 383), p, 6, 3, 8, 8, None) == 1                        # the last byte of in
    assert f(vp(4096 + 383), x, p, 6, 3, 8, 8, None) == 1
    assert f(x, out, p, -1, 1, 8, 8, None) == 1
    assert f(x, out, p, -3, 3, 8, 8, None) == 1
    for ppi in (0, -1):
        assert f(x, out, p, 6, ppi, 8, 8, None) == 1, ppi
    assert f(x, out, p, 6, 4, 8, 8, None) == 1                                   # 6 % 4
    assert f(x, out, p, 2, 3, 8, 8, None) == 1
    assert f(x, out, p, 6, 3, 0, 8, None) == 1
    assert f(x, out, p, 6, 3, 8, 0, None) == 1
    assert f(x, out, p, 6, 3, -8, 8, None) == 1
    assert f(x, out, p, 0, 3, 0, 8, None) == 1                                   # ... also with nothing to do
    assert f(x, out, p, 0, 0, 8, 8, None) == 1
    assert f(x, out, p, 1, 1, 46341, 46341, None) == 2                           # a plane beyond 2^31 - 4097 bytes
    assert f(x, out, p, 3 << 29, 3, 64, 65, None) == 2                           # 2^31 workgroups and more
    # nothing to do: MIL_OK without a launch
    assert f(x, out, p, 0, 3, 8, 8, None) == 0
    assert f(x, out, p, 0, 1, 1, 1, None) == 0
    assert f(x, x, p, 0, 1, 300, 300, None) == 0                                 # no byte to overlap in
