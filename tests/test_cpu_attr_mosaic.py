"""CPU (-m "not gpu"): slide mosaics of attribution maps (mil_amd.attr_mosaic, `mil_attr_mosaic`) — the numpy reference
(tests/attr_mosaic_reference.py) against an independent brute force in exact fractions and against its closed forms, every
status code of the C entry and every refusal of the host layer, all of which fire before a launch."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import attr_mosaic_reference as ref
import mil_amd
from mil_amd import _lib


def _brute(m, n):
    """The area average by its definition: output pixel (a, b) covers [a Hm/n, (a+1) Hm/n) x [b Wm/n, (b+1) Wm/n) of the map in
    map pixels; the mean is the integral of the piecewise constant map over it divided by its area, rounded half up."""
    m = np.asarray(m)
    hm, wm = m.shape[:2]
    m = m.reshape(hm, wm, -1)
    out = np.zeros((n, n, m.shape[2]), dtype=np.int64)
    for a in range(n):
        y0, y1 = Fraction(a * hm, n), Fraction((a + 1) * hm, n)
        for b in range(n):
            x0, x1 = Fraction(b * wm, n), Fraction((b + 1) * wm, n)
            for c in range(m.shape[2]):
                acc = Fraction(0)
                for k in range(hm):
                    ly = min(y1, Fraction(k + 1)) - max(y0, Fraction(k))
                    if ly <= 0:
                        continue
                    for l in range(wm):
                        lx = min(x1, Fraction(l + 1)) - max(x0, Fraction(l))
                        if lx > 0:
                            acc += ly * lx * int(m[k, l, c])
                mean = acc / ((y1 - y0) * (x1 - x0))
                out[a, b, c] = (mean + Fraction(1, 2)).__floor__()
    return out


@pytest.mark.parametrize("hm,wm,n,ch", [(4, 4, 4, 1), (8, 8, 4, 1), (7, 5, 4, 1), (3, 9, 4, 3), (1, 1, 4, 1), (3, 3, 5, 3), (5, 7, 1, 1),
                                        (2, 3, 7, 1)])
def test_reference_equals_the_exact_area_average(hm, wm, n, ch):
    rng = np.random.default_rng(100 * hm + 10 * wm + n)
    m = rng.integers(0, 256, (hm, wm) if ch == 1 else (hm, wm, ch), dtype=np.uint8)
    m.flat[0] = 255
    got = ref.resample(m, n)
    assert got.shape == ((n, n) if ch == 1 else (n, n, ch))
    assert np.array_equal(got.reshape(n, n, -1), _brute(m, n))
    assert np.array_equal(ref.resample(np.full_like(m, 255), n), np.full(got.shape, 255))


def test_reference_weights_sum_and_single_pixel():
    for size, n in ((7, 4), (256, 75), (3, 5), (64, 1), (1, 9)):
        w = np.stack([ref.weights(i, size, n) for i in range(n)])
        assert (w.sum(axis=1) == size).all() and (w.sum(axis=0) == n).all() and w.min() >= 0
    # one bright pixel: its 255 spreads with the weights, 7 x 5 -> 4 x 4
    m = np.zeros((7, 5), dtype=np.uint8)
    m[3, 2] = 255
    got = ref.resample(m, 4)
    wy = np.array([ref.weights(a, 7, 4)[3] for a in range(4)])
    wx = np.array([ref.weights(b, 5, 4)[2] for b in range(4)])
    want = (np.outer(wy, wx) * 255 + 17) // 35
    assert np.array_equal(got, want) and got.max() > 0


def test_reference_closed_forms():
    rng = np.random.default_rng(5)
    m = rng.integers(0, 256, (6, 6, 3), dtype=np.uint8)
    assert np.array_equal(ref.resample(m, 6), m)                                         # Hm == n: the identity
    g = rng.integers(0, 256, (5, 5), dtype=np.uint8)
    assert np.array_equal(ref.resample(g, 10), np.kron(g, np.ones((2, 2), dtype=np.int64)))   # n = 2 Hm: replication
    # Hm = k n: the k x k box mean with mil_heatmap_render's rounding
    b = rng.integers(0, 256, (12, 12), dtype=np.uint8)
    box = (b.astype(np.int64).reshape(4, 3, 4, 3).sum(axis=(1, 3)) + 4) // 9
    assert np.array_equal(ref.resample(b, 4), box)


@pytest.mark.parametrize("factor", [2, 4])
def test_reference_equals_pillow_reduce(factor):
    """Image.reduce by 2 and 4 (shifts; factors 3, 5 and 7 multiply by a rounded reciprocal and are not compared)."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(40 + factor)
    for i in range(6):
        n = int(rng.integers(1, 6))
        g = rng.integers(0, 256, (n * factor, n * factor), dtype=np.uint8)
        if i == 0:
            g[:] = 255
        want = np.asarray(Image.fromarray(g).reduce(factor))
        assert np.array_equal(ref.resample(g, n), want)
    rgb = rng.integers(0, 256, (3 * factor, 3 * factor, 3), dtype=np.uint8)
    assert np.array_equal(ref.resample(rgb, 3), np.asarray(Image.fromarray(rgb).reduce(factor)))


def test_reference_composite_and_clipping():
    d = np.arange(256, dtype=np.int64)
    assert np.array_equal(ref.composite(np.full(256, 200), d, 0), d)                     # alpha 0 keeps the tissue
    assert np.array_equal(ref.composite(d, np.full(256, 17), 255), d)                    # alpha 255 replaces it
    assert ref.composite(255, 255, 102) == 255 and ref.composite(0, 0, 102) == 0
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(8)
    src, dst = rng.integers(0, 256, (9, 11, 3), dtype=np.uint8), rng.integers(0, 256, (9, 11, 3), dtype=np.uint8)
    top = np.dstack([src, np.full((9, 11, 1), 102, dtype=np.uint8)])
    want = np.asarray(Image.alpha_composite(Image.fromarray(dst).convert("RGBA"), Image.fromarray(top, "RGBA")))[:, :, :3]
    assert np.array_equal(ref.composite(src.astype(np.int64), dst.astype(np.int64), 102), want)
    # blocks that hang over the edges: only the in-canvas part changes, by_value scales the alpha
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    maps = rng.integers(0, 256, (2, 4, 4), dtype=np.uint8)
    heat, tissue = np.full((5, 6, 3), 0x5A, np.uint8), np.full((5, 6, 3), 0x5A, np.uint8)
    ref.render(heat, tissue, maps, [(4, 5), (-2, -3)], 4, lut, 102, True)
    assert np.array_equal(heat[4, 5], lut[maps[0, 0, 0]]) and np.array_equal(heat[0:2, 0], lut[maps[1, 2:4, 3]])
    untouched = np.ones((5, 6), dtype=bool)
    untouched[4, 5] = untouched[0:2, 0] = False
    assert (heat[untouched] == 0x5A).all() and (tissue[untouched] == 0x5A).all()
    a = (102 * int(maps[0, 0, 0]) + 127) // 255
    assert np.array_equal(tissue[4, 5], ref.composite(lut[maps[0, 0, 0]].astype(np.int64), np.int64(0x5A), a))


def test_symbol_is_bound():
    assert "mil_attr_mosaic" in _lib.EXPORTS
    assert mil_amd.lib().mil_abi_version() == 2
    assert "AttributionMosaic" in mil_amd.__all__ and mil_amd.AttributionMosaic is not None


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = mil_amd.lib()
    assert lib.mil_attr_mosaic(None, 1, 0, 4, 4, 4, None, None, 102, 0, None, None, 4, 4, None) == 1
    buf = np.zeros(4096, dtype=np.uint8)
    one = buf.ctypes.data                                                            # any non-null address: nothing is read

    def call(maps=one, ch=1, T=0, hm=4, wm=4, n=4, pos=one, lut=one, alpha=102, by_value=0, heat=one, tissue=one, ht=4, wt=4):
        return lib.mil_attr_mosaic(maps, ch, T, hm, wm, n, pos, lut, alpha, by_value, heat, tissue, ht, wt, None)
    assert call() == 0                                                               # T == 0: MIL_OK, no launch
    assert call(ch=3, lut=None) == 0 and call(heat=None) == 0 and call(tissue=None) == 0 and call(by_value=1) == 0
    assert call(alpha=0) == 0 and call(alpha=255) == 0
    assert call(maps=None) == 1 and call(pos=None) == 1 and call(heat=None, tissue=None) == 1 and call(lut=None) == 1
    assert call(ch=0) == 1 and call(ch=2) == 1 and call(ch=4) == 1
    assert call(alpha=-1) == 1 and call(alpha=256) == 1
    assert call(by_value=2) == 1 and call(by_value=-1) == 1 and call(ch=3, by_value=1) == 1
    assert call(T=-1) == 1 and call(hm=0) == 1 and call(wm=0) == 1 and call(n=0) == 1 and call(ht=0) == 1 and call(wt=0) == 1
    assert call(hm=4096, wm=4097) == 2 and call(hm=1, wm=(1 << 24) + 1) == 2         # 32-bit sums stop at Hm Wm = 2^24
    assert call(hm=4096, wm=4096) == 0 and call(hm=1 << 24, wm=1) == 0
    assert call(hm=4096, wm=4097, alpha=256) == 1                                    # an argument error comes first
    assert call(n=(1 << 31) - 1) == 0


def test_host_layer_refuses_before_the_device_check():
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8)
    ok = [(0, 0), (48, 64)]
    maps = torch.zeros((2, 8, 8), dtype=torch.uint8)
    r = mil_amd.AttributionMosaic(48, 16)
    assert (r.alpha_byte, r.alpha_by_value, r.roi_size, r.scale) == (127, False, 48, 16)
    assert mil_amd.AttributionMosaic(48, 16, alpha=0.4).alpha_byte == 102
    assert torch.equal(r.table, mil_amd.attr_render.colour_table("jet"))
    with pytest.raises(ValueError, match="AttributionRenderer.grayscale"):
        r.render(slide, ok, maps.float())                                              # a float map
    with pytest.raises(ValueError, match="AttributionRenderer.grayscale"):
        r.render(slide, ok, maps.to(torch.int32))
    with pytest.raises(ValueError, match="AttributionRenderer.grayscale"):
        r.render(slide, ok, maps.numpy())
    for bad in (torch.zeros((2, 8), dtype=torch.uint8), torch.zeros((2, 8, 8, 4), dtype=torch.uint8),
                torch.zeros((2, 3, 8, 8), dtype=torch.uint8), torch.zeros((2, 0, 8), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="Hm,Wm"):
            r.render(slide, ok, bad)
    with pytest.raises(ValueError, match="contiguous"):
        r.render(slide, ok, torch.zeros((2, 8, 16), dtype=torch.uint8)[:, :, ::2])
    with pytest.raises(ValueError, match="3 maps for 2 windows"):
        r.render(slide, ok, torch.zeros((3, 8, 8), dtype=torch.uint8))
    with pytest.raises(ValueError, match="divide"):
        mil_amd.AttributionMosaic(48, 5).render(slide, ok, maps)
    for bad in ([(53, 0), (0, 0)], [(0, 73), (0, 0)], [(-1, 0), (0, 0)]):               # a window leaves the slide
        with pytest.raises(ValueError, match="inside"):
            r.render(slide, bad, maps)
    for bad in ([(0, 0), (47, 47)], [(0, 0), (0, 0)], [(16, 16), (0, 63)]):             # overlapping windows
        with pytest.raises(ValueError, match="own the same"):
            r.render(slide, bad, maps)
    with pytest.raises(ValueError):
        r.render(slide.float(), ok, maps)
    with pytest.raises(ValueError):
        r.render(slide, [(0.5, 0.0), (48.0, 64.0)], maps)
    with pytest.raises(ValueError, match="one-channel"):
        mil_amd.AttributionMosaic(48, 16, alpha_by_value=True).render(slide, ok, torch.zeros((2, 8, 8, 3), dtype=torch.uint8))
    for kw in ({"alpha": 1.5}, {"alpha": -0.1}, {"cmap": "nope"}, {"cmap": torch.zeros((256, 4), dtype=torch.uint8)},
               {"cmap": torch.zeros((256, 3))}, {"scale": 0}, {"roi_size": 0}):
        with pytest.raises(ValueError):
            mil_amd.AttributionMosaic(**{"roi_size": 48, "scale": 16, **kw})
    # valid arguments on a CPU slide: the package's usual refusal, after all of the above
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render(slide, ok, maps)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render(slide, ok, torch.zeros((2, 8, 8, 3), dtype=torch.uint8))


def test_render_into_refuses_before_the_device_check():
    r = mil_amd.AttributionMosaic(48, 16)
    ok = [(0, 0), (48, 64)]
    maps = torch.zeros((2, 8, 8), dtype=torch.uint8)
    canvas = torch.zeros((6, 7, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="nothing to draw on"):
        r.render_into(None, None, ok, maps)
    with pytest.raises(ValueError, match="AttributionRenderer.grayscale"):
        r.render_into(canvas, None, ok, maps.float())
    for bad in (torch.zeros((6, 7, 4), dtype=torch.uint8), torch.zeros((6, 7, 3)), torch.zeros((6, 14, 3), dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError, match="canvases"):
            r.render_into(bad, None, ok, maps)
        with pytest.raises(ValueError, match="canvases"):
            r.render_into(None, bad, ok, maps)
    with pytest.raises(ValueError, match="canvases"):
        r.render_into(canvas, torch.zeros((6, 8, 3), dtype=torch.uint8), ok, maps)
    with pytest.raises(ValueError, match="inside"):
        r.render_into(canvas, None, [(0, 0), (64, 64)], maps)                          # rows 4..6 of a 6-row canvas
    with pytest.raises(ValueError, match="inside"):
        r.render_into(canvas, None, [(0, 0), (-16, 64)], maps)
    with pytest.raises(ValueError, match="own the same"):
        r.render_into(canvas, canvas.clone(), [(0, 0), (47, 47)], maps)
    with pytest.raises(ValueError, match="divide"):
        mil_amd.AttributionMosaic(48, 5).render_into(canvas, None, ok, maps)
    with pytest.raises(ValueError, match="2 maps for 1 windows"):
        r.render_into(canvas, None, [(0, 0)], maps)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render_into(canvas, canvas.clone(), ok, maps)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render_into(None, canvas, ok, maps)


def test_ops_wrapper_refuses_bad_arguments():
    from mil_amd import ops
    maps = torch.zeros((2, 8, 8), dtype=torch.uint8)
    pos = torch.zeros((2, 2), dtype=torch.int32)
    lut = torch.zeros((256, 3), dtype=torch.uint8)
    canvas = torch.zeros((6, 7, 3), dtype=torch.uint8)
    for args in ((maps.float(), pos, 3, lut, 102), (maps, pos, 0, lut, 102), (maps, pos, 3, lut, 256), (maps, pos, 3, lut, 1.5),
                 (maps, pos, 3, None, 102), (maps, None, 3, lut, 102)):
        with pytest.raises(ValueError):
            ops.attr_mosaic(*args, heat=canvas)
    with pytest.raises(ValueError, match="nothing to draw on"):
        ops.attr_mosaic(maps, pos, 3, lut, 102)
    with pytest.raises(ValueError, match="one-channel"):
        ops.attr_mosaic(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), pos, 3, None, 102, True, heat=canvas)
    with pytest.raises(ValueError, match="CUDA"):                                    # CPU tensors: no fallback
        ops.attr_mosaic(maps, pos, 3, lut, 102, heat=canvas)


def test_slide_bag_attribution_maps_needs_build_and_checks_maps():
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8)
    bag = mil_amd.SlideBag(slide, 48, 7, resolution=32)
    with pytest.raises(RuntimeError, match="build"):
        bag.attribution_maps(torch.zeros((2, 8, 8), dtype=torch.uint8), 16)
    bag = mil_amd.SlideBag(slide, 48, coords=[(0, 0), (48, 64)])
    with pytest.raises(ValueError, match="AttributionRenderer.grayscale"):
        bag.attribution_maps(torch.zeros((2, 8, 8)), 16)
    with pytest.raises(ValueError, match="1 maps for 2 windows"):
        bag.attribution_maps(torch.zeros((1, 8, 8), dtype=torch.uint8), 16)
    with pytest.raises(ValueError, match="divide"):
        bag.attribution_maps(torch.zeros((2, 8, 8), dtype=torch.uint8), 5)
    with pytest.raises(ValueError, match="own the same"):
        mil_amd.SlideBag(slide, 48, coords=[(0, 0), (40, 40)]).attribution_maps(torch.zeros((2, 8, 8), dtype=torch.uint8), 16)
    with pytest.raises(ValueError):
        bag.attribution_maps(torch.zeros((2, 8, 8), dtype=torch.uint8), 16, alpha=2.0)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        bag.attribution_maps(torch.zeros((2, 8, 8), dtype=torch.uint8), 16, cmap="viridis", alpha_by_value=True)
