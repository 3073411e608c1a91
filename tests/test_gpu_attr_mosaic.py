"""-m gpu: slide mosaics of per-tile attribution maps (`mil_attr_mosaic` through `ops.attr_mosaic`, `AttributionMosaic` and
`SlideBag.attribution_maps`).  Every comparison is equality with tests/attr_mosaic_reference.py, the numpy restatement of the
arithmetic include/mil_hip.h states.  The canvases handed to the lower calls are pre-filled with 0x5A (the tissue canvas: the
tissue thumbnail of tests/heatmap_reference.py on 0x5A), so a pixel the kernel should have written and did not, or wrote and
should not have, shows."""
import functools
import os

import numpy as np
import pytest
import torch

import attr_mosaic_reference as ref
import heatmap_reference as href
import mil_amd
from mil_amd import heatmap as hm
from mil_amd import ops

pytestmark = pytest.mark.gpu

H, W = 61, 53                                  # row pitch 159 bytes
FILL = 0x5A
# ((S, D), (Hm, Wm)): the issue's ratios, then one pair on each side of the switch between the two forms of the kernel, which
# is ceil(Hm/n) * ceil(Wm/n) >= 64: at n = 1 (8,8) = 64 against (9,7) = 63, at n = 4 (32,32) = 8*8 against (32,28) = 8*7
RATIOS = [((12, 3), (4, 4)), ((12, 3), (8, 8)), ((12, 3), (7, 5)), ((12, 3), (3, 9)), ((12, 3), (1, 1)), ((5, 1), (3, 3)),
          ((30, 15), (64, 48)), ((16, 16), (64, 64)),
          ((16, 16), (8, 8)), ((16, 16), (9, 7)), ((12, 3), (32, 32)), ((12, 3), (32, 28))]
WAVE_FORM = {((16, 16), (64, 64)), ((16, 16), (8, 8)), ((12, 3), (32, 32)), ((30, 15), (64, 48))}


def _takes_wave_form(n, hm, wm):
    return -(-hm // n) * -(-wm // n) >= 64


def test_the_cases_lie_on_both_sides_of_the_switch():
    assert {c for c in RATIOS if _takes_wave_form(c[0][0] // c[0][1], *c[1])} == WAVE_FORM
    assert not _takes_wave_form(1, 9, 7) and _takes_wave_form(1, 8, 8) and 9 * 7 == 63


@functools.lru_cache(maxsize=None)
def _slide():
    s = np.random.default_rng(3).integers(0, 256, (H, W, 3), dtype=np.uint8)
    s[:4, :4] = 255                                                # a saturated corner: the blend at the top of the range
    s.setflags(write=False)
    return s


def _coords(s):
    """The four corners, the last row and column next to a corner, and every column phase 0..15 that fits (two rows of them)."""
    cols = list(range(min(16, W - s + 1)))
    c = [(0, 0), (H - s, W - s), (H - s, 0), (0, W - s), (H - s, max(W - s - 1, 0))]
    c += [(3, col) for col in cols] + [((7 * col) % (H - s + 1), col) for col in cols]
    c = list(dict.fromkeys(c))
    assert all(r + s <= H and q + s <= W for r, q in c)
    return c


def _groups(coords, s, d):
    """Greedy split into calls whose windows own disjoint output blocks."""
    n, groups = s // d, []
    for r, q in coords:
        for g in groups:
            if all(abs(r // d - y // d) >= n or abs(q // d - x // d) >= n for y, x in g):
                g.append((r, q))
                break
        else:
            groups.append([(r, q)])
    return groups


def _maps(t, hm, wm, ch, seed):
    """Random bytes; window 0 all 255 (the rounding at the top of the range), window 1 — where there is one — a single 255 in a
    field of zeros (a wrong weight shows)."""
    shape = (t, hm, wm) if ch == 1 else (t, hm, wm, 3)
    m = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    m[0] = 255
    if t > 1:
        m[1] = 0
        m[1, hm // 2, (2 * wm) // 3] = 255
    return m


@functools.lru_cache(maxsize=None)
def _ratio_case(case, ch):
    """The groups of one case with their maps and the reference's resampled values, shared by the tests that use the case."""
    (s, d), (hm, wm) = case
    out = []
    for i, g in enumerate(_groups(_coords(s), s, d)):
        m = _maps(len(g), hm, wm, ch, 1000 * s + 10 * hm + wm + i)
        m.setflags(write=False)
        out.append((g, m, [ref.resample(x, s // d) for x in m]))
    assert sum(len(g) for g, _, _ in out) == len(_coords(s))
    return out


@functools.lru_cache(maxsize=None)
def _tissue(s, d, coords):
    """uint8 [H//d, W//d, 3]: the box mean of every window where it lies (tests/heatmap_reference.py), 0x5A elsewhere."""
    canvas = np.full((5, H // d, W // d, 3), FILL, np.uint8)
    t = href.render(canvas, _slide(), list(coords), s, d, np.full((4, len(coords)), -1), None, hm.JET105, hm.VIRIDIS256)[0]
    t.setflags(write=False)
    return t


def _random_table(seed=77):
    return np.random.default_rng(seed).integers(0, 256, (256, 3), dtype=np.uint8)


def _compare(got, want, what):
    got = got.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first (y,x,c)={bad[0].tolist()} got {got[tuple(bad[0])]} "
                             f"want {want[tuple(bad[0])]}")


def _check_group(r, s, d, g, m, values, heat=True, tissue=True):
    pos = [(y // d, x // d) for y, x in g]
    lut = r.table.numpy()
    tis = _tissue(s, d, tuple(g))
    want_heat = np.full((H // d, W // d, 3), FILL, np.uint8) if heat else None
    want_tis = tis.copy() if tissue else None
    ref.render(want_heat, want_tis, m, pos, s // d, lut, r.alpha_byte, r.alpha_by_value, values)
    dev_heat = torch.full((H // d, W // d, 3), FILL, dtype=torch.uint8, device="cuda") if heat else None
    dev_tis = torch.from_numpy(tis.copy()).cuda() if tissue else None
    got = r.render_into(dev_heat, dev_tis, g, torch.from_numpy(m.copy()).cuda())
    assert got[0] is dev_heat and got[1] is dev_tis
    what = f"S={s} D={d} maps={m.shape[1:]} coords={g[:3]}..."
    if heat:
        _compare(dev_heat, want_heat, what + " heat")
    if tissue:
        _compare(dev_tis, want_tis, what + " on_tissue")
    return want_heat, want_tis, tis


@pytest.mark.parametrize("colour", ["jet", "table", "rgb"])
@pytest.mark.parametrize("case", RATIOS, ids=lambda c: f"S{c[0][0]}D{c[0][1]}-{c[1][0]}x{c[1][1]}")
def test_ratios_through_render_into(case, colour):
    (s, d), _ = case
    cmap = torch.from_numpy(_random_table()) if colour == "table" else "jet"
    r = mil_amd.AttributionMosaic(s, d, cmap=cmap, alpha=0.4)
    assert r.alpha_byte == 102
    groups = _ratio_case(case, 3 if colour == "rgb" else 1)
    assert s > H // 2 or max(len(g) for g, _, _ in groups) > 1                # several windows per call where they fit
    seen = False
    for g, m, values in groups:
        want_heat, want_tis, tis = _check_group(r, s, d, g, m, values)
        seen = seen or ((want_heat != FILL).any() and (want_tis != tis).any())
    assert seen


@pytest.mark.parametrize("by_value", [False, True])
@pytest.mark.parametrize("alpha,byte", [(0.0, 0), (0.4, 102), (1.0, 255)])
def test_alpha_bytes_and_alpha_by_value(alpha, byte, by_value):
    for case in (((12, 3), (7, 5)), ((12, 3), (32, 32))):                       # one case of each form
        (s, d), _ = case
        r = mil_amd.AttributionMosaic(s, d, cmap=torch.from_numpy(_random_table(5)), alpha=alpha, alpha_by_value=by_value)
        assert r.alpha_byte == byte
        for g, m, values in _ratio_case(case, 1)[:2]:
            want_heat, want_tis, tis = _check_group(r, s, d, g, m, values)
            if byte == 0:
                assert np.array_equal(want_tis, tis)                            # the tissue keeps its bytes (the device equals want_tis)
        if not by_value:
            r3 = mil_amd.AttributionMosaic(s, d, alpha=alpha)
            for g, m, values in _ratio_case(case, 3)[:1]:
                _check_group(r3, s, d, g, m, values)


def test_alpha_zero_leaves_the_tissue_bytes_on_the_device():
    s, d = 12, 3
    g, m, _ = _ratio_case(((12, 3), (7, 5)), 1)[0]
    tis = _tissue(s, d, tuple(g))
    dev = torch.from_numpy(tis.copy()).cuda()
    heat = torch.full((H // d, W // d, 3), FILL, dtype=torch.uint8, device="cuda")
    for by_value in (False, True):
        mil_amd.AttributionMosaic(s, d, alpha=0.0, alpha_by_value=by_value).render_into(heat, dev, g, torch.from_numpy(m.copy()).cuda())
        assert np.array_equal(dev.cpu().numpy(), tis)
    assert bool((heat != FILL).any())


@pytest.mark.parametrize("case", [((12, 3), (7, 5)), ((16, 16), (64, 64))], ids=["thread", "wave"])
def test_null_outputs(case):
    (s, d), _ = case
    for ch in (1, 3):
        r = mil_amd.AttributionMosaic(s, d, alpha=0.4)
        g, m, values = _ratio_case(case, ch)[0]
        _check_group(r, s, d, g, m, values, heat=False)
        _check_group(r, s, d, g, m, values, tissue=False)


@pytest.mark.parametrize("hm,wm", [(4, 4), (7, 5), (32, 32)], ids=["identity", "fractional", "wave"])
def test_blocks_hanging_over_the_canvas_edges(hm, wm):
    """Through `ops.attr_mosaic`: blocks of n = 4 at (Ht-1, Wt-1), over the bottom edge, over the right edge and — a negative
    position — over the top-left corner; only the in-canvas part changes."""
    ht, wt, n = 9, 11, 4
    pos = [(ht - 1, wt - 1), (ht - 2, 2), (3, wt - 3), (-2, -1)]
    lut = _random_table(9)
    for ch in (1, 3):
        m = _maps(len(pos), hm, wm, ch, 50 + ch)
        tis = np.random.default_rng(51).integers(0, 256, (ht, wt, 3), dtype=np.uint8)
        want_heat, want_tis = np.full((ht, wt, 3), FILL, np.uint8), tis.copy()
        ref.render(want_heat, want_tis, m, pos, n, lut, 102, ch == 1)
        owned = np.zeros((ht, wt), dtype=bool)
        owned[ht - 1, wt - 1] = owned[ht - 2:, 2:6] = owned[3:7, wt - 3:] = owned[:2, :3] = True
        assert (want_heat[~owned] == FILL).all() and np.array_equal(want_tis[~owned], tis[~owned]) and owned.sum() == 1 + 8 + 12 + 6
        heat = torch.full((ht, wt, 3), FILL, dtype=torch.uint8, device="cuda")
        dev = torch.from_numpy(tis.copy()).cuda()
        out = ops.attr_mosaic(torch.from_numpy(m).cuda(), torch.tensor(pos, dtype=torch.int32, device="cuda"), n,
                              torch.from_numpy(lut).cuda() if ch == 1 else None, 102, ch == 1, heat, dev)
        assert out[0] is heat and out[1] is dev
        _compare(heat, want_heat, f"clipped heat {ch}")
        _compare(dev, want_tis, f"clipped on_tissue {ch}")


def test_two_calls_give_the_same_bytes_and_a_side_stream_works():
    for case in (((30, 15), (64, 48)), ((12, 3), (7, 5))):
        (s, d), _ = case
        r = mil_amd.AttributionMosaic(s, d, alpha=0.4, alpha_by_value=True)
        g, m, values = _ratio_case(case, 1)[0]
        dm = torch.from_numpy(m.copy()).cuda()
        tis = _tissue(s, d, tuple(g))
        outs = []
        for _ in range(2):
            heat = torch.full((H // d, W // d, 3), FILL, dtype=torch.uint8, device="cuda")
            dev = torch.from_numpy(tis.copy()).cuda()
            r.render_into(heat, dev, g, dm)
            outs.append((heat, dev))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
        side = torch.cuda.Stream()
        heat = torch.full((H // d, W // d, 3), FILL, dtype=torch.uint8, device="cuda")
        dev = torch.from_numpy(tis.copy()).cuda()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            r.render_into(heat, dev, g, dm)
        side.synchronize()
        assert torch.equal(heat, outs[0][0]) and torch.equal(dev, outs[0][1])
        want_heat, want_tis = np.full((H // d, W // d, 3), FILL, np.uint8), tis.copy()
        ref.render(want_heat, want_tis, m, [(y // d, x // d) for y, x in g], s // d, r.table.numpy(), 102, True, values)
        _compare(heat, want_heat, "side stream heat")
        _compare(dev, want_tis, "side stream on_tissue")


def test_more_windows_than_one_launch_and_none():
    """70 000 one-pixel windows with 1 x 1 maps (the identity): two launches; T = 0: the canvases come back untouched."""
    hh = ww = 300
    rng = np.random.default_rng(31)
    pick = np.concatenate([[0, hh * ww - 1], rng.permutation(np.arange(1, hh * ww - 1))[:69998]])
    pos = np.stack([pick // ww, pick % ww], axis=1)
    m = rng.integers(0, 256, (70000, 1, 1), dtype=np.uint8)
    lut = _random_table(32)
    want = np.full((hh, ww, 3), FILL, np.uint8)
    want[pos[:, 0], pos[:, 1]] = lut[m[:, 0, 0]]
    heat = torch.full((hh, ww, 3), FILL, dtype=torch.uint8, device="cuda")
    ops.attr_mosaic(torch.from_numpy(m).cuda(), torch.from_numpy(pos).to(torch.int32).cuda(), 1, torch.from_numpy(lut).cuda(), 102,
                    heat=heat)
    _compare(heat, want, "70000 windows")
    assert (want[pos[65535:, 0], pos[65535:, 1]] != FILL).any()
    r = mil_amd.AttributionMosaic(1, 1)
    heat.fill_(FILL)
    out = r.render_into(heat, None, np.zeros((0, 2), dtype=np.int64), torch.zeros((0, 1, 1), dtype=torch.uint8, device="cuda"))
    assert out[0] is heat and bool((heat == FILL).all())
    slide = torch.zeros((4, 4, 3), dtype=torch.uint8, device="cuda")
    assert bool((r.render(slide, [], torch.zeros((0, 2, 2), dtype=torch.uint8, device="cuda")) == 255).all())


def _expect_pixels(m, n, pixels):
    """{(a, b): value} of one one-channel map from the reference's weights, for a block too large to walk."""
    hm, wm = m.shape
    out = {}
    for a, b in pixels:
        wy, wx = ref.weights(a, hm, n), ref.weights(b, wm, n)
        ky, kx = np.nonzero(wy)[0], np.nonzero(wx)[0]
        total = int(wy[ky] @ m[np.ix_(ky, kx)].astype(np.int64) @ wx[kx])
        out[(a, b)] = (total + hm * wm // 2) // (hm * wm)
    return out


def test_sub_pixel_coordinates_beyond_32_bits():
    """n (max(Hm, Wm) + 1) >= 2^31 takes the 64-bit coordinates; the canvas shows the few pixels of the block around the border
    between the last two map pixels.  Thread form: a 4096 x 4096 map into a block of n = 2^20 + 3 (sub-pixel coordinates reach
    2^32); wave form: a 1 x 2^24 map into n = 129 columns of 130 055.8 map pixels each."""
    lut = _random_table(61)
    dlut = torch.from_numpy(lut).cuda()
    rng = np.random.default_rng(62)
    for (hm, wm), n, (ht, wt) in (((4096, 4096), (1 << 20) + 3, (8, 8)), ((1, 1 << 24), 129, (2, 4))):
        assert n * (max(hm, wm) + 1) >= 1 << 31
        owner = np.arange(wm, dtype=np.int64) * 8 // wm if hm > 1 else np.arange(wm, dtype=np.int64) * n // wm
        m = (rng.integers(0, 256, (hm, wm)) % (40 + 30 * (owner % 7))[None, :]).astype(np.uint8)
        # the first owned row / column shown: two before the pixel that straddles the last border, or row 0 of a one-row map
        a0 = (hm - 1) * n // hm - 2 if hm > 1 else 0
        b0 = (wm - 1) * n // wm - 2
        px = [(a, b) for a in range(a0, min(a0 + ht, n)) for b in range(b0, min(b0 + wt, n))]
        vals = _expect_pixels(m, n, px)
        want = np.full((ht, wt, 3), FILL, np.uint8)
        for (a, b), v in vals.items():
            want[a - a0, b - b0] = lut[v]
        assert len(set(vals.values())) > 1 and (hm > 1 or len(px) == 2 * 3)
        heat = torch.full((ht, wt, 3), FILL, dtype=torch.uint8, device="cuda")
        ops.attr_mosaic(torch.from_numpy(m).cuda().view(1, hm, wm), torch.tensor([(-a0, -b0)], dtype=torch.int32, device="cuda"), n, dlut,
                        102, heat=heat)
        _compare(heat, want, f"64-bit coordinates {hm}x{wm} n={n}")


def test_slide_bag_attribution_maps_end_to_end(golden_dir):
    """slide -> tiles of the flat chain -> saliency -> bytes -> mosaic: equals the reference applied to the downloaded map
    bytes and to the tissue thumbnail of tests/heatmap_reference.py."""
    host = np.random.default_rng(71).integers(0, 256, (110, 130, 3), dtype=np.uint8)
    coords = [(3, 5), (51, 7), (5, 60), (55, 70)]
    scale = 16
    bag = mil_amd.SlideBag(torch.from_numpy(host).cuda(), 48, resolution=32, coords=coords)
    bag.build()
    tiles, kept = bag.get_inference_data()
    assert kept.tolist() == [list(c) for c in coords] and tuple(tiles.shape) == (4, 3, 32, 32)
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    torch.manual_seed(20261020)
    net = mil_amd.Attention(3, compute_dtype=torch.bfloat16)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    net.eval()
    sal = mil_amd.TileSaliency(net).maps(tiles, 1)
    maps = mil_amd.AttributionRenderer(normalize="bag").grayscale(sal)
    assert maps.dtype == torch.uint8 and tuple(maps.shape) == (4, 32, 32) and int(maps.max()) == 255
    got = bag.attribution_maps(maps, scale, alpha=0.4)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 110 // scale, 130 // scale, 3) and got.is_cuda
    assert torch.equal(got, bag.attribution_maps(maps, scale, alpha=0.4))
    thumb = href.render(np.full((5, 6, 8, 3), 255, np.uint8), host, coords, 48, scale, np.full((4, 4), -1), None, hm.JET105,
                        hm.VIRIDIS256)[0]
    want_heat, want_tis = np.full((6, 8, 3), 255, np.uint8), thumb.copy()
    lut = mil_amd.attr_render.colour_table("jet").numpy()
    ref.render(want_heat, want_tis, maps.cpu().numpy(), [(r // scale, c // scale) for r, c in coords], 3, lut, 102)
    got = got.cpu().numpy()
    assert np.array_equal(got[0], want_heat) and np.array_equal(got[1], want_tis)
    owned = np.zeros((6, 8), dtype=bool)
    for r, c in coords:
        owned[r // scale:r // scale + 3, c // scale:c // scale + 3] = True
    assert owned.sum() == 36 and (got[:, ~owned] == 255).all()                     # white where no window lies
    assert (got[1] != thumb).any() and (got[0][owned] != 255).any()                # something was drawn, on both panels
    by_value = bag.attribution_maps(maps, scale, alpha=0.4, alpha_by_value=True, cmap="viridis").cpu().numpy()
    want_heat, want_tis = np.full((6, 8, 3), 255, np.uint8), thumb.copy()
    ref.render(want_heat, want_tis, maps.cpu().numpy(), [(r // scale, c // scale) for r, c in coords], 3,
               mil_amd.attr_render.colour_table("viridis").numpy(), 102, True)
    assert np.array_equal(by_value[0], want_heat) and np.array_equal(by_value[1], want_tis)
