"""-m gpu: the colour jitter on the device (mil_color_jitter_u8 through `ColorJitter.apply`, `TilePreprocessor(..., jitter=)` and
`SlideBag(color_jitter=)`; RoiBuilder.py:200).  Every comparison is equality of bytes (or of fp32 bits): against Pillow's
recorded bytes (tests/golden/jitter_chain.npz), against Pillow itself on all 2^24 colours where it is installed, and against the
numpy restatement tests/jitter_reference.py, which tests/test_cpu_color_jitter.py pins to Pillow."""
import itertools
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd.color_jitter import JitterParams

import jitter_reference as jr

pytestmark = pytest.mark.gpu

JIT = mil_amd.ColorJitter(brightness=0.2, contrast=0.1, saturation=0.05, hue=0.02)          # RoiBuilder.py:200
ORDERS = list(itertools.permutations(range(4)))


def _params(order, factors, shift):
    return JitterParams(torch.as_tensor(np.asarray(order), dtype=torch.int32), torch.as_tensor(np.asarray(factors), dtype=torch.float32),
                        torch.as_tensor(np.asarray(shift), dtype=torch.int32))


def _apply(tiles_np, order, factors, shift):
    """numpy uint8 [T,3,R,R] through ColorJitter.apply on the device, back as numpy."""
    h = mil_amd.U8Tiles(torch.from_numpy(np.ascontiguousarray(tiles_np)).cuda())
    out = JIT.apply(h, _params(order, factors, shift))
    assert out is h
    return h.u8.cpu().numpy()


def test_fixture_equals_pillows_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "jitter_chain.npz"))
    for g in ("19", "32", "2", "1"):
        got = _apply(z[f"in_{g}"], z[f"order_{g}"], z[f"factors_{g}"], z[f"shift_{g}"])
        bad = np.flatnonzero((got != z[f"out_{g}"]).any(axis=(1, 2, 3)))
        assert bad.size == 0, (g, bad.tolist(), z[f"order_{g}"][bad].tolist())


def _pillow_or_helper_cube():
    """(cube uint8 [4096,4096,3] with pixel v = (v & 255, (v >> 8) & 255, v >> 16), hue(shift) -> image, saturation(f) -> image),
    from Pillow itself where it imports, else from the restatement."""
    v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    cube = np.stack([v & 255, (v >> 8) & 255, v >> 16], axis=-1).astype(np.uint8)
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return cube, lambda s: np.concatenate([jr.hue(cube[y:y + 512], s) for y in range(0, 4096, 512)]), lambda f: jr.saturation(cube, f)
    img = Image.fromarray(cube, "RGB")
    hsv = np.asarray(img.convert("HSV"))

    def hue(shift):
        sh = hsv.copy()
        sh[..., 0] = ((hsv[..., 0].astype(np.int64) + shift) % 256).astype(np.uint8)
        return np.asarray(Image.frombytes("HSV", (4096, 4096), sh.tobytes()).convert("RGB"))

    return cube, hue, lambda f: np.asarray(ImageEnhance.Color(img).enhance(f))


def test_all_colours_hue_and_saturation():
    """The device's rounding, (non-)contraction and division against the host's, exhaustively: 16 tiles of 1024 x 1024 hold every
    colour once."""
    v = torch.arange(1 << 24, dtype=torch.int32, device="cuda").view(16, 1, 1024, 1024)
    tiles = torch.cat([v & 255, (v >> 8) & 255, v >> 16], dim=1).to(torch.uint8)
    cube, hue, saturation = _pillow_or_helper_cube()
    assert np.array_equal(tiles.permute(0, 2, 3, 1).reshape(4096, 4096, 3).cpu().numpy(), cube)
    ones, zeros = torch.ones((16, 3)), torch.zeros(16, dtype=torch.int32)

    def run(op, factor, shift):
        h = mil_amd.U8Tiles(tiles.clone())
        order = torch.tensor([[-1, op, -1, -1]] * 16, dtype=torch.int32)
        JIT.apply(h, JitterParams(order, ones * factor, zeros + shift))
        return h.u8.permute(0, 2, 3, 1).reshape(4096, 4096, 3).cpu().numpy()

    for shift in (0, 251):
        got, want = run(jr.HUE, 1.0, shift), hue(shift)
        assert int((got != want).any(axis=-1).sum()) == 0, shift
    for f in (0.95, 1.05):
        f = float(np.float32(f))
        got, want = run(jr.SATURATION, f, 0), saturation(f)
        assert int((got != want).any(axis=-1).sum()) == 0, f


@pytest.mark.parametrize("r,n", [(300, 3), (301, 2)])
def test_contrast_mean_across_workgroups(r, n):
    """Tiles of many workgroups (301 * 301 is odd: misaligned planes, a partial last group), contrast first, in the middle and
    last: the mean is taken of the tile as it is when contrast is reached; repeated, the bytes are the same."""
    rng = np.random.default_rng(r)
    tiles = rng.integers(0, 256, (n, 3, r, r), dtype=np.uint8)
    tiles[0] = tiles[0] // 3 + 90                                        # another mean than 127
    order = [(1, 0, 2, 3), (3, 0, 2, 1), (2, 1, 3, 0)][:n] if r == 300 else [(0, 3, 1, 2), (1, -1, 3, -1)]
    factors = np.array([(1.17, 0.93, 1.04), (0.83, 1.08, 0.96), (1.2, 0.9, 1.05)], np.float32)[:n]
    shift = [251, 4, 0][:n]
    want = jr.jitter_tiles(tiles, order, factors, shift)
    got = _apply(tiles, order, factors, shift)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=(1, 2, 3))).tolist()
    assert np.array_equal(_apply(tiles, order, factors, shift), got)
    assert jr.contrast_mean(np.moveaxis(tiles[0], 0, -1)) != jr.contrast_mean(np.moveaxis(tiles[1], 0, -1))


def test_more_tiles_than_one_launch_and_none():
    rng = np.random.default_rng(12)
    t, rows = 70000, 70
    tiles = rng.integers(0, 256, (t, 3, 2, 2), dtype=np.uint8)
    order = np.array([ORDERS[i % 24] for i in range(rows)], np.int32)
    order[24:48][order[24:48] == 2] = -1
    factors = np.stack([rng.uniform(0.8, 1.2, rows), rng.uniform(0.9, 1.1, rows), rng.uniform(0.95, 1.05, rows)], axis=1).astype(np.float32)
    shift = rng.integers(0, 256, rows).astype(np.int32)
    idx = np.arange(t) % rows
    got = _apply(tiles, order[idx], factors[idx], shift[idx])
    want = np.empty_like(tiles)
    for i in range(rows):
        want[i::rows] = jr.jitter_batch(tiles[i::rows], order[i], factors[i], shift[i])
    bad = np.flatnonzero((got != want).any(axis=(1, 2, 3)))
    assert bad.size == 0, (bad[:10].tolist(), bad.size)
    assert (got[65535:] != tiles[65535:]).any()                          # the second launch ran
    e = mil_amd.U8Tiles(torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda"))
    assert JIT.apply(e, JIT.draw_params(0)) is e and JIT(e) is e


def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], **kw)


def test_preprocessor_and_slide_bag_plumbing(golden_dir):
    z, dev, bag = _golden_bag(golden_dir, color_jitter=JIT)
    _, _, plain = _golden_bag(golden_dir)
    kept = z["kept"]
    n = len(kept)
    assert n == 4 and bag.build() and plain.build()
    prep = bag.prep
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    p = JIT.draw_params(n, torch.Generator().manual_seed(21))
    assert bool((p.order >= 0).all())
    base = prep.from_slide(dev, kept, params, out="u8")
    want = JIT.apply(mil_amd.U8Tiles(base.u8.clone()), p)
    assert not torch.equal(want.u8, base.u8)
    assert np.array_equal(want.u8.cpu().numpy(), jr.jitter_tiles(base.u8.cpu().numpy(), p.order.numpy(), p.factors.numpy(), p.hue_shift.numpy()))
    got = prep.from_slide(dev, kept, params, out="u8", jitter=p)
    assert isinstance(got, mil_amd.U8Tiles) and torch.equal(got.u8, want.u8)
    nchw = prep.from_slide(dev, kept, params, out="nchw", jitter=p)
    assert nchw.dtype == torch.float32 and torch.equal(nchw.view(torch.int32), want.float().view(torch.int32))
    # the stack entry takes the same argument
    stack = torch.stack([dev[r:r + 48, c:c + 48] for r, c in kept])
    assert torch.equal(prep(stack, params, out="u8", jitter=p).u8, want.u8)
    assert torch.equal(prep(stack, params, jitter=p).view(torch.int32), want.float().view(torch.int32))
    # jitter=None is today's call, bit for bit
    for out in ("u8", "nchw", "s2d"):
        a, b = prep.from_slide(dev, kept, params, out=out, jitter=None), prep.from_slide(dev, kept, params, out=out)
        bits = (lambda x: x.u8 if out == "u8" else x.xs.view(torch.int16) if out == "s2d" else x.view(torch.int32))
        assert torch.equal(bits(a), bits(b)), out
    # the bag: train data with injected parameters are jittered, validation and inference data never
    assert torch.equal(bag.get_train_data(params=params, jitter_params=p).u8, want.u8)
    assert torch.equal(bag.get_train_data(params=params, jitter_params=p, out="nchw").view(torch.int32), want.float().view(torch.int32))
    assert torch.equal(plain.get_train_data(params=params).u8, base.u8)
    assert torch.equal(bag.get_validation_data().u8, plain.get_validation_data().u8)
    assert torch.equal(bag.get_inference_data()[0].u8, plain.get_validation_data().u8)
    # drawn from the generator: the crop / flip parameters first, then the jitter's
    g = torch.Generator().manual_seed(8)
    pp = prep.draw_params(n, g)
    pj = JIT.draw_params(n, g)
    drawn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    assert torch.equal(drawn.u8, prep.from_slide(dev, kept, pp, out="u8", jitter=pj).u8)


def test_attention_forward_on_jittered_tiles():
    """The u8 feed's contract on jittered bytes: outputs are finite and those of the same bytes fed as the fp32 tensor."""
    rng = np.random.default_rng(31)
    tiles = mil_amd.U8Tiles(torch.from_numpy(rng.integers(0, 256, (8, 3, 64, 64), dtype=np.uint8)).cuda())
    before = tiles.u8.clone()
    JIT(tiles, torch.Generator().manual_seed(4))
    assert not torch.equal(tiles.u8, before)
    torch.manual_seed(0)
    net = mil_amd.Attention(3).eval()
    a, b = net(tiles, torch.tensor([1])), net(tiles.float(), torch.tensor([1]))
    assert set(a) == set(b) and len(a) > 3
    for k in a:
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
