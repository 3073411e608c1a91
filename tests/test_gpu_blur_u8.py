"""GPU (-m gpu): Pillow's Gaussian blur for uint8 tiles and maps (`mil_gaussian_blur_u8`).  Every comparison is
byte equality: against the numpy restatement tests/blur_u8_reference.py (held against Pillow in tests/test_cpu_blur_u8.py), against the
bytes Pillow wrote into tests/golden/gaussian_blur_u8.npz, and between the ways the package reaches the kernel."""
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import ops

import blur_u8_reference as ref

pytestmark = pytest.mark.gpu

FIVE = [0.0, 0.3, 8.0, (0.0, 4.0), (4.0, 0.0)]                 # identity, r = 0, r = 7, one axis off each way


def _image(rng, p, h, w):
    """Noise with a flat 0 and a flat 255 region and a ramp: saturation and borders that differ from what lies beside them."""
    x = rng.integers(0, 256, (p, h, w), dtype=np.uint8)
    x[:, : h // 3, : w // 2] = 0
    x[:, : h // 3, w // 2:] = 255
    x[:, h - max(h // 4, 1):] = np.linspace(0, 255, w).astype(np.uint8)
    return x


def _run(planes, sigmas, ppi):
    """(the kernel's bytes, the restatement's) for planes [P,H,W] with one sigma (or pair) per item."""
    params = ref.params_array(sigmas)
    sx = [s[0] if isinstance(s, tuple) else s for s in sigmas]
    sy = [s[1] if isinstance(s, tuple) else s for s in sigmas]
    mine = ops.box_blur_params(sx, sy)
    assert np.array_equal(mine.numpy(), params)
    got = ops.gaussian_blur_u8(torch.from_numpy(planes).cuda(), mine, ppi)
    return got.cpu().numpy(), ref.gaussian_blur_u8(planes, params, ppi)


def _diff(got, want):
    bad = np.argwhere(got != want)
    return [] if not len(bad) else [len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]]


@pytest.mark.parametrize("h,w,sigmas", [
    (1, 1, [8.0, 0.3]),                    # a plane narrower than the box: every tap is the one pixel
    (5, 3, [8.0, (8.0, 1.0)]),
    (3, 5, [8.0, 2.0]),
    (64, 64, [1.0, 8.0]),                  # exactly one block
    (65, 63, [1.4, 4.0, 8.0]),             # block seams, odd pitch, partial blocks
    (70, 67, [0.6, 2.0, 5.0, 8.0]),
    (300, 300, [2.0]),                     # the live tile size: five blocks a side, the last 44 wide
])
def test_planes_equal_the_restatement(h, w, sigmas):
    rng = np.random.default_rng(1000 * h + w)
    x = _image(rng, len(sigmas), h, w)
    got, want = _run(x, sigmas, 1)
    assert _diff(got, want) == []
    assert (got != x).any() or h * w == 1                                  # one pixel is its own blur


def test_three_planes_per_item_with_mixed_sigmas_and_the_same_stack_as_maps():
    """130 x 129: three blocks a side.  Items: the identity, r = 0, r = 7, and each axis switched off — mixed halos in one launch."""
    rng = np.random.default_rng(7)
    x = _image(rng, 15, 130, 129)
    got, want = _run(x, FIVE, 3)
    assert _diff(got, want) == []
    assert np.array_equal(got[:3], x[:3])                                   # the sigma-0 item is a bit copy
    assert all((got[3 * i:3 * i + 3] != x[3 * i:3 * i + 3]).any() for i in range(1, 5))
    # the same planes as fifteen maps, each with the sigma of the item it belonged to
    got1, want1 = _run(x, [s for s in FIVE for _ in range(3)], 1)
    assert _diff(got1, want1) == [] and np.array_equal(got1, got)
    # the public entry: U8Tiles equal the per-plane map call, and each returns the type it was given
    tiles = mil_amd.U8Tiles(torch.from_numpy(x.reshape(5, 3, 130, 129)).cuda())
    sig = torch.tensor([[s, s] if not isinstance(s, tuple) else list(s) for s in FIVE], dtype=torch.float64)
    a = mil_amd.gaussian_blur_u8(tiles, sig)
    b = mil_amd.gaussian_blur_u8(tiles.u8.reshape(15, 130, 129), sig.repeat_interleave(3, dim=0))
    assert isinstance(a, mil_amd.U8Tiles) and isinstance(b, torch.Tensor) and b.shape == (15, 130, 129)
    assert torch.equal(a.u8.reshape(15, 130, 129), b) and np.array_equal(b.cpu().numpy(), want)
    assert np.array_equal(tiles.u8.cpu().numpy().reshape(15, 130, 129), x)  # the input stack is not modified
    # a number and a pair for the whole stack; out= is filled and returned
    out = mil_amd.U8Tiles(torch.empty_like(tiles.u8))
    assert mil_amd.gaussian_blur_u8(tiles, (1.4, 0.6), out=out) is out
    assert np.array_equal(out.u8.cpu().numpy().reshape(15, 130, 129), ref.gaussian_blur_u8(x, ref.params_array([(1.4, 0.6)] * 5), 3))
    assert torch.equal(mil_amd.gaussian_blur_u8(tiles, 1.0).u8, mil_amd.gaussian_blur_u8(tiles, torch.ones(5)).u8)


def test_pillows_recorded_bytes(golden_dir):
    z = np.load(os.path.join(golden_dir, "gaussian_blur_u8.npz"))
    n = 0
    for name in ("rgb_70x67", "rgb_33x47", "l_64x64", "l_5x3"):
        img, sigmas, want = z[name + "_in"], z[name + "_sigmas"], z[name + "_out"]
        sig = torch.from_numpy(sigmas)
        k = len(sigmas)
        if img.ndim == 3:
            stack = np.ascontiguousarray(np.broadcast_to(img.transpose(2, 0, 1), (k,) + img.transpose(2, 0, 1).shape))
            got = mil_amd.gaussian_blur_u8(mil_amd.U8Tiles(torch.from_numpy(stack).cuda()), sig).u8.permute(0, 2, 3, 1)
        else:
            stack = np.ascontiguousarray(np.broadcast_to(img, (k,) + img.shape))
            got = mil_amd.gaussian_blur_u8(torch.from_numpy(stack).cuda(), sig)
        assert _diff(got.cpu().numpy(), want) == [], name
        n += k
    assert n == 10


def test_a_stack_of_more_than_two_gib():
    """2049 maps of 1024 x 1024: the last plane starts past byte 2^31 of both stacks.  Only the first and the last plane hold chosen
    bytes (the rest is whatever the allocation held) and only they are compared."""
    n, s = 2049, 1024
    rng = np.random.default_rng(11)
    first, last = _image(rng, 1, s, s), _image(rng, 1, s, s)
    x = torch.empty((n, s, s), dtype=torch.uint8, device="cuda")
    assert x.numel() > 2 ** 31
    x[0].copy_(torch.from_numpy(first[0]))
    x[n - 1].copy_(torch.from_numpy(last[0]))
    sig = torch.full((n,), 0.6, dtype=torch.float64)
    sig[n - 1] = 3.0
    got = mil_amd.gaussian_blur_u8(x, sig)
    assert _diff(got[0].cpu().numpy()[None], ref.gaussian_blur_u8(first, ref.params_array([0.6]), 1)) == []
    assert _diff(got[n - 1].cpu().numpy()[None], ref.gaussian_blur_u8(last, ref.params_array([3.0]), 1)) == []


def test_nothing_to_do_and_the_caller_owned_output():
    e = mil_amd.gaussian_blur_u8(mil_amd.U8Tiles(torch.empty((0, 3, 9, 9), dtype=torch.uint8, device="cuda")), 2.0)
    assert isinstance(e, mil_amd.U8Tiles) and tuple(e.shape) == (0, 3, 9, 9)
    m = mil_amd.gaussian_blur_u8(torch.empty((0, 9, 9), dtype=torch.uint8, device="cuda"), torch.zeros(0))
    assert tuple(m.shape) == (0, 9, 9)
    x = torch.from_numpy(_image(np.random.default_rng(3), 3, 40, 50)).cuda()
    keep = x.clone()
    with pytest.raises(ValueError, match="overlaps"):
        mil_amd.gaussian_blur_u8(x, 1.0, out=x)
    with pytest.raises(ValueError, match="radius|weights"):
        ops.gaussian_blur_u8(x, torch.tensor([[8, 1, 0, 0, 1 << 24, 0]] * 3, dtype=torch.int32), 1)
    with pytest.raises(ValueError, match="radius|weights"):
        ops.gaussian_blur_u8(x, torch.tensor([[0, 1 << 24, 1, 0, 1 << 24, 0]] * 3, dtype=torch.int32).cuda(), 1)
    assert torch.equal(x, keep)
    zero = mil_amd.gaussian_blur_u8(x, 0.0)
    assert zero.data_ptr() != x.data_ptr() and torch.equal(zero, x)             # sigma 0: a bit copy


def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], **kw)


def test_from_slide_with_blur_is_apply_on_the_call_without_it(golden_dir):
    z, dev, bag = _golden_bag(golden_dir)
    kept, prep = z["kept"], bag.prep
    n = len(kept)
    assert n == 4
    blur = mil_amd.GaussianBlurU8((0.5, 3.0), p=1.0)
    sig = torch.tensor([0.0, 0.7, 3.0, 8.0], dtype=torch.float64)
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    jp = jit.draw_params(n, torch.Generator().manual_seed(4))
    st = mil_amd.StainJitter(0.1, 0.05)
    stain = st.affine(st.draw_params(n, torch.Generator().manual_seed(5)), n)
    for kw in (dict(), dict(jitter=jp), dict(jitter=jp, stain=stain)):
        base = prep.from_slide(dev, kept, params, out="u8", **kw)
        want = blur.apply(base, sig)
        assert torch.equal(want.u8[0], base.u8[0]) and not torch.equal(want.u8[1:], base.u8[1:])
        got = prep.from_slide(dev, kept, params, out="u8", blur=sig, **kw)
        assert isinstance(got, mil_amd.U8Tiles) and torch.equal(got.u8, want.u8), sorted(kw)
        assert np.array_equal(got.u8.cpu().numpy().reshape(12, 32, 32),
                              ref.gaussian_blur_u8(base.u8.cpu().numpy().reshape(12, 32, 32), ref.params_array(sig.tolist()), 3))
        f = prep.from_slide(dev, kept, params, out="nchw", blur=sig, **kw)
        assert f.dtype == torch.float32 and torch.equal(f.view(torch.int32), want.float().view(torch.int32))
        a, b = prep.from_slide(dev, kept, params, out="u8", blur=None, **kw), base
        assert torch.equal(a.u8, b.u8)                                          # blur=None is the call made before
    # the stack entry point takes the keyword too
    rois = torch.stack([dev[r:r + 48, q:q + 48] for r, q in kept.tolist()])
    assert torch.equal(prep(rois, params, out="u8", jitter=jp, blur=sig).u8, blur.apply(prep(rois, params, out="u8", jitter=jp), sig).u8)
    with pytest.raises(ValueError, match="s2d|resized"):
        prep.from_slide(dev, kept, params, out="s2d", blur=sig)
    with pytest.raises(ValueError, match="blur"):
        prep.from_slide(dev, kept, params, out="u8", blur=sig[:3])
    e = prep.from_slide(dev, kept[:0], None, out="u8", blur=sig[:0])
    assert isinstance(e, mil_amd.U8Tiles) and tuple(e.shape) == (0, 3, 32, 32)


def test_slide_bag_with_blur(golden_dir):
    blur = mil_amd.GaussianBlurU8((0.5, 2.0), p=0.5)
    jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    z, dev, bag = _golden_bag(golden_dir, color_jitter=jit, blur=blur)
    _, _, plain = _golden_bag(golden_dir, color_jitter=jit)
    n = len(z["kept"])
    assert bag.build() and plain.build()
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    jp = jit.draw_params(n, torch.Generator().manual_seed(2))
    sig = torch.tensor([1.0, 0.0, 2.0, 0.5], dtype=torch.float64)
    train = bag.get_train_data(params=params, jitter_params=jp, blur_params=sig)
    base = plain.get_train_data(params=params, jitter_params=jp)
    assert torch.equal(train.u8, blur.apply(base, sig).u8) and not torch.equal(train.u8, base.u8)
    assert torch.equal(bag.get_validation_data().u8, plain.get_validation_data().u8)        # never blurred
    assert torch.equal(bag.get_inference_data()[0].u8, plain.get_inference_data()[0].u8)
    # drawn from the generator: the sigmas are the last draw, so the bag without blur= sees the stream it always saw
    g = torch.Generator().manual_seed(8)
    p0 = bag.prep.draw_params(n, g)
    j0 = jit.draw_params(n, g)
    s0 = blur.draw_params(n, g)
    drawn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    before = plain.get_train_data(generator=torch.Generator().manual_seed(8))
    assert torch.equal(before.u8, plain.get_train_data(params=p0, jitter_params=j0).u8)
    assert torch.equal(drawn.u8, blur.apply(before, s0).u8)
    with pytest.raises(ValueError, match="blur"):
        plain.get_train_data(params=params, blur_params=sig)
