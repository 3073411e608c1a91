"""-m gpu: stain normalisation and stain jitter on the device (mil_stain_affine_u8, mil_od_moments_u8, mil_od_project_u8 through
`mil_amd.ops`, `StainNormalizer`, `StainJitter`, `TilePreprocessor(..., stain=)` and `SlideBag(stain_normalizer=, stain_jitter=)`).
Bytes and fp32 maps are compared for equality with the numpy restatement tests/stain_reference.py (which tests/test_cpu_stain.py
holds to the fp64 formulas); the fp64 moments to `math.fsum` within the first-order bound of their summation tree."""
import math
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import ops
from mil_amd import stain as st

import stain_reference as sr

pytestmark = pytest.mark.gpu

# (3,3,5,7): 35-byte planes start at odd addresses, every access goes by bytes; (5,3,33,31): 1023-byte planes, dword and byte
# accesses mixed, a partial last group; (4,3,64,64): one full workgroup of 4096 pixels; (2,3,300,300): 22 workgroups per tile
SHAPES = [(3, 3, 5, 7), (2, 3, 16, 12), (5, 3, 33, 31), (4, 3, 64, 64), (2, 3, 300, 300)]
GUARD = 64
_cache = {}


def _tiles(shape):
    """The stack of a shape (H&E-like bytes; in the larger stacks every byte value is present), made once and left unchanged."""
    if shape not in _cache:
        tiles, _ = sr.synthetic_tiles(shape, seed=shape[2])
        flat = tiles.reshape(-1)
        if flat.size >= 1 << 14:
            flat[np.arange(256) * (flat.size // 256)] = np.arange(256, dtype=np.uint8)
        tiles.setflags(write=False)
        _cache[shape] = tiles
    return _cache[shape]


def _on_device(tiles_np, offset=GUARD):
    """(the stack as a view `offset` bytes into a larger allocation filled with a pattern, the allocation, the pattern)."""
    n = tiles_np.size
    pattern = (np.arange(n + offset + GUARD) * 37 + 11).astype(np.uint8)
    buf = torch.from_numpy(pattern.copy()).cuda()
    view = buf[offset:offset + n].view(tiles_np.shape)
    view.copy_(torch.from_numpy(np.array(tiles_np)))
    return view, buf, pattern


def _guards_untouched(buf, pattern, offset, n):
    got = buf.cpu().numpy()
    return np.array_equal(got[:offset], pattern[:offset]) and np.array_equal(got[offset + n:], pattern[offset + n:])


def _affine(tiles_np, params, offset=GUARD):
    view, buf, pattern = _on_device(tiles_np, offset)
    out = ops.stain_affine(view, torch.as_tensor(params, dtype=torch.float32))
    assert out is view
    assert _guards_untouched(buf, pattern, offset, tiles_np.size), "bytes around the stack were written"
    return view.cpu().numpy()


def _jitter_params(n, seed):
    jit = st.StainJitter(0.2, 0.1)
    return jit.affine(jit.draw_params(n, torch.Generator().manual_seed(seed))).params().numpy()


# ---- stain_affine: bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_stain_affine_equals_the_restatement(shape):
    tiles = _tiles(shape)
    t = shape[0]
    per_tile, shared = _jitter_params(t, 1), _jitter_params(1, 2)
    for params in (per_tile, shared):
        want = sr.stain_affine(tiles, params)
        got = _affine(tiles, params)
        assert np.array_equal(got, want), int((got != want).sum())
        assert not np.array_equal(got, tiles)
    ident = st.StainAffine.identity().params().numpy()
    assert np.array_equal(_affine(tiles, ident), tiles)
    assert np.array_equal(_affine(tiles, np.repeat(ident, t, axis=0)), tiles)
    # saturation to 255 and to 0 (and both inside one map), a NaN OD (inf - inf) to 0
    sat = np.zeros((1, 12), dtype=np.float32)
    sat[0, [3, 7, 11]] = (-1.0, 9.0, 0.5)
    got = _affine(tiles, sat)
    assert (got[:, 0] == 255).all() and (got[:, 1] == 0).all() and np.array_equal(got, sr.stain_affine(tiles, sat))
    steep = np.zeros((1, 12), dtype=np.float32)
    steep[0, [0, 5, 10]] = 40.0
    steep[0, [3, 7, 11]] = -20.0
    got = _affine(tiles, steep)
    assert np.array_equal(got, sr.stain_affine(tiles, steep)) and (got == 0).any() and (got == 255).any()
    big = np.zeros((1, 12), dtype=np.float32)
    big[0, [0, 1]] = (3e38, -3e38)
    assert np.array_equal(_affine(tiles, big), sr.stain_affine(tiles, big))


@pytest.mark.parametrize("shape", SHAPES[:3])
def test_stain_affine_exact_ties_go_to_the_brighter_byte(shape):
    """A = 0, b = TH[k]: o == TH[k] exactly, the byte is k; one ulp above it, k - 1.  Per tile another k, all 255 of them."""
    tiles = _tiles(shape)
    t = shape[0]
    for first in range(1, 256, t):
        ks = np.array([min(first + i, 255) for i in range(t)])
        tie = np.zeros((t, 12), dtype=np.float32)
        tie[:, 3], tie[:, 7] = sr.TH[ks], np.nextafter(sr.TH[ks], np.float32(np.inf))
        tie[:, 11] = np.nextafter(sr.TH[ks], np.float32(-np.inf))
        got = _affine(tiles, tie)
        for i, k in enumerate(ks):
            assert (got[i, 0] == k).all() and (got[i, 1] == k - 1).all() and (got[i, 2] == k).all(), k


def test_stain_affine_no_tiles_and_a_stack_at_byte_offset_one():
    e = torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda")
    assert ops.stain_affine(e, torch.zeros((1, 12))) is e
    h = mil_amd.U8Tiles(e)
    assert st.StainJitter()(h) is h
    for shape in SHAPES[:4]:
        tiles = _tiles(shape)
        params = _jitter_params(shape[0], 3)
        want = sr.stain_affine(tiles, params)
        for offset in (1, 2, 3):
            assert np.array_equal(_affine(tiles, params, offset=offset), want), (shape, offset)


# ---- od_moments ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_od_moments_within_the_bound_of_the_tree_and_repeatable(shape):
    """Every term (1, od_c, od_c od_d) is exact in fp64 and non-negative, and a pixel that is not tissue adds exact zeros, so a
    group's sum is a sum of its n tissue terms in SOME order: a thread adds its four-pixel groups in order, 64 lanes meet in a
    6-level butterfly, 4 waves in order, then 16 slices in order (bag 0) or the stack's slice sums by thread, butterfly and
    waves again (bag 1).  Each rounded addition errs by at most 2^-53 of its result, every partial result is at most the sum S of
    all terms, and adding a zero is exact, so at most n - 1 additions err: |got - exact| <= (n - 1) 2^-53 S (1 + O(2^-53)),
    which n 2^-52 S covers with a factor of two to spare.  `math.fsum` is the exact sum, correctly rounded (2^-53 S more)."""
    tiles = _tiles(shape)
    view, buf, pattern = _on_device(tiles, offset=1)
    for bag in (0, 1):
        got = ops.od_moments(view, 0.15, "bag" if bag else "tile")
        again = ops.od_moments(view, 0.15, "bag" if bag else "tile")
        assert got.dtype == torch.float64 and tuple(got.shape) == (1 if bag else shape[0], 10)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))
        got = got.cpu().numpy()
        groups = [tiles] if bag else [tiles[i:i + 1] for i in range(shape[0])]
        for g, row in zip(groups, got):
            terms = sr.od_moment_terms(g, 0.15)
            n = terms[0].size
            assert row[0] == n
            for k in range(1, 10):
                exact = math.fsum(terms[k])
                bound = n * 2.0 ** -52 * exact
                assert abs(row[k] - exact) <= bound, (bag, k, row[k], exact, bound)
    assert _guards_untouched(buf, pattern, 1, tiles.size)


def test_od_moments_of_a_stack_without_tissue_are_zero():
    blank = torch.full((3, 3, 33, 31), 250, dtype=torch.uint8, device="cuda")           # OD 0.02 < beta
    blank[:, 1] = 3                                                                      # one dark channel is not tissue
    for group in ("tile", "bag"):
        got = ops.od_moments(blank, 0.15, group)
        assert bool((got == 0).all()) and not bool(torch.signbit(got).any())
    assert float(ops.od_moments(blank, 0.0, "bag")[0, 0]) == 3 * 33 * 31                 # beta 0: every pixel


# ---- od_project ----------------------------------------------------------------------------------------------------------------------
PLANES = [np.array([[0.56, 0.72, 0.41], [0.62, -0.08, -0.78]]),                          # a Macenko-like plane: p_0 > 0
          np.array([[1.0, -0.8, 0.1], [0.3, 0.5, -0.2]])]                                 # p_0 <= 0 on many tissue pixels


@pytest.mark.parametrize("shape", SHAPES)
def test_od_project_equals_the_restatement(shape):
    tiles = _tiles(shape)
    view, buf, pattern = _on_device(tiles, offset=3)
    dropped = 0
    for P in PLANES:
        for mode, name in enumerate(ops.PROJECT_MODES):
            maps, valid = ops.od_project(view, P, name, 0.15)
            want, want_valid = sr.od_project(tiles, P, mode, 0.15)
            assert maps.dtype == torch.float32 and tuple(maps.shape) == want.shape
            assert np.array_equal(maps.cpu().numpy().view(np.int32), want.view(np.int32)), (name, P.tolist())
            assert np.array_equal(valid.cpu().numpy(), want_valid)
            assert np.isinf(want).any() and not np.isnan(want).any()
            if mode == 1:
                dropped += int(sr.tissue(tiles, 0.15).sum() - want_valid.sum())
    assert dropped > 0                                                                   # the second plane drops tissue pixels
    assert _guards_untouched(buf, pattern, 3, tiles.size)
    e = torch.empty((0, 3, 4, 4), dtype=torch.uint8, device="cuda")
    assert tuple(ops.od_project(e, PLANES[0], "ratio")[0].shape) == (0, 4, 4)


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    tiles, _ = sr.synthetic_tiles((4, 3, 32, 32), seed=1)
    return tiles, sr.fit(tiles), mil_amd.U8Tiles(torch.from_numpy(tiles).cuda())


def test_fit_equals_the_restated_fit(synthetic):
    """stains within 1e-5 absolute, max_conc within 1e-5 relative: the two fits differ only through the summation order of the
    moments and, at most, one ulp of an fp32 projection entry — measured in tests/test_cpu_stain.py at 5.1e-8 and 2.5e-7."""
    tiles, want, handle = synthetic
    norm = mil_amd.StainNormalizer()
    got = norm.fit(handle)
    print("stains", np.abs(got.stains - want["stains"]).max(), "max_conc", np.abs(got.max_conc / want["max_conc"] - 1).max())
    assert got.n_tissue == want["n_tissue"] and got.n_dropped == want["n_dropped"] == 0
    assert np.abs(got.stains - want["stains"]).max() <= 1e-5
    assert np.abs(got.max_conc / want["max_conc"] - 1.0).max() <= 1e-5
    assert np.array_equal(handle.u8.cpu().numpy(), tiles)                               # a fit writes no tile
    # other bytes (the red channel inverted) and other parameters
    dark = tiles.copy()
    dark[:, 0] = 255 - dark[:, 0] // 2
    w = sr.fit(dark, beta=0.05, q=5.0, conc_q=90.0)
    g = mil_amd.StainNormalizer(beta=0.05, q=5.0, conc_q=90.0).fit(mil_amd.U8Tiles(torch.from_numpy(dark).cuda()))
    assert (g.n_tissue, g.n_dropped) == (w["n_tissue"], w["n_dropped"])
    assert np.abs(g.stains - w["stains"]).max() <= 1e-5 and np.abs(g.max_conc / w["max_conc"] - 1.0).max() <= 1e-5
    with pytest.raises(ValueError):
        norm.fit(mil_amd.U8Tiles(torch.full((2, 3, 8, 8), 255, dtype=torch.uint8, device="cuda")))       # no tissue


def test_transform_and_separate(synthetic):
    tiles, want, handle = synthetic
    norm = mil_amd.StainNormalizer()
    fit = norm.fit(handle)
    direct = ops.stain_affine(handle.u8.clone(), norm.affine(fit).params())
    for given in (fit, None):
        h = mil_amd.U8Tiles(handle.u8.clone())
        assert norm.transform(h, given) is h and torch.equal(h.u8, direct)
    assert np.array_equal(direct.cpu().numpy(), sr.stain_affine(tiles, norm.affine(fit).params().numpy()))
    assert not torch.equal(direct, handle.u8)
    conc = norm.separate(handle, fit)
    wc, _ = sr.od_project(tiles, np.linalg.pinv(fit.stains), 0, 0.15)
    assert tuple(conc.shape) == (2, 4, 32, 32) and np.array_equal(conc.cpu().numpy().view(np.int32), wc.view(np.int32))


# ---- the pre-processor and the bag -----------------------------------------------------------------------------------------------
def _golden_bag(golden_dir, **kw):
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    return z, dev, mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], **kw)


class _Count:
    """Counts the stain_affine launches through the ops' timer hook."""

    def __enter__(self):
        self.timer = ops.KernelTimer(lambda label: label[0] == "stain_affine")
        self.keep, ops.TIMER = ops.TIMER, self.timer
        return self

    def __exit__(self, *exc):
        ops.TIMER = self.keep

    @property
    def n(self):
        return len(self.timer.spans)


def test_preprocessor_and_slide_bag_plumbing(golden_dir):
    norm, jit = mil_amd.StainNormalizer(beta=0.05), mil_amd.StainJitter(0.2, 0.1)
    z, dev, bag = _golden_bag(golden_dir, stain_normalizer=norm, stain_jitter=jit)
    _, _, plain = _golden_bag(golden_dir)
    _, _, only_norm = _golden_bag(golden_dir, stain_normalizer=norm)
    kept = z["kept"]
    n = len(kept)
    assert n == 4 and bag.build() and plain.build() and only_norm.build()
    prep = plain.prep
    params = torch.tensor([[0, 20, 1, 0], [20, 0, 0, 1], [7, 13, 1, 1], [3, 3, 0, 0]], dtype=torch.int32)
    base = prep.from_slide(dev, kept, params, out="u8")
    flat = prep.from_slide(dev, kept, None, out="u8")
    # TilePreprocessor(..., stain=): from_slide followed by stain_affine, and .float() of that
    aff = jit.affine(jit.draw_params(n, torch.Generator().manual_seed(5)))
    want = ops.stain_affine(base.u8.clone(), aff.params())
    assert not torch.equal(want, base.u8)
    got = prep.from_slide(dev, kept, params, out="u8", stain=aff)
    assert isinstance(got, mil_amd.U8Tiles) and torch.equal(got.u8, want)
    nchw = prep.from_slide(dev, kept, params, out="nchw", stain=aff)
    assert nchw.dtype == torch.float32 and torch.equal(nchw.view(torch.int32), mil_amd.U8Tiles(want).float().view(torch.int32))
    stack = torch.stack([dev[r:r + 48, c:c + 48] for r, c in kept])
    assert torch.equal(prep(stack, params, out="u8", stain=aff).u8, want)
    # the stain map comes before the colour jitter
    cj = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
    pj = cj.draw_params(n, torch.Generator().manual_seed(6))
    both = prep.from_slide(dev, kept, params, out="u8", jitter=pj, stain=aff)
    assert torch.equal(both.u8, cj.apply(mil_amd.U8Tiles(want.clone()), pj).u8)
    # stain=None is today's call, bit for bit
    for out in ("u8", "nchw", "s2d"):
        a, b = prep.from_slide(dev, kept, params, out=out, stain=None), prep.from_slide(dev, kept, params, out)
        bits = (lambda x: x.u8 if out == "u8" else x.xs.view(torch.int16) if out == "s2d" else x.view(torch.int32))
        assert torch.equal(bits(a), bits(b)), out
    # the bag: the fit is made once, at first use, on the flat chain's tiles, and kept
    assert bag.stain_fit is None
    sp = jit.draw_params(n, torch.Generator().manual_seed(7))
    with _Count() as count:
        got = bag.get_train_data(params=params, stain_jitter_params=sp)
        assert count.n == 1                                                              # normaliser and jitter: ONE launch
        fit = bag.stain_fit
        assert fit is not None and fit.n_tissue > 100
        bag.get_train_data(params=params, stain_jitter_params=sp)
        assert count.n == 2 and bag.stain_fit is fit
    ref = norm.fit(flat)
    assert np.array_equal(ref.stains, fit.stains) and np.array_equal(ref.max_conc, fit.max_conc)
    f = dict(stains=fit.stains, max_conc=fit.max_conc)
    A1 = sr.REFERENCE_STAINS @ np.diag(sr.REFERENCE_MAX_CONC / fit.max_conc) @ np.linalg.pinv(fit.stains)
    A2, b2 = sr.jitter_affine(sr.HED, sp.alpha.numpy(), sp.beta.numpy())
    cA, cb = sr.compose(A1[None], np.zeros((1, 3)), A2, b2)
    assert np.array_equal(got.u8.cpu().numpy(), sr.stain_affine(base.u8.cpu().numpy(), sr.pack(cA, cb)))
    # validation and inference data are normalised and never jittered
    wv = sr.stain_affine(flat.u8.cpu().numpy(), sr.normalizer_affine(sr.REFERENCE_STAINS, sr.REFERENCE_MAX_CONC, f))
    assert np.array_equal(bag.get_validation_data().u8.cpu().numpy(), wv)
    assert np.array_equal(bag.get_inference_data()[0].u8.cpu().numpy(), wv)
    assert np.array_equal(only_norm.get_validation_data().u8.cpu().numpy(), wv)
    assert not np.array_equal(wv, flat.u8.cpu().numpy())
    # drawn from the generator: crop / flip parameters first, then the stain jitter's
    g = torch.Generator().manual_seed(8)
    pp, ps = prep.draw_params(n, g), jit.draw_params(n, g)
    drawn = bag.get_train_data(generator=torch.Generator().manual_seed(8))
    assert torch.equal(drawn.u8, bag.get_train_data(params=pp, stain_jitter_params=ps).u8)
    # with both options None the bag returns the bytes of the call that bypasses the new arguments, with no stain launch
    with _Count() as count:
        assert torch.equal(plain.get_train_data(params=params).u8, base.u8)
        assert torch.equal(plain.get_validation_data().u8, flat.u8) and torch.equal(plain.get_inference_data()[0].u8, flat.u8)
        assert count.n == 0 and plain.stain_fit is None


def test_attention_forward_on_normalised_tiles(synthetic):
    """The u8 feed's contract on normalised bytes: outputs are finite and those of the same bytes fed as the fp32 tensor."""
    tiles = mil_amd.U8Tiles(synthetic[2].u8.clone())
    mil_amd.StainNormalizer().transform(tiles)
    torch.manual_seed(0)
    net = mil_amd.Attention(3).eval()
    a, b = net(tiles, torch.tensor([1])), net(tiles.float(), torch.tensor([1]))
    assert set(a) == set(b) and len(a) > 3
    for k in a:
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k
