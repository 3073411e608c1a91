"""-m gpu: Vahadane's stain fit on the device (mil_od_snmf_sums_u8, mil_od_snmf_fit_u8, mil_od_code_u8 through `mil_amd.ops`,
`StainNormalizer(method="vahadane")`, `separate(sparse=True)` and `SlideBag(stain_normalizer=)`).  The fp32 codes are compared
for equality with the numpy restatement tests/stain_snmf_reference.py (which tests/test_cpu_stain_snmf.py holds to a brute-force
lasso, to the generating stains and to scikit-learn), the fp64 sums to `math.fsum` within the first-order bound of their tree,
one update to the restated update of the device's own sums bit for bit, and the whole fit within the measured sensitivity."""
import math
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import ops
from mil_amd import stain as st

import stain_reference as sr
import stain_snmf_reference as sn

pytestmark = pytest.mark.gpu

# tests/test_gpu_stain.py's shapes: byte-by-byte planes, mixed accesses with a partial last group, one full workgroup, many
SHAPES = [(3, 3, 5, 7), (2, 3, 16, 12), (5, 3, 33, 31), (4, 3, 64, 64), (2, 3, 300, 300)]
GUARD = 64
GPU_GATE = 1.6e-5                     # tests/test_cpu_stain_snmf.py: forty times the largest measured move of the restated fit
BETA = 0.15
START = sr.HED[:, :2]
ZERO_BYTE = 100                       # a red byte whose OD is the penalty of the dictionary with zero entries: q_0 == 0 there


def _unit(W):
    W = np.asarray(W, dtype=np.float64)
    return W / np.linalg.norm(W, axis=0, keepdims=True)


# (dictionary, lam): the published vectors; Ruifrok's with a small penalty; one with zero entries whose penalty is the OD of
# ZERO_BYTE exactly, so that q_0 = (1 L[r] + 0 L[g]) + 0 L[b] - lam is exactly 0 at red byte ZERO_BYTE; a nearly collinear pair
DICTS = [(_unit(sr.REFERENCE_STAINS), 0.1), (START, 0.02), (_unit([[1.0, 0.2], [0.0, 0.8], [0.0, 0.55]]), float(sr.L[ZERO_BYTE])),
         (_unit([[0.56, 0.54], [0.72, 0.74], [0.41, 0.40]]), 0.05)]
_cache = {}


def _tiles(shape):
    """The stack of a shape (H&E-like bytes, with two tissue pixels of red byte ZERO_BYTE planted), made once, read-only."""
    if shape not in _cache:
        tiles, _ = sr.synthetic_tiles(shape, seed=shape[2])
        tiles[0, :, 0, 0] = (ZERO_BYTE, 80, 90)
        tiles[-1, :, -1, -1] = (ZERO_BYTE, 30, 200)
        tiles.setflags(write=False)
        _cache[shape] = tiles
    return _cache[shape]


def _on_device(tiles_np, offset=GUARD):
    n = tiles_np.size
    pattern = (np.arange(n + offset + GUARD) * 37 + 11).astype(np.uint8)
    buf = torch.from_numpy(pattern.copy()).cuda()
    view = buf[offset:offset + n].view(tiles_np.shape)
    view.copy_(torch.from_numpy(np.array(tiles_np)))
    return view, buf, pattern


def _guards_untouched(buf, pattern, offset, n):
    got = buf.cpu().numpy()
    return np.array_equal(got[:offset], pattern[:offset]) and np.array_equal(got[offset + n:], pattern[offset + n:])


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


# ---- the "sparse" projection: bit for bit ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_sparse_projection_equals_the_restatement(shape):
    tiles = _tiles(shape)
    view, buf, pattern = _on_device(tiles, offset=3)
    lr, lg, lb = sn.tissue_od(tiles, BETA)
    branches = set()
    for W, lam in DICTS:
        maps, valid = ops.od_project(view, W, "sparse", BETA, lam=lam)
        want, want_valid = sn.sparse_maps(tiles, W, lam, BETA)
        assert maps.dtype == torch.float32 and tuple(maps.shape) == want.shape == (2, shape[0]) + shape[2:]
        assert np.array_equal(_bits(maps.cpu().numpy()), _bits(want)), (W.tolist(), lam)
        assert np.array_equal(valid.cpu().numpy(), want_valid)
        assert np.isinf(want).any() and not np.isnan(want).any() and (want >= 0).all()
        branches |= set(np.unique(sn.code(lr, lg, lb, sn.coder(W, lam))[2]).tolist())
    assert branches == {0, 1, 2}                                          # both stains, the first alone, the second alone
    # the dictionary with zero entries: q_0 is exactly 0 at the planted pixels, and the code's first entry with it
    W, lam = DICTS[2]
    k = sn.coder(W, lam)
    assert k[2] == 0 and k[4] == 0 and ((k[0] * sr.L[ZERO_BYTE] + k[2] * sr.L[80]) + k[4] * sr.L[90]) - k[8] == 0
    want, _ = sn.sparse_maps(tiles, W, lam, BETA)
    assert want[0, 0, 0, 0] == 0 and want[0, -1, -1, -1] == 0 and np.isfinite(want[1, 0, 0, 0])
    assert _guards_untouched(buf, pattern, 3, tiles.size)


def test_sparse_projection_at_every_byte_offset_and_without_tiles():
    W, lam = DICTS[0]
    for shape in SHAPES[:4]:
        tiles = _tiles(shape)
        want, want_valid = sn.sparse_maps(tiles, W, lam, BETA)
        for offset in (1, 2, 3):
            view, buf, pattern = _on_device(tiles, offset=offset)
            maps, valid = ops.od_project(view, W, "sparse", BETA, lam=lam)
            assert np.array_equal(_bits(maps.cpu().numpy()), _bits(want)), (shape, offset)
            assert np.array_equal(valid.cpu().numpy(), want_valid)
            assert _guards_untouched(buf, pattern, offset, tiles.size)
    e = torch.empty((0, 3, 4, 4), dtype=torch.uint8, device="cuda")
    maps, valid = ops.od_project(e, W, "sparse", BETA, lam=lam)
    assert tuple(maps.shape) == (2, 0, 4, 4) and tuple(valid.shape) == (0,)
    # collinear columns: every code is zero, nothing is NaN
    tiles = _tiles(SHAPES[1])
    flat = np.stack([START[:, 0], START[:, 0]], axis=1)
    maps = ops.od_project(torch.from_numpy(np.array(tiles)).cuda(), flat, "sparse", BETA, lam=0.1)[0].cpu().numpy()
    assert np.array_equal(_bits(maps), _bits(sn.sparse_maps(tiles, flat, 0.1, BETA)[0])) and not np.isnan(maps).any()
    assert (maps[np.isfinite(maps)] == 0).all()


# ---- the twelve sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_snmf_sums_within_the_bound_of_the_tree_and_repeatable(shape):
    """Every term (1, h_j h_k, v_c h_j, h_j) is exact in fp64 and non-negative and a pixel that is not tissue adds exact zeros,
    so tests/test_gpu_stain.py's argument for the moments holds as it stands: the tree's sum of the n tissue terms is within
    (n - 1) 2^-53 S of the exact sum S; n 2^-52 S covers it with a factor of two to spare."""
    tiles = _tiles(shape)
    view, buf, pattern = _on_device(tiles, offset=1)
    for W, lam in DICTS[:3]:
        got = ops.od_snmf_sums(view, W, lam, BETA)
        again = ops.od_snmf_sums(view, W, lam, BETA)
        assert got.dtype == torch.float64 and tuple(got.shape) == (12,)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64))
        got = got.cpu().numpy()
        terms = sn.sum_terms(tiles, sn.coder(W, lam), BETA)
        n = terms[0].size
        assert got[0] == n and n > 10
        for k in range(1, 12):
            assert (terms[k] >= 0).all()
            exact = math.fsum(terms[k])
            bound = n * 2.0 ** -52 * exact
            assert abs(got[k] - exact) <= bound, (k, got[k], exact, bound)
        assert got[1] + got[3] > 0
    assert _guards_untouched(buf, pattern, 1, tiles.size)


def test_snmf_sums_without_tissue_without_tiles_and_with_one_stain_idle():
    blank = torch.full((3, 3, 33, 31), 250, dtype=torch.uint8, device="cuda")           # OD 0.02 < beta
    blank[:, 1] = 3                                                                      # one dark channel is not tissue
    got = ops.od_snmf_sums(blank, START, 0.1, BETA)
    assert bool((got == 0).all()) and not bool(torch.signbit(got).any())
    e = torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda")
    assert bool((ops.od_snmf_sums(e, START, 0.1, BETA) == 0).all())
    W, hist, count = ops.od_snmf_fit(e, START, 0.1, 3, BETA)
    assert np.array_equal(W.cpu().numpy(), START) and bool((hist == 0).all()) and float(count) == 0
    W, hist, count = ops.od_snmf_fit(blank, START, 0.1, 3, BETA)
    assert np.array_equal(W.cpu().numpy(), START) and bool((hist == 0).all()) and float(count) == 0
    # a penalty above every q_1: the second stain codes no pixel, its column stays to the bit, the first one moves
    tiles = _tiles(SHAPES[2])
    dev = torch.from_numpy(np.array(tiles)).cuda()
    idle = _unit([[0.6, 0.0], [0.7, 0.05], [0.4, 1.0]])
    big = 1.5
    s = ops.od_snmf_sums(dev, idle, big, BETA).cpu().numpy()
    assert s[1] > 0 and s[3] == 0 and s[2] == 0 and s[11] == 0
    W, hist, _ = ops.od_snmf_fit(dev, idle, big, 2, BETA)
    W = W.cpu().numpy()
    assert np.array_equal(W[:, 1], idle[:, 1]) and not np.array_equal(W[:, 0], idle[:, 0]) and bool(torch.isfinite(hist).all())


# ---- one iteration: the update, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_one_iteration_equals_the_restated_update_of_the_device_sums(shape):
    tiles = _tiles(shape)
    dev = torch.from_numpy(np.array(tiles)).cuda()
    sv2 = sn.sv2_of(ops.od_moments(dev, BETA, "bag")[0].cpu().numpy())
    for W0, lam in DICTS:
        s = ops.od_snmf_sums(dev, W0, lam, BETA).cpu().numpy()
        W, hist, count = ops.od_snmf_fit(dev, W0, lam, 1, BETA)
        want_W, want_f, want_move = sn.update(W0, s, sv2, lam)
        W, hist = W.cpu().numpy(), hist.cpu().numpy()
        print(shape, lam, "W ulps", np.abs(_bits(W) - _bits(want_W)).max(), "history", hist[0].tolist(), [want_f, want_move])
        assert float(count) == s[0]
        assert np.array_equal(_bits(W), _bits(want_W)), (W.tolist(), want_W.tolist())
        assert np.array_equal(_bits(hist), _bits(np.array([[want_f, want_move]])))
        assert tuple(W.shape) == (3, 2) and (want_move > 0) == (s[1] + s[3] > 0)          # a stain that coded a pixel moves
        # two iterations: the second codes with the dictionary the first one left on the device
        W2, hist2, _ = ops.od_snmf_fit(dev, W0, lam, 2, BETA)
        s2 = ops.od_snmf_sums(dev, W, lam, BETA).cpu().numpy()
        want_W2, want_f2, want_move2 = sn.update(W, s2, sv2, lam)
        assert np.array_equal(_bits(W2.cpu().numpy()), _bits(want_W2))
        assert np.array_equal(_bits(hist2.cpu().numpy()), _bits(np.array([[want_f, want_move], [want_f2, want_move2]])))


# ---- the fit -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synthetic():
    tiles, _ = sr.synthetic_tiles((4, 3, 64, 64), seed=1)
    return tiles, sn.fit(tiles), mil_amd.U8Tiles(torch.from_numpy(tiles).cuda())


def test_vahadane_fit_equals_the_restated_fit(synthetic):
    tiles, want, handle = synthetic
    norm = mil_amd.StainNormalizer(method="vahadane")
    got, again = norm.fit(handle), norm.fit(handle)
    ds, dc = np.abs(got.stains - want["stains"]).max(), np.abs(got.max_conc / want["max_conc"] - 1.0).max()
    print("stains", ds, "max_conc", dc, "last_move", got.last_move, "objective", got.objective[0], got.objective[-1])
    assert ds <= GPU_GATE and dc <= GPU_GATE
    assert (got.n_tissue, got.n_dropped) == (want["n_tissue"], 0) and got.stains[0, 0] > got.stains[0, 1]
    assert got.objective.shape == (64,) and np.allclose(got.objective, want["objective"], rtol=1e-6, atol=0)
    assert got.last_move < 1e-6 and abs(np.linalg.norm(got.stains, axis=0) - 1.0).max() < 1e-12
    for a, b in ((got.stains, again.stains), (got.max_conc, again.max_conc), (got.objective, again.objective)):
        assert np.array_equal(_bits(a), _bits(b))
    assert got.last_move == again.last_move
    assert np.array_equal(handle.u8.cpu().numpy(), tiles)                               # a fit writes no tile
    for k in (0, 1):
        assert sr.angle_deg(got.stains[:, k], sr.REFERENCE_STAINS[:, k]) < 1.5 * (0.815, 1.349)[k]
    # other parameters: a smaller penalty, fewer iterations, another tissue threshold
    w = sn.fit(tiles, lam=0.02, iters=20, beta=0.05, conc_q=90.0)
    g = mil_amd.StainNormalizer(beta=0.05, conc_q=90.0, method="vahadane", lam=0.02, iters=20).fit(handle)
    assert g.n_tissue == w["n_tissue"] and g.objective.shape == (20,)
    assert np.abs(g.stains - w["stains"]).max() <= GPU_GATE and np.abs(g.max_conc / w["max_conc"] - 1.0).max() <= GPU_GATE


def test_vahadane_fit_of_degenerate_stacks_and_from_a_macenko_start(synthetic):
    tiles, _, handle = synthetic
    norm = mil_amd.StainNormalizer(method="vahadane")
    with pytest.raises(ValueError):
        norm.fit(mil_amd.U8Tiles(torch.full((2, 3, 8, 8), 255, dtype=torch.uint8, device="cuda")))       # no tissue
    with pytest.raises(ValueError):
        norm.fit(mil_amd.U8Tiles(torch.empty((0, 3, 8, 8), dtype=torch.uint8, device="cuda")))
    # haematoxylin alone: both columns are drawn to the one vector and end within 1.8 degrees of each other
    rng = np.random.default_rng(7)
    n = 2 * 24 * 20
    od = rng.uniform(0.3, 2.0, n)[:, None] * sr.unit(sr.REFERENCE_STAINS[:, 0])[None] + rng.normal(0.0, 0.01, (n, 3))
    by = np.clip(np.rint(256.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8)
    single = np.ascontiguousarray(by.reshape(2, 24, 20, 3).transpose(0, 3, 1, 2))
    with pytest.raises(ValueError):
        sn.fit(single)
    dev = torch.from_numpy(single).cuda()
    with pytest.raises(ValueError, match="no two stains"):
        norm.fit(mil_amd.U8Tiles(dev))
    W, hist, _ = ops.od_snmf_fit(dev, START, 0.1, 64, BETA)
    assert bool(torch.isfinite(hist).all()) and bool(torch.isfinite(W).all())
    W = W.cpu().numpy()
    assert 0.0 < 1.0 - float(W[:, 0] @ W[:, 1]) ** 2 < st.SNMF_MIN_SIN2
    # exactly collinear columns from the start: every code is zero, the dictionary stays, the fit is refused
    flat = np.stack([START[:, 0], START[:, 0]], axis=1)
    W, hist, _ = ops.od_snmf_fit(handle.u8, flat, 0.1, 3, BETA)
    assert np.array_equal(W.cpu().numpy(), flat) and bool(torch.isfinite(hist).all()) and float(hist[0, 1]) == 0
    with pytest.raises(ValueError, match="no two stains"):
        mil_amd.StainNormalizer(method="vahadane", init=flat).fit(handle)
    # polishing a Macenko fit: the objective does not end above where it began
    mac = mil_amd.StainNormalizer().fit(handle)
    pol = mil_amd.StainNormalizer(method="vahadane", init=mac).fit(handle)
    print("from macenko: objective", pol.objective[0], "->", pol.objective[-1])
    assert pol.objective[-1] <= pol.objective[0] and pol.n_tissue == mac.n_tissue


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def test_transform_and_separate(synthetic):
    tiles, _, handle = synthetic
    norm = mil_amd.StainNormalizer(method="vahadane")
    fit = norm.fit(handle)
    direct = st.apply_stain(mil_amd.U8Tiles(handle.u8.clone()), norm.affine(fit)).u8
    for given in (fit, None):
        h = mil_amd.U8Tiles(handle.u8.clone())
        assert norm.transform(h, given) is h and torch.equal(h.u8, direct)
    assert np.array_equal(direct.cpu().numpy(), sr.stain_affine(tiles, norm.affine(fit).params().numpy()))
    assert not torch.equal(direct, handle.u8)
    conc = norm.separate(handle, fit)
    wc, _ = sr.od_project(tiles, np.linalg.pinv(fit.stains), 0, BETA)
    assert np.array_equal(_bits(conc.cpu().numpy()), _bits(wc))
    for lam, kw in ((0.1, {}), (0.03, dict(lam=0.03))):
        sparse = norm.separate(handle, fit, sparse=True, **kw)
        assert torch.equal(sparse.view(torch.int32), ops.od_project(handle.u8, fit.stains, "sparse", BETA, lam=lam)[0].view(torch.int32))
        assert np.array_equal(_bits(sparse.cpu().numpy()), _bits(sn.sparse_maps(tiles, fit.stains, lam, BETA)[0]))
    assert not torch.equal(sparse, conc)
    # a Vahadane fit is a StainFit: the jitter takes it as its basis
    assert np.array_equal(mil_amd.StainJitter(0.1, 0.0, basis=fit).R, fit.basis())


def test_slide_bag_takes_a_vahadane_normalizer(golden_dir):
    """`SlideBag` and `from_slide` are unchanged: the bag fits once with whatever normaliser it was given and maps with the
    one shared affine of that fit."""
    z = np.load(os.path.join(golden_dir, "roi_select_small.npz"))
    dev = torch.from_numpy(z["slide"]).cuda()
    norm = mil_amd.StainNormalizer(beta=0.05, method="vahadane")
    bag = mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"], stain_normalizer=norm)
    plain = mil_amd.SlideBag(dev, 48, 7, resolution=32, pad=10, coords=z["kept"])
    assert bag.build() and plain.build() and bag.stain_fit is None
    flat = plain.prep.from_slide(dev, z["kept"], None, out="u8")
    got = bag.get_validation_data()
    fit = bag.stain_fit
    ref = norm.fit(flat)
    assert fit is not None and fit.objective is not None and fit.n_tissue > 100
    assert np.array_equal(ref.stains, fit.stains) and np.array_equal(ref.max_conc, fit.max_conc)
    want = sr.stain_affine(flat.u8.cpu().numpy(), norm.affine(fit).params().numpy())
    assert np.array_equal(got.u8.cpu().numpy(), want) and not np.array_equal(want, flat.u8.cpu().numpy())
    assert np.array_equal(bag.get_inference_data()[0].u8.cpu().numpy(), want) and bag.stain_fit is fit
    via = plain.prep.from_slide(dev, z["kept"], None, out="u8", stain=norm.affine(fit))
    assert np.array_equal(via.u8.cpu().numpy(), want)
    # against the restated fit of the same bytes
    w = sn.fit(flat.u8.cpu().numpy(), beta=0.05)
    assert np.abs(fit.stains - w["stains"]).max() <= GPU_GATE and np.abs(fit.max_conc / w["max_conc"] - 1.0).max() <= GPU_GATE


def test_attention_forward_on_normalised_tiles(synthetic):
    tiles = mil_amd.U8Tiles(synthetic[2].u8.clone())
    mil_amd.StainNormalizer(method="vahadane").transform(tiles)
    torch.manual_seed(0)
    net = mil_amd.Attention(3).eval()
    out = net(tiles, torch.tensor([1]))
    assert len(out) > 3
    for k in out:
        assert bool(torch.isfinite(out[k]).all()), k
