"""CPU (-m "not gpu"): the stain contract's numpy restatement (tests/stain_reference.py) against the fp64 formulas and Macenko's
method, and the host layer of mil_amd/stain.py — tables, `StainAffine`, `StainJitter.draw_params`, every refusal that needs no
GPU, the C entries' host-side status codes."""
import ctypes
import math

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import _lib, ops
from mil_amd import stain as st

import stain_reference as sr


def _triples(n=200_000, seed=5):
    return np.random.default_rng(seed).integers(0, 256, (n, 3), dtype=np.uint8)


def _as_tiles(triples):
    return np.ascontiguousarray(triples.T.reshape(1, 3, 1, -1))


def _as_triples(tiles):
    return tiles.reshape(3, -1).T


# ---- tables and the byte contract ------------------------------------------------------------------------------------------------
def test_tables_are_the_contract():
    tab = ops.od_tables_host()
    assert tab.dtype == np.float32 and tab.shape == (511,)
    assert np.array_equal(tab[:256], sr.L) and np.array_equal(tab[256:], sr.TH[1:])
    assert tab[255] == 0.0 and tab[0] == np.float32(-math.log(1 / 256.0))
    assert bool((np.diff(sr.TH[1:]) < 0).all())                                  # strictly decreasing in fp32
    assert np.array_equal(sr.od_byte(sr.L), np.arange(256))                      # byte(L[v]) == v
    assert np.array_equal(sr.od_byte_by_count(sr.L), np.arange(256))
    # ties go to the brighter byte; the ends; NaN
    assert np.array_equal(sr.od_byte(sr.TH[1:]), np.arange(1, 256))
    assert np.array_equal(sr.od_byte(np.nextafter(sr.TH[1:], np.float32(np.inf))), np.arange(0, 255))
    assert sr.od_byte(np.float32(-3.0)) == 255 and sr.od_byte(np.float32(np.inf)) == 0 and sr.od_byte(np.float32(np.nan)) == 0
    o = np.random.default_rng(0).uniform(-0.5, 6.5, 20000).astype(np.float32)
    assert np.array_equal(sr.od_byte(o), sr.od_byte_by_count(o))
    assert ops.od_tables("cpu") is ops.od_tables("cpu") and np.array_equal(ops.od_tables("cpu").numpy(), tab)


def test_identity_maps_return_every_byte():
    tr = _triples()
    tiles = _as_tiles(tr)
    assert np.array_equal(sr.stain_affine(tiles, st.StainAffine.identity().params().numpy()), tiles)
    hed = st.StainJitter(0.0, 0.0, basis=mil_amd.HED)
    aff = hed.affine((np.ones((1, 3)), np.zeros((1, 3))))                        # R diag(1) R^-1 rounded to fp32
    assert np.array_equal(sr.stain_affine(tiles, aff.params().numpy()), tiles)
    assert np.allclose(mil_amd.HED, sr.HED) and np.allclose(np.linalg.norm(mil_amd.HED, axis=0), 1.0)
    assert np.allclose(mil_amd.HED[:, 0], np.array([0.65, 0.70, 0.29]) / np.linalg.norm([0.65, 0.70, 0.29]))


def test_agreement_with_the_fp64_formula():
    """50 drawn jitter maps (sigma_alpha 0.2, sigma_beta 0.1) on 200 000 byte triples: the table contract against
    round(256 exp(-(A od + b)) - 1).  Measured here: largest difference 1, share of differing bytes 3.8e-6."""
    tr = _triples()
    tiles = _as_tiles(tr)
    jit = st.StainJitter(0.2, 0.1)
    p = jit.draw_params(50, torch.Generator().manual_seed(3))
    aff = jit.affine(p)
    worst, differing = 0, 0
    for k in range(50):
        got = _as_triples(sr.stain_affine(tiles, aff.params().numpy()[k:k + 1]))
        want = sr.formula_bytes(tr, aff.A[k], aff.b[k])
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        worst, differing = max(worst, int(d.max())), differing + int((d != 0).sum())
    share = differing / (50 * tr.size)
    print(f"largest byte difference {worst}, share of differing bytes {share:.3g}")
    assert worst <= 1 and share < 1e-4


# ---- the restated fit is Macenko's -----------------------------------------------------------------------------------------------
def test_restated_fit_recovers_the_stain_vectors():
    tiles, _ = sr.synthetic_tiles((4, 3, 32, 32), seed=1)
    f = sr.fit(tiles)
    angles = [sr.angle_deg(f["stains"][:, k], sr.REFERENCE_STAINS[:, k]) for k in (0, 1)]
    print("angles to the generating vectors (degrees):", angles, "n_tissue", f["n_tissue"], "n_dropped", f["n_dropped"])
    assert max(angles) < 2.0
    assert f["n_dropped"] == 0 and 0 < f["n_tissue"] < tiles.size // 3
    assert f["stains"][0, 0] > f["stains"][0, 1]                                 # haematoxylin first
    assert np.allclose(np.linalg.norm(f["stains"], axis=0), 1.0)
    # A tile set mapped onto its own fit: A = S pinv(S) is the projector onto the plane of the two fitted stains, so a pixel whose
    # OD lies in that plane up to its byte rounding moves by no more than 1 — the tile set for this is the same mixture WITHOUT
    # the OD noise.  (With the noise the projector removes the noise's out-of-plane part, 0.01 OD = up to 6 byte steps at these
    # brightnesses: that is the normalisation at work, not an error; measured 6 on the noisy set, 1 on the clean one.)
    clean, _ = sr.synthetic_tiles((4, 3, 32, 32), seed=1, noise=0.0)
    fc = sr.fit(clean)
    own = sr.normalizer_affine(fc["stains"], fc["max_conc"], fc)
    out = sr.stain_affine(clean, own)
    assert int(np.abs(out.astype(np.int32) - clean.astype(np.int32)).max()) <= 1
    own = sr.normalizer_affine(f["stains"], f["max_conc"], f)
    # the same objects through the host layer: affine(fit) is the restated map
    norm = st.StainNormalizer(target=st.StainFit(f["stains"], f["max_conc"]))
    assert np.array_equal(norm.affine(st.StainFit(f["stains"], f["max_conc"], f["n_tissue"], 0)).params().numpy(), own)


@pytest.mark.parametrize("shape", [(3, 3, 16, 12), (4, 3, 32, 32)])
def test_fit_sensitivity_to_one_ulp_of_a_projection_and_to_the_summation_order(shape):
    """What the GPU test's 1e-5 margin on `stains` / `max_conc` rests on: the device's fit can differ from the restated one
    through the summation order of the moments and through nothing else (both projections are the same fp32 numbers unless the
    moments move them by an ulp).  Measured here: one ulp of any entry of either projection moves stains by at most 5.1e-8 and
    max_conc by 2.5e-7 (relative); moments perturbed by 1e-12 (relative) move neither (the fp32 projection does not change).
    1e-5 is forty times the larger, more than the ten it must be, so it stays."""
    tiles, _ = sr.synthetic_tiles(shape, seed=2)
    base = sr.fit(tiles)
    ds = dc = 0.0
    for which in (0, 1):
        for k in range(2):
            for j in range(3):
                for d in (1, -1):
                    f = sr.fit(tiles, nudge=(which, k, j, d))
                    assert f["n_tissue"] == base["n_tissue"]
                    ds = max(ds, float(np.abs(f["stains"] - base["stains"]).max()))
                    dc = max(dc, float(np.abs(f["max_conc"] / base["max_conc"] - 1.0).max()))
    m = sr.od_moments(tiles, 0.15, True)[0]
    rng = np.random.default_rng(0)
    dm = 0.0
    for _ in range(8):
        pm = m * (1.0 + 1e-12 * rng.uniform(-1, 1, 10))
        pm[0] = m[0]
        f = sr.fit(tiles, moments=pm)
        dm = max(dm, float(np.abs(f["stains"] - base["stains"]).max()), float(np.abs(f["max_conc"] / base["max_conc"] - 1.0).max()))
    print(f"{shape}: one ulp of P moves stains by {ds:.3g}, max_conc by {dc:.3g} (relative); moments at 1e-12: {dm:.3g}")
    assert ds * 10 <= 1e-5 and dc * 10 <= 1e-5 and dm * 10 <= 1e-5


def test_effective_percentile_never_reaches_an_inf():
    for q in (1.0, 50.0, 99.0, 100.0):
        for nv, n in ((2, 3), (2, 1000), (999, 1000), (7, 7), (123457, 262144), (3, 2 ** 24)):
            qe = st.effective_q(q, nv, n)
            assert qe == sr.effective_q(q, nv, n) and 0.0 < qe <= 100.0
            assert (n - 1) * (qe / 100.0) <= nv - 1
    v = np.array([3.0, 1.0, np.inf, 2.0, np.inf], dtype=np.float32)
    assert sr.percentile_of_valid(v, 100.0, 3) == 3.0 and sr.percentile_of_valid(v, 50.0, 3) == 2.0
    # the restated interpolation is np.percentile's, and the host layer's from the two bracketing order statistics is the same
    w = np.random.default_rng(9).normal(size=1001).astype(np.float32)
    s = np.sort(w).astype(np.float64)
    for q in (1.0, 37.3, 50.0, 99.0, 100.0):
        want = float(np.percentile(w.astype(np.float64), q))
        lo = int(math.floor(1000 * (q / 100.0)))
        assert sr.percentile_of_valid(w, q, w.size) == want
        assert st.percentile_from_stats(s[lo], s[min(lo + 1, 1000)], q, w.size) == want
    assert st.percentile_from_stats(3.0, np.inf, st.effective_q(100.0, 3, 5), 5) == 3.0


# ---- host objects ------------------------------------------------------------------------------------------------------------
def test_stain_affine_composition_and_shapes():
    rng = np.random.default_rng(4)
    a = st.StainAffine(rng.normal(size=(3, 3)), rng.normal(size=3))
    b = st.StainAffine(rng.normal(size=(5, 3, 3)), rng.normal(size=(5, 3)))
    assert len(a) == 1 and len(b) == 5 and a.params().shape == (1, 12) and b.params().dtype == torch.float32
    assert np.array_equal(b.params().numpy()[2], np.concatenate([b.A[2], b.b[2][:, None]], axis=1).reshape(12).astype(np.float32))
    x = rng.normal(size=3)
    for first, second in ((a, b), (b, a), (b, b), (a, a)):
        c = first.then(second)
        assert len(c) == max(len(first), len(second))
        for k in range(len(c)):
            f, s = min(k, len(first) - 1), min(k, len(second) - 1)
            want = second.A[s] @ (first.A[f] @ x + first.b[f]) + second.b[s]
            assert np.allclose(c.A[k] @ x + c.b[k], want, rtol=1e-12, atol=1e-12)
    cA, cb = sr.compose(a.A, a.b, b.A, b.b)
    assert np.array_equal(a.then(b).A, cA) and np.array_equal(a.then(b).b, cb)
    i = st.StainAffine.identity(4)
    assert len(i) == 4 and np.array_equal(i.then(st.StainAffine(b.A[:4], b.b[:4])).A, b.A[:4])
    assert st.StainAffine(np.eye(3)).b.shape == (1, 3)
    for bad in (lambda: st.StainAffine(np.eye(4)), lambda: st.StainAffine(np.eye(3), np.zeros(4)),
                lambda: st.StainAffine(np.full((3, 3), np.nan)), lambda: st.StainAffine(np.eye(3), [0, np.inf, 0]),
                lambda: st.StainAffine(np.zeros((2, 3, 3)), np.zeros((3, 3))), lambda: a.then(5),
                lambda: b.then(st.StainAffine.identity(4)), lambda: st.StainAffine("x")):
        with pytest.raises(ValueError):
            bad()


def test_reference_fit_and_jitter_parameters():
    ref = mil_amd.StainFit.reference()
    assert np.array_equal(ref.stains, sr.REFERENCE_STAINS) and np.array_equal(ref.max_conc, sr.REFERENCE_MAX_CONC)
    basis = ref.basis()
    assert basis.shape == (3, 3) and abs(np.linalg.norm(basis[:, 2]) - 1) < 1e-12 and abs(basis[:, 2] @ basis[:, 0]) < 1e-12
    jit = mil_amd.StainJitter(0.05, 0.01)
    p1, p2 = jit.draw_params(7, torch.Generator().manual_seed(11)), jit.draw_params(7, torch.Generator().manual_seed(11))
    assert torch.equal(p1.alpha, p2.alpha) and torch.equal(p1.beta, p2.beta) and p1.alpha.dtype == torch.float64
    u = torch.rand((7, 6), dtype=torch.float64, generator=torch.Generator().manual_seed(11))            # ONE draw of [n,6]
    assert torch.equal(p1.alpha, 1.0 + 0.05 * (2.0 * u[:, :3] - 1.0)) and torch.equal(p1.beta, 0.01 * (2.0 * u[:, 3:] - 1.0))
    assert float((p1.alpha - 1).abs().max()) <= 0.05 and float(p1.beta.abs().max()) <= 0.01
    aff = jit.affine(p1, 7)
    A, b = sr.jitter_affine(sr.HED, p1.alpha.numpy(), p1.beta.numpy())
    assert np.allclose(aff.A, A, rtol=0, atol=1e-14) and np.allclose(aff.b, b, rtol=0, atol=1e-15)
    fitted = mil_amd.StainJitter(0.1, 0.0, basis=ref)
    assert np.array_equal(fitted.R, basis)
    for bad in (lambda: mil_amd.StainJitter(-0.1), lambda: mil_amd.StainJitter(0.1, float("nan")),
                lambda: mil_amd.StainJitter(basis=np.ones((3, 3))), lambda: mil_amd.StainJitter(basis=np.eye(2)),
                lambda: jit.affine(p1, 6), lambda: jit.affine((p1.alpha, p1.beta[:3])), lambda: jit.affine(5),
                lambda: jit.affine((torch.full((7, 3), float("nan")), p1.beta)),
                lambda: mil_amd.StainNormalizer(target=5), lambda: mil_amd.StainNormalizer(q=50.0),
                lambda: mil_amd.StainNormalizer(beta=-1.0), lambda: mil_amd.StainNormalizer(conc_q=0.0),
                lambda: mil_amd.StainFit(np.ones((3, 2)), [1, 1]),
                lambda: mil_amd.StainNormalizer().affine(mil_amd.StainFit(sr.REFERENCE_STAINS, [1.0, 0.0]))):
        with pytest.raises(ValueError):
            bad()


def test_refusals_need_no_gpu():
    cpu = mil_amd.U8Tiles(torch.zeros((2, 3, 8, 6), dtype=torch.uint8))
    raw = torch.zeros((2, 3, 8, 6), dtype=torch.uint8)
    jit, norm = mil_amd.StainJitter(), mil_amd.StainNormalizer()
    p = jit.draw_params(2)
    ref = mil_amd.StainFit.reference()
    for call in (lambda: jit.apply(raw, p), lambda: jit(raw), lambda: norm.fit(raw), lambda: norm.transform(raw, ref),
                 lambda: norm.separate(raw, ref), lambda: st.apply_stain(raw, st.StainAffine.identity()),
                 lambda: jit.apply(cpu, jit.draw_params(3)), lambda: st.apply_stain(cpu, st.StainAffine.identity(3)),
                 lambda: st.apply_stain(cpu, np.eye(3)), lambda: norm.separate(cpu, None), lambda: norm.transform(cpu, 7),
                 lambda: st.apply_stain(cpu, st.StainAffine(np.eye(3) * 1e39))):                          # overflows fp32
        with pytest.raises(ValueError):
            call()
    for call in (lambda: jit.apply(cpu, p), lambda: jit(cpu), lambda: norm.fit(cpu), lambda: norm.transform(cpu, ref),
                 lambda: norm.transform(cpu), lambda: norm.separate(cpu, ref), lambda: st.apply_stain(cpu, st.StainAffine.identity())):
        with pytest.raises(RuntimeError):
            call()
    # the ops: argument checks in the style of their neighbours
    good = torch.zeros((1, 12))
    for call in (lambda: ops.stain_affine(raw.float(), good), lambda: ops.stain_affine(raw[:, :2], good),
                 lambda: ops.stain_affine(raw, torch.zeros((3, 12))), lambda: ops.stain_affine(raw, torch.zeros((2, 11))),
                 lambda: ops.stain_affine(raw, good.double()), lambda: ops.stain_affine(raw, torch.full((1, 12), float("inf"))),
                 lambda: ops.stain_affine(raw, good),                                                      # a CPU stack
                 lambda: ops.od_moments(raw, group="slide"), lambda: ops.od_moments(raw, beta=float("nan")),
                 lambda: ops.od_moments(raw), lambda: ops.od_project(raw, np.zeros((2, 3)), mode="angle"),
                 lambda: ops.od_project(raw, np.zeros((3, 2))), lambda: ops.od_project(raw, np.full((2, 3), np.nan)),
                 lambda: ops.od_project(raw, np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            call()


def test_preprocessor_and_bag_refusals():
    prep = mil_amd.TilePreprocessor(16, 8, pad=4)
    rois = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    slide = torch.zeros((40, 40, 3), dtype=torch.uint8)
    one = st.StainAffine.identity()
    with pytest.raises(ValueError, match="out='u8'"):
        prep(rois, None, out="s2d", stain=one)
    with pytest.raises(ValueError, match="out='u8'"):
        prep.from_slide(slide, [(0, 0), (3, 5)], None, out="s2d", stain=one)
    for out in ("u8", "nchw"):
        with pytest.raises(ValueError):
            prep(rois, None, out=out, stain=st.StainAffine.identity(3))                          # one map, or one per tile
        with pytest.raises(ValueError):
            prep.from_slide(slide, [(0, 0), (3, 5)], None, out=out, stain=np.eye(3))
        with pytest.raises(RuntimeError):
            prep(rois, None, out=out, stain=one)                                                 # CPU ROIs: no fallback
    with pytest.raises(TypeError):
        prep(rois, None, "u8", None, one)                                                        # keyword-only
    bag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=[(0, 0), (3, 5)])
    assert bag.stain_normalizer is None and bag.stain_jitter is None and bag.stain_fit is None
    with pytest.raises(ValueError, match="stain_jitter"):
        bag.get_train_data(stain_jitter_params=mil_amd.StainJitter().draw_params(2))
    with pytest.raises(TypeError):
        mil_amd.SlideBag(slide, 16, 0, 8, 4, 2500, None, [(0, 0)], None, mil_amd.StainNormalizer())     # keyword-only
    jbag = mil_amd.SlideBag(slide, 16, 0, resolution=8, pad=4, coords=[(0, 0), (3, 5)], stain_jitter=mil_amd.StainJitter())
    with pytest.raises(ValueError):
        jbag.get_train_data(stain_jitter_params=mil_amd.StainJitter().draw_params(3))            # one row per tile
    with pytest.raises(ValueError, match="out='u8'"):
        jbag.get_train_data(out="s2d")


# ---- the C entries' host-side checks -------------------------------------------------------------------------------------------
def test_entry_status_codes_need_no_gpu():
    lib = mil_amd.lib()
    for name in ("mil_stain_affine_u8", "mil_od_moments_u8", "mil_od_project_u8"):
        assert name in _lib.EXPORTS and hasattr(ctypes.CDLL(mil_amd.LIB_PATH), name)
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    ARG, UNSUPPORTED = 1, 2
    big = 46341                                                                                  # 46341^2 > 2^31 - 1
    assert lib.mil_stain_affine_u8(None, p, p, 1, 4, 4, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, None, p, 1, 4, 4, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, None, 1, 4, 4, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, p, -1, 4, 4, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, p, 1, 0, 4, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, p, 1, 4, 0, 0, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, p, 1, 4, 4, 2, None) == ARG
    assert lib.mil_stain_affine_u8(p, p, p, 1, big, big, 0, None) == UNSUPPORTED
    assert lib.mil_stain_affine_u8(p, p, p, 0, 4, 4, 1, None) == 0                               # T == 0: no launch
    assert lib.mil_od_moments_u8(None, p, 1, 4, 4, 0.15, 0, p, 4096, p, None) == ARG
    assert lib.mil_od_moments_u8(p, p, 1, 4, 4, 0.15, 2, p, 4096, p, None) == ARG
    assert lib.mil_od_moments_u8(p, p, 1, 4, 4, float("nan"), 0, p, 4096, p, None) == ARG
    assert lib.mil_od_moments_u8(p, p, 1, 4, 4, 0.15, 0, p, 16 * 10 * 8 - 1, p, None) == ARG     # a workspace too small
    assert lib.mil_od_moments_u8(p, p, 1, 4, 4, 0.15, 0, None, 4096, p, None) == ARG
    assert lib.mil_od_moments_u8(p, p, 1, big, big, 0.15, 0, p, 4096, p, None) == UNSUPPORTED
    assert lib.mil_od_moments_u8(p, p, 0, 4, 4, 0.15, 0, p, 0, p, None) == 0
    assert lib.mil_od_project_u8(p, p, None, 1, 4, 4, 0, 0.15, p, p, None) == ARG
    assert lib.mil_od_project_u8(p, p, p, 1, 4, 4, 2, 0.15, p, p, None) == ARG
    assert lib.mil_od_project_u8(p, p, p, 1, 4, 4, 0, 0.15, None, p, None) == ARG
    assert lib.mil_od_project_u8(p, p, p, 1, 4, 4, 0, 0.15, p, None, None) == ARG
    assert lib.mil_od_project_u8(p, p, p, -1, 4, 4, 0, 0.15, p, p, None) == ARG
    assert lib.mil_od_project_u8(p, p, p, 1, big, big, 1, 0.15, p, p, None) == UNSUPPORTED
    assert lib.mil_od_project_u8(p, p, p, 0, 4, 4, 1, 0.15, p, p, None) == 0
