"""CPU (-m "not gpu"): Vahadane's stain fit without a GPU — the numpy restatement
tests/stain_snmf_reference.py against a brute-force lasso, against the generating stain vectors, against scikit-learn's
dictionary learning and against its own perturbations (the measurements the GPU gates of tests/test_gpu_stain_snmf.py rest on),
the host layer's refusals and the C entries' host-side status codes."""
import ctypes
import inspect
import warnings

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import _lib, ops
from mil_amd import stain as st

import stain_reference as sr
import stain_snmf_reference as sn

START = sr.HED[:, :2]
# what tests/test_gpu_stain_snmf.py allows between the device's fit and the restated one (stains absolute, max_conc relative):
# forty times the largest move measured in test_fit_sensitivity below (3.8e-7), section 3.49's rule
GPU_GATE = 1.6e-5
# the relative rise of the objective from one iteration to the next that the fp32 coder may cause near convergence: measured
# at most 2.4e-12 (the all-fp64 prototype needed 0); forty times that
RISE_SLACK = 1e-10


def _unit_columns(rng, n):
    W = rng.uniform(0.0, 1.0, (n, 3, 2))
    W[rng.uniform(size=(n, 3, 2)) < 0.15] = 0.0
    W[:, 0, :] += 1e-3                                                    # no zero column
    return W / np.linalg.norm(W, axis=1, keepdims=True)


# ---- the coder -----------------------------------------------------------------------------------------------------------------
def test_coder_is_the_minimiser_of_the_nonnegative_lasso():
    """The closed form against the fp64 minimum over the four active sets, on random non-negative unit dictionaries and ODs,
    for penalties that make every branch and q <= 0 occur.  The coder works in fp32: its objective may exceed the fp64
    minimum by the rounding of h, about 2^-23 |h| |v| — 1e-5 absolute covers ODs up to 5.5 with two decades to spare."""
    rng = np.random.default_rng(0)
    n = 1500
    Ws = _unit_columns(rng, n)
    vs = rng.uniform(0.0, 2.5, (n, 3)) * (rng.uniform(size=(n, 1)) < 0.9)
    vs[rng.uniform(size=n) < 0.3] *= 0.05                                 # small ODs: q <= 0 on one or both stains
    seen, nonpos = set(), 0
    for W, v, lam in zip(Ws, vs, rng.choice([0.0, 0.02, 0.1, 0.5], n)):
        if 1.0 - float(W[:, 0] @ W[:, 1]) ** 2 < 1e-6:                    # collinear columns are the degenerate case, tested below
            continue
        k = sn.coder(W, lam)
        a0, a1, branch = sn.code(np.float32(v[0]), np.float32(v[1]), np.float32(v[2]), k)
        v32 = v.astype(np.float32).astype(np.float64)
        h = np.array([float(a0), float(a1)])
        assert (h >= 0).all()
        r = v32 - W @ h
        got = 0.5 * float(r @ r) + float(np.float32(lam)) * h.sum()
        want, hb = sn.lasso_bruteforce(v32, W, float(np.float32(lam)))
        assert got <= want + 1e-5, (W.tolist(), v.tolist(), lam, h, hb)
        if 1.0 - float(W[:, 0] @ W[:, 1]) ** 2 > 1e-2:                    # a well-conditioned dictionary: the codes agree too
            assert np.abs(h - hb).max() <= 1e-3, (W.tolist(), v.tolist(), lam, h, hb)
        seen.add(int(branch))
        nonpos += int(h.max() == 0.0)
    assert seen == {0, 1, 2} and nonpos > 20


def test_degenerate_dictionaries_code_to_zero():
    """Collinear columns: d = 0, every code is (+-0, +-0), every sum 0, the update leaves W alone — and no NaN anywhere."""
    tiles, _ = sr.synthetic_tiles((2, 3, 16, 12), seed=4)
    W = np.stack([START[:, 0], START[:, 0]], axis=1)
    k = sn.coder(W, 0.1)
    assert k[7] == 0.0 and ops.snmf_coder(W, 0.1).numpy()[7] == 0.0
    s = sn.sums(tiles, k, 0.15)
    assert s[0] > 100 and (s[1:] == 0).all()
    W2, f, move = sn.update(W, s, 3.0, 0.1)
    assert np.array_equal(W2, W) and f == 1.5 and move == 0.0
    maps, _ = sn.sparse_maps(tiles, W, 0.1, 0.15)
    assert not np.isnan(maps).any() and (maps[np.isfinite(maps)] == 0).all()
    with pytest.raises(ValueError):
        sn.fit(tiles, W0=W)
    # the host's coder is the restatement's, bit for bit
    for W in _unit_columns(np.random.default_rng(3), 50):
        assert np.array_equal(ops.snmf_coder(W, 0.07).numpy().view(np.int32), sn.coder(W, 0.07).view(np.int32))


# ---- the fit ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    """The restated fits the tests below share: {(shape, noise): (tiles, fit)} at lam = 0.1, 64 iterations from Ruifrok's columns."""
    out = {}
    for shape, noise in (((4, 3, 32, 32), 0.01), ((4, 3, 64, 64), 0.01), ((4, 3, 64, 64), 0.05)):
        tiles, _ = sr.synthetic_tiles(shape, seed=1, noise=noise)
        out[shape, noise] = (tiles, sn.fit(tiles, lam=0.1, iters=64))
    return out


def test_objective_never_rises(fits):
    for key in (((4, 3, 32, 32), 0.01), ((4, 3, 64, 64), 0.01)):
        o = fits[key][1]["objective"]
        rise = max((o[i + 1] - o[i]) / abs(o[i]) for i in range(len(o) - 1))
        print(f"{key}: objective {o[0]:.6g} -> {o[-1]:.6g}, largest relative rise {rise:.3g}")
        assert o[-1] < 0.9 * o[0] and rise <= RISE_SLACK


def test_fit_recovers_the_generating_stains(fits):
    """Angles to REFERENCE_STAINS (H / E) measured with this restatement at lam = 0.1: 0.815 / 1.349 degrees at noise 0.01 and
    0.282 / 1.691 at noise 0.05 (Macenko's fit: 0.626 / 0.664 and 4.444 / 2.959).  Gated at 1.5 times those."""
    for noise, measured in ((0.01, (0.815, 1.349)), (0.05, (0.282, 1.691))):
        tiles, f = fits[(4, 3, 64, 64), noise]
        got = [sr.angle_deg(f["stains"][:, k], sr.REFERENCE_STAINS[:, k]) for k in (0, 1)]
        mac = sr.fit(tiles)
        mac = [sr.angle_deg(mac["stains"][:, k], sr.REFERENCE_STAINS[:, k]) for k in (0, 1)]
        print(f"noise {noise}: vahadane {got[0]:.3f} / {got[1]:.3f} degrees, macenko {mac[0]:.3f} / {mac[1]:.3f}")
        assert got[0] <= 1.5 * measured[0] and got[1] <= 1.5 * measured[1]
        assert f["stains"][0, 0] > f["stains"][0, 1] and f["n_dropped"] == 0 and f["last_move"] < 1e-6
        if noise == 0.05:
            assert got[0] < mac[0] and got[1] < mac[1]


def test_fit_agrees_with_sklearn_dictionary_learning():
    """An independent solver of the same objective, started from the same dictionary, ends at the same minimum: scikit-learn's
    coordinate-descent dictionary learning (columns renormalised) within 0.01 degrees — ten times the 1e-3 measured."""
    skd = pytest.importorskip("sklearn.decomposition")
    tiles, _ = sr.synthetic_tiles((2, 3, 24, 20), seed=3, noise=0.02)
    lam = 0.1
    W, hist, n = sn.snmf(tiles, START, lam, iters=160)
    assert hist[-1, 1] < 1e-7 and n > 400
    lr, lg, lb = sn.tissue_od(tiles, 0.15)
    V = np.stack([lr, lg, lb], axis=1).astype(np.float64)
    a0, a1, _ = sn.code(lr, lg, lb, sn.coder(START, lam))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dl = skd.DictionaryLearning(n_components=2, alpha=lam, max_iter=1000, tol=1e-10, fit_algorithm="cd", transform_algorithm="lasso_cd",
                                    positive_code=True, positive_dict=True, dict_init=START.T.copy(),
                                    code_init=np.stack([a0, a1], axis=1).astype(np.float64), random_state=0)
        dl.fit(V)
    D = dl.components_.T
    angles = [sr.angle_deg(W[:, k], D[:, k]) for k in (0, 1)]
    print(f"vahadane restated against sklearn: {angles[0]:.3g} / {angles[1]:.3g} degrees")
    assert max(angles) <= 0.01


@pytest.mark.parametrize("shape", [(3, 3, 16, 12), (4, 3, 32, 32)])
def test_fit_sensitivity(shape):
    """What GPU_GATE rests on.  The device's fit differs from the restated one through the summation order of the twelve sums
    of every iteration (2^-52-sized, taken here a thousand times larger: 1e-12 relative) and, when such a change carries an
    entry of W across an fp32 rounding boundary, through one ulp of that entry in a coding pass — worst in the last one, which
    no later iteration contracts.  Measured, with the ulp applied in iteration 0, 30 or 63 of 64: sums at 1e-12 move stains by 1.2e-12 and max_conc not at all; one ulp of an entry
    moves stains by at most 1.3e-7 and max_conc by 3.8e-7 (relative).  GPU_GATE is forty times the larger."""
    tiles, _ = sr.synthetic_tiles(shape, seed=2)
    base = sn.fit(tiles)
    moved = {"ulp": [0.0, 0.0], "sums": [0.0, 0.0]}

    def note(kind, f):
        assert f["n_tissue"] == base["n_tissue"]
        moved[kind][0] = max(moved[kind][0], float(np.abs(f["stains"] - base["stains"]).max()))
        moved[kind][1] = max(moved[kind][1], float(np.abs(f["max_conc"] / base["max_conc"] - 1.0).max()))

    for it in (0, 30, 63):
        for entry in range(6):
            for d in (1, -1):
                note("ulp", sn.fit(tiles, nudge=(it, entry, d)))
    for seed in range(3):
        note("sums", sn.fit(tiles, perturb=(1e-12, np.random.default_rng(seed))))
    print(f"{shape}: one ulp of W moves stains by {moved['ulp'][0]:.3g}, max_conc by {moved['ulp'][1]:.3g} (relative); "
          f"sums at 1e-12: {moved['sums'][0]:.3g}, {moved['sums'][1]:.3g}")
    assert max(moved["ulp"] + moved["sums"]) * 40 <= GPU_GATE


# ---- the host layer ----------------------------------------------------------------------------------------------------------------
def test_normalizer_arguments_and_refusals():
    norm = mil_amd.StainNormalizer(method="vahadane")
    assert (norm.method, norm.lam, norm.iters) == ("vahadane", 0.1, 64) and np.array_equal(norm.init, sr.HED[:, :2])
    default = mil_amd.StainNormalizer()
    assert default.method == "macenko"
    assert list(inspect.signature(default.fit).parameters) == ["tiles"]
    assert list(inspect.signature(mil_amd.StainNormalizer).parameters)[:4] == ["target", "beta", "q", "conc_q"]
    with pytest.raises(TypeError):
        mil_amd.StainNormalizer(None, 0.15, 1.0, 99.0, "vahadane")                                # keyword-only
    ref = mil_amd.StainFit.reference()
    assert np.array_equal(mil_amd.StainNormalizer(method="vahadane", init=ref).init, ref.stains)
    assert np.array_equal(mil_amd.StainNormalizer(method="vahadane", init=START.tolist()).init, START)
    bad_cols = START.copy()
    bad_cols[:, 1] *= 1.1
    neg = START.copy()
    neg[2, 0] = -neg[2, 0]
    for kw in (dict(method="reinhard"), dict(lam=-0.1), dict(lam=float("nan")), dict(lam=float("inf")), dict(iters=0),
               dict(init="ruifrok"), dict(init=bad_cols), dict(init=neg), dict(init=np.eye(3)), dict(init=np.full((3, 2), np.nan))):
        with pytest.raises(ValueError):
            mil_amd.StainNormalizer(**{"method": "vahadane", **kw})
    # StainFit: the positional signature stays; the history is read-only
    f = mil_amd.StainFit(sr.REFERENCE_STAINS, [1.0, 2.0], 7, 1)
    assert (f.n_tissue, f.n_dropped, f.objective, f.last_move) == (7, 1, None, None)
    g = mil_amd.StainFit(sr.REFERENCE_STAINS, [1.0, 2.0], 7, objective=[3.0, 2.0], last_move=1e-9)
    assert g.objective.tolist() == [3.0, 2.0] and g.last_move == 1e-9 and not g.objective.flags.writeable
    with pytest.raises(AttributeError):
        g.objective = None
    with pytest.raises(TypeError):
        mil_amd.StainFit(sr.REFERENCE_STAINS, [1.0, 2.0], 7, 1, [3.0])
    # refusals before any launch: CPU tiles, wrong types, bad lam
    cpu = mil_amd.U8Tiles(torch.zeros((2, 3, 8, 6), dtype=torch.uint8))
    raw = torch.zeros((2, 3, 8, 6), dtype=torch.uint8)
    for call in (lambda: norm.fit(raw), lambda: norm.separate(cpu, ref, sparse=True, lam=-1.0), lambda: norm.separate(cpu, ref, lam=0.1),
                 lambda: norm.separate(raw, ref, sparse=True),
                 lambda: ops.od_snmf_sums(raw, START, -0.1), lambda: ops.od_snmf_sums(raw, np.zeros((2, 3)), 0.1),
                 lambda: ops.od_snmf_sums(raw, np.full((3, 2), np.inf), 0.1), lambda: ops.od_snmf_sums(raw, START, 0.1, float("nan")),
                 lambda: ops.od_snmf_sums(raw, START, 0.1),                                        # a CPU stack
                 lambda: ops.od_snmf_fit(raw, START, 0.1, 0), lambda: ops.od_snmf_fit(raw, START, float("nan"), 4),
                 lambda: ops.od_snmf_fit(raw.float(), START, 0.1, 4), lambda: ops.od_snmf_fit(raw, START, 0.1, 4),
                 lambda: ops.od_project(raw, START, "sparse"), lambda: ops.od_project(raw, START, "sparse", lam=-1.0),
                 lambda: ops.od_project(raw, np.zeros((2, 3)), "ratio", lam=0.1), lambda: ops.od_project(raw, START, "sparse", lam=0.1)):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: norm.fit(cpu), lambda: norm.transform(cpu), lambda: norm.separate(cpu, ref, sparse=True)):
        with pytest.raises(RuntimeError):
            call()


def test_entry_status_codes_need_no_gpu():
    lib = mil_amd.lib()
    for name in ("mil_od_snmf_sums_u8", "mil_od_snmf_fit_u8", "mil_od_code_u8"):
        assert name in _lib.EXPORTS and hasattr(ctypes.CDLL(mil_amd.LIB_PATH), name)
    ARG, UNSUPPORTED = 1, 2
    p = ctypes.addressof(ctypes.create_string_buffer(64))              # never dereferenced: every call below returns first
    big = 46341
    one = 16 * 12 * 8                                                   # the slice sums of one tile, in bytes
    assert lib.mil_od_snmf_sums_u8(None, p, p, 1, 4, 4, 0.15, p, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, None, 1, 4, 4, 0.15, p, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, 4, 4, 0.15, None, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, 4, 4, 0.15, p, one, None, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, -1, 4, 4, 0.15, p, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, 0, 4, 0.15, p, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, 4, 4, float("nan"), p, one, p, None) == ARG
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, 4, 4, 0.15, p, one - 1, p, None) == ARG            # a workspace too small
    assert lib.mil_od_snmf_sums_u8(p, p, p, 1, big, big, 0.15, p, one, p, None) == UNSUPPORTED
    extra = 20 * 8
    fit = lib.mil_od_snmf_fit_u8
    assert fit(None, p, p, p, 1, 4, 4, 0.1, 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, None, p, 1, 4, 4, 0.1, 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, None, 1, 4, 4, 0.1, 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, 0.1, 4, 0.15, None, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, 0.1, 4, 0.15, p, one + extra, None, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, -0.1, 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, float("nan"), 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, float("inf"), 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, 0.1, 0, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, 0.1, 4, float("nan"), p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, -1, 4, 4, 0.1, 4, 0.15, p, one + extra, p, None) == ARG
    assert fit(p, p, p, p, 1, 4, 4, 0.1, 4, 0.15, p, one + extra - 1, p, None) == ARG             # a workspace too small
    assert fit(p, p, p, p, 1, big, big, 0.1, 4, 0.15, p, one + extra, p, None) == UNSUPPORTED
    assert lib.mil_od_code_u8(p, p, None, 1, 4, 4, 0.15, p, p, None) == ARG
    assert lib.mil_od_code_u8(p, p, p, 1, 4, 4, 0.15, None, p, None) == ARG
    assert lib.mil_od_code_u8(p, p, p, 1, 4, 4, float("nan"), p, p, None) == ARG
    assert lib.mil_od_code_u8(p, p, p, -1, 4, 4, 0.15, p, p, None) == ARG
    assert lib.mil_od_code_u8(p, p, p, 1, big, big, 0.15, p, p, None) == UNSUPPORTED
    assert lib.mil_od_code_u8(p, p, p, 0, 4, 4, 0.15, p, p, None) == 0                            # T == 0: no launch
    assert lib.mil_od_project_u8(p, p, p, 1, 4, 4, 2, 0.15, p, p, None) == ARG                    # "sparse" has its own entry
