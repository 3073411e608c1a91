"""H&E stain normalisation and stain jitter on the device.  The reference's slides come from many staining batches and its only
colour handling is an HSV tissue filter and the commented-out `ColorJitter` line (RoiBuilder.py:200); the two standard tools of
the field are
  * stain normalisation (Macenko et al. 2009): map every slide onto one reference appearance before the encoder sees it, and
  * stain augmentation (Tellez et al. 2018, "HED jitter"): perturb the haematoxylin and eosin amounts, not hue and saturation.
Both are ONE affine map in optical-density space, od' = A od + b per pixel (`StainAffine`), applied in place to the resized
bytes of a `U8Tiles` stack by `mil_stain_affine_u8` (csrc/stain.hip) under a byte contract that has an exact numpy restatement
(`ops.od_tables`: od = L[byte], byte = #{k : od <= TH[k]}; no exp on the device).  The Macenko fit takes its tissue moments
(`ops.od_moments`), its two projections (`ops.od_project`) and its percentiles (`ops.map_quantile`) on the device; the 3 x 3
eigen-decomposition and the 3 x 2 pseudo-inverse stay on the host, in fp64.

Instead of the angle atan2(p_1, p_0) in the plane of the two leading eigenvectors the fit ranks the ratio p_1 / p_0: with
p_0 > 0 the angle is monotone in it, so the order statistics are the same pixels; only the interpolation between two adjacent
order statistics is taken in tan instead of in the angle.  Tissue pixels with p_0 <= 0 are dropped and counted (`n_dropped`).

`StainNormalizer(method="vahadane")` fits the same two vectors as the dictionary of a sparse non-negative factorisation of the
tissue pixels' ODs (Vahadane et al. 2016): `ops.od_snmf_fit` enqueues every coding pass and every dictionary update from one C
call and the host reads the result back once; what follows the fit (pseudo-inverse, concentration percentiles, the affine map)
is Macenko's tail unchanged."""
import collections
import math

import numpy as np
import torch

from . import ops
from .preprocess import U8Tiles

# Ruifrok & Johnston's fixed basis: the COLUMNS are the haematoxylin, eosin and DAB vectors (the normalised rows of their matrix)
_RUIFROK = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]], dtype=np.float64)
HED = (_RUIFROK / np.linalg.norm(_RUIFROK, axis=1, keepdims=True)).T.copy()
HED.setflags(write=False)

StainJitterParams = collections.namedtuple("StainJitterParams", ["alpha", "beta"])
StainJitterParams.__doc__ = """Per tile, on the host, fp64: `alpha` [n,3] the factors of the three stain amounts, `beta` [n,3] what is
added to them."""


def _finite(a, shape, name):
    try:
        a = np.array(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must hold numbers") from None
    if a.shape[-len(shape):] != shape or a.ndim not in (len(shape), len(shape) + 1):
        raise ValueError(f"{name} must be [{', '.join(map(str, shape))}] or [n, {', '.join(map(str, shape))}], got {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{name} holds a non-finite entry")
    return a.reshape((-1,) + shape)


class StainAffine:
    """od' = A od + b per pixel: A fp64 [n,3,3], b fp64 [n,3] on the host — one map per tile, or n = 1 for one map shared by a
    stack.  Non-finite entries raise ValueError."""

    def __init__(self, A, b=None):
        self.A = _finite(A, (3, 3), "A")
        self.b = np.zeros((len(self.A), 3)) if b is None else _finite(b, (3,), "b")
        if len(self.A) != len(self.b) or len(self.A) < 1:
            raise ValueError(f"A holds {len(self.A)} maps and b {len(self.b)}")

    def __len__(self):
        return len(self.A)

    @staticmethod
    def identity(n=1):
        return StainAffine(np.broadcast_to(np.eye(3), (int(n), 3, 3)), np.zeros((int(n), 3)))

    def then(self, other):
        """The map that applies `self` first and `other` after it, composed in fp64: A = A_o A_s, b = A_o b_s + b_o.  One of
        the two may be shared (n = 1)."""
        if not isinstance(other, StainAffine):
            raise ValueError(f"then() takes a StainAffine, got {type(other).__name__}")
        if len(self) != len(other) and 1 not in (len(self), len(other)):
            raise ValueError(f"cannot compose {len(self)} maps with {len(other)}")
        return StainAffine(other.A @ self.A, (other.A @ self.b[..., None])[..., 0] + other.b)

    def params(self):
        """fp32 [n,12] on the host, rows A[i,0], A[i,1], A[i,2], b[i]: what `ops.stain_affine` takes."""
        p = np.concatenate([self.A, self.b[:, :, None]], axis=2).reshape(len(self), 12)
        return torch.from_numpy(p).to(torch.float32)


def checked_affine(affine, n):
    """`affine` when it is a StainAffine for a stack of `n` tiles (n maps or one); ValueError otherwise."""
    if not isinstance(affine, StainAffine):
        raise ValueError(f"expected a StainAffine, got {type(affine).__name__}")
    if len(affine) not in (1, n):
        raise ValueError(f"{len(affine)} stain maps for {n} tiles")
    if not bool(torch.isfinite(affine.params()).all()):
        raise ValueError("the stain map overflows fp32")
    return affine


def _device_tiles(tiles, what):
    """The uint8 stack of a `U8Tiles` on the GPU; the refusals of the colour jitter, before any launch."""
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"{what} works on U8Tiles (TilePreprocessor(..., out='u8')), got {type(tiles).__name__}")
    return tiles.u8


def _on_gpu(u8, what):
    if not u8.is_cuda:
        raise RuntimeError(f"{what} runs on an AMD GPU only (no CPU fallback)")
    return u8


def apply_stain(tiles, affine):
    """Maps the `U8Tiles` in place with the `StainAffine` (shared, or one map per tile) and returns the handle; every refusal
    comes before a launch."""
    u8 = _device_tiles(tiles, "the stain map")
    checked_affine(affine, len(tiles))
    _on_gpu(u8, "the stain map")
    ops.stain_affine(u8, affine.params())
    return tiles


def _unit(v):
    return v / np.linalg.norm(v)


class StainFit:
    """What a stain fit finds: `stains` fp64 [3,2], unit columns, haematoxylin first (the column with the larger red-channel
    OD); `max_conc` [2], the `conc_q`-th percentile of each stain's concentration over the tissue pixels; `n_tissue`, the tissue
    pixels of the fit; `n_dropped`, those of them left out of Macenko's ranking because p_0 <= 0 (0 for a Vahadane fit).  A
    Vahadane fit also carries, read-only, `objective` (fp64 [iters]: the factorisation's objective before each update) and
    `last_move` (the largest change of an entry of the dictionary in the last iteration); both are None otherwise."""

    def __init__(self, stains, max_conc, n_tissue=0, n_dropped=0, *, objective=None, last_move=None):
        self.stains = _finite(stains, (3, 2), "stains")[0]
        self.max_conc = _finite(max_conc, (2,), "max_conc")[0]
        if abs(np.linalg.norm(self.stains, axis=0) - 1.0).max() > 1e-3:
            raise ValueError("the stain vectors must be unit columns")
        self.n_tissue, self.n_dropped = int(n_tissue), int(n_dropped)
        self._objective = None if objective is None else np.array(objective, dtype=np.float64).reshape(-1)
        if self._objective is not None:
            self._objective.setflags(write=False)
        self._last_move = None if last_move is None else float(last_move)

    @property
    def objective(self):
        return self._objective

    @property
    def last_move(self):
        return self._last_move

    @staticmethod
    def reference():
        """The published Macenko target appearance (its four-digit vectors as printed: unit to 1e-4)."""
        return StainFit([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]], [1.9705, 1.0308])

    def basis(self):
        """fp64 [3,3]: the two stains and, third, the normalised cross product of them."""
        return np.column_stack([self.stains, _unit(np.cross(self.stains[:, 0], self.stains[:, 1]))])

    def __repr__(self):
        return f"StainFit(stains={self.stains.tolist()}, max_conc={self.max_conc.tolist()}, n_tissue={self.n_tissue}, n_dropped={self.n_dropped})"


# ---- the host side of the fit: fp64 numpy on ten sums and four percentiles ----------------------------------------------------
def fit_plane(moments):
    """P fp64 [2,3] from the ten tissue sums (count, sum od_c, sum od_c od_d for rr rg rb gg gb bb): the two leading
    eigenvectors of the OD covariance (`numpy.linalg.eigh`), the leading one first, signed so that its components sum to a
    positive number; the second signed so that its component of largest magnitude is positive."""
    m = np.asarray(moments, dtype=np.float64)
    n, s = m[0], m[1:4]
    ss = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    cov = (ss - np.outer(s, s) / n) / (n - 1.0)
    _, v = np.linalg.eigh(cov)
    e0, e1 = v[:, 2], v[:, 1]
    e0 = e0 if e0.sum() > 0 else -e0
    e1 = e1 if e1[np.argmax(np.abs(e1))] > 0 else -e1
    return np.stack([e0, e1])


def stains_from_ratios(P, r_lo, r_hi):
    """The two stain vectors [3,2] from the plane P (as the device used it: rounded to fp32) and the two extreme ratios:
    unit(e0 + r e1), haematoxylin — the larger red-channel OD — first."""
    p = np.asarray(P, dtype=np.float32).astype(np.float64)
    a, b = _unit(p[0] + float(r_lo) * p[1]), _unit(p[0] + float(r_hi) * p[1])
    return np.column_stack([a, b] if a[0] > b[0] else [b, a])


def effective_q(q, n_valid, n_total):
    """The percentile to ask `ops.map_quantile` for over a map of n_total values of which n_total - n_valid are +inf (they sort
    last), so that it is the q-th percentile of the valid ones: q (n_valid - 1) / (n_total - 1), stepped down while the
    kernel's own position (n_total - 1) * (q_eff / 100) would pass the last valid value."""
    if n_valid == n_total:
        return float(q)
    qe = float(q) * (n_valid - 1) / (n_total - 1)
    while (n_total - 1) * (qe / 100.0) > n_valid - 1:
        qe = math.nextafter(qe, 0.0)
    return qe


def percentile_from_stats(s_lo, s_hi, q_eff, n_total):
    """numpy's linear percentile from the two order statistics `ops.map_quantile` brackets it with (its `stats[:, 2:4]`), in
    fp64 as the kernel forms it — vi = (n_total - 1) (q_eff / 100), t = vi - floor(vi); s_lo + (s_hi - s_lo) t for t < 0.5,
    s_hi - (s_hi - s_lo) (1 - t) otherwise — except that t == 0 returns s_lo itself: the kernel's own p is inf * 0 there when
    s_lo is the last valid value and s_hi the first +inf."""
    vi = (n_total - 1) * (q_eff / 100.0)
    t = vi - math.floor(vi)
    s_lo, s_hi = float(s_lo), float(s_hi)
    if t == 0.0:
        return s_lo
    d = s_hi - s_lo
    return s_lo + d * t if t < 0.5 else s_hi - d * (1.0 - t)


STAIN_METHODS = ("macenko", "vahadane")
SNMF_MIN_SIN2 = 1e-3            # a Vahadane fit whose columns have 1 - (W_0 . W_1)^2 below this (within 1.8 degrees) is refused


def snmf_start(init):
    """The fp64 [3,2] dictionary a Vahadane fit starts from: "hed" (Ruifrok's haematoxylin and eosin columns of `HED`), a
    `StainFit` (its stains: a Macenko fit can be polished) or a 3 x 2 array.  A negative entry or a column that is not unit to
    1e-3 (the `StainFit` rule) raises ValueError."""
    if isinstance(init, str):
        if init != "hed":
            raise ValueError(f"init must be 'hed', a StainFit or a 3 x 2 array, got {init!r}")
        return HED[:, :2].copy()
    W = init.stains.copy() if isinstance(init, StainFit) else _finite(init, (3, 2), "init")
    if W.ndim == 3:
        if len(W) != 1:
            raise ValueError(f"init must be one 3 x 2 dictionary, got {W.shape}")
        W = W[0]
    if (W < 0).any() or abs(np.linalg.norm(W, axis=0) - 1.0).max() > 1e-3:
        raise ValueError("init must have non-negative unit columns")
    return W


class StainNormalizer:
    """Stain normalisation for `U8Tiles` on the GPU: `fit` estimates a stack's two stain vectors and their strengths,
    `affine` turns a fit into the `StainAffine` that maps the stack onto `target`, `transform` applies it in place.  beta: the
    OD below which a pixel is background (all three channels must reach it); q: the percentile (and 100 - q) of the ratio that
    gives Macenko's two stain vectors; conc_q: the percentile of the concentrations that stands for "fully stained".
    method: "macenko" (the default: the plane of the OD covariance and two percentiles of an angle in it) or "vahadane" (the
    sparse non-negative factorisation of Vahadane et al. 2016 with penalty `lam`, `iters` iterations from `init`, see
    `snmf_start`); every other step, and the normalising map, are the same for both."""

    def __init__(self, target=None, beta=0.15, q=1.0, conc_q=99.0, *, method="macenko", lam=0.1, iters=64, init="hed"):
        self.target = StainFit.reference() if target is None else target
        if not isinstance(self.target, StainFit):
            raise ValueError(f"target must be a StainFit, got {type(self.target).__name__}")
        self.beta, self.q, self.conc_q = float(beta), float(q), float(conc_q)
        if not (self.beta >= 0.0 and math.isfinite(self.beta)) or not 0.0 < self.q < 50.0 or not 0.0 < self.conc_q <= 100.0:
            raise ValueError(f"beta must be finite and >= 0, q in (0, 50) and conc_q in (0, 100], got {beta}, {q}, {conc_q}")
        if method not in STAIN_METHODS:
            raise ValueError(f"method must be one of {STAIN_METHODS}, got {method!r}")
        self.method, self.lam, self.iters = method, float(lam), int(iters)
        if not (0.0 <= self.lam < math.inf) or self.iters < 1:
            raise ValueError(f"lam must be finite and >= 0 and iters at least 1, got {lam}, {iters}")
        self.init = snmf_start(init)

    def fit(self, tiles):
        """`StainFit` of the stack by the normaliser's `method`: Macenko's plane and percentiles, or Vahadane's factorisation."""
        if self.method == "vahadane":
            return self._fit_vahadane(tiles)
        return self._fit_macenko(tiles)

    def _fit_vahadane(self, tiles):
        """Vahadane's fit (method="vahadane"): the two stain vectors as the dictionary of a sparse non-negative factorisation of
        the tissue pixels' ODs — `ops.od_snmf_fit` runs `iters` iterations from `init` on the device and the host reads the
        dictionary, the history and the tissue count back once; the columns are ordered haematoxylin first and the tail of
        Macenko's fit (pseudo-inverse, concentration maps, conc_q percentiles) follows unchanged: two synchronisations per fit.
        Fewer than 2 tissue pixels, or a dictionary that is not finite or whose columns are collinear (1 - (W_0 . W_1)^2 below
        `SNMF_MIN_SIN2`: the two vectors within 1.8 degrees of each other), raise ValueError."""
        u8 = _on_gpu(_device_tiles(tiles, "the stain fit"), "the stain fit")
        total = u8.shape[0] * u8.shape[2] * u8.shape[3]
        if not total:
            raise ValueError("a stain fit needs at least 2 tissue pixels, the stack has 0")
        W, history, count = ops.od_snmf_fit(u8, self.init, self.lam, self.iters, self.beta)
        back = torch.cat([W.reshape(-1), history.reshape(-1), count]).cpu().numpy()
        W, history, n = back[:6].reshape(3, 2), back[6:-1].reshape(-1, 2), int(back[-1])
        if n < 2:
            raise ValueError(f"a stain fit needs at least 2 tissue pixels, the stack has {n}")
        sin2 = 1.0 - float(W[:, 0] @ W[:, 1]) ** 2
        if not (np.isfinite(W).all() and np.isfinite(history).all()) or not sin2 >= SNMF_MIN_SIN2:
            raise ValueError(f"the factorisation found no two stains: 1 - (W_0 . W_1)^2 = {sin2:.3g} (at least {SNMF_MIN_SIN2} needed)")
        stains = W if W[0, 0] > W[0, 1] else W[:, ::-1].copy()
        conc, _ = ops.od_project(u8, np.linalg.pinv(stains), "concentrations", self.beta)
        c = self._percentiles([(conc[0], self.conc_q, n), (conc[1], self.conc_q, n)], total)
        return StainFit(stains, c, n, 0, objective=history[:, 0], last_move=history[-1, 1])

    def _fit_macenko(self, tiles):
        """`StainFit` of the stack: one moments launch over the whole stack, the covariance and `numpy.linalg.eigh` on the
        host, the ratio map and its q / 100 - q percentiles, `pinv` of the stain vectors, the concentration maps and their
        conc_q percentiles.  The host steps read ten sums, a count and twice two percentiles back: four synchronisations per
        fit — a fit is made once per slide, not per step.  Fewer than 2 tissue pixels (or fewer than 2 with p_0 > 0) raise
        ValueError."""
        u8 = _on_gpu(_device_tiles(tiles, "the stain fit"), "the stain fit")
        total = u8.shape[0] * u8.shape[2] * u8.shape[3]
        m = ops.od_moments(u8, self.beta, "bag")[0].cpu().numpy() if total else np.zeros(10)
        n = int(m[0])
        if n < 2:
            raise ValueError(f"a stain fit needs at least 2 tissue pixels, the stack has {n}")
        P = fit_plane(m)
        ratio, valid = ops.od_project(u8, P, "ratio", self.beta)
        nv = int(valid.sum())
        if nv < 2:
            raise ValueError(f"a stain fit needs at least 2 tissue pixels with p_0 > 0, the stack has {nv}")
        r = self._percentiles([(ratio, self.q, nv), (ratio, 100.0 - self.q, nv)], total)
        stains = stains_from_ratios(P, r[0], r[1])
        conc, _ = ops.od_project(u8, np.linalg.pinv(stains), "concentrations", self.beta)
        c = self._percentiles([(conc[0], self.conc_q, n), (conc[1], self.conc_q, n)], total)
        return StainFit(stains, c, n, n - nv)

    @staticmethod
    def _percentiles(jobs, total):
        """[the q-th percentile of the n_valid finite values of map m for (m, q, n_valid) in jobs]: one exact radix select
        (`ops.map_quantile`, group "bag") per job, ONE read-back for all of them."""
        qs = [effective_q(q, nv, total) for _, q, nv in jobs]
        stats = torch.cat([ops.map_quantile(m, qe, "bag").stats for (m, _, _), qe in zip(jobs, qs)]).cpu().numpy()
        return [percentile_from_stats(s[2], s[3], qe, total) for s, qe in zip(stats, qs)]

    def affine(self, fit):
        """A = target.stains diag(target.max_conc / fit.max_conc) pinv(fit.stains), b = 0, as a shared `StainAffine`."""
        if not isinstance(fit, StainFit):
            raise ValueError(f"expected a StainFit, got {type(fit).__name__}")
        if not (fit.max_conc > 0).all():
            raise ValueError(f"the fit's stain strengths must be positive, got {fit.max_conc.tolist()}")
        return StainAffine(self.target.stains @ np.diag(self.target.max_conc / fit.max_conc) @ np.linalg.pinv(fit.stains))

    def transform(self, tiles, fit=None):
        """Normalises the `U8Tiles` in place (with `fit`, or with the stack's own) and returns the handle."""
        u8 = _device_tiles(tiles, "the stain normalisation")
        if fit is None:
            fit = self.fit(tiles)
        aff = self.affine(fit)
        _on_gpu(u8, "the stain normalisation")
        return apply_stain(tiles, aff)

    def separate(self, tiles, fit, *, sparse=False, lam=None):
        """fp32 [2,T,H,W]: the haematoxylin and the eosin concentration of every tissue pixel (+inf elsewhere) — the images
        colour deconvolution gives.  sparse=True: the non-negative lasso code of every pixel with the fit's stains as the
        dictionary and the penalty `lam` (None: the normaliser's) — what Vahadane's method calls the concentrations — instead
        of the pseudo-inverse's."""
        u8 = _device_tiles(tiles, "the stain separation")
        if not isinstance(fit, StainFit):
            raise ValueError(f"expected a StainFit, got {type(fit).__name__}")
        if not sparse and lam is not None:
            raise ValueError("lam belongs to sparse=True")
        lam = self.lam if lam is None else float(lam)
        if sparse and not 0.0 <= lam < math.inf:
            raise ValueError(f"lam must be finite and >= 0, got {lam}")
        _on_gpu(u8, "the stain separation")
        if sparse:
            return ops.od_project(u8, fit.stains, "sparse", self.beta, lam=lam)[0]
        return ops.od_project(u8, np.linalg.pinv(fit.stains), "concentrations", self.beta)[0]


class StainJitter:
    """Stain augmentation for `U8Tiles` on the GPU: per tile the amounts c of the three stains of `basis` R (od = R c) become
    alpha c + beta with alpha = 1 + sigma_alpha (2u - 1) and beta = sigma_beta (2u - 1), u uniform — in OD space the affine map
    A = R diag(alpha) R^-1, b = R beta.  basis: `HED` (Ruifrok's fixed vectors) or a `StainFit` (its two stains and their
    normalised cross product)."""

    def __init__(self, sigma_alpha=0.05, sigma_beta=0.01, basis=HED):
        self.sigma_alpha, self.sigma_beta = float(sigma_alpha), float(sigma_beta)
        if not (math.isfinite(self.sigma_alpha) and math.isfinite(self.sigma_beta) and self.sigma_alpha >= 0 and self.sigma_beta >= 0):
            raise ValueError(f"sigma_alpha and sigma_beta must be finite and non-negative, got {sigma_alpha}, {sigma_beta}")
        self.R = basis.basis() if isinstance(basis, StainFit) else _finite(basis, (3, 3), "basis")[0]
        if not abs(np.linalg.det(self.R)) > 1e-6:
            raise ValueError("the stain basis is singular")
        self.Rinv = np.linalg.inv(self.R)

    def draw_params(self, n, generator=None):
        """`StainJitterParams` for n tiles from ONE `torch.rand(n, 6, dtype=float64)` draw u: alpha = 1 + sigma_alpha (2 u[:, :3]
        - 1), beta = sigma_beta (2 u[:, 3:] - 1)."""
        u = torch.rand((n, 6), dtype=torch.float64, generator=generator)
        return StainJitterParams(1.0 + self.sigma_alpha * (2.0 * u[:, :3] - 1.0), self.sigma_beta * (2.0 * u[:, 3:] - 1.0))

    def affine(self, params, n=None):
        """The per-tile `StainAffine` of `params` (a StainJitterParams or any (alpha [n,3], beta [n,3]) pair), in fp64; with
        `n`, the number of tiles they must be for.  A wrong shape or a non-finite entry raises ValueError."""
        try:
            alpha, beta = params
        except (TypeError, ValueError):
            raise ValueError("stain jitter parameters are (alpha [n,3], beta [n,3])") from None
        alpha, beta = _finite(alpha, (3,), "alpha"), _finite(beta, (3,), "beta")
        if len(alpha) != len(beta) or (n is not None and len(alpha) != n) or len(alpha) < 1:
            raise ValueError(f"expected alpha and beta [{'n' if n is None else n},3], got {alpha.shape} and {beta.shape}")
        A = self.R[None] @ (alpha[:, :, None] * self.Rinv[None])
        return StainAffine(A, beta @ self.R.T)

    def apply(self, tiles, params):
        """tiles: `U8Tiles` on the GPU, params: `draw_params(len(tiles))` or injected ones.  Jitters in place and returns the
        handle.  Not `U8Tiles`: ValueError; bad parameters: ValueError; CPU tiles: RuntimeError — all before any launch."""
        _device_tiles(tiles, "the stain jitter")
        if len(tiles) == 0:
            return tiles
        return apply_stain(tiles, self.affine(params, len(tiles)))

    def __call__(self, tiles, generator=None):
        _device_tiles(tiles, "the stain jitter")
        return self.apply(tiles, self.draw_params(len(tiles), generator))
