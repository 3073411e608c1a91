"""The numpy restatement of the stain kernels' contracts (include/mil_hip.h: mil_stain_affine_u8, mil_od_moments_u8,
mil_od_project_u8) and of the host layer built on them (mil_amd/stain.py), with no torch device code: what
tests/test_gpu_stain.py holds the device to, bit for bit where the contract is one, and what tests/test_cpu_stain.py holds to
the fp64 formulas.  fp32 arithmetic is numpy float32 arithmetic: every product and sum rounded once, nothing fused."""
import math

import numpy as np

REFERENCE_STAINS = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]])
REFERENCE_MAX_CONC = np.array([1.9705, 1.0308])
RUIFROK = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]])
HED = (RUIFROK / np.linalg.norm(RUIFROK, axis=1, keepdims=True)).T


def tables():
    """(L fp32 [256], TH fp32 [256] with TH[0] = +inf standing for "always"): fp64 `math.log`, rounded once."""
    L = np.array([-math.log((v + 1) / 256.0) for v in range(256)]).astype(np.float32)
    TH = np.array([math.inf] + [-math.log((k + 0.5) / 256.0) for k in range(1, 256)]).astype(np.float32)
    return L, TH


L, TH = tables()
_TH_ASC = TH[1:][::-1].copy()


def od_byte(o):
    """byte(o) = #{k in 1..255 : o <= TH[k]} for an fp32 array; a NaN gives 0."""
    o = np.asarray(o, dtype=np.float32)
    return (255 - np.searchsorted(_TH_ASC, o, side="left")).astype(np.uint8)      # a NaN sorts last: 255 - 255


def od_byte_by_count(o):
    """The same by the definition's comparison count (for small arrays)."""
    o = np.asarray(o, dtype=np.float32)
    return (o[..., None] <= TH[1:]).sum(axis=-1).astype(np.uint8)


def _od(tiles):
    t = np.asarray(tiles)
    assert t.dtype == np.uint8 and t.ndim == 4 and t.shape[1] == 3
    return L[t[:, 0]], L[t[:, 1]], L[t[:, 2]]


def stain_affine(tiles, params):
    """uint8 [T,3,H,W] through the fp32 maps params [T,12] or [1,12] (rows A[i,0..2], b[i])."""
    p = np.asarray(params, dtype=np.float32)
    lr, lg, lb = _od(tiles)
    p = np.broadcast_to(p, (len(lr), 12))[:, :, None, None]
    out = np.empty_like(np.asarray(tiles))
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(3):
            o = ((p[:, 4 * i] * lr + p[:, 4 * i + 1] * lg) + p[:, 4 * i + 2] * lb) + p[:, 4 * i + 3]
            assert o.dtype == np.float32
            out[:, i] = od_byte(o)
    return out


def tissue(tiles, beta):
    lr, lg, lb = _od(tiles)
    b = np.float32(beta)
    return (lr >= b) & (lg >= b) & (lb >= b)


def od_moment_terms(tiles, beta):
    """[10] lists of the exact fp64 terms of the tissue pixels of the stack (count terms are ones)."""
    lr, lg, lb = (x.astype(np.float64) for x in _od(tiles))
    m = tissue(tiles, beta)
    x, y, z = lr[m], lg[m], lb[m]
    return [np.ones(x.size), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]


def od_moments(tiles, beta, bag):
    """fp64 [G,10] with every sum correctly rounded (`math.fsum`)."""
    tiles = np.asarray(tiles)
    groups = [tiles] if bag else [tiles[i:i + 1] for i in range(len(tiles))]
    return np.array([[math.fsum(v) for v in od_moment_terms(g, beta)] for g in groups]).reshape(len(groups), 10)


def od_project(tiles, P, mode, beta):
    """(maps, valid): mode 0 fp32 [2,T,H,W], mode 1 fp32 [T,H,W]; +inf where no value is written."""
    P = np.asarray(P, dtype=np.float64).astype(np.float32)
    lr, lg, lb = _od(tiles)
    p0 = (P[0, 0] * lr + P[0, 1] * lg) + P[0, 2] * lb
    p1 = (P[1, 0] * lr + P[1, 1] * lg) + P[1, 2] * lb
    m = tissue(tiles, beta)
    inf = np.float32(np.inf)
    if mode == 0:
        maps = np.stack([np.where(m, p0, inf), np.where(m, p1, inf)])
    else:
        m = m & (p0 > 0)
        maps = np.full(p0.shape, inf, dtype=np.float32)
        maps[m] = p1[m] / p0[m]
    assert maps.dtype == np.float32
    return maps, m.sum(axis=(1, 2)).astype(np.int32)


def effective_q(q, n_valid, n_total):
    if n_valid == n_total:
        return float(q)
    qe = float(q) * (n_valid - 1) / (n_total - 1)
    while (n_total - 1) * (qe / 100.0) > n_valid - 1:
        qe = math.nextafter(qe, 0.0)
    return qe


def percentile_of_valid(m, q, n_valid):
    """The q-th percentile of the finite values of a map as the device takes it: numpy's linear method (`np.percentile`'s
    arithmetic, restated) over ALL values, +inf sorting last, at the effective percentile; a position that falls exactly on an
    order statistic returns it (np.percentile itself gives inf * 0 when the next one is +inf)."""
    s = np.sort(np.asarray(m, dtype=np.float32).reshape(-1)).astype(np.float64)
    vi = (s.size - 1) * (effective_q(q, n_valid, s.size) / 100.0)
    lo = int(math.floor(vi))
    hi, t = min(lo + 1, s.size - 1), vi - lo
    if t == 0.0:
        return float(s[lo])
    d = s[hi] - s[lo]
    return float(s[lo] + d * t if t < 0.5 else s[hi] - d * (1.0 - t))


def unit(v):
    return v / np.linalg.norm(v)


def fit_plane(m):
    n, s = m[0], m[1:4]
    ss = np.array([[m[4], m[5], m[6]], [m[5], m[7], m[8]], [m[6], m[8], m[9]]])
    cov = (ss - np.outer(s, s) / n) / (n - 1.0)
    _, v = np.linalg.eigh(cov)
    e0, e1 = v[:, 2], v[:, 1]
    e0 = e0 if e0.sum() > 0 else -e0
    e1 = e1 if e1[np.argmax(np.abs(e1))] > 0 else -e1
    return np.stack([e0, e1])


def _nudged(P, nudge, which):
    """P rounded to fp32, with entry nudge[1:3] moved by nudge[3] ulps when nudge[0] == which."""
    P = np.asarray(P, dtype=np.float64).astype(np.float32)
    if nudge is not None and nudge[0] == which:
        _, k, j, d = nudge
        P[k, j] = np.nextafter(P[k, j], np.float32(np.inf if d > 0 else -np.inf))
    return P


def fit(tiles, beta=0.15, q=1.0, conc_q=99.0, moments=None, nudge=None):
    """Macenko's fit as mil_amd.StainNormalizer.fit makes it: dict(stains [3,2], max_conc [2], n_tissue, n_dropped).  moments:
    the ten sums to use in place of the correctly rounded ones; nudge = (which P, row, column, +-1): one entry of the first (0)
    or second (1) fp32 projection moved by one ulp — both for the sensitivity measurements."""
    m = od_moments(tiles, beta, True)[0] if moments is None else np.asarray(moments, dtype=np.float64)
    n = int(m[0])
    if n < 2:
        raise ValueError("fewer than 2 tissue pixels")
    P = _nudged(fit_plane(m), nudge, 0)
    ratio, valid = od_project(tiles, P, 1, beta)
    nv = int(valid.sum())
    if nv < 2:
        raise ValueError("fewer than 2 tissue pixels with p_0 > 0")
    r_lo, r_hi = percentile_of_valid(ratio, q, nv), percentile_of_valid(ratio, 100.0 - q, nv)
    p = P.astype(np.float64)
    a, b = unit(p[0] + r_lo * p[1]), unit(p[0] + r_hi * p[1])
    stains = np.column_stack([a, b] if a[0] > b[0] else [b, a])
    conc, _ = od_project(tiles, _nudged(np.linalg.pinv(stains), nudge, 1), 0, beta)
    max_conc = np.array([percentile_of_valid(conc[k], conc_q, n) for k in (0, 1)])
    return dict(stains=stains, max_conc=max_conc, n_tissue=n, n_dropped=n - nv)


def normalizer_affine(target_stains, target_max_conc, f):
    """fp32 [1,12] of A = target.stains diag(target.max_conc / fit.max_conc) pinv(fit.stains), b = 0."""
    A = np.asarray(target_stains) @ np.diag(np.asarray(target_max_conc) / f["max_conc"]) @ np.linalg.pinv(f["stains"])
    return pack(A[None], np.zeros((1, 3)))


def jitter_affine(R, alpha, beta):
    """(A fp64 [n,3,3], b fp64 [n,3]) = (R diag(alpha) R^-1, R beta) per tile."""
    R = np.asarray(R, dtype=np.float64)
    alpha, beta = np.asarray(alpha, dtype=np.float64).reshape(-1, 3), np.asarray(beta, dtype=np.float64).reshape(-1, 3)
    Rinv = np.linalg.inv(R)
    return np.stack([R @ np.diag(a) @ Rinv for a in alpha]), beta @ R.T


def compose(A1, b1, A2, b2):
    """First (A1, b1), then (A2, b2), in fp64."""
    return A2 @ A1, (A2 @ b1[..., None])[..., 0] + b2


def pack(A, b):
    return np.concatenate([A, b[:, :, None]], axis=2).reshape(len(A), 12).astype(np.float32)


def formula_bytes(triples, A, b):
    """The fp64 formula the contract approximates: round(256 exp(-(A od + b)) - 1) clipped to 0..255, with od = -ln((v+1)/256)
    in fp64; triples uint8 [N,3]."""
    od = -np.log((triples.astype(np.float64) + 1.0) / 256.0)
    o = od @ np.asarray(A, dtype=np.float64).T + np.asarray(b, dtype=np.float64)
    return np.clip(np.rint(256.0 * np.exp(-o) - 1.0), 0, 255).astype(np.uint8)


def synthetic_tiles(shape, seed=0, stains=REFERENCE_STAINS, noise=0.01):
    """H&E-like tiles uint8 [T,3,H,W] from known stain vectors: a quarter background, a quarter mostly haematoxylin, a quarter
    mostly eosin, a quarter mixed; OD noise of `noise` per channel; bytes round(256 exp(-od) - 1).  Returns (tiles, the kind of
    every pixel 0..3)."""
    t, c, h, w = shape
    assert c == 3
    rng = np.random.default_rng(seed)
    n = t * h * w
    kind = rng.integers(0, 4, n)
    ch = np.where(kind == 1, rng.uniform(0.6, 2.0, n), np.where(kind == 2, rng.uniform(0.0, 0.04, n), rng.uniform(0.3, 1.5, n)))
    ce = np.where(kind == 2, rng.uniform(0.5, 1.2, n), np.where(kind == 1, rng.uniform(0.0, 0.04, n), rng.uniform(0.2, 1.0, n)))
    ch[kind == 0] = 0.0
    ce[kind == 0] = 0.0
    od = np.stack([ch, ce], axis=1) @ np.asarray(stains).T + rng.normal(0.0, noise, (n, 3))
    by = np.clip(np.rint(256.0 * np.exp(-od) - 1.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(by.reshape(t, h, w, 3).transpose(0, 3, 1, 2)), kind.reshape(t, h, w)


def angle_deg(a, b):
    return float(np.degrees(np.arccos(np.clip(abs(unit(a) @ unit(b)), -1.0, 1.0))))
