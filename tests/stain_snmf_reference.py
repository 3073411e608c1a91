"""The numpy restatement of Vahadane's stain fit as the device makes it (include/mil_hip.h: mil_od_snmf_sums_u8,
mil_od_snmf_fit_u8, mil_od_code_u8): the closed-form two-variable non-negative lasso code in float32
with one rounding per operation, the twelve sums correctly rounded (`math.fsum`), the dictionary update in fp64 with the
operation order written out, and the fit built from them.  Tables, tissue and percentiles are tests/stain_reference.py's."""
import math

import numpy as np

import stain_reference as sr

F = np.float32
TERMS = 12
MIN_SIN2 = 1e-3


def coder(W, lam):
    """float32 [9]: W row-major rounded to fp32, c = W_0 . W_1 and d = 1 / (1 - c c) formed in fp64 (python floats, the
    header's order; d = 0 for collinear columns) and rounded once, lam."""
    w = [float(v) for v in np.asarray(W, dtype=np.float64).reshape(6)]
    c = (w[0] * w[1] + w[2] * w[3]) + w[4] * w[5]
    e = 1.0 - c * c
    d = 1.0 / e if e > 0.0 else 0.0
    return np.array(w + [c, d, float(lam)], dtype=np.float64).astype(F)


def code(lr, lg, lb, k):
    """(h0, h1) float32 for float32 OD arrays and the coder's nine values k; every operation rounded once."""
    lr, lg, lb = (np.asarray(x, dtype=F) for x in (lr, lg, lb))
    k = np.asarray(k, dtype=F)
    q0 = ((k[0] * lr + k[2] * lg) + k[4] * lb) - k[8]
    q1 = ((k[1] * lr + k[3] * lg) + k[5] * lb) - k[8]
    h0 = (q0 - k[6] * q1) * k[7]
    h1 = (q1 - k[6] * q0) * k[7]
    z = F(0)
    both = (h0 >= z) & (h1 >= z)
    first = ~both & (h1 < z)
    a0 = np.where(both, h0, np.where(first, np.where(q0 > z, q0, z), z))
    a1 = np.where(both, h1, np.where(first, z, np.where(q1 > z, q1, z)))
    assert a0.dtype == F and a1.dtype == F
    branch = np.where(both, 0, np.where(first, 1, 2))
    return a0, a1, branch


def tissue_od(tiles, beta):
    """The float32 ODs (L[r], L[g], L[b]) of the tissue pixels of the stack."""
    lr, lg, lb = sr._od(tiles)
    m = sr.tissue(tiles, beta)
    return lr[m], lg[m], lb[m]


def sparse_maps(tiles, W, lam, beta):
    """(maps float32 [2,T,H,W], valid int32 [T]): the code of every tissue pixel, +inf elsewhere."""
    lr, lg, lb = sr._od(tiles)
    a0, a1, _ = code(lr, lg, lb, coder(W, lam))
    m = sr.tissue(tiles, beta)
    inf = F(np.inf)
    return np.stack([np.where(m, a0, inf), np.where(m, a1, inf)]), m.sum(axis=(1, 2)).astype(np.int32)


def sum_terms(tiles, k, beta):
    """[12] arrays of the exact fp64 terms over the tissue pixels: ones, h0 h0, h0 h1, h1 h1, v_c h_j (r0 r1 g0 g1 b0 b1), h0, h1."""
    lr, lg, lb = tissue_od(tiles, beta)
    a0, a1, _ = code(lr, lg, lb, k)
    h0, h1 = a0.astype(np.float64), a1.astype(np.float64)
    x, y, z = (v.astype(np.float64) for v in (lr, lg, lb))
    return [np.ones(h0.size), h0 * h0, h0 * h1, h1 * h1, x * h0, x * h1, y * h0, y * h1, z * h0, z * h1, h0, h1]


def sums(tiles, k, beta):
    """fp64 [12], every sum correctly rounded."""
    return np.array([math.fsum(t) for t in sum_terms(tiles, k, beta)])


def sv2_of(moments):
    m = [float(v) for v in moments]
    return (m[4] + m[7]) + m[9]


def update(W, s, sv2, lam):
    """One dictionary update in fp64 (python floats: one rounding per operation, in the header's order) from the twelve sums:
    (new W [3,2], objective of the W coded with, largest |change of an entry|).  lam: the fp32 penalty the coder used."""
    w = [float(v) for v in np.asarray(W, dtype=np.float64).reshape(6)]
    s = [float(v) for v in s]
    lam = float(F(lam))
    old = list(w)
    A = [[s[1], s[2]], [s[2], s[3]]]
    n00 = (w[0] * w[0] + w[2] * w[2]) + w[4] * w[4]
    n01 = (w[0] * w[1] + w[2] * w[3]) + w[4] * w[5]
    n11 = (w[1] * w[1] + w[3] * w[3]) + w[5] * w[5]
    wb = (w[0] * s[4] + w[2] * s[6]) + w[4] * s[8]
    wb = ((wb + w[1] * s[5]) + w[3] * s[7]) + w[5] * s[9]
    quad = (A[0][0] * n00 + (2.0 * A[0][1]) * n01) + A[1][1] * n11
    f = ((sv2 * 0.5 - wb) + quad * 0.5) + lam * (s[10] + s[11])
    for j in (0, 1):
        ajj = A[j][j]
        if not ajj > 0.0:
            continue
        u = []
        for c in range(3):
            wa = w[2 * c] * A[0][j] + w[2 * c + 1] * A[1][j]
            x = w[2 * c + j] + (s[4 + 2 * c + j] - wa) / ajj
            u.append(0.0 if x < 0.0 else x)
        nn = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]
        if not nn > 0.0:
            continue
        length = math.sqrt(nn)
        for c in range(3):
            w[2 * c + j] = u[c] / length
    move = max(abs(a - b) for a, b in zip(w, old))
    return np.array(w).reshape(3, 2), f, move


def snmf(tiles, W0, lam=0.1, iters=64, beta=0.15, perturb=None, nudge=None):
    """`iters` iterations from W0: (W [3,2], history [iters,2], count).  perturb = (relative size, numpy Generator): every sum
    of every iteration but the count multiplied by 1 + size * uniform(-1, 1); nudge = (iteration, entry 0..5, +-1): one fp32
    entry of the coder's W moved by one ulp in that iteration — both for the sensitivity measurements."""
    W = np.array(W0, dtype=np.float64).reshape(3, 2)
    sv2 = sv2_of(sr.od_moments(tiles, beta, True)[0])
    hist = np.zeros((iters, 2))
    count = 0
    for it in range(iters):
        k = coder(W, lam)
        if nudge is not None and nudge[0] == it:
            k[nudge[1]] = np.nextafter(k[nudge[1]], F(np.inf if nudge[2] > 0 else -np.inf))
        s = sums(tiles, k, beta)
        count = int(s[0])
        if perturb is not None:
            s[1:] = s[1:] * (1.0 + perturb[0] * perturb[1].uniform(-1, 1, TERMS - 1))
        W, hist[it, 0], hist[it, 1] = update(W, s, sv2, lam)
    return W, hist, count


def fit(tiles, W0=None, lam=0.1, iters=64, beta=0.15, conc_q=99.0, **kw):
    """Vahadane's fit as mil_amd.StainNormalizer(method="vahadane").fit makes it: dict(stains, max_conc, n_tissue, n_dropped,
    objective, last_move)."""
    W, hist, n = snmf(tiles, sr.HED[:, :2] if W0 is None else W0, lam, iters, beta, **kw)
    if n < 2:
        raise ValueError("fewer than 2 tissue pixels")
    sin2 = 1.0 - float(W[:, 0] @ W[:, 1]) ** 2
    if not np.isfinite(W).all() or not sin2 >= MIN_SIN2:
        raise ValueError("collinear stains")
    stains = W if W[0, 0] > W[0, 1] else W[:, ::-1].copy()
    conc, _ = sr.od_project(tiles, np.linalg.pinv(stains), 0, beta)
    max_conc = np.array([sr.percentile_of_valid(conc[k], conc_q, n) for k in (0, 1)])
    return dict(stains=stains, max_conc=max_conc, n_tissue=n, n_dropped=0, objective=hist[:, 0].copy(), last_move=float(hist[-1, 1]))


def lasso_bruteforce(v, W, lam):
    """The fp64 minimum of 1/2 |v - W h|^2 + lam (h0 + h1) over h >= 0 by its four active sets: (objective, h)."""
    v, W = np.asarray(v, dtype=np.float64), np.asarray(W, dtype=np.float64)

    def obj(h):
        r = v - W @ h
        return 0.5 * float(r @ r) + lam * float(h.sum())

    cands = [np.zeros(2)]
    for j in (0, 1):
        h = np.zeros(2)
        h[j] = max((W[:, j] @ v - lam) / (W[:, j] @ W[:, j]), 0.0)
        cands.append(h)
    G = W.T @ W
    if abs(np.linalg.det(G)) > 1e-14:
        h = np.linalg.solve(G, W.T @ v - lam)
        if (h >= 0).all():
            cands.append(h)
    best = min(cands, key=obj)
    return obj(best), best
