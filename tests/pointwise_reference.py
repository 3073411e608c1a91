"""fp64 numpy references, with derived error bounds, for the small kernels every training step runs around the convolutions:
max-pool, global average pool + linear, the linear layer's weight gradient and Adam (`mil_maxpool_*`, `mil_avgpool_fc_*`,
`mil_fc_wgrad`, `mil_adam_step` in include/mil_hip.h).  Written from the operations as include/mil_hip.h and torch state them
(`MaxPool2d(3, 2, 1)`, `AdaptiveAvgPool2d(1)` + `Linear`, `torch.optim.Adam`), not from the kernels.  numpy only; nothing of the
package is imported.  tests/test_cpu_pointwise_bounds.py checks the bounds in both directions, tests/test_gpu_pointwise.py holds
the kernels to them, element by element.

The bounds.  u = 2^-24.  A sum of m fp32 terms, each of which went through k further fp32 operations, is within (m + k) u of the
exact value RELATIVE TO THE SUM OF THE TERMS' MAGNITUDES, in any summation order and with or without fused multiply-adds; a factor
2 covers the second-order terms.  Nothing is relative to the result, so cancelling sums stay covered.  A kernel that stores bf16
adds one round-to-nearest on top: 2^-8 (|ref| + bound)  (`store_bound`).  Every tensor is the array the kernel reads (channel-
padded NHWC for maps), as float32 or float64 values; bf16 inputs are float arrays that hold bf16 values (`to_bf16`).

  maxpool          y, first-maximum tap in (ky, kx) scan order, "winner <= 0" bit           exact
  maxpool_bwd      gx and 4 u sum|gy|                  (at most four windows: three additions and the product by the slope)
  avgpool_fc_fwd   pooled: 2 (hw + 1) u mean|x|        feats: 2 (hw + C + 3) u (|bias| + sum_i mean_p|x| |W|)
  avgpool_fc_bwd   g = dfeats W / hw: 2 (NF + 2) u sum_o |df||W| / hw; dz = g lrelu'(act), the factor (1 or the slope) is exact
  fc_wgrad         dW: 2 (n + 1) u sum_t |df||pooled|, dbias: 2 (n + 1) u sum_t |df|;  accumulating: + u |previous + sum|
  adam_step        see its docstring

The second half of the file lists the cases of the GPU tests and builds their inputs, so that the CPU test runs its fp32
restatements on exactly the arrays the kernels get."""
import zlib

import numpy as np

U = 2.0 ** -24
BF16_U = 2.0 ** -8            # (__bf16)float rounds to nearest: half a unit in the 8th significant bit


def to_bf16(x):
    """float32 array -> float32 array of the nearest bf16 values (ties to even)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def store_bound(ref, bound, bf16):
    """The bound of a value that is then stored as bf16 (or as fp32: unchanged)."""
    return bound + BF16_U * (np.abs(ref) + bound) if bf16 else bound


# ---- MaxPool2d(3, stride 2, pad 1) ------------------------------------------------------------------------------------------
def _pool_out(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def maxpool(x):
    """x [n,H,W,c] -> (y float64 [n,Ho,Wo,c], tap uint8, neg bool): -inf padding; among equal maxima the FIRST in (ky, kx) scan
    order wins (torch); tap = ky * 3 + kx; neg = the winner is <= 0."""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    ho, wo = _pool_out(h, w)
    xp = np.full((n, 2 * ho + 1, 2 * wo + 1, c), -np.inf)
    xp[:, 1:h + 1, 1:w + 1] = x
    best = np.full((n, ho, wo, c), -np.inf)
    tap = np.zeros((n, ho, wo, c), dtype=np.uint8)
    for ky in range(3):
        for kx in range(3):
            v = xp[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2]
            take = v > best
            best = np.where(take, v, best)
            tap = np.where(take, np.uint8(ky * 3 + kx), tap)
    return best, tap, best <= 0


def maxpool_bwd(gy, tap, neg, slope, use_mask, in_hw, bf16=False):
    """gx [n,H,W,c] = sum over the windows whose winner is this pixel of gy, times the slope where use_mask and the winner is
    <= 0 -> (gx, bound).  slope is rounded to fp32 first: the C ABI takes a float."""
    gy = np.asarray(gy, dtype=np.float64)
    n, ho, wo, c = gy.shape
    h, w = in_hw
    assert (ho, wo) == _pool_out(h, w) and tap.shape == gy.shape == neg.shape
    f = np.where(neg, float(np.float32(slope)), 1.0) if use_mask else np.ones_like(gy)
    gx = np.zeros((n, 2 * ho + 1, 2 * wo + 1, c))
    mag = np.zeros_like(gx)
    for ky in range(3):
        for kx in range(3):
            sel = tap == ky * 3 + kx
            gx[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] += np.where(sel, gy * f, 0.0)
            mag[:, ky:ky + 2 * ho:2, kx:kx + 2 * wo:2] += np.where(sel, np.abs(gy), 0.0)
    gx, mag = gx[:, 1:h + 1, 1:w + 1], mag[:, 1:h + 1, 1:w + 1]
    return gx, store_bound(gx, 4 * U * mag, bf16)


# ---- AdaptiveAvgPool2d(1) + Linear -------------------------------------------------------------------------------------------
def avgpool_fc_fwd(x, wfc, bias, c):
    """x [n,h,w,cp] (or [n,hw,cp]), wfc [nf,c], bias [nf] or None -> (pooled [n,c], pooled_bound, feats [n,nf], feats_bound)."""
    x = np.asarray(x, dtype=np.float64)
    x = x.reshape(x.shape[0], -1, x.shape[-1])[..., :c]
    w = np.asarray(wfc, dtype=np.float64)
    nf = w.shape[0]
    b = np.zeros(nf) if bias is None else np.asarray(bias, dtype=np.float64)
    hw = x.shape[1]
    pooled, amean = x.mean(axis=1), np.abs(x).mean(axis=1)
    feats = pooled @ w.T + b
    mag = np.abs(b) + amean @ np.abs(w).T
    return pooled, 2 * (hw + 1) * U * amean, feats, 2 * (hw + c + 3) * U * mag


def avgpool_fc_bwd(dfeats, wfc, act, c, slope, masked, bf16=False):
    """dz [n,h,w,cp] = (dfeats @ wfc) / hw, times lrelu'(act) when masked (act > 0: 1, else the slope: an input of exactly 0 takes
    the slope); padded channels 0 -> (dz, bound)."""
    act = np.asarray(act, dtype=np.float64)
    df, w = np.asarray(dfeats, dtype=np.float64), np.asarray(wfc, dtype=np.float64)
    n, cp = act.shape[0], act.shape[-1]
    hw = int(np.prod(act.shape[1:-1]))
    nf = w.shape[0]
    expand = (n,) + (1,) * (act.ndim - 2) + (c,)
    g = (df @ w / hw).reshape(expand)
    gb = (2 * (nf + 2) * U * (np.abs(df) @ np.abs(w)) / hw).reshape(expand)
    f = np.where(act[..., :c] > 0, 1.0, float(np.float32(slope))) if masked else np.ones_like(act[..., :c])
    dz, bound = np.zeros_like(act), np.zeros_like(act)
    dz[..., :c] = g * f
    bound[..., :c] = store_bound(g * f, gb * np.abs(f), bf16)
    return dz, bound


def fc_wgrad(dfeats, pooled, prev_w=None, prev_b=None):
    """dW [nf,c] = dfeats^T pooled, dbias [nf] = column sums of dfeats, each added to prev_* when given
    -> (dW, dW_bound, dbias, dbias_bound)."""
    df, p = np.asarray(dfeats, dtype=np.float64), np.asarray(pooled, dtype=np.float64)
    n = df.shape[0]
    dw, db = df.T @ p, df.sum(axis=0)
    dwb = 2 * (n + 1) * U * (np.abs(df).T @ np.abs(p))
    dbb = 2 * (n + 1) * U * np.abs(df).sum(axis=0)
    if prev_w is not None:
        dw = dw + np.asarray(prev_w, dtype=np.float64)
        dwb = dwb + U * np.abs(dw)
    if prev_b is not None:
        db = db + np.asarray(prev_b, dtype=np.float64)
        dbb = dbb + U * np.abs(db)
    return dw, dwb, db, dbb


# ---- Adam ----------------------------------------------------------------------------------------------------------------------
def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale):
    """One step of torch.optim.Adam (no amsgrad; L2 decay folded into the gradient; the gradient multiplied by grad_scale first)
    in fp64, with the hyper-parameters rounded to fp32 (the C ABI takes floats: that is the operation the kernel is asked for):

        gi = g s + wd p;   m' = b1 m + (1 - b1) gi;   v' = b2 v + (1 - b2) gi^2
        p' = p - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

    -> dict(m, v, p, m_bound, v_bound, p_bound).  The bounds, with w = 2 u for "first order, times 2" and every error relative to
    magnitudes (G = |g s| + |wd p| for the gradient, so a decay term that cancels the gradient stays covered):

      gi   two products and an addition: a leaf sees 2 roundings                       e_gi = 2 w G
      m'   (1 - b1) is exact in fp32 (Sterbenz); product, addition                    e_m  = 4 w (b1 |m| + (1 - b1) G)
      v'   gi twice (2 + 2), two products, the addition                               e_v  = 7 w (b2 |v| + (1 - b2) G^2)
      1 - b^t   formed in fp32: pow to an ulp, then the subtraction cancels          r_b  = w (b^t / (1 - b^t) + 1)   (relative)
                (b2^t / (1 - b2^t) is 1000 at t = 1); sqrt(1 - b2^t): r_b2 / 2 + w
      sqrt(v')  |sqrt(a + e) - sqrt(a)| <= min(sqrt|e|, |e| / sqrt(a)), plus its rounding
      D = sqrt(v') / sqrt(1 - b2^t) + eps      e_D = e_sqrt / sqrt(bc2) + q (r_b2 / 2 + 2 w) + w D,  q = sqrt(v') / sqrt(bc2)
      R = m' / D          |m_c / D_c - m' / D| <= e_m / D_low + |m'| e_D / (D D_low) + w |R|,  D_low = max(D - e_D, eps (1 - w)):
                          the computed denominator is never below eps (1 - u)
      T = (lr / bc1) R    e_T = (lr / bc1)(1 + r_A) e_R + (r_A + w) |T|,  r_A = r_b1 + w
      p' = p - T          p_bound = e_T + w max(|p|, |p'|)

    An fp32 numpy restatement of the same formulas stays at or below about 1.0 x (u |p| + e_T) on the cases below (printed by
    tests/test_cpu_pointwise_bounds.py), which is why the subtraction gets 2 u |p| and not u |p|."""
    f32 = lambda a: float(np.float32(a))
    lr, b1, b2, eps, wd, s = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay), f32(grad_scale)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    w = 2 * U
    gs, wp = g * s, wd * p
    gi, G = gs + wp, np.abs(gs) + np.abs(wp)
    m2 = b1 * m + (1 - b1) * gi
    v2 = b2 * v + (1 - b2) * gi * gi
    e_m = 4 * w * (b1 * np.abs(m) + (1 - b1) * G)
    e_v = 7 * w * (b2 * np.abs(v) + (1 - b2) * G * G)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    r1, r2 = w * (b1 ** step / bc1 + 1), w * (b2 ** step / bc2 + 1)
    sv, sb = np.sqrt(v2), np.sqrt(bc2)
    with np.errstate(divide="ignore", invalid="ignore"):
        e_sv = np.where(sv > 0, np.minimum(np.sqrt(e_v), e_v / sv), np.sqrt(e_v)) + w * sv
    q = sv / sb
    D = q + eps
    e_D = e_sv / sb + q * (r2 / 2 + 2 * w) + w * D
    D_low = np.maximum(D - e_D, eps * (1 - w))
    R = m2 / D
    e_R = e_m / D_low + np.abs(m2) * e_D / (D * D_low) + w * np.abs(R)
    A, r_A = lr / bc1, r1 + w
    T = A * R
    e_T = A * (1 + r_A) * e_R + (r_A + w) * np.abs(T)
    p2 = p - T
    return dict(m=m2, v=v2, p=p2, m_bound=e_m, v_bound=e_v, p_bound=e_T + w * np.maximum(np.abs(p), np.abs(p2)), update_bound=e_T)


# ================================================================================================================================
# The cases of tests/test_gpu_pointwise.py and their inputs (float32 arrays; with bf16=True they hold bf16 values).
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def cpad(c):
    return (c + 7) // 8 * 8


def _padded(a, cp):
    out = np.zeros(a.shape[:-1] + (cp,), dtype=np.float32)
    out[..., :a.shape[-1]] = a
    return out


MAXPOOL_SHAPES = [(2, 20, 1, 1), (2, 20, 1, 5), (3, 20, 2, 2), (2, 20, 7, 9), (3, 20, 25, 35),          # (n, c, H, W); cp 24
                  (2, 64, 3, 4), (1, 64, 5, 5), (2, 64, 16, 16)]                                         # cp 64: the wide encoder
MAXPOOL_KINDS = ["lrelu", "relu"]
MAXPOOL_SLOPES = [0.1, 0.0]


def maxpool_inputs(shape, kind, bf16):
    """-> x [n,H,W,cp], gy [n,Ho,Wo,cp] (padded channels 0).  "lrelu": a LeakyReLU-like map quantised to halves (ties, zeros,
    windows without a positive value); "relu": the same clamped at 0, so most windows tie at 0."""
    n, c, h, w = shape
    r = _rng("maxpool", shape, kind)
    x = np.round(r.standard_normal((n, h, w, c)) * 2) / 2
    x = np.where(x < 0, x / 2 if kind == "lrelu" else 0.0, x)              # halves and quarters: exact in bf16
    x[r.random(x.shape) < 0.1] = 0.0
    if h * w > 4:
        x[0, :3, :3, :2] = -0.5                                            # a window with no positive value in every kind
        if kind == "relu":
            x[0, :3, :3, :2] = 0.0
    ho, wo = _pool_out(h, w)
    gy = r.standard_normal((n, ho, wo, c)).astype(np.float32)
    x, gy = _padded(x, cpad(c)), _padded(gy, cpad(c))
    return (to_bf16(x), to_bf16(gy)) if bf16 else (x, gy)


# (n, h, w, C, CP, NF, bias): PCH = 4096 / CP pixels are staged at a time (51 at CP 80, 8 at CP 512); C = 512 takes 512 threads
POOLFC_CASES = ([(5, 8, 8, 80, 80, 80, False), (1, 1, 1, 80, 80, 80, False)]
                + [(3, 1, hw, 80, 80, 80, False) for hw in (50, 51, 52, 103)]
                + [(2, 7, 9, 20, 24, 80, False), (2, 4, 4, 64, 64, 10, True)]
                + [(3, 1, hw, 512, 512, 80, True) for hw in (7, 8, 9, 17)]
                + [(2, 2, 3, 512, 512, 3, True)])


def poolfc_slope(case):
    """0.1 as the 80-channel encoder calls the kernels, 0.0 as alt_resnet does (C = 64 and C = 512)."""
    return 0.1 if case[3] in (20, 80) else 0.0


def poolfc_inputs(case, bf16):
    """-> x [n,h,w,CP] with exact zeros (and non-negative for slope 0: a ReLU output), wfc [NF,C], bias [NF] or None, dfeats."""
    n, h, w, c, cp, nf, has_bias = case
    r = _rng("poolfc", case)
    x = r.standard_normal((n, h, w, c))
    if poolfc_slope(case) == 0.0:
        x = np.maximum(x, 0.0)
    x[r.random(x.shape) < 0.1] = 0.0
    x = _padded(x.astype(np.float32), cp)
    wfc = (r.standard_normal((nf, c)) / np.sqrt(c)).astype(np.float32)
    bias = r.standard_normal(nf).astype(np.float32) if has_bias else None
    df = r.standard_normal((n, nf)).astype(np.float32)
    return (to_bf16(x) if bf16 else x), wfc, bias, df


FCW_SHAPES = [(80, 80), (512, 80), (64, 10)]          # (C, NF)
FCW_N = [1, 63, 64, 65, 129, 300]                     # 64-row slices: below, at and above one and two of them, several
FCW_MAX_NF_AT_512 = 127                               # 64 rows of [dfeats | pooled | 1] in 160 KiB of LDS: (NF + 512 + 2) & ~1 <= 640


def fcw_inputs(c, nf, n):
    """-> dfeats [n,nf], pooled [n,c], prev_w [nf,c], prev_b [nf] (the non-zero contents accumulated into)."""
    r = _rng("fcw", c, nf, n)
    return (r.standard_normal((n, nf)).astype(np.float32), r.standard_normal((n, c)).astype(np.float32),
            r.standard_normal((nf, c)).astype(np.float32), r.standard_normal(nf).astype(np.float32))


ADAM_N = [1, 255, 257, 4096 * 256 + 257]              # the launch is capped at 4096 x 256 threads: the last size wraps the loop
ADAM_WD_SCALE = [(0.0, 1.0), (0.01, 0.25), (0.1, 1.0 / 3.0)]
ADAM_STEPS = [1, 2, 3, 10, 1000]
ADAM_HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8)
# elements with g = 0; p = 0; g = m = v = p = 0; g = m = v = 0 (sizes of 255 and more; index = position from the end + 1)
ADAM_SPECIAL = dict(g0=-1, p0=-2, all0=-3, gmv0=-4)


def adam_inputs(n):
    """-> p, g, m, v: gradients of either sign spanning 1e-6 .. 10, moments of that scale, v >= 0."""
    r = _rng("adam", n)
    mag = 10.0 ** r.uniform(-6, 1, n)
    g = (mag * r.choice([-1.0, 1.0], n)).astype(np.float32)
    p = (r.standard_normal(n) * 0.1).astype(np.float32)
    m = (mag * r.standard_normal(n) * 0.5).astype(np.float32)
    v = (mag * mag * r.uniform(0.1, 2.0, n)).astype(np.float32)
    if n >= 255:
        g[ADAM_SPECIAL["g0"]] = 0.0
        p[ADAM_SPECIAL["p0"]] = 0.0
        for a in (p, g, m, v):
            a[ADAM_SPECIAL["all0"]] = 0.0
        for a in (g, m, v):
            a[ADAM_SPECIAL["gmv0"]] = 0.0
    return p, g, m, v
