"""numpy restatement of `mil_pixel_blur` (include/mil_hip.h), written from the header and not from the kernel: a separable
symmetric filter over planes [..., H, W], the horizontal pass first, each pass
    acc = w[0] * v[0];   for k = 1 .. radius:   acc = acc + w[k] * (v[-k] + v[+k])
as single fp32 operations on numpy fp32 arrays (numpy never fuses a product into a sum), the samples outside a line taken at the
source index of the edge rule.  `blur64` is the same filter as two `scipy.ndimage.correlate1d` calls in fp64."""
import numpy as np

EDGES = ("reflect", "replicate", "wrap")
SCIPY_MODES = {"reflect": "mirror", "replicate": "nearest", "wrap": "wrap"}
MAX_RADIUS = 16
U = 2.0 ** -24                                    # the unit roundoff of fp32


def gauss_taps(sigma):
    """(radius, fp64 w[0..radius]): scipy.ndimage's Gaussian kernel at truncate=4.0, its centre and one half."""
    radius = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1)
    p = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    p = p / p.sum()
    return radius, p[radius:]


def source_index(i, n, edge):
    """The source index of the samples i (an integer array, any values the rule is defined for) of a line of length n."""
    i = np.asarray(i)
    if edge == "reflect":
        assert i.min() >= -(n - 1) and i.max() <= 2 * (n - 1), "reflect needs radius <= n - 1"
        i = np.where(i < 0, -i, i)
        return np.where(i > n - 1, 2 * (n - 1) - i, i)
    if edge == "replicate":
        return np.clip(i, 0, n - 1)
    assert edge == "wrap"
    return np.mod(i, n)


def filter_pass(x, w, axis, edge):
    """One pass along `axis` of the fp32 array x with the fp32 taps w[0..radius], in the header's order."""
    assert x.dtype == np.float32 and w.dtype == np.float32
    n, at = x.shape[axis], np.arange(x.shape[axis])

    def v(d):
        return np.take(x, source_index(at + d, n, edge), axis=axis)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = w[0] * v(0)
        for k in range(1, len(w)):
            acc = acc + w[k] * (v(-k) + v(k))
    assert acc.dtype == np.float32
    return acc


def pixel_blur(x, taps, edge):
    """out fp32 like x [..., H, W]: the taps (any numbers w[0..radius]) rounded to fp32, along W, then along H."""
    w = np.asarray(taps, dtype=np.float64).astype(np.float32)
    assert 1 <= len(w) - 1 <= MAX_RADIUS
    x = np.ascontiguousarray(x, dtype=np.float32)
    return filter_pass(filter_pass(x, w, x.ndim - 1, edge), w, x.ndim - 2, edge)


def blur64(x, taps, edge):
    """The same filter in fp64 with the fp64 taps: `scipy.ndimage.correlate1d` along W, then along H, in the scipy mode of the edge."""
    from scipy import ndimage
    half = np.asarray(taps, dtype=np.float64)
    full = np.concatenate([half[:0:-1], half])
    x = np.asarray(x, dtype=np.float64)
    y = ndimage.correlate1d(x, full, axis=x.ndim - 1, mode=SCIPY_MODES[edge])
    return ndimage.correlate1d(y, full, axis=x.ndim - 2, mode=SCIPY_MODES[edge])


def error_bound(x, taps, edge):
    """The bound on |pixel_blur - blur64| per element.  A term of a pass goes through at most the tap's rounding to fp32, one sum
    of the pair, one product and `radius` additions: radius + 3 roundings, so one pass lies within gamma (|w| (*) |x|) of the
    exact pass, gamma = (radius + 3) u / (1 - (radius + 3) u).  The second pass filters values that carry the first one's relative
    error and adds its own: both together lie within ((1 + gamma)^2 - 1) B|x|, B|x| the two fp64 correlations of |x| with |w|."""
    radius = len(taps) - 1
    gamma = (radius + 3) * U / (1 - (radius + 3) * U)
    return ((1 + gamma) ** 2 - 1) * blur64(np.abs(np.asarray(x, dtype=np.float64)), np.abs(np.asarray(taps, dtype=np.float64)), edge)
