"""CPU (-m "not gpu"): the Gaussian blur without a GPU — the numpy restatement of `mil_pixel_blur` against scipy within a derived
bound, the taps against scipy's kernel, the status codes of the entry point, and every argument check of `ops.pixel_blur`,
`mil_amd.gaussian_blur` and the blur options of `mil_amd.PixelRegularizer`, which fire on CPU tensors before anything is launched."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import pixel_blur_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMAS = [0.125, 0.25, 1.0, 2.3, 4.0]
SHAPES = [(1, 1), (1, 9), (3, 40), (5, 7), (17, 17), (33, 37), (50, 70)]


@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("sigma", SIGMAS)
def test_the_restatement_against_scipy_within_the_derived_bound(sigma, edge):
    """`scipy.ndimage.correlate1d` along W, then along H, on the fp64 copy with the fp64 taps, in the scipy mode of the edge.

    The bound is derived, not measured.  A term of one pass goes through at most the tap's rounding to fp32, one sum of the pair,
    one product and `radius` additions — radius + 3 roundings — so the pass lies within gamma (|w| (*) |x|) of the exact one, with
    gamma = (radius + 3) u / (1 - (radius + 3) u) and u = 2^-24.  The second pass filters values that carry that relative error
    and adds its own, so both lie within ((1 + gamma)^2 - 1) B|x|, where B|x| is the same two fp64 correlations of |x|
    (`pixel_blur_reference.error_bound`).  Reflect needs radius <= min(H, W) - 1: the shapes it cannot take are skipped for it
    alone; wrap and replicate take every shape, radius >= n included."""
    radius, taps = ref.gauss_taps(sigma)
    worst = 0.0
    for h, w in SHAPES:
        if edge == "reflect" and radius > min(h, w) - 1:
            continue
        rng = np.random.default_rng(1000 * h + w)
        x = (rng.standard_normal((2, h, w)) * 10.0 ** rng.integers(-3, 3, (2, 1, 1))).astype(np.float32)
        got = ref.pixel_blur(x, taps, edge)
        assert got.dtype == np.float32 and got.shape == x.shape
        want, bound = ref.blur64(x, taps, edge), ref.error_bound(x, taps, edge)
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= bound).all(), (h, w, float((err / bound).max()))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"restatement[sigma={sigma}, {edge}]: radius {radius}, worst error / bound {worst:.3f}")
    assert worst > 0.0


def test_the_source_index_maps_are_the_three_padding_rules():
    """Against numpy's own padding of a ramp: reflect is np.pad's "reflect" (the edge sample not repeated), replicate "edge", wrap
    "wrap" — also for a halo longer than the line, which reflect does not take."""
    for n, r in ((7, 6), (5, 4), (9, 1)):
        line = np.arange(n)
        for edge, mode in (("reflect", "reflect"), ("replicate", "edge"), ("wrap", "wrap")):
            assert np.array_equal(ref.source_index(np.arange(-r, n + r), n, edge), np.pad(line, r, mode=mode)), (n, r, edge)
    for edge, mode in (("replicate", "edge"), ("wrap", "wrap")):
        assert np.array_equal(ref.source_index(np.arange(-16, 3 + 16), 3, edge), np.pad(np.arange(3), 16, mode=mode))
        assert np.array_equal(ref.source_index(np.arange(-2, 3), 1, edge), np.zeros(5, dtype=int))
    with pytest.raises(AssertionError):
        ref.source_index(np.arange(-5, 10), 5, "reflect")


@pytest.mark.parametrize("sigma", SIGMAS + [0.4, 3.3, 4.1])
def test_gauss_taps_are_scipys_kernel(sigma):
    """`ops.gauss_taps` equals the kernel `scipy.ndimage.gaussian_filter1d` applies (read off its response to a unit impulse, which
    is exact: every product is a tap times 1 or 0), and the two fp64 correlations equal `gaussian_filter(..., truncate=4.0)` within
    1e-12 relative to the largest value (scipy filters the axes in the other order)."""
    import mil_amd  # noqa: F401
    from mil_amd import ops
    radius, taps = ops.gauss_taps(sigma)
    assert radius == int(4.0 * sigma + 0.5) and taps.dtype == np.float64 and taps.shape == (radius + 1,)
    r2, t2 = ref.gauss_taps(sigma)
    assert radius == r2 and np.array_equal(taps, t2)
    impulse = np.zeros(2 * radius + 1)
    impulse[radius] = 1.0
    kernel = ndimage.gaussian_filter1d(impulse, sigma, truncate=4.0, mode="constant")
    assert np.array_equal(kernel[radius:], taps) and np.array_equal(kernel[:radius + 1][::-1], taps)
    t32 = taps.astype(np.float32)
    assert (t32 >= 2.0 ** -126).all() and np.isfinite(t32).all()                 # no tap is zero or denormal
    x = np.random.default_rng(int(sigma * 1000)).standard_normal((2, 40, 52))
    for edge in ref.EDGES:
        want = ndimage.gaussian_filter(x, (0, sigma, sigma), truncate=4.0, mode=ref.SCIPY_MODES[edge])
        assert np.abs(ref.blur64(x, taps, edge) - want).max() <= 1e-12 * np.abs(want).max()


def test_gauss_taps_refuses_a_sigma_outside_its_range():
    import mil_amd  # noqa: F401
    from mil_amd import ops
    assert ops.BLUR_EDGES == ("reflect", "replicate", "wrap") and mil_amd._lib.BLUR_MAX_RADIUS == 16
    assert ops.gauss_taps(0.125)[0] == 1 and ops.gauss_taps(4.124)[0] == 16
    for sigma in (0.0, 0.1, 0.124, 4.125, 5.0, -1.0, float("nan"), float("inf"), None, "1", True):
        with pytest.raises(ValueError, match="sigma"):
            ops.gauss_taps(sigma)


def test_the_entry_point_is_declared_bound_and_returns_status_codes_without_a_gpu():
    import mil_amd
    from mil_amd import _lib
    header = open(os.path.join(ROOT, "include", "mil_hip.h")).read()
    assert "int mil_pixel_blur(" in header and "#define MIL_BLUR_MAX_RADIUS 16" in header
    assert "mil_pixel_blur" in _lib.EXPORTS
    lib = mil_amd.lib()
    assert lib.mil_abi_version() == 2
    # mil_pixel_blur(x, out, taps, planes, H, W, radius, edge, stream): two planes of 8x8 (512 bytes)
    x, out, taps = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 512), ctypes.c_void_p(1 << 20)
    assert lib.mil_pixel_blur(None, out, taps, 2, 8, 8, 2, 0, None) == 1
    assert lib.mil_pixel_blur(x, None, taps, 2, 8, 8, 2, 0, None) == 1
    assert lib.mil_pixel_blur(x, out, None, 2, 8, 8, 2, 0, None) == 1
    assert lib.mil_pixel_blur(x, x, taps, 2, 8, 8, 2, 0, None) == 1                                  # never in place
    assert lib.mil_pixel_blur(x, ctypes.c_void_p(4096 + 508), taps, 2, 8, 8, 2, 0, None) == 1        # the last word of x
    assert lib.mil_pixel_blur(ctypes.c_void_p(4096 + 508), x, taps, 2, 8, 8, 2, 0, None) == 1
    assert lib.mil_pixel_blur(x, out, taps, -1, 8, 8, 2, 0, None) == 1
    assert lib.mil_pixel_blur(x, out, taps, 2, 0, 8, 2, 1, None) == 1
    assert lib.mil_pixel_blur(x, out, taps, 2, 8, 0, 2, 1, None) == 1
    for radius in (0, -1, 17, 100):
        assert lib.mil_pixel_blur(x, out, taps, 2, 8, 8, radius, 1, None) == 1, radius
    for edge in (-1, 3):
        assert lib.mil_pixel_blur(x, out, taps, 2, 8, 8, 2, edge, None) == 1, edge
    assert lib.mil_pixel_blur(x, out, taps, 2, 8, 8, 8, 0, None) == 1                                # reflect: radius <= n - 1
    assert lib.mil_pixel_blur(x, out, taps, 2, 8, 3, 3, 0, None) == 1
    assert lib.mil_pixel_blur(x, out, taps, 2, 3, 8, 3, 0, None) == 1
    assert lib.mil_pixel_blur(x, out, taps, 0, 1, 1, 1, 0, None) == 1                                # ... also with nothing to do
    assert lib.mil_pixel_blur(x, out, taps, 1, 32768, 32768, 2, 1, None) == 2                        # mil_pixel_shift's limit
    assert lib.mil_pixel_blur(x, out, taps, 1 << 30, 64, 65, 2, 1, None) == 2                        # 2^31 workgroups
    # nothing to do: MIL_OK without a launch, for every edge and the radii at both ends
    for edge in (0, 1, 2):
        assert lib.mil_pixel_blur(x, out, taps, 0, 64, 64, 1, edge, None) == 0
        assert lib.mil_pixel_blur(x, out, taps, 0, 64, 64, 16, edge, None) == 0
    assert lib.mil_pixel_blur(x, x, taps, 0, 8, 8, 2, 1, None) == 0                                  # no byte to overlap in
    assert lib.mil_pixel_blur(x, out, taps, 0, 1, 1, 16, 2, None) == 0                               # wrap and replicate take radius >= n
    assert lib.mil_pixel_blur(x, out, taps, 0, 1, 1, 16, 1, None) == 0


def test_pixel_blur_argument_checks_fire_on_cpu_tensors():
    import mil_amd
    from mil_amd import ops
    x = torch.zeros(2, 3, 9, 12)
    with pytest.raises(ValueError, match="exactly one"):
        ops.pixel_blur(x)
    with pytest.raises(ValueError, match="exactly one"):
        ops.pixel_blur(x, sigma=1.0, taps=[0.5, 0.25])
    for sigma in (0.0, 0.1, 4.2, float("nan"), "1"):
        with pytest.raises(ValueError, match="sigma"):
            ops.pixel_blur(x, sigma=sigma)
        with pytest.raises(ValueError, match="sigma"):
            mil_amd.gaussian_blur(x, sigma)
    for taps in ([1.0], [], [0.1] * 18, [0.5, float("nan")], [0.5, float("inf")], 0.5, ["a", "b"], None):
        with pytest.raises(ValueError, match="taps" if taps is not None else "exactly one"):
            ops.pixel_blur(x, taps=taps)
    for edge in ("mirror", "constant", 0, None):
        with pytest.raises(ValueError, match="edge"):
            ops.pixel_blur(x, sigma=1.0, edge=edge)
        with pytest.raises(ValueError, match="edge"):
            mil_amd.gaussian_blur(x, 1.0, edge=edge)
    with pytest.raises(ValueError, match="reflect"):                              # sigma 2.25: radius 9 > min(9, 12) - 1
        ops.pixel_blur(x, sigma=2.25)
    with pytest.raises(ValueError, match="reflect"):
        mil_amd.gaussian_blur(x, 2.25)
    with pytest.raises(ValueError, match="reflect"):
        ops.pixel_blur(torch.zeros(4, 12, 9), taps=[0.2] * 10)
    with pytest.raises(ValueError, match="reflect"):
        ops.pixel_blur(torch.zeros(1, 1), sigma=0.25)
    with pytest.raises(ValueError, match="fp32"):
        ops.pixel_blur(x.double(), sigma=1.0)
    with pytest.raises(ValueError, match="fp32"):
        ops.pixel_blur(x.to(torch.bfloat16), sigma=1.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_blur(x.transpose(2, 3), sigma=1.0)
    with pytest.raises(ValueError, match="contiguous"):
        ops.pixel_blur(x[:, :, :, ::2], sigma=1.0)
    with pytest.raises(ValueError, match="H, W"):
        ops.pixel_blur(torch.zeros(9), sigma=1.0)
    with pytest.raises(ValueError, match="H, W"):
        ops.pixel_blur(None, sigma=1.0)
    with pytest.raises(ValueError, match="planes of"):
        ops.pixel_blur(torch.zeros(2, 0, 9), sigma=1.0, edge="wrap")
    with pytest.raises(ValueError, match="overlaps"):
        ops.pixel_blur(x, x, sigma=1.0)
    flat = torch.zeros(2 * x.numel())
    a, b = flat[:x.numel()].view(x.shape), flat[x.numel() - 1:2 * x.numel() - 1].view(x.shape)
    with pytest.raises(ValueError, match="overlaps"):
        ops.pixel_blur(a, b, sigma=1.0)
    with pytest.raises(ValueError, match="out must"):
        ops.pixel_blur(x, torch.zeros(2, 3, 9, 11), sigma=1.0)
    with pytest.raises(ValueError, match="out must"):
        ops.pixel_blur(x, torch.zeros(x.shape, dtype=torch.float64), sigma=1.0)
    with pytest.raises(ValueError, match="out must"):
        ops.pixel_blur(x, torch.zeros(2, 3, 12, 9).transpose(2, 3), sigma=1.0)
    # the public name takes stacks [T,3,H,W] and maps [T,H,W] only
    assert "gaussian_blur" in mil_amd.__all__
    for bad in (torch.zeros(9, 12), torch.zeros(2, 4, 9, 12), torch.zeros(1, 2, 3, 9, 12), None):
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            mil_amd.gaussian_blur(bad, 1.0)
    # a well-formed call gets as far as the device check
    for call in (lambda: ops.pixel_blur(x, sigma=1.0), lambda: ops.pixel_blur(x, torch.zeros_like(x), taps=[0.5, 0.25], edge="wrap"),
                 lambda: mil_amd.gaussian_blur(x[:, 0].contiguous(), 2.0, edge="replicate")):
        with pytest.raises(ValueError, match="CUDA"):
            call()


def test_the_regularisers_blur_options_are_checked_and_off_by_default():
    import mil_amd
    reg = mil_amd.PixelRegularizer()
    assert (reg.blur_sigma, reg.blur_every, reg.grad_blur_sigma, reg.blur_edge) == (0.0, 4, 0.0, "reflect")
    assert repr(reg) == ("PixelRegularizer(alpha=6, alpha_weight=1e-07, tv_weight=1e-08, jitter=0, seed=0, blur_sigma=0.0, blur_every=4, "
                         "grad_blur_sigma=0.0, blur_edge='reflect')")
    with pytest.raises(TypeError):                                               # keyword only
        mil_amd.PixelRegularizer(6, 1e-7, 1e-8, 0, 0, 1.0)
    on = mil_amd.PixelRegularizer(jitter=2, blur_sigma=1, blur_every=2, grad_blur_sigma=0.5, blur_edge="wrap")
    assert (on.blur_sigma, on.blur_every, on.grad_blur_sigma, on.blur_edge) == (1.0, 2, 0.5, "wrap")
    assert "blur_sigma=1.0, blur_every=2, grad_blur_sigma=0.5, blur_edge='wrap'" in repr(on)
    for kw in (dict(blur_sigma=-1.0), dict(blur_sigma=0.1), dict(blur_sigma=4.2), dict(blur_sigma=float("nan")), dict(blur_sigma="1"),
               dict(blur_sigma=True), dict(grad_blur_sigma=-0.5), dict(grad_blur_sigma=5.0), dict(grad_blur_sigma=float("inf")),
               dict(blur_every=0), dict(blur_every=-2), dict(blur_every=1.5), dict(blur_every=True), dict(blur_edge="mirror"),
               dict(blur_edge=None)):
        with pytest.raises(ValueError):
            mil_amd.PixelRegularizer(**kw)
            pytest.fail(f"{kw} was accepted")
    # off: the scratch stacks are those of the jitter alone, no step starts with a blur and the pair comes back as given
    x = torch.zeros(2, 3, 8, 8)
    assert reg.scratch(x) == (None, None)
    xs, out = mil_amd.PixelRegularizer(jitter=1).scratch(x)
    assert xs.shape == out.shape == x.shape and xs.data_ptr() != out.data_ptr()
    for k in range(9):
        got = reg.blurred(x, None, k)
        assert got[0] is x and got[1] is None
    # on: one stack for both blurs without jitter, none beyond the jitter's with it
    xs, out = mil_amd.PixelRegularizer(blur_sigma=1.0).scratch(x)
    assert xs.shape == x.shape and out is None
    xs, out = mil_amd.PixelRegularizer(grad_blur_sigma=1.0).scratch(x)
    assert xs.shape == x.shape and out is None
    xs, out = on.scratch(x)
    assert xs.shape == out.shape == x.shape
    # reflect on images too small for the radius is refused before the first step; wrap takes them
    for kw in (dict(blur_sigma=2.0), dict(grad_blur_sigma=2.0)):
        with pytest.raises(ValueError, match="reflect"):
            mil_amd.PixelRegularizer(**kw).scratch(x)
        assert mil_amd.PixelRegularizer(blur_edge="wrap", **kw).scratch(x)[0].shape == x.shape
        assert mil_amd.PixelRegularizer(**kw).scratch(torch.zeros(1, 3, 9, 9))[0].shape == (1, 3, 9, 9)      # radius 8 = 9 - 1
    # the schedule: a blur starts step k for k > 0 and k % blur_every == 0 (on CPU tensors the launch is refused: it was reached)
    for k in range(7):
        if k in (2, 4, 6):
            with pytest.raises(ValueError, match="CUDA"):
                on.blurred(x, xs, k)
        else:
            got = on.blurred(x, xs, k)
            assert got[0] is x and got[1] is xs
