"""CPU (-m "not gpu"): feature inversion without a GPU — the formulas of `mil_pixel_momentum_step`, `mil_pixel_reg` and
`mil_stage_match` (their numpy restatements in fp64 against torch.optim and torch.autograd), the status codes of every new entry
point, and every argument check of the new wrappers and classes, which fire on CPU tensors before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import feature_inv_reference as ref


@pytest.mark.parametrize("wd", [0.0, 1e-4])
def test_the_restated_momentum_step_is_torch_optim_in_fp64(wd):
    """30 steps with random gradients: the restatement in fp64 and torch.optim.SGD(momentum=0.9) in fp64 agree within 1e-12
    (relative to the largest value), the bound of test_the_restated_step_is_torch_optim_in_fp64.  The fp32 kernel is held to the
    same code bit for bit (tests/test_gpu_feature_inv.py)."""
    rng = np.random.default_rng(6)
    x = rng.uniform(-1, 1, (2, 3, 9, 7))
    p = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.SGD([p], lr=6.0, momentum=0.9, weight_decay=wd)
    buf = np.zeros_like(x)
    for step in range(1, 31):
        g = rng.standard_normal(x.shape) * 10.0 ** rng.integers(-6, 1)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        x, buf, _codes = ref.momentum_step(x, g, buf, lr=6.0, momentum=0.9, weight_decay=wd)
        want = p.detach().numpy()
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max(), (step, np.abs(x - want).max())
    want = opt.state[p]["momentum_buffer"].numpy()
    assert np.abs(buf - want).max() <= 1e-12 * np.abs(want).max()


def test_a_zero_buffer_gives_torchs_first_step():
    """torch's first step clones the gradient into the buffer instead of forming momentum * buf + g': with a zero buffer the
    restated step does the same bit for bit in fp32 — buf ends as g' = g + wd x and x as the plain SGD rule leaves it (torch's own
    CPU kernels fuse x + (-lr) * buf into one FMA, so torch's fp32 x is not the yardstick for bits; its buffer, with no decay, is)."""
    import feature_vis_reference as fv_ref
    rng = np.random.default_rng(7)
    x = rng.uniform(-1, 1, (2, 3, 9, 7)).astype(np.float32)
    g = rng.standard_normal(x.shape).astype(np.float32)
    for wd in (0.0, 1e-4):
        got, buf, _codes = ref.momentum_step(x, g, np.zeros_like(x), lr=100.0, momentum=0.9, weight_decay=wd)
        plain, _m, _v, _c = fv_ref.pixel_step(x, g, None, None, rule="sgd", lr=100.0, weight_decay=wd)
        assert np.array_equal(got.view(np.int32), plain.view(np.int32))
        assert np.array_equal(buf.view(np.int32), (g + np.float32(wd) * x).view(np.int32))
    p = torch.tensor(x, requires_grad=True)
    p.grad = torch.tensor(g)
    opt = torch.optim.SGD([p], lr=100.0, momentum=0.9)
    opt.step()
    _x, buf, _codes = ref.momentum_step(x, g, np.zeros_like(x), lr=100.0, momentum=0.9)
    assert np.array_equal(buf.view(np.int32), opt.state[p]["momentum_buffer"].numpy().view(np.int32))


@pytest.mark.parametrize("alpha", [2, 4, 6, 8])
@pytest.mark.parametrize("shape", [(2, 3, 9, 7), (1, 3, 1, 9), (1, 3, 6, 1)], ids=lambda s: "x".join(map(str, s)))
def test_the_restated_regulariser_gradient_is_autograd_of_the_toolkits_norms(shape, alpha):
    """out - (the shifted g) in fp64 against torch.autograd of alpha_weight * alpha_norm + tv_weight * total_variation_norm, the
    toolkit's two functions restated in torch: within 1e-12 relative.  A map with one row or one column has no total variation."""
    rng = np.random.default_rng(sum(shape) + alpha)
    x = rng.uniform(-1.5, 1.5, shape)
    g = rng.standard_normal(shape)
    aw, tw, shift = 0.3, 0.7, (2, -3)
    xt = torch.tensor(x, requires_grad=True)
    (aw * ref.torch_alpha_norm(xt, alpha) + tw * ref.torch_tv_norm(xt)).backward()
    want = xt.grad.numpy() + np.roll(g, (-shift[0], -shift[1]), axis=(2, 3))
    got = ref.pixel_reg(x, g, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    terms = ref.reg_terms64(x, alpha)
    assert np.allclose(terms[0].sum(), float(ref.torch_alpha_norm(xt, alpha).detach()), rtol=1e-12, atol=0)
    assert np.allclose(terms[1].sum(), float(ref.torch_tv_norm(xt).detach()), rtol=1e-12, atol=0)
    if min(shape[2:]) == 1:
        assert np.all(ref.tv_stencil(x) == 0) and np.all(terms[1] == 0)
    # the shifted copy and the index map of the gradient are inverse to each other
    assert np.array_equal(ref.pixel_reg(x, ref.shift_copy(g, shift), alpha=alpha, alpha_weight=0, tv_weight=0, shift=shift), g)


def test_the_restated_stage_match_seed_is_autograd_through_the_leaky_relu():
    """dz in fp64 against autograd of sum_t weight * sum (lrelu(z) - target)^2 / sum target^2 with respect to the pre-activation z."""
    rng = np.random.default_rng(8)
    c, cp = 20, 24
    z = rng.standard_normal((3, 5, 7, cp))
    z[0, 0, 0, 3] = 0.0                                                          # lrelu'(0) is the slope (torch's rule)
    target = np.abs(rng.standard_normal((3, 5, 7, cp)))
    zt = torch.tensor(z, requires_grad=True)
    act = torch.nn.functional.leaky_relu(zt, 0.1)
    tt = torch.tensor(target)
    loss = (0.1 * ((act - tt)[..., :c] ** 2).sum(dim=(1, 2, 3)) / (tt[..., :c] ** 2).sum(dim=(1, 2, 3))).sum()
    loss.backward()
    a = act.detach().numpy()
    dz = ref.stage_match_dz(a, target, c, ref.stage_energy64(target, c), 0.1, slope=0.1)
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-12 * np.abs(dz).max()
    assert np.all(dz[..., c:] == 0) and np.all(zt.grad.numpy()[..., c:] == 0)


def test_entry_points_return_status_codes_without_a_gpu():
    import mil_amd
    lib = mil_amd.lib()
    one, two, far = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 64), ctypes.c_void_p(1 << 20)
    # mil_stage_energy(target, energy, ws, n, h, w, cp, c, dtype, stream)
    assert lib.mil_stage_energy(None, one, one, 1, 8, 8, 24, 20, 1, None) == 1
    assert lib.mil_stage_energy(one, None, one, 1, 8, 8, 24, 20, 1, None) == 1
    assert lib.mil_stage_energy(one, one, None, 1, 8, 8, 24, 20, 1, None) == 1
    assert lib.mil_stage_energy(one, one, one, -1, 8, 8, 24, 20, 1, None) == 1
    assert lib.mil_stage_energy(one, one, one, 1, 8, 0, 24, 20, 1, None) == 1
    assert lib.mil_stage_energy(one, one, one, 1, 8, 8, 20, 20, 1, None) == 1            # cp not a multiple of 8
    assert lib.mil_stage_energy(one, one, one, 1, 8, 8, 24, 25, 1, None) == 1            # c > cp
    assert lib.mil_stage_energy(one, one, one, 1, 8, 8, 24, 20, 3, None) == 1            # no such storage
    assert lib.mil_stage_energy(one, one, one, 1, 4096, 4096, 24, 20, 1, None) == 2      # h w = 2^24
    assert lib.mil_stage_energy(one, one, one, 0, 8, 8, 24, 20, 1, None) == 0            # nothing to do
    # mil_stage_match(act, target, energy, loss, dz, ws, n, h, w, cp, c, weight, slope, dtype, stream)
    for k in range(6):
        ptrs = [one] * 6
        ptrs[k] = None
        assert lib.mil_stage_match(*ptrs, 1, 8, 8, 24, 20, 0.1, 0.1, 1, None) == 1, k
    six = [one] * 6
    assert lib.mil_stage_match(*six, -1, 8, 8, 24, 20, 0.1, 0.1, 1, None) == 1
    assert lib.mil_stage_match(*six, 1, 0, 8, 24, 20, 0.1, 0.1, 1, None) == 1
    assert lib.mil_stage_match(*six, 1, 8, 8, 20, 20, 0.1, 0.1, 1, None) == 1            # cp not a multiple of 8
    assert lib.mil_stage_match(*six, 1, 8, 8, 24, 25, 0.1, 0.1, 1, None) == 1            # c > cp
    assert lib.mil_stage_match(*six, 1, 8, 8, 24, 0, 0.1, 0.1, 1, None) == 1
    assert lib.mil_stage_match(*six, 1, 8, 8, 24, 20, 0.1, 0.1, 2, None) == 1
    assert lib.mil_stage_match(*six, 1, 4096, 4096, 24, 20, 0.1, 0.1, 0, None) == 2
    assert lib.mil_stage_match(*six, 0, 8, 8, 24, 20, 0.1, 0.1, 1, None) == 0
    # mil_pixel_reg(x, g, out, terms, ws, n, H, W, alpha, alpha_weight, tv_weight, dy, dx, stream): three tensors of 48 bytes
    x, g, out = one, two, ctypes.c_void_p(4096 + 128)
    assert lib.mil_pixel_reg(None, g, out, None, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, None, out, None, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, g, None, None, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, g, out, far, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1            # terms without a workspace
    for alpha in (0, 1, 3, 5, 7, 9, 10, -2):
        assert lib.mil_pixel_reg(x, g, out, None, None, 1, 2, 2, alpha, 0.1, 0.1, 0, 0, None) == 1, alpha
    assert lib.mil_pixel_reg(x, g, out, None, None, 1, 2, 2, 6, float("nan"), 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, g, out, None, None, -1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, g, out, None, None, 1, 0, 2, 6, 0.1, 0.1, 0, 0, None) == 1
    assert lib.mil_pixel_reg(x, g, g, None, None, 1, 2, 2, 6, 0.1, 0.1, 1, 0, None) == 1             # out is g under a shift
    assert lib.mil_pixel_reg(x, g, g, None, None, 1, 2, 2, 6, 0.1, 0.1, 0, -1, None) == 1
    assert lib.mil_pixel_reg(x, g, g, None, None, 0, 2, 2, 6, 0.1, 0.1, 1, 1, None) == 1             # ... also with nothing to do
    assert lib.mil_pixel_reg(x, g, ctypes.c_void_p(4096 + 64 + 16), None, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1   # partial overlap with g
    assert lib.mil_pixel_reg(x, g, x, None, None, 1, 2, 2, 6, 0.1, 0.1, 0, 0, None) == 1             # x is only read
    assert lib.mil_pixel_reg(x, g, out, None, None, 1, 32768, 32768, 6, 0.1, 0.1, 0, 0, None) == 2
    assert lib.mil_pixel_reg(x, g, g, None, None, 0, 2, 2, 6, 0.1, 0.1, 2, 4, None) == 0             # (2, 4) is no shift of a 2x2 map
    assert lib.mil_pixel_reg(x, g, out, None, None, 0, 2, 2, 6, 0.1, 0.1, 1, 1, None) == 0
    # mil_pixel_shift(x, out, n, H, W, dy, dx, stream)
    assert lib.mil_pixel_shift(None, out, 1, 2, 2, 1, 1, None) == 1
    assert lib.mil_pixel_shift(x, None, 1, 2, 2, 1, 1, None) == 1
    assert lib.mil_pixel_shift(x, x, 1, 2, 2, 1, 1, None) == 1
    assert lib.mil_pixel_shift(x, out, -1, 2, 2, 1, 1, None) == 1
    assert lib.mil_pixel_shift(x, out, 1, 2, 0, 1, 1, None) == 1
    assert lib.mil_pixel_shift(x, out, 1, 32768, 32768, 1, 1, None) == 2
    assert lib.mil_pixel_shift(x, out, 0, 2, 2, 1, 1, None) == 0
    # mil_pixel_momentum_step(x, g, buf, u8_out, table, total, project, lr, weight_decay, momentum, stream)
    assert lib.mil_pixel_momentum_step(None, g, out, None, None, 16, 0, 100.0, 0.0, 0.9, None) == 1
    assert lib.mil_pixel_momentum_step(x, None, out, None, None, 16, 0, 100.0, 0.0, 0.9, None) == 1
    assert lib.mil_pixel_momentum_step(x, g, None, None, None, 16, 0, 100.0, 0.0, 0.9, None) == 1
    assert lib.mil_pixel_momentum_step(x, g, out, None, None, 16, 3, 100.0, 0.0, 0.9, None) == 1
    assert lib.mil_pixel_momentum_step(x, g, out, None, None, 16, 2, 100.0, 0.0, 0.9, None) == 1          # "u8" without the table
    assert lib.mil_pixel_momentum_step(x, g, out, None, None, 16, 0, float("nan"), 0.0, 0.9, None) == 1
    assert lib.mil_pixel_momentum_step(x, g, out, None, None, 16, 0, 100.0, 0.0, float("nan"), None) == 1
    assert lib.mil_pixel_momentum_step(x, g, out, None, None, 0, 0, 100.0, 0.0, 0.9, None) == 0
    # the existing entry keeps its two rules
    f9 = (0.1, 0.0, 0.9, 0.1, 0.999, 0.001, 0.1, 0.03, 1e-8)
    assert lib.mil_pixel_step(x, g, out, None, None, None, 16, 2, 0, *f9, None) == 1


def test_wrapper_argument_checks_fire_on_cpu_tensors():
    import mil_amd  # noqa: F401
    from mil_amd import ops
    assert ops.PIXEL_RULES == ("sgd", "adam")
    act = torch.zeros(2, 5, 7, 24)
    with pytest.raises(ValueError, match="CUDA"):
        ops.stage_energy(act, 20)
    with pytest.raises(ValueError, match="stored"):
        ops.stage_energy(act, 30)
    with pytest.raises(ValueError, match=r"\[T,h,w,cp\]"):
        ops.stage_energy(act[0], 20)
    with pytest.raises(ValueError):
        ops.stage_energy(act.to(torch.float16), 20)
    with pytest.raises(ValueError, match="CUDA"):
        ops.stage_match(act, act.clone(), 20)
    with pytest.raises(ValueError, match="stored"):
        ops.stage_match(act, act.clone(), 0)
    with pytest.raises(ValueError, match="target"):
        ops.stage_match(act, None, 20)
    with pytest.raises(ValueError, match="weight"):
        ops.stage_match(act, act.clone(), 20, weight=float("nan"))
    x = torch.zeros(2, 3, 5, 7)
    with pytest.raises(ValueError, match="CUDA"):
        ops.pixel_reg(x, x.clone())
    for alpha in (1, 3, 10, 0, 6.5, True, "6"):
        with pytest.raises(ValueError, match="alpha"):
            ops.pixel_reg(x, x.clone(), alpha=alpha)
    with pytest.raises(ValueError, match="weight"):
        ops.pixel_reg(x, x.clone(), alpha_weight=-1.0)
    with pytest.raises(ValueError, match="weight"):
        ops.pixel_reg(x, x.clone(), tv_weight=float("nan"))
    for shift in (1, (1,), (1.5, 0), (0, 1, 2), "ab", (True, 0)):
        with pytest.raises(ValueError, match="shift"):
            ops.pixel_reg(x, x.clone(), shift=shift)
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        ops.pixel_reg(x[:, :2], x)
    with pytest.raises(ValueError, match="g must"):
        ops.pixel_reg(x, None)
    with pytest.raises(ValueError, match="CUDA"):
        ops.pixel_shift(x, None, (1, 1))
    with pytest.raises(ValueError, match="shift"):
        ops.pixel_shift(x, None, (0.5, 1))
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        ops.pixel_shift(x[0], None, (0, 1))
    with pytest.raises(ValueError, match="CUDA"):
        ops.pixel_momentum_step(x, x.clone(), x.clone(), lr=1.0)
    with pytest.raises(ValueError, match="project"):
        ops.pixel_momentum_step(x, x, x, lr=1.0, project="tanh")
    with pytest.raises(ValueError, match="momentum"):
        ops.pixel_momentum_step(x, x, x, lr=1.0, momentum=1.0)
    with pytest.raises(ValueError, match="momentum"):
        ops.pixel_momentum_step(x, x, x, lr=float("nan"))
    with pytest.raises(ValueError, match="weight_decay"):
        ops.pixel_momentum_step(x, x, x, lr=1.0, weight_decay=-1.0)
    with pytest.raises(ValueError, match="buf"):
        ops.pixel_momentum_step(x, x, None, lr=1.0)
    with pytest.raises(ValueError, match="rule"):                                # the two-rule entry stays as it is
        ops.pixel_step(x, x, None, rule="momentum")


def test_the_regulariser_is_a_checked_value_object():
    import mil_amd
    reg = mil_amd.PixelRegularizer()
    assert (reg.alpha, reg.alpha_weight, reg.tv_weight, reg.jitter, reg.seed) == (6, 1e-7, 1e-8, 0, 0)     # the toolkit's lambdas
    assert reg.shifts(3) == [(0, 0)] * 3
    for kw in (dict(alpha=5), dict(alpha=10), dict(alpha=0), dict(alpha_weight=-1e-7), dict(tv_weight=float("inf")), dict(jitter=-1),
               dict(jitter=1.5), dict(jitter=True), dict(seed=-1), dict(seed=0.5)):
        with pytest.raises(ValueError):
            mil_amd.PixelRegularizer(**kw)
    jit = mil_amd.PixelRegularizer(jitter=3, seed=5)
    state = torch.get_rng_state()
    shifts = jit.shifts(64)
    assert torch.equal(torch.get_rng_state(), state)                             # a generator of its own
    assert shifts == jit.shifts(64) == mil_amd.PixelRegularizer(jitter=3, seed=5).shifts(64)
    assert shifts != mil_amd.PixelRegularizer(jitter=3, seed=6).shifts(64)
    assert {v for s in shifts for v in s} == set(range(-3, 4))
    assert shifts == [tuple(s) for s in torch.randint(-3, 4, (64, 2), generator=torch.Generator().manual_seed(5)).tolist()]


def test_feature_inverter_argument_checks_fire_without_a_gpu():
    import mil_amd
    model = mil_amd.Attention(3, device="cpu")
    fi = mil_amd.FeatureInverter(model)
    assert (fi.lr, fi.momentum, fi.lr_decay, fi.weight, fi.project) == (100.0, 0.9, None, 0.1, "none")
    assert isinstance(fi.regularizer, mil_amd.PixelRegularizer) and fi.regularizer.jitter == 0
    bare = mil_amd.FeatureInverter(model.cnn.module, lr=1e4, lr_decay=(40, 0.1), regularizer=mil_amd.PixelRegularizer(jitter=2), project="clamp")
    assert bare.lr_decay == (40, 0.1)
    with pytest.raises(ValueError, match="Attention"):
        mil_amd.FeatureInverter(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="wide encoder"):
        mil_amd.FeatureInverter(mil_amd.alt_resnet.ResNet(layers=(1, 1, 1, 1), num_classes=8))
    for kw in (dict(lr=float("nan")), dict(momentum=1.0), dict(momentum=-0.1), dict(lr_decay=40), dict(lr_decay=(0, 0.1)), dict(lr_decay=(40, 0.0)),
               dict(lr_decay=(2.5, 0.1)), dict(weight=0.0), dict(weight=float("nan")), dict(regularizer=None), dict(regularizer="tv"),
               dict(project="tanh")):
        with pytest.raises(ValueError):
            mil_amd.FeatureInverter(model, **kw)
    tiles = torch.zeros(2, 3, 32, 32)
    bad_calls = [
        lambda: fi.invert(tiles, "layer5"),
        lambda: fi.invert(tiles, 0),
        lambda: fi.invert(tiles[:, :2], "layer1"),
        lambda: fi.invert(tiles.to(torch.uint8), "layer1"),
        lambda: fi.invert(mil_amd.S2dTiles(torch.zeros((2, 16, 16, 16), dtype=torch.bfloat16)), "layer1"),
        lambda: fi.invert(tiles[:0], "layer1"),
        lambda: fi.invert(tiles, "layer1", steps=0),
        lambda: fi.invert(tiles, "layer1", steps=2.5),
        lambda: fi.invert(tiles, "layer1", init_std=-1.0),
        lambda: fi.invert(tiles, "layer1", init_std=float("nan")),
        lambda: fi.invert(tiles, "layer1", seed=-1),
        lambda: fi.distance(tiles, tiles, "layer9"),
        lambda: fi.distance(tiles[:1], tiles, "layer1"),
        lambda: fi.distance(tiles, tiles[:, :2], "layer1"),
        lambda: fi.distance(None, tiles, "layer1"),
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # a well-formed call gets as far as the device check: the model is on the CPU
    for call in (lambda: fi.invert(tiles, "layer1", steps=1), lambda: bare.invert(mil_amd.U8Tiles(tiles.to(torch.uint8)), 4, steps=1),
                 lambda: fi.distance(tiles, mil_amd.U8Tiles(tiles.to(torch.uint8)), "layer2")):
        with pytest.raises(RuntimeError, match="AMD GPU"):
            call()


def test_feature_visualizer_takes_a_regulariser_by_keyword_only():
    import mil_amd
    model = mil_amd.Attention(3, device="cpu")
    assert mil_amd.FeatureVisualizer(model).regularizer is None
    reg = mil_amd.PixelRegularizer(jitter=2)
    fv = mil_amd.FeatureVisualizer(model, regularizer=reg)
    assert fv.regularizer is reg
    with pytest.raises(TypeError):
        mil_amd.FeatureVisualizer(model, "adam", 0.1, 1e-6, (0.9, 0.999), 1e-8, "none", reg)
    with pytest.raises(ValueError, match="PixelRegularizer"):
        mil_amd.FeatureVisualizer(model, regularizer=1e-8)
    for call in (lambda: fv.filters("layer1", channels=[0], size=(32, 32), steps=1), lambda: fv.dream(torch.zeros(2, 3, 32, 32), 2, 0, steps=1),
                 lambda: fv.classes(2, 4, size=(32, 32), steps=1)):
        with pytest.raises(RuntimeError, match="AMD GPU"):
            call()
