"""-m gpu: integrated gradients and SmoothGrad on the device — `ops.path_point` (the path point and its counter-based noise),
`ops.stem_dgrad_acc` (the stem's data gradient added into a running sum), `ops.attr_finish` (attributions, maps, per-tile sums)
bit for bit against fp32 arithmetic on the CPU, and `mil_amd.TileIntegratedGradients` / `TileSmoothGrad` against the loop they
replace, against the CPU oracle, and for what they must leave alone."""
import functools
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import path_attr_reference as ref
import slice_sum_reference as tree
from fixture_inputs import synth_bag
from gpu_util import X3, rel_err, round_to, to_nhwc
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]
# tests/test_gpu_saliency.py's KERNEL_TOL, for the reasons given there (exact bf16 operands, fp32 accumulation never rounded)
KERNEL_TOL = {torch.float32: 2e-5, X3: 6e-5, torch.bfloat16: 3e-5}
BASE = (0.25, -0.5, 1.0)                 # per-channel baselines of the kernel tests


def _ids(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _f32(v):
    return torch.tensor(v, dtype=torch.float32)


def _to_u8(x):
    return ((x * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _tiles(shape):
    """(uint8 codes, the fp32 values they stand for) of one kernel case, on the CPU; made once, never changed."""
    import mil_amd
    n, h, w = shape
    g = torch.Generator().manual_seed(7 * h + w)
    u8 = torch.randint(0, 256, (n, 3, h, w), generator=g, dtype=torch.uint8)
    return u8, mil_amd.U8Tiles(u8).float()


def _feed(kind, shape):
    """(what the wrapper is handed, the fp32 values on the CPU)."""
    import mil_amd
    u8, x = _tiles(shape)
    return (mil_amd.U8Tiles(u8.cuda()) if kind == "u8" else x.cuda()), x


# ---- path_point ----------------------------------------------------------------------------------------------------------------
POINT_SHAPES = [(1, 5, 7), (2, 33, 37), (3, 64, 64)]


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("shape", POINT_SHAPES, ids=_ids)
def test_path_point_without_noise_is_the_cpu_fp32_expression(ops, shape, kind):
    tiles, x = _feed(kind, shape)
    b = _f32(BASE).view(1, 3, 1, 1)
    for alpha in (0.0, 0.3125, 1.0 / 3.0, 1.0):
        want = b + _f32(alpha) * (x - b)                                        # a difference, a product, a sum: no fma on the CPU
        nan = torch.full(x.shape, float("nan"), device="cuda")
        got = ops.path_point(tiles, alpha, BASE, out=nan)
        assert got is nan and torch.equal(got.cpu(), want), (alpha, kind)
        assert torch.equal(ops.path_point(tiles, alpha, BASE), got)
    assert torch.equal(ops.path_point(tiles, 0.0, BASE).cpu(), b.expand_as(x))  # alpha = 0: the baseline bag itself
    assert torch.equal(ops.path_point(tiles, 0.7, 0.25).cpu(), 0.25 + _f32(0.7) * (x - 0.25))     # a scalar baseline


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_path_point_off_the_16_byte_grid_takes_the_scalar_path(ops, kind):
    """Tiles and output that start one element behind an aligned address: no vector access, the same values."""
    import mil_amd
    shape = (2, 33, 37)
    u8, x = _tiles(shape)
    n = x.numel()
    b = _f32(BASE).view(1, 3, 1, 1)
    if kind == "u8":
        buf = torch.zeros(n + 1, dtype=torch.uint8, device="cuda")
        buf[1:] = u8.cuda().flatten()
        tiles = mil_amd.U8Tiles(buf[1:].view(x.shape))
        assert tiles.u8.data_ptr() % 4 == 1
    else:
        buf = torch.zeros(n + 1, device="cuda")
        buf[1:] = x.cuda().flatten()
        tiles = buf[1:].view(x.shape)
        assert tiles.data_ptr() % 16 == 4
    out = torch.full((n + 1,), float("nan"), device="cuda")
    got = ops.path_point(tiles, 0.3125, BASE, noise_level=0.0, out=out[1:].view(x.shape))
    assert torch.equal(got.cpu(), b + _f32(0.3125) * (x - b)) and bool(torch.isnan(out[0]))
    z = torch.zeros(x.shape, device="cuda")
    noisy = ops.path_point(z, 0.0, 0.0, noise_level=1.0, seed=3, out=out[1:].view(x.shape))
    assert torch.equal(noisy, ops.path_point(z, 0.0, 0.0, noise_level=1.0, seed=3))          # the noise does not depend on the path taken


@pytest.mark.parametrize("shape", POINT_SHAPES, ids=_ids)
def test_path_point_noise_against_the_fp64_restatement(ops, shape):
    """x = 0, base = 0, alpha = 0, noise_level = 1: the output is the noise itself.  Against Box-Muller in fp64 from the same
    Philox bits within 16 * 2^-23 * |n|: `logf` and `sincospif` are good to a few ulp each (the HIP math library documents 1
    and 2), the correctly rounded square root halves the relative error of the logarithm, 2 u2 is exact so `sincospif` sees the
    exact argument, and the product rounds once: about 8 ulp of |n| with 3-4 ulp functions, times a margin of 2."""
    n, h, w = shape
    z = torch.zeros(n, 3, h, w, device="cuda")
    got = ops.path_point(z, 0.0, 0.0, noise_level=1.0, seed=0, sample=0)
    want = ref.normals(z.numel(), 0, 0).reshape(z.shape)
    err = np.abs(got.double().cpu().numpy() - want)
    worst = float((err / np.maximum(np.abs(want), 1e-300)).max() / 2.0 ** -23)
    print(f"path_point noise {shape}: worst error {worst:.2f} ulp of |n| (bound 16)")
    assert bool(torch.isfinite(got).all())
    assert bool((err <= 16 * 2.0 ** -23 * np.abs(want)).all())
    assert torch.equal(ops.path_point(z, 0.0, 0.0, noise_level=1.0, seed=0, sample=0), got)     # two launches
    for kw in ({"sample": 1}, {"seed": 1}, {"seed": 1 << 32}):
        other = ops.path_point(z, 0.0, 0.0, noise_level=1.0, **{"seed": 0, "sample": 0, **kw})
        assert not torch.equal(other, got), kw
        want_o = ref.normals(z.numel(), kw.get("seed", 0), kw.get("sample", 0)).reshape(z.shape)
        assert bool((np.abs(other.double().cpu().numpy() - want_o) <= 16 * 2.0 ** -23 * np.abs(want_o)).all()), kw


def test_path_point_noise_edge_view_and_range(ops):
    # u1 == 1 (r0 >> 8 == 0xffffff): the logarithm is zero and both normals of the pair are exactly 0
    z = torch.zeros(1, 3, 5, 7, device="cuda")
    edge = ops.path_point(z, 0.0, 0.0, noise_level=1.0, seed=ref.SEED_WITH_U1_ONE).flatten().cpu()
    assert float(edge[0]) == 0.0 and float(edge[1]) == 0.0 and float(edge[2]) != 0.0
    # a value is a function of (seed, sample, linear index): the same elements through a differently shaped stack
    a = ops.path_point(torch.zeros(2, 3, 32, 64, device="cuda"), 0.0, 0.0, noise_level=1.0, seed=5, sample=2)
    b = ops.path_point(torch.zeros(4, 3, 32, 32, device="cuda"), 0.0, 0.0, noise_level=1.0, seed=5, sample=2)
    assert torch.equal(a.flatten(), b.flatten())
    # with a range: sigma = noise_level * (hi - lo), formed unfused in fp32, times the same normals
    rng = torch.tensor([-0.8125, 0.9], device="cuda")
    got = ops.path_point(torch.zeros(2, 3, 32, 64, device="cuda"), 0.0, 0.0, noise_level=0.15, value_range=rng, seed=5, sample=2)
    sigma = _f32(0.15) * (_f32(0.9) - _f32(-0.8125))
    assert torch.equal(got.cpu(), sigma * a.cpu())
    # and on top of a path point: the third term is added last
    tiles, x = _feed("u8", (2, 33, 37))
    bb = _f32(BASE).view(1, 3, 1, 1)
    n1 = ops.path_point(torch.zeros(x.shape, device="cuda"), 0.0, 0.0, noise_level=1.0, seed=9, sample=4).cpu()
    got = ops.path_point(tiles, 1.0 / 3.0, BASE, noise_level=0.15, value_range=rng, seed=9, sample=4)
    assert torch.equal(got.cpu(), (bb + _f32(1.0 / 3.0) * (x - bb)) + sigma * n1)


# ---- stem_dgrad_acc ------------------------------------------------------------------------------------------------------------
ACC_SHAPES = [(2, 32, 32), (2, 33, 37), (3, 50, 70), (1, 300, 300), (520, 64, 64)]


@functools.lru_cache(maxsize=None)
def _dgrad_case(shape, dtype):
    """(filter, four dstem, fp64 dx of the first) built as tests/test_gpu_saliency.py::_dgrad_case builds its case: operands
    rounded as the kernel sees them, sparse gradients as the pool backward leaves them; made once, shared, never changed."""
    n, h, w = shape
    g = torch.Generator().manual_seed(31 * h + w)
    wt = torch.randn(20, 3, 7, 7, generator=g) / 147 ** 0.5
    if dtype == torch.bfloat16:
        wt = round_to(wt, dtype)
    x64 = torch.zeros(n, 3, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, wt.double(), stride=2, padding=3)
    assert tuple(y.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
    ds = [round_to(torch.randn(y.shape, generator=g) * (torch.rand(y.shape, generator=g) < 0.5), dtype) for _ in range(4)]
    y.backward(ds[0].double())
    return wt, ds, x64.grad.detach()


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", ACC_SHAPES, ids=_ids)
def test_stem_dgrad_acc_is_acc_plus_scale_times_dx(ops, dtype, shape):
    """(520,64,64) is 2080 space-to-depth tiles on the 2048-workgroup grid: the one case that walks `t += gridDim.x` with its
    prefetch; there the kernel is also held to the fp64 transposed convolution (acc = 0, scale = 1)."""
    from mil_amd import _lib as L
    n, h, w = shape
    wt, ds, want64 = _dgrad_case(shape, dtype)
    with L.f32_mma(L.MIL_DT_F32S if dtype == X3 else L.MIL_DT_F32):
        wp, _ = ops.pack_weights(wt.cuda(), None, L.PACK_STEM_DGRAD, dtype)
        dz = [to_nhwc(d, dtype) for d in ds]
        dxs = [ops.stem_dgrad(d, wp, (h, w))[0].cpu() for d in dz]
        acc0 = torch.randn(n, 3, h, w, generator=torch.Generator().manual_seed(5))
        scales = (0.3, -1.7, 1.0, 1.0 / 3.0)
        acc = acc0.cuda()
        assert ops.stem_dgrad_acc(dz[0], wp, (h, w), acc, scales[0]) is acc
        want = acc0 + _f32(scales[0]) * dxs[0]                                   # a product, then a sum
        assert torch.equal(acc.cpu(), want)
        again = acc0.cuda()
        ops.stem_dgrad_acc(dz[0], wp, (h, w), again, scales[0])
        assert torch.equal(again, acc)                                          # two runs: bit-identical
        for k in range(1, 4):                                                   # four successive launches = the sequential sum
            ops.stem_dgrad_acc(dz[k], wp, (h, w), acc, scales[k])
            want = want + _f32(scales[k]) * dxs[k]
        assert torch.equal(acc.cpu(), want)
        if n == 520:
            zero = torch.zeros(n, 3, h, w, device="cuda")
            ops.stem_dgrad_acc(dz[0], wp, (h, w), zero, 1.0)
            e = rel_err(zero.cpu(), want64)
            print(f"stem_dgrad_acc[{dtype}, {shape}]: rel. error vs fp64 {e:.2e}")
            assert e < KERNEL_TOL[dtype]
            assert torch.equal(zero.cpu(), dxs[0] + 0.0)                        # 0 + 1 * dx: dx itself (a -0 becomes +0)


# ---- attr_finish ---------------------------------------------------------------------------------------------------------------
FINISH_SHAPES = [(1, 5, 7), (2, 33, 37), (2, 50, 70), (1, 192, 192)]        # the last: a thread takes a second group of four pixels


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("shape", FINISH_SHAPES, ids=_ids)
def test_attr_finish_against_the_cpu_fp32_restatement(ops, shape, kind):
    n, h, w = shape
    tiles, x = _feed(kind, shape)
    acc = torch.randn(x.shape, generator=torch.Generator().manual_seed(h)) * 1e-2
    b = _f32(BASE).view(1, 3, 1, 1)
    a = (x - b) * acc
    maps = {"sum": ((a[:, 0] + a[:, 1]) + a[:, 2]).abs(), "max": a.abs().amax(1), "grad_max": acc.abs().amax(1)}
    g = acc.cuda()
    attr, m, sums = ops.attr_finish(g, tiles, BASE, want_attr=True, want_map=True, map_mode="sum", want_sums=True)
    assert attr.shape == x.shape and m.shape == (n, h, w) and sums.shape == (n,)
    assert torch.equal(attr.cpu(), a) and torch.equal(m.cpu(), maps["sum"])
    # any-order fp32 summation of 3 h w terms
    s64 = attr.double().cpu().sum((1, 2, 3))
    bound = 3 * h * w * 2.0 ** -24 * attr.double().cpu().abs().sum((1, 2, 3))
    print(f"attr_finish tile sums {shape} {kind}: error / bound {float(((sums.double().cpu() - s64).abs() / bound).max()):.3f}")
    assert bool(((sums.double().cpu() - s64).abs() <= bound).all())
    assert np.array_equal(sums.cpu().numpy().view(np.int32), tree.attr_tile_sums(a.numpy()).view(np.int32))     # the summation tree itself
    # every subset of the outputs, every map mode: the same values, bit for bit (two launches included)
    for wa, wm, ws in itertools.product((False, True), repeat=3):
        if not (wa or wm or ws):
            continue
        for mode in maps if wm else ("sum",):
            a2, m2, s2 = ops.attr_finish(g, tiles, BASE, want_attr=wa, want_map=wm, map_mode=mode, want_sums=ws)
            assert (a2 is None) == (not wa) and (m2 is None) == (not wm) and (s2 is None) == (not ws)
            assert a2 is None or torch.equal(a2, attr)
            assert m2 is None or torch.equal(m2.cpu(), maps[mode]), mode
            assert s2 is None or torch.equal(s2, sums)
    assert torch.equal(ops.attr_finish(g, None, 0.0, want_attr=False, want_map=True, map_mode="grad_max")[1].cpu(), maps["grad_max"])


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _weights(golden_dir):
    return np.load(os.path.join(golden_dir, "weights.npz"))


def _model(golden_dir, dtype):
    import mil_amd
    w = _weights(golden_dir)
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net.eval()


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_integrated_gradients_equal_the_loop_they_replace(golden_dir, dtype, ops):
    import mil_amd
    net = _model(golden_dir, dtype)
    sal = mil_amd.TileSaliency(net)
    x = synth_bag(8, 64, 64, 20260301).cuda()
    for rule in ("midpoint", "toolkit"):
        ig = mil_amd.TileIntegratedGradients(net, steps=4, rule=rule, baseline="white")
        got = ig.gradients(x, 2)
        assert got.shape == x.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        path = ig.path()
        assert len(path) == (4 if rule == "midpoint" else 5)
        want = torch.zeros(x.shape)
        for alpha, weight in path:
            g = sal.input_gradient(ops.path_point(x, alpha, ig.baseline), 2).cpu()
            want = want + _f32(weight) * g
        assert torch.equal(got.cpu(), want), rule
        assert torch.equal(ig.gradients(x, 2), got)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_smoothgrad_equals_the_loop_it_replaces(golden_dir, dtype, ops):
    import mil_amd
    net = _model(golden_dir, dtype)
    sal = mil_amd.TileSaliency(net)
    x = synth_bag(8, 64, 64, 20260302).cuda()
    sg = mil_amd.TileSmoothGrad(net, n=3, noise_level=0.15, seed=11)
    got = sg.gradients(x, 1)
    rng = torch.stack((x.amin(), x.amax()))
    want = torch.zeros(x.shape)
    for k in range(3):
        pt = ops.path_point(x, 1.0, 0.0, noise_level=0.15, value_range=rng, seed=11, sample=k)
        want = want + _f32(1.0 / 3) * sal.input_gradient(pt, 1).cpu()
    assert torch.equal(got.cpu(), want)
    assert torch.equal(sg.gradients(x, 1), got)                                  # the same seed: the same bits
    assert not torch.equal(mil_amd.TileSmoothGrad(net, n=3, noise_level=0.15, seed=12).gradients(x, 1), got)
    assert torch.equal(sg.maps(x, 1), got.abs().amax(1))
    # no noise, one sample: the plain input gradient
    assert torch.equal(mil_amd.TileSmoothGrad(net, n=1, noise_level=0.0).gradients(x, 1), sal.input_gradient(x, 1))


@functools.lru_cache(maxsize=None)
def _oracle_integrated_gradients(golden_dir, label):
    """(tiles, fp32 oracle IG, fp64 oracle IG): midpoint rule, 4 steps, baseline 0, each gradient made as
    tests/test_gpu_saliency.py::_oracle_input_gradients makes its one; computed once."""
    torch.set_num_threads(max(1, min(64, os.cpu_count() or 1)))
    x = synth_bag(8, 64, 64, 20260209)
    w = _weights(golden_dir)
    y = torch.tensor([label])
    out = []
    for dt in (torch.float32, torch.float64):
        sd = {k: torch.tensor(w[k], dtype=dt) for k, _s in orc.state_dict_spec()}
        total = torch.zeros(x.shape, dtype=dt)
        for k in range(4):
            xl = (x.to(dt) * ((k + 0.5) / 4)).requires_grad_()
            orc.mil_head(sd, orc.backbone(sd, xl), y)["loss"].backward()
            total += xl.grad.detach() / 4
        out.append(total)
    return x, out[0], out[1]


@pytest.mark.parametrize("dtype", [torch.float32, X3], ids=["fp32", "bf16x3"])
def test_integrated_gradients_against_the_cpu_oracle(golden_dir, dtype):
    """The convention of test_tile_saliency_against_the_cpu_oracle: L2 distance from the fp64 oracle at most 3x the fp32
    oracle's own, or 2e-2 (fp32) / 8e-2 (bf16x3), whichever is larger."""
    import mil_amd
    x, g32, g64 = _oracle_integrated_gradients(golden_dir, 2)
    net = _model(golden_dir, dtype)
    got = mil_amd.TileIntegratedGradients(net, steps=4, rule="midpoint", baseline=0.0).gradients(x.cuda(), 2)
    e_orc = float((g32.double() - g64).norm() / g64.norm())
    e_hip = float((got.double().cpu() - g64).norm() / g64.norm())
    print(f"TileIntegratedGradients.gradients [{dtype}]: L2 distance from fp64 {e_hip:.2e} (fp32 oracle: {e_orc:.2e})")
    assert e_hip <= max(3.0 * e_orc, 2e-2 if dtype == torch.float32 else 8e-2), (e_hip, e_orc)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_uint8_tiles_derived_methods_and_completeness(golden_dir, dtype, ops):
    import mil_amd
    net = _model(golden_dir, dtype)
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(8, 64, 64, 20260303)).cuda())
    x = u8.float()
    base = (1.0, 0.9, 0.8)
    ig = mil_amd.TileIntegratedGradients(net, steps=3, baseline=base)
    g = ig.gradients(x, 0)
    assert torch.equal(ig.gradients(u8, 0), g)                                   # decoded inside the kernels, losslessly
    attr = ig.attributions(x, 0)
    assert torch.equal(attr, ops.attr_finish(g, x, base)[0]) and torch.equal(ig.attributions(u8, 0), attr)
    a = attr.cpu()
    m_sum, m_max = ig.maps(u8, 0), ig.maps(x, 0, reduce="max")
    assert m_sum.shape == m_max.shape == (8, 64, 64)
    assert torch.equal(m_sum.cpu(), ((a[:, 0] + a[:, 1]) + a[:, 2]).abs()) and torch.equal(m_max.cpu(), a.abs().amax(1))
    sg = mil_amd.TileSmoothGrad(net, n=2, seed=4)
    assert torch.equal(sg.gradients(u8, 0), sg.gradients(x, 0))
    # completeness(): the sum of the attributions, and the loss difference the axiom compares it with
    total, delta = ig.completeness(u8, 0)
    assert total.is_cuda and delta.is_cuda and total.dim() == 0 and delta.dim() == 0
    s64, abs64 = float(a.double().sum()), float(a.double().abs().sum())
    print(f"completeness [{dtype}]: sum of attributions {float(total):.6e} (fp64 of the same attributions {s64:.6e}), "
          f"loss(tiles) - loss(baseline) {float(delta):.6e}, sum |attributions| {abs64:.3e}")
    assert abs(float(total.double()) - s64) <= a.numel() * 2.0 ** -24 * abs64
    y = torch.tensor([0], device="cuda")
    with torch.no_grad():
        la = float(net(u8, y)["loss"].double())
        lb = float(net(_f32(base).view(1, 3, 1, 1).expand(8, 3, 64, 64).contiguous().cuda(), y)["loss"].double())
    assert abs(float(delta.double()) - (la - lb)) <= 4 * 2.0 ** -24 * (abs(la) + abs(lb)), (float(delta), la, lb)


def _calls(net):
    import mil_amd
    ig = mil_amd.TileIntegratedGradients(net, steps=2, baseline="white")
    sg = mil_amd.TileSmoothGrad(net, n=2)
    return ig, sg


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_path_attribution_side_effects(golden_dir, dtype):
    """tests/test_gpu_saliency.py::test_tile_saliency_maps_feeds_and_side_effects for the two new classes."""
    import mil_amd
    net = _model(golden_dir, dtype)
    ig, sg = _calls(net)
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(8, 64, 64, 20260210)).cuda())
    x = u8.float()
    y = torch.tensor([1], device="cuda")

    def step():
        for p in net.parameters():
            p.grad = None
        net(x, y)["loss"].backward()
        return [p.grad.clone() for p in net.parameters()]
    before = step()
    net.train()                                                                  # the flag is left alone, whatever it is
    marks = {k: torch.full_like(p, 0.5) if i % 2 else None for i, (k, p) in enumerate(net.named_parameters())}
    for k, p in net.named_parameters():
        p.grad = None if marks[k] is None else marks[k].clone()
    rng, rng_dev = torch.get_rng_state(), torch.cuda.get_rng_state()
    outs = [ig.gradients(x, 1), ig.attributions(u8, 1), ig.maps(x, 1), ig.maps(u8, 1, reduce="max"), *ig.completeness(x, 1),
            sg.gradients(u8, 1), sg.maps(x, 1)]
    assert torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), rng_dev) and net.training
    for k, p in net.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k
    assert all(bool(torch.isfinite(o).all()) for o in outs) and float(outs[0].abs().max()) > 0 and float(outs[6].abs().max()) > 0
    net.eval()
    after = step()                                                               # a training step is not disturbed
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_path_attribution_with_flat_params_leaves_the_bucket_alone(golden_dir):
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260211).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    ig, sg = _calls(net)
    ig.maps(x, 0)
    ig.completeness(x, 0)
    sg.maps(x, 0)
    assert torch.equal(flat.flat_grad, bucket)
