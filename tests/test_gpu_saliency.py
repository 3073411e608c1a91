"""-m gpu: tile saliency — the stem's data-gradient kernel (`ops.stem_dgrad`) against fp64, the encoder's input gradient on its
own activation pattern, the autograd surface of `ResNet.forward`, and `mil_amd.TileSaliency` against the CPU oracle."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fixture_inputs import synth_bag
from gpu_util import X3, rel_err, round_to, storage, to_nhwc
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]
# tests/test_gpu_kernels.py: TOL[float32], TOL[X3], and WTOL[bfloat16] — the bf16 operands are exact and the output is an fp32
# accumulation that is never rounded to bf16, the reasoning that file gives for its weight gradients
KERNEL_TOL = {torch.float32: 2e-5, X3: 6e-5, torch.bfloat16: 3e-5}


@pytest.fixture(autouse=True)
def _mma_mode(request):
    """dtype == "bf16x3": the wrappers pass MIL_DT_F32S for their fp32 tensors inside the test."""
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    if params.get("dtype") == X3 and request.node.name.startswith("test_stem_dgrad"):
        from mil_amd import _lib as L
        with L.f32_mma(L.MIL_DT_F32S):
            yield
    else:
        yield


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


# ---- kernel level ------------------------------------------------------------------------------------------------------------
STEM_DGRAD_SHAPES = [(2, 32, 32), (5, 64, 64), (3, 50, 70), (2, 33, 37), (1, 300, 300), (2, 256, 256)]


@functools.lru_cache(maxsize=None)
def _dgrad_case(shape, dtype):
    """(filter, dstem, fp64 dx) of one case, operands rounded as the kernel sees them; made once, shared, never changed."""
    n, h, w = shape
    g = torch.Generator().manual_seed(31 * h + w)
    wt = torch.randn(20, 3, 7, 7, generator=g) / 147 ** 0.5
    if dtype == torch.bfloat16:
        wt = round_to(wt, dtype)
    x64 = torch.zeros(n, 3, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, wt.double(), stride=2, padding=3)
    assert tuple(y.shape[2:]) == ((h + 1) // 2, (w + 1) // 2)
    dstem = torch.randn(y.shape, generator=g) * (torch.rand(y.shape, generator=g) < 0.5)      # the pool backward leaves sparse maps
    dstem = round_to(dstem, dtype)
    y.backward(dstem.double())
    return wt, dstem, x64.grad.detach()


def _borders(t):
    """The first and last three rows and columns: where the 7x7 filter's padding lives."""
    return torch.cat([t[..., :3, :].flatten(), t[..., -3:, :].flatten(), t[..., :, :3].flatten(), t[..., :, -3:].flatten()])


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", STEM_DGRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stem_dgrad_against_fp64(ops, dtype, shape):
    from mil_amd import _lib as L
    n, h, w = shape
    wt, dstem, want = _dgrad_case(shape, dtype)
    wp, _ = ops.pack_weights(wt.cuda(), None, L.PACK_STEM_DGRAD, dtype)
    dz = to_nhwc(dstem, dtype)
    nan = float("nan")
    dx = torch.full((n, 3, h, w), nan, device="cuda")
    got, none = ops.stem_dgrad(dz, wp, (h, w), dx=dx)
    assert got is dx and none is None
    assert bool(torch.isfinite(dx).all())                                       # every element written, odd sizes included
    e_all, e_border = rel_err(dx.cpu(), want), rel_err(_borders(dx.cpu()), _borders(want))
    print(f"stem_dgrad[{dtype}, {shape}]: rel. error vs fp64 {e_all:.2e}, border rows / columns {e_border:.2e}")
    assert e_all < KERNEL_TOL[dtype] and e_border < KERNEL_TOL[dtype]
    # the fused epilogue: max_c |dx| from the same accumulators, bit for bit; with and without the three-channel store
    dx2 = torch.full_like(dx, nan)
    sal2 = torch.full((n, h, w), nan, device="cuda")
    assert ops.stem_dgrad(dz, wp, (h, w), reduce="max_abs", dx=dx2, sal=sal2) == (dx2, sal2)
    assert torch.equal(dx2, dx)                                                 # two launches: bit-identical
    assert bool(torch.isfinite(sal2).all()) and torch.equal(sal2, dx2.abs().amax(1))
    sal3 = torch.full_like(sal2, nan)
    none, got = ops.stem_dgrad(dz, wp, (h, w), reduce="max_abs", sal=sal3)
    assert none is None and got is sal3 and torch.equal(sal3, sal2)
    fresh_dx, _ = ops.stem_dgrad(dz, wp, (h, w))
    assert torch.equal(fresh_dx, dx)


# ---- encoder level -----------------------------------------------------------------------------------------------------------
def _weights(golden_dir):
    return np.load(os.path.join(golden_dir, "weights.npz"))


def _model(golden_dir, dtype):
    import mil_amd
    w = _weights(golden_dir)
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net.eval()


def _hip_patterns(saved):
    """Activation pattern of a HIP encoder run in the form `orc.backbone(patterns=...)` takes (as tests/test_gpu_configs.py)."""
    widx = saved["widx"][..., :20].permute(0, 3, 1, 2).cpu()
    pat = {"stem_tap": (widx & 15).long(), "stem_pos": ((widx >> 4) & 1) == 0}
    names = [f"layer{li}.{b}" for li in range(1, 5) for b in range(3)]
    for name, (_xin, o1, out) in zip(names, saved["blocks"]):
        c = orc.STAGES[int(name[5]) - 1][1]
        pat[name + ".o1"] = (o1[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
        pat[name] = (out[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
    return pat


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [(6, 64, 64), (3, 50, 70)], ids=["6x64x64", "3x50x70"])
def test_encoder_input_gradient_on_its_own_activation_pattern(golden_dir, dtype, case, monkeypatch):
    """The encoder's vector-Jacobian product for the TILES against fp64 on the linear piece the HIP forward took (the rule of
    test_encoder_gradients_on_its_own_activation_pattern): L2 error of dx relative to its norm within 1e-5 (fp32), 2e-4
    (bf16x3), and for bf16 max(4e-2, 3 e) with e the error of the conv1.weight gradient of the same run, which is computed
    from the same pooled gradient.
    Measured on MI355X, dx / conv1.weight of the same run: fp32 1.08e-6 / 1.03e-6 (6x64x64) and 1.05e-6 / 1.02e-6 (3x50x70);
    bf16x3 1.53e-5 / 1.45e-5 and 1.50e-5 / 1.49e-5; bf16 9.02e-3 / 8.36e-3 and 8.79e-3 / 8.66e-3 — the per-pixel sums of the
    data gradient average the bf16 noise of the pooled gradient no better and no worse than the weight gradient's sums.
    In the same run: the parameter gradients under want_dx are bit for bit those of a want_dx=False run with the padded
    gradient layout (the same kernels), and without want_dx `ops.stem_dgrad` is never called."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    n, h, w = case
    x = synth_bag(n, h, w, 20260207)
    wts = _weights(golden_dir)
    net = _model(golden_dir, dtype)
    enc = net.cnn.module
    st = L.storage_dtype(dtype)
    dfe = torch.randn(n, 80, generator=torch.Generator().manual_seed(9))
    calls = []
    real = ops.stem_dgrad
    monkeypatch.setattr(ops, "stem_dgrad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with L.f32_mma(L.mma_code(dtype)):
        with torch.no_grad():
            feats, saved = encoder.encoder_forward(enc, x.cuda(), st)
            pat = _hip_patterns(saved)
            grads, dx, sal = encoder.encoder_backward(enc, saved, dfe.cuda(), st, want_dx=True)
            assert len(calls) == 1 and sal is None
            enc.dense_grads = False
            _f2, saved2 = encoder.encoder_forward(enc, x.cuda(), st)
            plain = encoder.encoder_backward(enc, saved2, dfe.cuda(), st)
            assert len(calls) == 1                                              # want_dx=False: no stem_dgrad launch
            enc.dense_grads = True
            _f3, saved3 = encoder.encoder_forward(enc, x.cuda(), st)
            assert isinstance(encoder.encoder_backward(enc, saved3, dfe.cuda(), st), list) and len(calls) == 1
    torch.cuda.synchronize()
    assert len(plain) == len(grads) and all(torch.equal(a, b) for a, b in zip(grads, plain))
    assert dx.shape == x.shape and dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    sd64 = {k: torch.tensor(wts[k], dtype=torch.float64, requires_grad=True) for k, _s in orc.state_dict_spec()}
    x64 = x.double().requires_grad_()
    orc.backbone(sd64, x64, patterns=pat).backward(dfe.double())
    e_dx = float((dx.double().cpu() - x64.grad).norm() / x64.grad.norm())
    g64 = sd64["cnn.module.conv1.weight"].grad
    e_w = float((grads[0].double().cpu() - g64).norm() / g64.norm())
    print(f"own-pattern input gradient [{dtype}, {case}]: dx {e_dx:.2e}; conv1.weight gradient of the same run {e_w:.2e}")
    gate = {torch.float32: 1e-5, X3: 2e-4, torch.bfloat16: max(4e-2, 3 * e_w)}[dtype]
    assert e_dx < gate, (e_dx, e_w)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_resnet_forward_honours_requires_grad(golden_dir, dtype, monkeypatch):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    net = _model(golden_dir, dtype)
    enc = net.cnn.module
    x = synth_bag(6, 64, 64, 20260208).cuda()
    v = torch.randn(6, 80, generator=torch.Generator().manual_seed(10)).cuda()
    calls = []
    real = ops.stem_dgrad
    monkeypatch.setattr(ops, "stem_dgrad", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    xg = x.clone().requires_grad_()
    net.cnn(xg).backward(v)
    assert len(calls) == 1 and xg.grad is not None and xg.grad.shape == x.shape
    with L.f32_mma(L.mma_code(dtype)):
        with torch.no_grad():
            _feats, saved = encoder.encoder_forward(enc, x, L.storage_dtype(dtype))
            _g, dx, _s = encoder.encoder_backward(enc, saved, v, L.storage_dtype(dtype), want_dx=True)
    assert torch.equal(xg.grad, dx)
    calls.clear()
    for p in net.parameters():
        p.grad = None
    plain = x.clone()
    net.cnn(plain).backward(v)
    assert plain.grad is None and not calls                                      # no gradient asked for: no launch
    if dtype == torch.bfloat16:
        import mil_amd
        xs = ops.stem_s2d(x, torch.bfloat16).requires_grad_()
        with pytest.raises(NotImplementedError, match="fp32"):
            enc(mil_amd.S2dTiles(xs))


# ---- model level -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_input_gradients(golden_dir, label):
    """(tiles, fp32 oracle dx, fp64 oracle dx) for the model-level case; computed once.  `orc.attention_forward` detaches its
    input (as gbm/model.py:194-196 does), so the same two calls it makes in eval mode are made here on a leaf."""
    torch.set_num_threads(max(1, min(64, os.cpu_count() or 1)))
    x = synth_bag(8, 64, 64, 20260209)
    w = _weights(golden_dir)
    y = torch.tensor([label])
    out = []
    for dt in (torch.float32, torch.float64):
        sd = {k: torch.tensor(w[k], dtype=dt) for k, _s in orc.state_dict_spec()}
        xl = x.clone().to(dt).requires_grad_()
        orc.mil_head(sd, orc.backbone(sd, xl), y)["loss"].backward()
        out.append(xl.grad.detach())
    return x, out[0], out[1]


def _to_u8(x):
    return ((x * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, X3], ids=["fp32", "bf16x3"])
def test_tile_saliency_against_the_cpu_oracle(golden_dir, dtype):
    """d loss / d tiles of an 8-tile bag against the CPU oracle.  LeakyReLU branch flips make the distance a property of the
    function, so the bound is test_gradients_anchored_to_fp64's: L2 distance from the fp64 oracle at most 3x the fp32 oracle's
    own, or 2e-2 (fp32) / 8e-2 (bf16x3), whichever is larger."""
    import mil_amd
    label = 2
    x, g32, g64 = _oracle_input_gradients(golden_dir, label)
    net = _model(golden_dir, dtype)
    dx = mil_amd.TileSaliency(net).input_gradient(x.cuda(), label)
    assert dx.shape == x.shape and dx.dtype == torch.float32
    e_orc = float((g32.double() - g64).norm() / g64.norm())
    e_hip = float((dx.double().cpu() - g64).norm() / g64.norm())
    print(f"TileSaliency.input_gradient [{dtype}]: L2 distance from fp64 {e_hip:.2e} (fp32 oracle: {e_orc:.2e})")
    assert e_hip <= max(3.0 * e_orc, 2e-2 if dtype == torch.float32 else 8e-2), (e_hip, e_orc)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_tile_saliency_maps_feeds_and_side_effects(golden_dir, dtype):
    import mil_amd
    net = _model(golden_dir, dtype)
    sal = mil_amd.TileSaliency(net)
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
    rng = torch.get_rng_state()
    dx = sal.input_gradient(x, 1)
    dx_u8 = sal.input_gradient(u8, 1)
    m_grad = sal.maps(x, 1)
    m_gxi = sal.maps(u8, 1, method="grad_x_input")
    assert torch.equal(torch.get_rng_state(), rng) and net.training
    for k, p in net.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k
    assert bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    assert torch.equal(dx_u8, dx)                                                # the decode is lossless
    assert m_grad.shape == (8, 64, 64) and torch.equal(m_grad, dx.abs().amax(1))
    assert torch.equal(sal.maps(u8, 1), m_grad)
    assert torch.equal(m_gxi, (dx * x).sum(1).abs())
    net.eval()
    after = step()                                                               # a training step is not disturbed
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_tile_saliency_with_flat_params_leaves_the_bucket_alone(golden_dir):
    """`dist.FlatParams` switches direct accumulation into the flat gradient bucket on: a saliency call must not add to it."""
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260211).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    mil_amd.TileSaliency(net).maps(x, 0)
    assert torch.equal(flat.flat_grad, bucket)


# ---- the step on the data-gradient-only walk ------------------------------------------------------------------------------------
WGRAD_OPS = ("conv_wgrad", "conv_wgrad_pair", "conv_entry_bwd", "stem_backward", "avgpool_fc_bwd")
# (3, 50, 70): odd map extents and a width that is no multiple of 16; (6, 64, 64): the smallest bag whose 8x8 layer-3 maps take the
# LDS-resident chain
WALK_BAGS = [(3, 50, 70), (6, 64, 64)]


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32).cpu(), b.contiguous().view(torch.int32).cpu())


@pytest.mark.parametrize("feed", ["fp32", "u8"])
@pytest.mark.parametrize("bag", WALK_BAGS, ids=["3x50x70", "6x64x64"])
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_saliency_step_is_encoder_backwards_dx_and_launches_no_weight_gradient(golden_dir, monkeypatch, ops, dtype, bag, feed):
    """`TileSaliency` and `bag_step` against `encoder_backward(want_dx=True)` written out by hand as `bag_step` used to run it: the
    same bits for dx, for the max-|dx| map and for the accumulator, and not one launch of a weight-gradient wrapper."""
    import mil_amd
    from mil_amd import _lib as L
    from mil_amd.encoder import encoder_backward, encoder_forward
    from mil_amd.head import head_apply
    from mil_amd.saliency import bag_setup, bag_step, device_tiles
    label = 1
    model = _model(golden_dir, dtype)
    net = model.cnn.module
    tiles = synth_bag(*bag, 20260301)
    if feed == "u8":
        tiles = mil_amd.U8Tiles(_to_u8(tiles))
    counts = {}

    def counted(name, real):
        def call(*a, **k):
            counts[name] += 1
            return real(*a, **k)
        return call
    for name in WGRAD_OPS + ("stem_dgrad", "stem_dgrad_acc"):
        counts[name] = 0
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))

    def tail_launches():
        n = counts["stem_dgrad"] + counts["stem_dgrad_acc"]
        counts["stem_dgrad"] = counts["stem_dgrad_acc"] = 0
        return n

    x = device_tiles(model, tiles)
    setup = bag_setup(model, x.shape[0], label)
    layout, y, cw = setup
    mode = net.compute_dtype
    st = L.storage_dtype(mode)

    def by_hand(**kw):
        with L.f32_mma(L.mma_code(mode)):
            with torch.no_grad():
                feats, saved = encoder_forward(net, x, st)
            H = feats.detach().requires_grad_()
            loss = head_apply(H, layout, y, None, cw, [w.detach() for w in model.head_weights()], None, direct=False)[0]
            (dH,) = torch.autograd.grad(loss.sum(), H)
            with torch.no_grad():
                return encoder_backward(net, saved, dH, st, allow_direct=False, want_dx=True, **kw)[1:]
    dx_ref = by_hand()[0]
    sal_ref = by_hand(dx_reduce="max_abs")[1]
    acc_ref = torch.zeros_like(dx_ref)
    by_hand(dx_acc=(acc_ref, 0.25))
    assert counts["conv_wgrad"] > 0 and counts["avgpool_fc_bwd"] == 3 and tail_launches() == 3     # the counters see launches
    assert bool(torch.isfinite(dx_ref).all()) and float(dx_ref.abs().max()) > 0
    for name in WGRAD_OPS:
        counts[name] = 0

    sal = mil_amd.TileSaliency(model)
    training, rng, dev_rng = model.training, torch.get_rng_state(), torch.cuda.get_rng_state()
    dx = sal.input_gradient(tiles, label)
    assert tail_launches() == 1
    m = sal.maps(tiles, label, method="gradient")
    assert tail_launches() == 1
    acc = torch.zeros_like(dx_ref)
    assert bag_step(model, setup, x, dx_acc=(acc, 0.25))[:2] == (None, None)
    assert tail_launches() == 1
    assert all(counts[name] == 0 for name in WGRAD_OPS), counts
    assert _same_bits(dx, dx_ref) and _same_bits(m, sal_ref) and _same_bits(acc, acc_ref)
    assert all(p.grad is None for p in model.parameters())
    assert model.training == training and torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), dev_rng)
