"""-m gpu: guided backpropagation and guided Grad-CAM — the four new entry points against their plain siblings (bit for bit) and
against fp64, the guided encoder walk against tests/guided_reference.py on the HIP forward's own activation pattern, and
`mil_amd.TileGuidedBackprop` / `mil_amd.TileGuidedGradCam`: bits, launches, feeds and side effects.

`gate / 255`: the kernel's quotient is an IEEE division.  torch on the device may divide a tensor by a Python scalar as a product
with the reciprocal, which differs from the division for 126 of the 256 byte values (csrc/u8_feed.cuh), so every expected value
here takes the quotient on the CPU — torch's fp32 `gate.float() / 255` there is the IEEE division — and only the product on the
device."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guided_reference as gref
from fixture_inputs import synth_bag
from gpu_util import X3, cpad, from_nhwc, poison_allocations, rel_err, round_to, storage, to_nhwc
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]
TOL = {torch.float32: 2e-5, torch.bfloat16: 8e-3, X3: 6e-5}          # tests/test_gpu_kernels.py: its conv data-gradient bound
WALK_FLOOR = {torch.float32: 1e-5, X3: 2e-4, torch.bfloat16: 4e-2}    # the project's plain-walk gates (tests/test_gpu_saliency.py)
LEAK = 0.1


@pytest.fixture(autouse=True)
def _mma_mode(request):
    """dtype == "bf16x3": the wrappers pass MIL_DT_F32S for their fp32 tensors inside the KERNEL tests (the encoder and class
    tests set the mode themselves)."""
    params = request.node.callspec.params if hasattr(request.node, "callspec") else {}
    if params.get("dtype") == X3 and request.node.name.startswith("test_kernel_"):
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


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _gated(p, act):
    """where((act > 0) & (p > 0), p, +0) in p's dtype."""
    return torch.where((act > 0) & (p > 0), p, torch.zeros_like(p))


def _quotient(gate_u8):
    """gate / 255 as the IEEE division, taken on the CPU (module docstring)."""
    return (gate_u8.cpu().float() / 255).to(gate_u8.device)


# ---- kernel level: conv_dgrad_rule -----------------------------------------------------------------------------------------------
# (cout of the forward conv = channels of dz, cin = channels of the result, stride of the forward conv, n, H, W of the result)
# 13x11: ragged tiles on both axes; 8x8 with three images: several images per tile and an empty slot; the three stage entries:
# zero-insert from 7x6 to 13x11 with an addend
DGRAD_CASES = [(c, c, 1, 2, 13, 11) for c in (20, 40, 60, 80)] + [(c, c, 1, 3, 8, 8) for c in (20, 40, 60, 80)] + \
              [(40, 20, 2, 2, 13, 11), (60, 40, 2, 2, 13, 11), (80, 60, 2, 2, 13, 11)]


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "{}to{}_s{}_n{}_{}x{}".format(*c))
def test_kernel_conv_dgrad_rule(ops, dtype, case):
    from mil_amd import _lib as L
    cout, cin, stride, n, h, w = case
    g = torch.Generator().manual_seed(7 * cout + cin + h)
    wt = round_to(torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5, dtype)
    x64 = torch.zeros(n, cin, h, w, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x64, wt.double(), None, stride=stride, padding=1)
    dz = round_to(torch.randn(y.shape, generator=g), dtype)
    y.backward(dz.double())
    # the walk adds the shortcut's gradient at every masked launch but the first of a block; the 8x8 cases run without
    res = round_to(torch.randn(n, cin, h, w, generator=g), dtype) if (h, w) != (8, 8) else None
    act = round_to(torch.randn(n, cin, h, w, generator=g), dtype)
    lin = x64.grad + (0 if res is None else res.double())
    if stride == 2:
        assert tuple(y.shape[2:]) == (7, 6)
    dzg, actg = to_nhwc(dz, dtype), to_nhwc(act, dtype)
    resg = None if res is None else to_nhwc(res, dtype)
    wd, _ = ops.pack_weights(wt.cuda(), None, L.PACK_DGRAD, dtype)
    kw = dict(ks=3, pad=1, res=resg)
    if stride == 2:
        kw.update(zero_insert=True, out_hw=(h, w))
    with poison_allocations(reduce_batch=False):                                 # the outputs start as NaNs
        p = ops.conv_dgrad_rule(dzg, wd, cpad(cin), rule=0, **kw)
        guided = ops.conv_dgrad_rule(dzg, wd, cpad(cin), rule=1, act=actg, **kw)
        masked = ops.conv_dgrad_rule(dzg, wd, cpad(cin), rule=0, act=actg, **kw)
    for t in (p, guided, masked):
        assert t.shape == (n, h, w, cpad(cin)) and t.dtype == storage(dtype) and bool(torch.isfinite(t.float()).all())
    assert _same_bits(guided, _gated(p, actg))                                  # the gate on rule 0's very output, zeros +0
    opened = int((guided != 0).sum())
    assert 0 < opened < guided.numel() // 2 and float(guided.float().min()) >= 0
    e_lin = rel_err(from_nhwc(p, cin), lin)
    e_mask = rel_err(from_nhwc(masked, cin), lin * torch.where(act > 0, 1.0, LEAK))
    print(f"conv_dgrad_rule[{dtype}, {case}]: rule 0 vs fp64 {e_lin:.2e} plain, {e_mask:.2e} masked; {opened} of {guided.numel()} gates open")
    assert e_lin < TOL[dtype] and e_mask < TOL[dtype]


# ---- kernel level: the guided pool gradients ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("hw", [(33, 37), (64, 64)], ids=["33x37", "64x64"])
def test_kernel_maxpool_bwd_guided(ops, dtype, hw):
    """gx = where(winner > 0 and s > 0, s, 0) with s the summed window contributions (`maxpool_bwd(lrelu_mask=False)`): the gate
    sees the sum.  Pixel (1, 2) of image 0 wins windows (0, 1) and (1, 1): channel 0 receives +1 and -3 (sum -2: closed, though
    one contribution is positive), channel 1 receives +3 and -1 (sum +2: open with 2, not 3); channel 2 wins window (2, 2) with a
    negative value and a positive gradient (closed)."""
    h, w = hw
    n, c = 2, 20
    g = torch.Generator().manual_seed(h + w)
    x = torch.randn(n, c, h, w, generator=g)
    x[0, 0:2, 1, 2] = 10.0
    x[0, 2, 3:6, 3:6] = -0.5 - torch.rand(3, 3, generator=g)
    x[0, 2, 4, 4] = -0.25
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    gy = torch.randn(n, c, ho, wo, generator=g)
    gy[0, 0, 0, 1], gy[0, 0, 1, 1] = 1.0, -3.0
    gy[0, 1, 0, 1], gy[0, 1, 1, 1] = 3.0, -1.0
    gy[0, 2, 2, 2] = 2.0
    xg, gyg = to_nhwc(round_to(x, dtype), dtype), to_nhwc(round_to(gy, dtype), dtype)
    _pool, widx = ops.maxpool_fwd(xg)
    with poison_allocations(reduce_batch=False):
        s = ops.maxpool_bwd(gyg, widx, (h, w), lrelu_mask=False)
        got = ops.maxpool_bwd(gyg, widx, (h, w), rule=1)
    assert got.shape == xg.shape and bool(torch.isfinite(got.float()).all())
    assert _same_bits(got, _gated(s, xg))                                      # a pixel's own value is its winner's value
    assert float(s[0, 1, 2, 0]) == -2.0 and float(got[0, 1, 2, 0]) == 0.0
    assert float(s[0, 1, 2, 1]) == 2.0 and float(got[0, 1, 2, 1]) == 2.0
    assert float(s[0, 4, 4, 2]) == 2.0 and float(got[0, 4, 4, 2]) == 0.0
    assert 0 < int((got != 0).sum()) < int((s != 0).sum())


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(3, 2, 2), (2, 3, 5)], ids=["3x2x2", "2x3x5"])
def test_kernel_avgpool_fc_bwd_data_guided(ops, dtype, shape):
    n, h, w = shape
    g = torch.Generator().manual_seed(17 * h + w)
    act = to_nhwc(round_to(torch.randn(n, 80, h, w, generator=g), dtype), dtype)
    dfe = torch.randn(n, 80, generator=g).cuda()
    wfc = (torch.randn(80, 80, generator=g) / 80 ** 0.5).cuda()
    pooled = torch.zeros(n, 80, device="cuda")
    with poison_allocations(reduce_batch=False):
        p = ops.avgpool_fc_bwd_data(dfe, wfc, pooled, act, masked=False)
        got = ops.avgpool_fc_bwd_data(dfe, wfc, pooled, act, rule=1)
    assert bool(torch.isfinite(got.float()).all()) and _same_bits(got, _gated(p, act))
    assert 0 < int((got != 0).sum()) < got.numel() // 2
    want = (dfe.double().cpu() @ wfc.double().cpu() / (h * w))[:, :, None, None].expand(n, 80, h, w)
    assert rel_err(from_nhwc(p, 80), want) < TOL[dtype]


# ---- kernel level: the gated stem data gradient ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("shape", [(2, 33, 37), (2, 64, 64)], ids=["2x33x37", "2x64x64"])
def test_kernel_stem_dgrad_gated(ops, dtype, shape):
    """`stem_dgrad(gate=)` is `stem_dgrad(...)[0] * (gate.float() / 255)[:, None]` bit for bit, for gates holding every byte value,
    runs of 0 and of 255 and random bytes.  Printed: how many elements a quotient taken on the DEVICE would have moved."""
    from mil_amd import _lib as L
    n, h, w = shape
    g = torch.Generator().manual_seed(31 * h + w)
    wt = round_to(torch.randn(20, 3, 7, 7, generator=g) / 147 ** 0.5, dtype)
    dstem = round_to(torch.randn(n, 20, (h + 1) // 2, (w + 1) // 2, generator=g), dtype)
    gate = torch.randint(0, 256, (n, h, w), generator=g, dtype=torch.uint8)
    gate[0].view(-1)[:256] = torch.arange(256, dtype=torch.uint8)
    gate[1, :5], gate[1, -4:], gate[1, 10:14, :7] = 0, 255, 255
    gate = gate.cuda()
    wp, _ = ops.pack_weights(wt.cuda(), None, L.PACK_STEM_DGRAD, dtype)
    dz = to_nhwc(dstem, dtype)
    plain = ops.stem_dgrad(dz, wp, (h, w))[0]
    dx = torch.full((n, 3, h, w), float("nan"), device="cuda")
    got, none = ops.stem_dgrad(dz, wp, (h, w), dx=dx, gate=gate)
    assert got is dx and none is None and bool(torch.isfinite(dx).all())
    want = plain * _quotient(gate)[:, None]
    assert _same_bits(dx, want)
    assert bool((dx[1, :, :5] == 0).all()) and torch.equal(dx[1, :, -4:], plain[1, :, -4:])
    on_device = plain * (gate.float() / 255)[:, None]
    print(f"stem_dgrad(gate=)[{dtype}, {shape}]: {int((on_device != want).sum())} of {want.numel()} elements differ with the quotient taken on the device")
    assert _same_bits(ops.stem_dgrad(dz, wp, (h, w), gate=gate)[0], dx)          # a fresh output: the same bits


# ---- encoder level -----------------------------------------------------------------------------------------------------------------
def _weights(golden_dir):
    return np.load(os.path.join(golden_dir, "weights.npz"))


def _model(golden_dir, dtype):
    import mil_amd
    w = _weights(golden_dir)
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net.eval()


def _sd64(golden_dir):
    w = _weights(golden_dir)
    return {k: torch.tensor(w[k], dtype=torch.float64) for k, _s in orc.state_dict_spec()}


def _hip_patterns(saved):
    """Activation pattern of a HIP encoder run in the form `orc.backbone(patterns=...)` takes (as tests/test_gpu_saliency.py);
    a forward cut short gives the blocks that ran."""
    widx = saved["widx"][..., :20].permute(0, 3, 1, 2).cpu()
    pat = {"stem_tap": (widx & 15).long(), "stem_pos": ((widx >> 4) & 1) == 0}
    names = [f"layer{li}.{b}" for li in range(1, 5) for b in range(3)]
    for name, (_xin, o1, out) in zip(names, saved["blocks"]):
        c = orc.STAGES[int(name[5]) - 1][1]
        pat[name + ".o1"] = (o1[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
        pat[name] = (out[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
    return pat


def _l2(got, want):
    return float((got.double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [(6, 64, 64), (3, 50, 70)], ids=["6x64x64", "3x50x70"])
def test_guided_walk_on_its_own_activation_pattern(golden_dir, dtype, case):
    """`encoder_pixel_gradient(rule="guided")` against fp64 (tests/guided_reference.py) on the linear piece the HIP forward took —
    the construction of test_encoder_input_gradient_on_its_own_activation_pattern — with a random dfeats.  The gate is 3x the
    error of the PLAIN walk measured here on the same inputs and pattern, and never below the plain walk's own gates (1e-5 fp32,
    2e-4 bf16x3, 4e-2 bf16): on a fixed forward pattern the guided map is continuous and piecewise linear in the gradient, so it has
    no flip discontinuity of its own, and 3 is the project's habitual margin.
    Measured on MI355X, L2 error relative to the norm, guided / plain of the same run: fp32 1.68e-7 / 1.08e-6 (6x64x64) and
    1.66e-7 / 1.05e-6 (3x50x70); bf16x3 4.86e-6 / 1.53e-5 and 4.80e-6 / 1.50e-5; bf16 3.17e-3 / 9.02e-3 and 2.83e-3 / 8.79e-3 —
    the gates pass sums of same-sign terms, which cancel less than the plain walk's.
    Also: the reference is nonzero in every tile and differs from the plain reference by more than 10 % of its norm, and a plain
    walk gives the same bits before and after a guided one."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    n, h, w = case
    x = synth_bag(n, h, w, 20260207)
    enc = _model(golden_dir, dtype).cnn.module
    st = L.storage_dtype(dtype)
    dfe = torch.randn(n, 80, generator=torch.Generator().manual_seed(9))
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        _feats, saved = encoder.encoder_forward(enc, x.cuda(), st)
        pat = _hip_patterns(saved)
        plain0, _ = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe.cuda())
        dx, sal = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe.cuda(), rule="guided")
        plain1, _ = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe.cuda())
    torch.cuda.synchronize()
    assert sal is None and dx.shape == x.shape and dx.dtype == torch.float32 and bool(torch.isfinite(dx).all())
    assert _same_bits(plain0, plain1)
    sd = _sd64(golden_dir)

    def grad_of(fn):
        xg = x.double().requires_grad_()
        fn(xg).backward(dfe.double())
        return xg.grad
    want = grad_of(lambda xg: gref.backbone(sd, xg, pat))
    want_plain = grad_of(lambda xg: orc.backbone(sd, xg, patterns=pat))
    assert all(float(want[t].abs().max()) > 0 for t in range(n))
    assert float((want - want_plain).norm() / want.norm()) > 0.1
    e_guided, e_plain = _l2(dx, want), _l2(plain0, want_plain)
    gate = max(WALK_FLOOR[dtype], 3 * e_plain)
    print(f"own-pattern guided walk [{dtype}, {case}]: guided {e_guided:.2e}, plain {e_plain:.2e}, gate {gate:.2e}; "
          f"|guided| {float(want.norm()):.3g}, |plain| {float(want_plain.norm()):.3g}")
    assert e_guided < gate, (e_guided, e_plain)


# ---- the classes -------------------------------------------------------------------------------------------------------------------
WGRAD_OPS = ("conv_wgrad", "conv_wgrad_pair", "conv_entry_bwd", "stem_backward", "avgpool_fc_bwd")        # tests/test_gpu_saliency.py
ONE_PASS_OPS = ("conv_bwd_fused", "conv_chain", "conv_pair", "conv_dgrad_s2")
COUNTED = WGRAD_OPS + ONE_PASS_OPS + ("stem_dgrad", "stem_dgrad_acc", "conv_dgrad_rule")


def _to_u8(x):
    return ((x * 0.5 + 0.5) * 255).round().clamp_(0, 255).to(torch.uint8)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_guided_backprop_class_bits_launches_feeds_and_side_effects(golden_dir, monkeypatch, ops, dtype):
    import mil_amd
    from mil_amd import _lib as L
    from mil_amd import guided
    from mil_amd.attribution import bag_setup, device_tiles
    from mil_amd.encoder import encoder_forward, encoder_pixel_gradient
    from mil_amd.head import head_apply
    label = 1
    model = _model(golden_dir, dtype)
    net = model.cnn.module
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(6, 64, 64, 20260207)).cuda())
    x = u8.float()
    counts = dict.fromkeys(COUNTED, 0)
    rules, walking = [], [False]

    def counted(name, real):
        def call(*a, **k):
            if walking[0]:                                                       # (the forward runs conv_pair / conv_chain too)
                counts[name] += 1
                if name == "conv_dgrad_rule":
                    rules.append(k["rule"])
            return real(*a, **k)
        return call
    for name in COUNTED:
        monkeypatch.setattr(ops, name, counted(name, getattr(ops, name)))

    def walk(*a, **k):
        """`encoder_pixel_gradient`, with the wrapper counters switched on for its duration: they count the backward walk."""
        walking[0] = True
        try:
            return encoder_pixel_gradient(*a, **k)
        finally:
            walking[0] = False
    monkeypatch.setattr(guided, "encoder_pixel_gradient", walk)

    def by_hand(**kw):
        xd = device_tiles(model, x)
        layout, y, cw = bag_setup(model, xd.shape[0], label)
        st = L.storage_dtype(dtype)
        with L.f32_mma(L.mma_code(dtype)):
            with torch.no_grad():
                feats, saved = encoder_forward(net, xd, st)
            H = feats.detach().requires_grad_()
            loss = head_apply(H, layout, y, None, cw, [w.detach() for w in model.head_weights()], None, direct=False)[0]
            (dH,) = torch.autograd.grad(loss.sum(), H)
            with torch.no_grad():
                return walk(net, saved, st, dfeats=-dH, **kw)
    by_hand()                                                                    # the plain walk: the counters see its launches
    assert counts["stem_dgrad"] == 1 and counts["conv_dgrad_rule"] == 0
    if dtype != torch.float32:                                                   # (the exact-fp32 mode has no one-pass kernels)
        assert sum(counts[k] for k in ONE_PASS_OPS) > 0
    want = by_hand(rule="guided")[0]
    want_map = by_hand(rule="guided", dx_reduce="max_abs")[1]
    for k in counts:
        counts[k] = 0
    rules.clear()

    gb = mil_amd.TileGuidedBackprop(model)
    model.train()                                                                # the flag is left alone, whatever it is
    marks = {k: torch.full_like(p, 0.5) if i % 2 else None for i, (k, p) in enumerate(model.named_parameters())}
    for k, p in model.named_parameters():
        p.grad = None if marks[k] is None else marks[k].clone()
    rng, dev_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    dx = gb.gradients(x, label)
    assert counts["stem_dgrad"] == 1 and counts["conv_dgrad_rule"] == 23 and set(rules) == {1}      # 12 blocks x 2, less block 0's conv1
    assert all(counts[k] == 0 for k in WGRAD_OPS + ONE_PASS_OPS + ("stem_dgrad_acc",)), counts
    dx_u8 = gb.gradients(u8, label)
    m = gb.maps(u8, label)
    assert counts["stem_dgrad"] == 3 and all(counts[k] == 0 for k in WGRAD_OPS + ONE_PASS_OPS + ("stem_dgrad_acc",)), counts
    assert model.training and torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), dev_rng)
    for k, p in model.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k
    assert dx.shape == x.shape and dx.dtype == torch.float32 and float(dx.abs().max()) > 0
    assert _same_bits(dx, want) and _same_bits(dx_u8, dx)
    assert m.shape == (6, 64, 64) and _same_bits(m, want_map) and torch.equal(m, dx.abs().amax(1))


def test_guided_classes_with_flat_params_leave_the_bucket_alone(golden_dir):
    """`dist.FlatParams` switches direct accumulation into the flat gradient bucket on: no guided call may add to it."""
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260211).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    gb = mil_amd.TileGuidedBackprop(net)
    gb.gradients(x, 0)
    gb.maps(x, 0)
    gb.filters(x, "layer2", 3)
    mil_amd.TileGuidedGradCam(net, "layer3").gradients(x, 0)
    assert torch.equal(flat.flat_grad, bucket)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_guided_filters_against_fp64_on_its_own_pattern(golden_dir, dtype):
    """`TileGuidedBackprop.filters` on layer2 with a different channel per tile, against the fp64 reference on the HIP forward's
    pattern: the gradient of sum_t mean(A[t, ch_t]) through the guided LeakyReLUs.  Same gate as the encoder walk: 3x the error of
    the plain walk from the plain seed (`ops.stage_seed`), measured here, and not below the plain walk's gates."""
    import mil_amd
    from mil_amd import _lib as L
    from mil_amd import ops
    from mil_amd.encoder import encoder_forward, encoder_pixel_gradient
    n, chans = 6, [0, 7, 13, 21, 30, 39]
    x = synth_bag(n, 64, 64, 20260207)
    model = _model(golden_dir, dtype)
    net = model.cnn.module
    got = mil_amd.TileGuidedBackprop(model).filters(x, "layer2", chans)
    assert got.shape == x.shape and bool(torch.isfinite(got).all())
    st = L.storage_dtype(dtype)
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        _f, saved = encoder_forward(net, x.cuda(), st, upto=2)
        pat = _hip_patterns(saved)
        _obj, seed = ops.stage_seed(saved["blocks"][-1][2], torch.tensor(chans, dtype=torch.int32).cuda(), 40)
        plain, _ = encoder_pixel_gradient(net, saved, st, dz=seed, stage=2)      # the gradient of MINUS the mean activation
    sd = _sd64(golden_dir)
    pick = torch.arange(n)

    def grad_of(stage_out):
        xg = x.double().requires_grad_()
        stage_out(xg)[pick, chans].mean(dim=(1, 2)).sum().backward()
        return xg.grad

    def plain_stage(xg):
        acts = {}
        orc.backbone(sd, xg, acts=acts, patterns={**pat, **{f"layer{li}.{b}{s}": torch.ones(1, dtype=torch.bool) for li in (3, 4) for b in range(3) for s in ("", ".o1")}})
        return acts["layer2"]
    want = grad_of(lambda xg: gref.backbone(sd, xg, pat, upto=2))
    want_plain = -grad_of(plain_stage)
    assert all(float(want[t].abs().max()) > 0 for t in range(n))
    e_guided, e_plain = _l2(got, want), _l2(plain, want_plain)
    gate = max(WALK_FLOOR[dtype], 3 * e_plain)
    print(f"guided filters [{dtype}, layer2 {chans}]: guided {e_guided:.2e}, plain {e_plain:.2e}, gate {gate:.2e}")
    assert e_guided < gate, (e_guided, e_plain)
    one = mil_amd.TileGuidedBackprop(model).filters(x, "layer2", 7)              # one int: that channel for every tile
    assert _same_bits(one[1], got[1]) and not torch.equal(one[0], got[0])


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("layer,normalize", [("layer4", "tile"), ("layer2", "bag")])
def test_guided_gradcam_is_the_product_of_its_two_classes_in_one_forward(golden_dir, monkeypatch, ops, dtype, layer, normalize):
    import mil_amd
    from mil_amd import attribution
    label = 2
    model = _model(golden_dir, dtype)
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(6, 64, 64, 20260207)).cuda())
    x = u8.float()
    guided = mil_amd.TileGuidedBackprop(model).gradients(x, label)
    cam = mil_amd.TileGradCam(model, layer).maps(x, label, offset=0.5, normalize=normalize)
    assert cam.dtype == torch.uint8 and int(cam.max()) > int(cam.min())
    want = guided * _quotient(cam)[:, None]
    forwards, stem_launches = [], []
    real_fwd, real_dgrad = attribution.encoder_forward, ops.stem_dgrad
    monkeypatch.setattr(attribution, "encoder_forward", lambda *a, **k: (forwards.append(1), real_fwd(*a, **k))[1])
    monkeypatch.setattr(ops, "stem_dgrad", lambda *a, **k: (stem_launches.append(k.get("gate")), real_dgrad(*a, **k))[1])
    both = mil_amd.TileGuidedGradCam(model, layer)
    got = both.gradients(x, label, offset=0.5, normalize=normalize)
    assert len(forwards) == 1 and len(stem_launches) == 1 and torch.equal(stem_launches[0], cam)     # one forward, one gated launch
    assert got.shape == x.shape and got.dtype == torch.float32 and _same_bits(got, want)
    assert _same_bits(both.gradients(u8, label, offset=0.5, normalize=normalize), got)
    assert all(p.grad is None for p in model.parameters())
