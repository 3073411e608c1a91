"""-m gpu: activation maximisation — `ops.stage_seed` and `ops.pixel_step` against their numpy restatements bit for bit, the
truncated forward and the weight-gradient-free walk against the passes they shorten, the filter gradient against fp64 on the
encoder's own activation pattern, and `mil_amd.FeatureVisualizer` against the loop it replaces and against the CPU oracle's gain.
Every output buffer a kernel is handed is NaN-filled or 255-filled first."""
import functools
import os

import numpy as np
import pytest
import torch

import feature_vis_reference as ref
import slice_sum_reference as tree
from fixture_inputs import synth_bag
from gpu_util import X3, cpad
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]
CASES = [(6, 64, 64), (3, 50, 70)]
CASE_IDS = ["6x64x64", "3x50x70"]
NAN = float("nan")


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _bits(t):
    """The tensor's bytes as integers, on the CPU: equality of these is equality bit for bit (a NaN equals itself, -0 is not +0)."""
    t = t.detach().contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _weights(golden_dir):
    return np.load(os.path.join(golden_dir, "weights.npz"))


def _model(golden_dir, dtype):
    import mil_amd
    w = _weights(golden_dir)
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net.eval()


def _to_u8(x):
    return ((x * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)


# ---- 1. stage_seed -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (33, 37)], ids=["5x7", "16x16", "33x37"])
@pytest.mark.parametrize("c", [20, 40, 60, 80])
def test_stage_seed_against_numpy(ops, c, hw, dtype):
    h, w = hw
    chans = [0, c // 2, c - 1]
    g = torch.Generator().manual_seed(1000 * c + 37 * h + w)
    a = torch.randn(3, h, w, cpad(c), generator=g)
    a[torch.rand(a.shape, generator=g) < 0.15] = 0.0                              # exact zeros: the branch rule is a strict > 0
    for t, k in enumerate(chans):                                                # every chosen channel holds a zero, a negative, a positive
        a[t, 0, 0, k], a[t, 1, 0, k], a[t, 2, 0, k] = 0.0, -0.5, 0.5
    act = a.to(dtype).cuda()
    stored = act.float().cpu().numpy()
    j64, dz_ref = ref.stage_seed(stored, chans, c)
    ch = torch.tensor(chans, dtype=torch.int32).cuda()
    obj = torch.full((3,), NAN, device="cuda")
    dz = torch.full(act.shape, NAN, device="cuda").to(dtype)
    got = ops.stage_seed(act, ch, c, objective=obj, dz=dz)
    assert got[0] is obj and got[1] is dz
    assert _same(dz, torch.from_numpy(dz_ref).to(dtype))                          # the channel, zero elsewhere, zero padding
    for t, k in enumerate(chans):
        other = [j for j in range(cpad(c)) if j != k]
        assert float(dz[t][..., other].float().abs().max()) == 0.0 and float(dz[t][..., k].float().max()) < 0.0
    bound = h * w * 2.0 ** -24 * np.abs(stored[np.arange(3), :, :, chans].astype(np.float64)).mean(axis=(1, 2))
    err = np.abs(obj.cpu().numpy().astype(np.float64) - j64)
    print(f"stage_seed[c={c}, {h}x{w}, {dtype}]: |J - J64| {err.max():.2e}, bound {bound.min():.2e}")
    assert (err <= bound).all(), (err, bound)
    assert _same(obj, torch.from_numpy(tree.stage_seed_objective(stored, chans)))  # the summation tree itself
    obj2, dz2 = ops.stage_seed(act, ch, c)                                       # fresh outputs, second run: the same bits
    assert _same(obj2, obj) and _same(dz2, dz)


# ---- 2. pixel_step -------------------------------------------------------------------------------------------------------------
def _buffer(values, misalign, dtype=torch.float32):
    """A contiguous device tensor holding `values`; misalign: its first element sits 4 bytes (uint8: 1 byte) off the 16-byte grid,
    which sends the kernel down its element-by-element path."""
    flat = torch.empty(values.numel() + 4, dtype=dtype, device="cuda")
    view = flat[1:1 + values.numel()] if misalign else flat[:values.numel()]
    view = view.view(values.shape)
    view.copy_(values.to(dtype))
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


@pytest.mark.parametrize("project", ["none", "clamp", "u8"])
@pytest.mark.parametrize("rule", ["sgd", "adam"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 33, 37), (3, 3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_pixel_step_bit_for_bit(ops, shape, rule, project):
    """30 steps carried through on the device and in numpy fp32; x, m, v and the bytes compared at steps 1, 2 and 30.  The start
    lies in [-1, 1] and the steps are large, so x leaves that range; a patch with x = g = 0 keeps v = 0 (a 0 / eps quotient);
    the smallest shape sits off the 16-byte grid and has a short last group."""
    rng = np.random.default_rng(sum(shape) + len(rule) + 7 * len(project))
    misalign = shape[0] == 1
    kw = dict(rule=rule, lr=6.0 if rule == "sgd" else 0.1, weight_decay=1e-4 if rule == "sgd" else 1e-6, betas=(0.9, 0.999), eps=1e-8,
              project=project)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    x[0, 0, :2, :3] = 0.0
    m, v = np.zeros_like(x), np.zeros_like(x)
    dx = _buffer(torch.from_numpy(x), misalign)
    plain = dx.clone()                                                           # the same steps without u8_out
    state = (_buffer(torch.zeros(shape), misalign), _buffer(torch.zeros(shape), misalign)) if rule == "adam" else None
    state_plain = tuple(torch.zeros(shape, device="cuda") for _ in range(2)) if rule == "adam" else None
    left = False
    for step in range(1, 31):
        g = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 0)).astype(np.float32)
        g[0, 0, :2, :3] = 0.0
        x, m, v, codes = ref.pixel_step(x, g, m, v, step=step, **kw)
        left = left or bool((np.abs(x) > 1).any())
        dg = _buffer(torch.from_numpy(g), misalign)
        u8 = _buffer(torch.full(shape, 255, dtype=torch.uint8), misalign, torch.uint8)
        assert ops.pixel_step(dx, dg, state, step=step, u8_out=u8, **kw) is dx
        ops.pixel_step(plain, dg.clone(), state_plain, step=step, **kw)
        if step in (1, 2, 30):
            assert _same(dx, torch.from_numpy(x)), step
            assert torch.equal(u8.cpu(), torch.from_numpy(codes)), step
            if rule == "adam":
                assert _same(state[0], torch.from_numpy(m)) and _same(state[1], torch.from_numpy(v)), step
    assert _same(plain, dx) and (rule == "sgd" or (_same(state_plain[0], state[0]) and _same(state_plain[1], state[1])))
    assert project != "none" or left                                             # x did reach outside [-1, 1]
    if project != "u8":                                                          # (code 128 decodes to 1/255, not to 0)
        assert np.all(x[0, 0, :2, :3] == 0) and np.all(v[0, 0, :2, :3] == 0)
    if project == "clamp":
        assert float(dx.abs().max()) == 1.0
    if project == "u8":
        assert _same(dx, torch.from_numpy(ref.decode_table())[torch.from_numpy(codes).long()])


# ---- 3. / 4. the truncated forward and the weight-gradient-free walk -----------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_truncated_forward_keeps_the_full_forwards_blocks(golden_dir, dtype, case):
    from mil_amd import _lib as L
    from mil_amd import encoder
    n, h, w = case
    x = synth_bag(n, h, w, 20260301).cuda()
    enc = _model(golden_dir, dtype).cnn.module
    st = L.storage_dtype(dtype)
    seen = []

    class Watcher:
        def observe(self, *a):
            seen.append(1)
    enc.activation_summary = Watcher()
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        feats, full = encoder.encoder_forward(enc, x, st)
        assert feats is not None and len(full["blocks"]) == 12 and len(seen) == 1
        for upto in (1, 2, 3, 4):
            none, cut = encoder.encoder_forward(enc, x, st, upto=upto)
            assert none is None and "pooled" not in cut and len(cut["blocks"]) == 3 * upto and len(seen) == 1
            for kept, whole in zip(cut["blocks"], full["blocks"]):
                assert all(_same(a, b) for a, b in zip(kept, whole))
            assert torch.equal(cut["widx"], full["widx"]) and cut["stem_hw"] == full["stem_hw"] and cut["tile_hw"] == full["tile_hw"]
    enc.activation_summary = None


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_pixel_gradient_is_encoder_backwards_dx_without_weight_gradients(golden_dir, dtype, case, monkeypatch):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    n, h, w = case
    x = synth_bag(n, h, w, 20260302).cuda()
    enc = _model(golden_dir, dtype).cnn.module
    st = L.storage_dtype(dtype)
    dfe = torch.randn(n, 80, generator=torch.Generator().manual_seed(11)).cuda()
    calls = {}
    for name in ("conv_wgrad", "conv_wgrad_pair", "conv_entry_bwd", "stem_backward", "stem_dgrad", "avgpool_fc_bwd"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, functools.partial(lambda real, name, *a, **k: (calls.__setitem__(name, calls.get(name, 0) + 1), real(*a, **k))[1], real, name))
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        _feats, saved = encoder.encoder_forward(enc, x, st)
        dx, sal = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe)
        assert calls == {"stem_dgrad": 1} and sal is None
        none, sal2 = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe, dx_reduce="max_abs")
        acc = torch.zeros_like(dx)
        assert encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dfe, dx_acc=(acc, 1.0)) == (None, None)
        assert calls == {"stem_dgrad": 2}
        _grads, want, _s = encoder.encoder_backward(enc, saved, dfe, st, want_dx=True)
        assert calls["conv_wgrad"] > 0 and calls["avgpool_fc_bwd"] == 1           # the counters do see the full backward's launches
    assert dx.shape == x.shape and bool(torch.isfinite(dx).all()) and float(dx.abs().max()) > 0
    assert _same(dx, want)
    assert none is None and _same(sal2, want.abs().amax(1)) and _same(acc, want)
    assert all(p.grad is None for p in enc.parameters())


# ---- 5. the filter gradient on its own activation pattern ----------------------------------------------------------------------
def _hip_patterns(saved):
    """Activation pattern of a HIP encoder run in the form `orc.backbone(patterns=...)` takes (as tests/test_gpu_saliency.py)."""
    widx = saved["widx"][..., :20].permute(0, 3, 1, 2).cpu()
    pat = {"stem_tap": (widx & 15).long(), "stem_pos": ((widx >> 4) & 1) == 0}
    names = [f"layer{li}.{b}" for li in range(1, 5) for b in range(3)]
    for name, (_xin, o1, out) in zip(names, saved["blocks"]):
        c = orc.STAGES[int(name[5]) - 1][1]
        pat[name + ".o1"] = (o1[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
        pat[name] = (out[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
    return pat


FILTER_GATES = {torch.float32: 1e-5, X3: 2e-4, torch.bfloat16: 4e-2}


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_filter_gradient_on_its_own_activation_pattern(golden_dir, dtype, case):
    """d(-sum_t J_t)/d tiles for every stage against fp64 on the linear piece the HIP forward took (the rule of
    test_encoder_input_gradient_on_its_own_activation_pattern and its gates: L2 error of dx relative to its norm within 1e-5 for
    fp32, 2e-4 for bf16x3, 4e-2 for bf16; the chain here is that test's or shorter).  The seed in bf16 storage carries the
    rounding of -(1/(h w)) to bf16, up to 2^-9, which that test's fp32 feature gradient does not.
    Measured on MI355X, layer1 / layer2 / layer3 / layer4 at 6x64x64: fp32 3.13e-7 / 6.74e-7 / 9.05e-7 / 1.06e-6; bf16x3
    7.47e-6 / 1.17e-5 / 1.34e-5 / 1.75e-5; bf16 4.61e-3 / 6.56e-3 / 8.08e-3 / 9.47e-3.  At 3x50x70: fp32 3.19e-7 / 7.01e-7 /
    8.96e-7 / 1.10e-6; bf16x3 7.31e-6 / 1.14e-5 / 1.50e-5 / 1.65e-5; bf16 4.23e-3 / 6.25e-3 / 8.47e-3 / 9.66e-3 — the error
    grows with the length of the chain, and the layer-4 figures are those of the full input gradient (1.08e-6, 1.53e-5, 9.02e-3)."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    n, h, w = case
    x = synth_bag(n, h, w, 20260303)
    wts = _weights(golden_dir)
    enc = _model(golden_dir, dtype).cnn.module
    st = L.storage_dtype(dtype)
    got = {}
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        _feats, saved = encoder.encoder_forward(enc, x.cuda(), st)
        pat = _hip_patterns(saved)
        for stage, c in enumerate(encoder.STAGE_WIDTHS, 1):
            chans = [(7 * t + 3) % c for t in range(n)]
            ch = torch.tensor(chans, dtype=torch.int32).cuda()
            _j, dz = ops.stage_seed(saved["blocks"][3 * stage - 1][2], ch, c)
            got[stage] = (chans, encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)[0].double().cpu())
    sd64 = {k: torch.tensor(wts[k], dtype=torch.float64) for k, _s in orc.state_dict_spec()}
    x64 = x.double().requires_grad_()
    acts = {}
    orc.backbone(sd64, x64, acts=acts, patterns=pat)
    errs = []
    for stage, (chans, dx) in got.items():
        loss = -sum(acts[f"layer{stage}"][t, k].mean() for t, k in enumerate(chans))
        (want,) = torch.autograd.grad(loss, x64, retain_graph=True)
        errs.append(float((dx - want).norm() / want.norm()))
    print(f"own-pattern filter gradient [{dtype}, {case}]: layer1..4 " + " / ".join(f"{e:.2e}" for e in errs))
    assert all(e < FILTER_GATES[dtype] for e in errs), errs


# ---- 6. the class equals the loop it replaces ----------------------------------------------------------------------------------
def _manual_filter_loop(fv, x, stage, chans, steps, kw):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    enc, mode = fv.net, fv.net.compute_dtype
    st = L.storage_dtype(mode)
    c = encoder.STAGE_WIDTHS[stage - 1]
    ch = torch.tensor(chans, dtype=torch.int32).cuda()
    state = (torch.zeros_like(x), torch.zeros_like(x)) if kw["rule"] == "adam" else None
    trace = torch.full((steps, x.shape[0]), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(mode)), torch.no_grad():
        for k in range(steps):
            _f, saved = encoder.encoder_forward(enc, x, st, upto=stage)
            j, dz = ops.stage_seed(saved["blocks"][-1][2], ch, c)
            trace[k] = j
            g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)
            ops.pixel_step(x, g, state, step=k + 1, u8_out=u8 if k == steps - 1 else None, **kw)
    return x, u8, trace


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_visualizer_equals_the_loop_it_replaces(golden_dir, dtype):
    import mil_amd
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    from mil_amd.head import head_apply
    from mil_amd.saliency import bag_setup
    model = _model(golden_dir, dtype)
    adam = dict(rule="adam", lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, project="none")
    # filters: three channels of layer2, odd tile size
    fv = mil_amd.FeatureVisualizer(model)
    chans = [0, 19, 39]
    res = fv.filters("layer2", channels=chans, size=(50, 70), steps=3, seed=4)
    start = torch.randint(150, 180, (3, 3, 50, 70), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    x, u8, trace = _manual_filter_loop(fv, mil_amd.U8Tiles(start.cuda()).float(), 2, chans, 3, adam)
    assert isinstance(res.u8, mil_amd.U8Tiles) and res.trace.shape == (3, 3) and bool(torch.isfinite(res.trace).all())
    assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace)
    again = fv.filters("layer2", channels=chans, size=(50, 70), steps=3, seed=4)
    assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace)
    assert not _same(fv.filters("layer2", channels=chans, size=(50, 70), steps=3, seed=5).x, res.x)
    # dream: SGD with the clamp, from real tiles as bytes and as the fp32 stack they decode to; the bare encoder is enough
    sgd = dict(rule="sgd", lr=12.0, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, project="clamp")
    fd = mil_amd.FeatureVisualizer(model.cnn.module, "sgd", lr=12, weight_decay=1e-4, project="clamp")
    tiles = mil_amd.U8Tiles(_to_u8(synth_bag(4, 64, 64, 20260304)).cuda())
    dres = fd.dream(tiles, "layer3", 31, steps=3)
    x, u8, trace = _manual_filter_loop(fd, tiles.float(), 3, [31] * 4, 3, sgd)
    assert _same(dres.x, x) and _same(dres.u8.u8, u8) and _same(dres.trace, trace)
    dres2 = fd.dream(tiles.float(), "layer3", [31] * 4, steps=3)
    assert _same(dres2.x, x) and _same(dres2.u8.u8, u8) and _same(dres2.trace, trace)
    # classes: the class-specific method's settings — SGD at lr 6 on an image that goes through bytes every step
    fc = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8")
    cres = fc.classes(2, 4, size=(64, 64), steps=3, seed=9)
    enc, st = model.cnn.module, L.storage_dtype(dtype)
    x = mil_amd.U8Tiles(torch.randint(0, 256, (4, 3, 64, 64), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).cuda()).float()
    layout, y, cw = bag_setup(model, 4, 2)
    trace = torch.full((3, 4), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(dtype)):
        for k in range(3):
            with torch.no_grad():
                feats, saved = encoder.encoder_forward(enc, x, st)
            H = feats.detach().requires_grad_(True)
            loss = head_apply(H, layout, y, None, cw, [p.detach() for p in model.head_weights()], None, direct=False)[0]
            (dH,) = torch.autograd.grad(loss.sum(), H)
            with torch.no_grad():
                trace[k] = -loss.detach()
                g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dH)
                ops.pixel_step(x, g, None, rule="sgd", lr=6, weight_decay=0, step=k + 1, project="u8", u8_out=u8 if k == 2 else None)
    assert _same(cres.x, x) and _same(cres.u8.u8, u8) and _same(cres.trace, trace)
    assert _same(cres.u8.float(), cres.x)                                        # project="u8": the stack IS its bytes
    again = fc.classes(2, 4, size=(64, 64), steps=3, seed=9)
    assert _same(again.x, cres.x) and _same(again.u8.u8, cres.u8.u8) and _same(again.trace, cres.trace)


# ---- 7. it climbs ---------------------------------------------------------------------------------------------------------------
CLIMB_CHANNELS = {"layer1": [0, 7, 19], "layer2": [0, 19, 39], "layer3": [0, 31, 59], "layer4": [0, 41, 79]}


def _start_stack(ntiles, size, init, seed):
    u8 = torch.randint(init[0], init[1], (ntiles, 3, size[0], size[1]), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)
    return torch.from_numpy(ref.decode_table())[u8.long()]


@functools.lru_cache(maxsize=None)
def _oracle_climb(golden_dir, layer, size):
    """Gain of the toolkit's loop on the CPU oracle (fp32): J after 10 Adam steps minus J at the start, per tile; computed once
    per case and shared by the three modes."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    w = _weights(golden_dir)
    sd = {k: torch.tensor(w[k]) for k, _s in orc.state_dict_spec()}
    _x, trace = ref.oracle_filter_loop(orc, sd, _start_stack(3, size, (150, 180), 0), layer, CLIMB_CHANNELS[layer], 10)
    assert bool((trace[1:] > trace[:-1]).all())                                  # the reference climbs at every step
    return trace[0], trace[-1] - trace[0]


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("size", [(64, 64), (50, 70)], ids=["64x64", "50x70"])
@pytest.mark.parametrize("layer", list(CLIMB_CHANNELS))
def test_filters_climb_at_least_half_as_far_as_the_oracle(golden_dir, layer, size, dtype):
    """Golden weights, 10 Adam steps with the toolkit's defaults from seed 0: objective(final) - trace[0] is at least half the
    gain of the same loop on the CPU oracle, per tile.  Trajectories are not compared point by point: Adam's m / sqrt(v) turns a
    rounding difference in a near-zero gradient into +-lr."""
    import mil_amd
    j0, gain = _oracle_climb(golden_dir, layer, size)
    fv = mil_amd.FeatureVisualizer(_model(golden_dir, dtype))
    chans = CLIMB_CHANNELS[layer]
    res = fv.filters(layer, channels=chans, size=size, steps=10, seed=0)
    final = fv.objective(res.x, layer, chans)
    got = (final - res.trace[0]).cpu()
    print(f"climb[{layer}, {size}, {dtype}]: J0 {res.trace[0].cpu().tolist()} (oracle {j0.tolist()}), gain {got.tolist()} (oracle {gain.tolist()})")
    assert bool((gain > 0).all()) and bool((got >= 0.5 * gain).all()), (got, gain)
    assert _same(fv.objective(res.u8, layer, chans), fv.objective(res.u8.float(), layer, chans))


@functools.lru_cache(maxsize=None)
def _oracle_class_descent(golden_dir, label):
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    w = _weights(golden_dir)
    sd = {k: torch.tensor(w[k]) for k, _s in orc.state_dict_spec()}
    x = _start_stack(4, (64, 64), (0, 256), 0).requires_grad_()
    opt = torch.optim.Adam([x], lr=0.1, weight_decay=1e-6)
    y = torch.tensor([label])
    losses = []
    for _ in range(10):
        opt.zero_grad()
        loss = orc.mil_head(sd, orc.backbone(sd, x), y)["loss"]
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        losses.append(float(orc.mil_head(sd, orc.backbone(sd, x), y)["loss"]))
    return losses[0], losses[0] - losses[-1]


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_classes_lower_the_loss_at_least_half_as_far_as_the_oracle(golden_dir, dtype):
    import mil_amd
    from mil_amd.saliency import bag_setup, bag_step
    label = 2
    loss0, gain = _oracle_class_descent(golden_dir, label)
    model = _model(golden_dir, dtype)
    res = mil_amd.FeatureVisualizer(model).classes(label, ntiles=4, size=(64, 64), steps=10)
    assert res.trace.shape == (10, 4) and bool((res.trace == res.trace[:, :1]).all())
    final = bag_step(model, bag_setup(model, 4, label), res.x, backward=False)[2]
    got = float(-res.trace[0, 0] - final[0])
    print(f"classes[{dtype}]: loss {float(-res.trace[0, 0]):.4f} -> {float(final[0]):.4f} (oracle {loss0:.4f}, gain {gain:.4f})")
    assert gain > 0 and got >= 0.5 * gain, (got, gain)


# ---- 8. side effects ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_visualizer_leaves_the_model_as_it_found_it(golden_dir, dtype):
    import mil_amd
    net = _model(golden_dir, dtype)
    net.train()                                                                  # the flag is left alone, whatever it is
    marks = {k: torch.full_like(p, 0.5) if i % 2 else None for i, (k, p) in enumerate(net.named_parameters())}
    for k, p in net.named_parameters():
        p.grad = None if marks[k] is None else marks[k].clone()
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(3, 64, 64, 20260305)).cuda())
    before = u8.u8.clone()
    f32 = u8.float()
    kept = f32.clone()
    rng, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    fv = mil_amd.FeatureVisualizer(net)
    fv.filters("layer1", channels=[0, 7], size=(64, 64), steps=2)
    fv.dream(u8, "layer4", 41, steps=2)
    fv.dream(f32, "layer2", [0, 1, 2], steps=2)
    fv.objective(u8, "layer3", 5)
    fv.classes(1, 4, size=(64, 64), steps=2)
    assert torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), rng_gpu) and net.training
    assert torch.equal(u8.u8, before) and torch.equal(f32, kept)
    for k, p in net.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k


def test_feature_visualizer_with_flat_params_leaves_the_bucket_alone(golden_dir):
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260306).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    fv = mil_amd.FeatureVisualizer(net)
    fv.filters("layer3", channels=[0, 31], size=(64, 64), steps=2)
    fv.classes(0, 4, size=(64, 64), steps=2)
    assert torch.equal(flat.flat_grad, bucket)
