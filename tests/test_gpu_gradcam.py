"""-m gpu: Grad-CAM on the device — `ops.grad_cam` (csrc/grad_cam.hip) against fp64 and against the numpy / Pillow restatement of
tests/gradcam_reference.py, `encoder.encoder_stage_gradient` against fp64 on the run's own activation pattern, and
`mil_amd.TileGradCam` against the CPU oracle, with its side effects and launch counts."""
import functools
import os

import numpy as np
import pytest
import torch

import gradcam_reference as ref
from fixture_inputs import synth_bag
from gpu_util import X3
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


# ---- kernel level ------------------------------------------------------------------------------------------------------------
# (n, h, w, c, cs, H, W)
SHAPES = [(3, 8, 8, 80, 80, 256, 256), (2, 2, 3, 80, 80, 50, 70), (2, 13, 18, 20, 24, 50, 70), (2, 7, 9, 40, 40, 50, 70),
          (2, 10, 10, 60, 64, 300, 300), (1, 1, 1, 80, 80, 32, 32),       # one pixel: a constant tile -> zeros
          (1, 64, 64, 20, 24, 256, 256), (1, 128, 128, 20, 24, 512, 512),  # the LDS limit
          (1, 16, 16, 60, 64, 16, 16)]                                     # both passes skipped


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    """(act, grad) [n,h,w,cs] on the CPU in the storage type: the values the kernel reads, NaN in the pad channels.  The
    gradients have a channel mean of either sign, so the channel weights do and the ReLU cuts about half the pixels at offset 0.
    Made once, shared, never changed."""
    n, h, w, c, cs, _H, _W = shape
    g = torch.Generator().manual_seed(1000 * h + 10 * w + c)
    act = torch.randn(n, h, w, cs, generator=g)
    grad = torch.randn(n, h, w, cs, generator=g) + torch.randn(n, 1, 1, cs, generator=g)
    act[..., c:] = float("nan")
    grad[..., c:] = float("nan")
    return act.to(dtype), grad.to(dtype)


def _tables(ops, h, H, w, W):
    from mil_amd import _lib as L
    _ks, yb, yk = ops.resample_tables(h, H, L.FILTER_LANCZOS, "cpu")
    _ks, xb, xk = ops.resample_tables(w, W, L.FILTER_LANCZOS, "cpu")
    return (yb.numpy(), yk.numpy()), (xb.numpy(), xk.numpy())


@pytest.mark.parametrize("offset", [0.0, 1.0], ids=["offset0", "offset1"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grad_cam_kernel(ops, shape, dtype, offset):
    """raw against fp64 within the forward error bound of fp32 summation in any order (gradcam_reference.raw_gate: derived, not
    measured); out bit for bit the numpy / Pillow restatement applied to the same launch's raw, with each tile's own range and
    with a given one; the same bytes with and without the raw store, and from a second launch."""
    n, h, w, c, cs, H, W = shape
    act, grad = _case(shape, dtype)
    a, g = act.cuda(), grad.cuda()
    raw, out = ops.grad_cam(a, g, c, (H, W), offset=offset)
    assert raw.shape == (n, h, w) and raw.dtype == torch.float32 and out.shape == (n, H, W) and out.dtype == torch.uint8
    assert bool(torch.isfinite(raw).all())                                      # the pad channels hold NaN
    r = raw.cpu().numpy()
    want = ref.raw_map(act.float().numpy(), grad.float().numpy(), c, offset)
    gate = ref.raw_gate(act.float().numpy(), grad.float().numpy(), c, offset)
    err = np.abs(r.astype(np.float64) - want)
    cut = float((want == 0).mean())
    print(f"grad_cam[{dtype}, {shape}, offset {offset}]: max |err| / gate {float((err / gate).max()):.3f}; the ReLU cuts {cut:.2f} of the pixels")
    assert (err <= gate).all(), float((err / gate).max())
    if offset == 0.0 and h * w >= 49:
        assert 0.2 < cut < 0.8
    ytab, xtab = _tables(ops, h, H, w, W)
    o = out.cpu().numpy()
    assert np.array_equal(o, ref.resize_u8(ref.quantise(r), ytab, xtab, H, W))
    if h * w == 1:
        assert not o.any()                                                      # mx == mn: zeros, where the toolkit divides by zero
    # one range for all tiles, inside the values' own range: the clamp works on both sides
    lo, hi = (float(v) for v in np.quantile(r, [0.3, 0.8]))
    rng = torch.tensor([lo, hi], dtype=torch.float32, device="cuda")
    none, out_r = ops.grad_cam(a, g, c, (H, W), offset=offset, value_range=rng, want_raw=False)
    assert none is None
    assert np.array_equal(out_r.cpu().numpy(), ref.resize_u8(ref.quantise(r, (rng[0].item(), rng[1].item())), ytab, xtab, H, W))
    # with and without the raw store; raw alone; a second launch
    none, out2 = ops.grad_cam(a, g, c, (H, W), offset=offset, want_raw=False)
    assert none is None and torch.equal(out2, out)
    raw2, none = ops.grad_cam(a, g, c, (H, W), offset=offset, want_map=False)
    assert none is None and torch.equal(raw2, raw)
    raw3, out3 = ops.grad_cam(a, g, c, (H, W), offset=offset)
    assert torch.equal(raw3, raw) and torch.equal(out3, out)


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
    """Activation pattern of a HIP encoder run in the form `orc.backbone(patterns=...)` takes (as tests/test_gpu_saliency.py)."""
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
def test_stage_gradient_on_its_own_activation_pattern(golden_dir, dtype, case):
    """The gradient of the OUTPUT of stages 2 and 4 against fp64 on the linear piece the HIP forward took (the rule and the gates
    of test_encoder_input_gradient_on_its_own_activation_pattern): L2 error relative to the norm within 1e-5 (fp32), 2e-4
    (bf16x3), and for bf16 max(4e-2, 3 e) with e the error of the conv1.weight gradient of a full backward of the same input.
    Measured on MI355X (stage 2 / stage 4 / conv1.weight of the same input): see DESIGN.md section 3.36."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    n, h, w = case
    x = synth_bag(n, h, w, 20260301)
    wts = _weights(golden_dir)
    net = _model(golden_dir, dtype)
    enc = net.cnn.module
    st = L.storage_dtype(dtype)
    dfe = torch.randn(n, 80, generator=torch.Generator().manual_seed(11))
    with L.f32_mma(L.mma_code(dtype)):
        with torch.no_grad():
            _feats, saved = encoder.encoder_forward(enc, x.cuda(), st)
            pat = _hip_patterns(saved)
            got = {k: encoder.encoder_stage_gradient(enc, saved, dfe.cuda(), st, k) for k in (2, 4)}
            _f2, saved2 = encoder.encoder_forward(enc, x.cuda(), st)
            full = encoder.encoder_backward(enc, saved2, dfe.cuda(), st)
    torch.cuda.synchronize()
    sd64 = {k: torch.tensor(wts[k], dtype=torch.float64, requires_grad=True) for k, _s in orc.state_dict_spec()}
    acts = {}
    feats64 = orc.backbone(sd64, x.double(), acts=acts, patterns=pat)
    for k in (2, 4):
        acts[f"layer{k}"].retain_grad()
    feats64.backward(dfe.double())
    g64 = sd64["cnn.module.conv1.weight"].grad
    e_w = float((full[0].double().cpu() - g64).norm() / g64.norm())
    gate = {torch.float32: 1e-5, X3: 2e-4, torch.bfloat16: max(4e-2, 3 * e_w)}[dtype]
    errs = {}
    for k in (2, 4):
        c = orc.STAGES[k - 1][1]
        want = acts[f"layer{k}"].grad
        g = got[k]
        assert g.dtype == st and g.shape == saved["blocks"][3 * k - 1][2].shape and g.shape[-1] == (c + 7) // 8 * 8
        gk = g[..., :c].double().permute(0, 3, 1, 2).cpu()
        assert gk.shape == want.shape and bool(torch.isfinite(gk).all())
        errs[k] = float((gk - want).norm() / want.norm())
    print(f"own-pattern stage gradient [{dtype}, {case}]: stage 2 {errs[2]:.2e}, stage 4 {errs[4]:.2e}; conv1.weight gradient of the same input {e_w:.2e}")
    assert errs[2] < gate and errs[4] < gate, (errs, e_w)


# ---- model level -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_raw(golden_dir, label):
    """(tiles, {layer: fp32 oracle raw}, {layer: fp64 oracle raw}) at offset 0 for layer2 and layer4: the toolkit's hooks as
    `acts=` and autograd of minus the loss.  Computed once."""
    torch.set_num_threads(max(1, min(64, os.cpu_count() or 1)))
    x = synth_bag(8, 64, 64, 20260302)
    w = _weights(golden_dir)
    y = torch.tensor([label])
    out = []
    for dt in (torch.float32, torch.float64):
        sd = {k: torch.tensor(w[k], dtype=dt) for k, _s in orc.state_dict_spec()}
        acts = {}
        xl = x.clone().to(dt).requires_grad_()
        loss = orc.mil_head(sd, orc.backbone(sd, xl, acts=acts), y)["loss"]
        a2, a4 = acts["layer2"], acts["layer4"]
        g2, g4 = torch.autograd.grad(-loss, [a2, a4])
        out.append({name: torch.relu((g.mean(dim=(2, 3), keepdim=True) * a).sum(1)).detach()
                    for name, a, g in (("layer2", a2, g2), ("layer4", a4, g4))})
    return x, out[0], out[1]


@pytest.mark.parametrize("layer", ["layer4", "layer2"])
@pytest.mark.parametrize("dtype", [torch.float32, X3], ids=["fp32", "bf16x3"])
def test_tile_grad_cam_raw_against_the_cpu_oracle(golden_dir, dtype, layer):
    """raw(offset=0) of an 8-tile bag against the CPU oracle.  This is test_tile_saliency_against_the_cpu_oracle's backward chain
    cut short, so its bound holds: L2 distance from the fp64 oracle at most 3x the fp32 oracle's own, or 2e-2 (fp32) / 8e-2
    (bf16x3), whichever is larger.  Measured on MI355X: see DESIGN.md section 3.36."""
    import mil_amd
    label = 2
    x, r32, r64 = _oracle_raw(golden_dir, label)
    net = _model(golden_dir, dtype)
    raw = mil_amd.TileGradCam(net, layer=layer).raw(x.cuda(), label, offset=0.0)
    want = r64[layer]
    assert raw.shape == want.shape and raw.dtype == torch.float32 and float(want.norm()) > 0
    e_orc = float((r32[layer].double() - want).norm() / want.norm())
    e_hip = float((raw.double().cpu() - want).norm() / want.norm())
    print(f"TileGradCam.raw [{dtype}, {layer}]: L2 distance from fp64 {e_hip:.2e} (fp32 oracle: {e_orc:.2e})")
    assert e_hip <= max(3.0 * e_orc, 2e-2 if dtype == torch.float32 else 8e-2), (e_hip, e_orc)


def _to_u8(x):
    return ((x * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8)


def _restated_maps(ops, raw, hw, value_range=None):
    n, h, w = raw.shape
    ytab, xtab = _tables(ops, h, hw[0], w, hw[1])
    return ref.resize_u8(ref.quantise(raw.cpu().numpy(), value_range), ytab, xtab, *hw)


@pytest.mark.parametrize("layer", ["layer4", "layer2"])
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_tile_grad_cam_maps_feeds_side_effects_and_launches(golden_dir, ops, dtype, layer, monkeypatch):
    import mil_amd
    from mil_amd import encoder
    net = _model(golden_dir, dtype)
    cam = mil_amd.TileGradCam(net, layer=layer)
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(8, 50, 70, 20260303)).cuda())           # non-square tiles: maps are [H,W]
    x = u8.float()
    y = torch.tensor([1], device="cuda")

    def step():
        for p in net.parameters():
            p.grad = None
        net(x, y)["loss"].backward()
        return [p.grad.clone() for p in net.parameters()]
    before = step()
    calls = {"stem_dgrad": 0, "maxpool_bwd": 0, "stage": 0}
    real_sd, real_mp, real_stage = ops.stem_dgrad, ops.maxpool_bwd, encoder._stage_backward
    monkeypatch.setattr(ops, "stem_dgrad", lambda *a, **k: (calls.__setitem__("stem_dgrad", calls["stem_dgrad"] + 1), real_sd(*a, **k))[1])
    monkeypatch.setattr(ops, "maxpool_bwd", lambda *a, **k: (calls.__setitem__("maxpool_bwd", calls["maxpool_bwd"] + 1), real_mp(*a, **k))[1])
    monkeypatch.setattr(encoder, "_stage_backward", lambda *a, **k: (calls.__setitem__("stage", calls["stage"] + 1), real_stage(*a, **k))[1])
    net.train()                                                                  # the flag is left alone, whatever it is
    marks = {k: torch.full_like(p, 0.5) if i % 2 else None for i, (k, p) in enumerate(net.named_parameters())}
    for k, p in net.named_parameters():
        p.grad = None if marks[k] is None else marks[k].clone()
    rng = torch.get_rng_state()
    raw = cam.raw(x, 1)
    # layer4: the pool gradient alone — no convolution backward, no stem; layer2: the two stages above it
    assert calls == {"stem_dgrad": 0, "maxpool_bwd": 0, "stage": 0 if layer == "layer4" else 2}, calls
    raw0 = cam.raw(x, 1, offset=0.0)
    m_tile = cam.maps(x, 1)
    m_bag = cam.maps(x, 1, normalize="bag")
    m_u8 = cam.maps(u8, 1)
    raw_u8 = cam.raw(u8, 1)
    assert calls["stem_dgrad"] == 0 and calls["maxpool_bwd"] == 0
    assert torch.equal(torch.get_rng_state(), rng) and net.training
    for k, p in net.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k
    hs, ws = {"layer4": (2, 3), "layer2": (7, 9)}[layer]
    assert raw.shape == (8, hs, ws) and raw.dtype == torch.float32 and bool(torch.isfinite(raw).all()) and float(raw.max()) > 0
    assert not torch.equal(raw0, raw) and float(raw0.min()) >= 0
    assert m_tile.shape == (8, 50, 70) and m_tile.dtype == torch.uint8
    assert np.array_equal(m_tile.cpu().numpy(), _restated_maps(ops, raw, (50, 70)))
    lo, hi = float(raw.min()), float(raw.max())
    assert np.array_equal(m_bag.cpu().numpy(), _restated_maps(ops, raw, (50, 70), (lo, hi)))
    assert torch.equal(raw_u8, raw) and torch.equal(m_u8, m_tile)                 # the decode is lossless
    if dtype == torch.bfloat16:                                                  # the space-to-depth feed of the bf16 mode
        s2d = mil_amd.S2dTiles(ops.stem_s2d(x, torch.bfloat16))
        raw_s = cam.raw(s2d, 1)
        assert raw_s.shape == raw.shape and bool(torch.isfinite(raw_s).all())
        assert np.array_equal(cam.maps(s2d, 1).cpu().numpy(), _restated_maps(ops, raw_s, (50, 70)))
    net.eval()
    monkeypatch.undo()
    after = step()                                                               # a training step is not disturbed
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_tile_grad_cam_with_flat_params_leaves_the_bucket_alone(golden_dir):
    """`dist.FlatParams` switches direct accumulation into the flat gradient bucket on: a Grad-CAM call must not add to it."""
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260304).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    mil_amd.TileGradCam(net, layer="layer1").maps(x, 0, normalize="bag")
    assert torch.equal(flat.flat_grad, bucket)
