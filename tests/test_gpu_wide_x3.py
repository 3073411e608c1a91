"""-m gpu: the split-precision (MIL_DT_F32S, `mil_amd.BF16X3`) forms of the channel-blocked wide kernels of csrc/conv_wide.hip
and the wide encoder (`alt_resnet.ResNet`) in that mode.

Kernel bound.  A split operand v = hi + lo + r with hi = bf16(v), lo = bf16(v - hi), |r| <= 2^-17 |v| (v - hi is at most
2^-8 |v| and its bf16 rounding loses at most 2^-9 of that).  A product a*b taken as a_lo*b_hi + a_hi*b_lo + a_hi*b_hi differs
from a*b by a_lo*b_lo + r_a*b + a*r_b (+ second order): at most 2^-16 + 2 * 2^-17 = 3 * 2^-18 |a*b| — 0.375 of the 2^-15 the
tests allow per product; the rest is room for the fp32 accumulation of the short contractions used here (cin <= 96 forward).
A CPU simulation of the split arithmetic stayed at <= 0.15 of the bound on the first four shapes below; plain bf16 operands exceed it
27-fold and a form with one cross term missing 19-fold, so the bound tells the split form from both.

Deep shapes (SHAPES[4:]: 128-512 channels, 4-16 input chunks, contractions up to K = 4608, eight 4x4 images per tile).  The same
CPU simulation (hi = bf16(v), lo = bf16(v - hi), three fp32 convolutions, this module's own seeded inputs) on those seven
shapes, worst error as a multiple of the bound the test uses:
    form                             correct split, largest     one cross term dropped, smallest   plain bf16, smallest
    forward                          0.073 (256->512 1x1 s2)    7.2  (512->512 3x3)                11.0 (512->512 3x3)
    data gradient + addend, gated    0.056 (128->256 s2 to 8x8) 6.9  (512->512 3x3)                 9.9 (512->512 3x3)
    weight gradient                  0.20  (128->256 s2, 10x10) 16.7 (128->128 3x3)                27.4 (128->128 3x3)
("dropped": the smaller of the two ways to drop a cross term; correct split at 512->512 3x3: 0.020 / 0.027 / 0.16.)  The
data-gradient bound is REL * conv_transpose(|dz|, |w|) plus one fp32 rounding of the sum with the addend,
2^-23 |conv_transpose(dz, w) + addend|.  REL separates right from wrong at every depth.

Which form a geometry selects (`launch_wide`, 128-pixel tiles from `mil_geom_tiles(g, 7)`): maps wider or taller than 8 run 16x8
tiles of one image (3x3 halo 10x18 = 180 pixels), maps up to 8x8 run 8x8 tiles of two images (2 x 10x10 = 200), maps up to 4x4 run
4x4 tiles of eight images, whose 3x3 halo is 8 x 6x6 = 288 pixels: more than the 256 the pipelined form holds.  So every 3x3
stride-1 or zero-insert launch on maps of at most 4x4 runs the plain wide_conv_kernel<F32S> by its geometry, no environment knob
involved: SHAPES[9] (512 -> 512 on 4x4) and SHAPES[10], the smallest such launch (two chunks, one output block, 4x3 maps, a
one-image second group).  1x1 launches (halo <= 128 pixels) always fit the pipelined form.  The fewer-images-per-tile fallback
(`mil_geom_set(a.g, 3, 3, 1)`) is taken in split precision exactly where exact fp32 takes it (the same 144-byte pixel record
and 72 KB filter slice): a 3x3 stride-2 FORWARD onto maps of at most 4x4, whose eight 9x9 halos are 648 pixels = 91 KB.
SHAPES[6] (128 -> 256, 8x8 -> 4x4) is such a launch.  No stride-1 or zero-insert launch reaches the fallback (288 pixels are
41 KB), and the weight gradient has none."""
import functools
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mil_amd
from mil_amd import _lib as L, ops
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

REL = 2.0 ** -15
# (n, H, W, cin, cout, ks, stride, pad)
SHAPES = [
    (3, 9, 9, 64, 128, 3, 1, 1),        # two chunks, two output blocks, ragged tiles
    (2, 10, 7, 96, 64, 1, 2, 0),        # 1x1 stride 2
    (3, 11, 11, 64, 128, 3, 2, 1),      # stride 2, odd map
    (5, 8, 8, 32, 64, 3, 1, 1),         # one chunk, two images per tile with a ragged last group
    # the deep layers of the encoder (WIDE_CASES of test_gpu_kernels.py)
    (2, 16, 16, 128, 128, 3, 1, 1),     # four chunks, 16x8 tiles
    (2, 10, 10, 128, 256, 3, 2, 1),     # stride 2 onto 5x5 maps
    (4, 8, 8, 128, 256, 3, 2, 1),       # stride 2 onto 4x4 maps: the forward takes the fewer-images-per-tile fallback
    (5, 8, 8, 256, 256, 3, 1, 1),       # eight chunks, four output blocks, a one-image last group
    (3, 8, 8, 256, 512, 1, 2, 0),       # the 1x1 stride-2 projection
    (9, 4, 4, 512, 512, 3, 1, 1),       # sixteen chunks, K = 4608, eight images per tile: the plain kernel by its geometry
    (9, 4, 3, 64, 64, 3, 1, 1),         # the smallest launch the geometry sends to the plain kernel (see the docstring)
]
DEEP = list(range(4, len(SHAPES)))
CASES = ["alt_l1111_n4_64", "alt_l2222_n2_96x80"]


def _nchw(t):
    return t.double().cpu().permute(0, 3, 1, 2)


@functools.lru_cache(maxsize=None)
def _problem(si):
    """Inputs of SHAPES[si] (fp32, on the GPU), the split-precision forward without epilogue, and its fp64 reference + bound."""
    n, h, w, cin, cout, ks, stride, pad = SHAPES[si]
    gen = torch.Generator().manual_seed(100 + si)
    x = torch.randn((n, h, w, cin), generator=gen).cuda()
    wt = (torch.randn((cout, cin, ks, ks), generator=gen) * (2.0 / (ks * ks * cin)) ** 0.5).cuda()
    ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    dz = torch.randn((n, ho, wo, cout), generator=gen).cuda()
    wp = ops.wide_pack_weights(wt, L.PACK_FWD, L.BF16X3)
    with L.f32_mma(L.MIL_DT_F32S):
        y = ops.wide_conv(x, wp, cout, ks=ks, stride=stride, pad=pad)
    y64 = F.conv2d(_nchw(x), wt.double().cpu(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    bound = REL * F.conv2d(_nchw(x).abs(), wt.double().cpu().abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    g2 = torch.Generator().manual_seed(300 + si)         # the encoder's data-gradient call: an addend and a gate, shaped like x
    addend, act = torch.randn((n, h, w, cin), generator=g2).cuda(), torch.randn((n, h, w, cin), generator=g2).cuda()
    return dict(x=x, w=wt, dz=dz, y=y, y64=y64, bound=bound, addend=addend, act=act)


def _dgrad_kw(si):
    """The keyword arguments of `_Conv.dgrad` (alt_resnet.py) for SHAPES[si]: stride 2 is the zero-insert form."""
    n, h, w, cin, cout, ks, stride, pad = SHAPES[si]
    return dict(ks=ks, stride=1, pad=pad, zero_insert=True, out_hw=(h, w)) if stride == 2 else dict(ks=ks, stride=1, pad=pad)


def _within(got, ref64, bound, what):
    err = (got.double().cpu() - ref64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst error / bound = {ratio:.3f}")
    assert bool(torch.isfinite(got).all()), what
    assert bool((err <= bound).all()), (what, ratio)


# ---- 4a ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [L.PACK_FWD, L.PACK_DGRAD])
def test_wide_pack_split_fragments_bit_for_bit(mode):
    gen = torch.Generator().manual_seed(7)
    w = torch.randn((128, 64, 3, 3), generator=gen).cuda()
    p32 = ops.wide_pack_weights(w, mode, torch.float32)
    px3 = ops.wide_pack_weights(w, mode, L.BF16X3)
    assert px3.dtype == torch.float32 and px3.numel() == p32.numel()       # the byte count of the fp32 packing
    v = p32.view(-1, 8)
    frag = px3.view(-1, 8).view(torch.bfloat16)
    assert frag.shape == (v.shape[0], 16)
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    assert torch.equal(frag[:, :8], hi)
    assert torch.equal(frag[:, 8:], lo)
    assert float(lo.float().abs().max()) > 0


# ---- 4b ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_wide_conv_split_forward_against_fp64(si):
    p = _problem(si)
    _within(p["y"], p["y64"], p["bound"], f"forward {SHAPES[si]}")


def test_wide_conv_split_zero_insert_dgrad_against_fp64():
    n, h, w, cin, cout, ks, stride, pad = SHAPES[2]
    p = _problem(2)
    wb = ops.wide_pack_weights(p["w"], L.PACK_DGRAD, L.BF16X3)
    with L.f32_mma(L.MIL_DT_F32S):
        dx = ops.wide_conv(p["dz"], wb, cin, ks=ks, stride=1, pad=pad, zero_insert=True, out_hw=(h, w))
    assert tuple(dx.shape) == (n, h, w, cin)
    w64 = p["w"].double().cpu()
    ref = F.conv_transpose2d(_nchw(p["dz"]), w64, stride=stride, padding=pad).permute(0, 2, 3, 1)
    bound = REL * F.conv_transpose2d(_nchw(p["dz"]).abs(), w64.abs(), stride=stride, padding=pad).permute(0, 2, 3, 1)
    assert tuple(ref.shape) == (n, h, w, cin)
    _within(dx, ref, bound, "zero-insert data gradient")


@pytest.mark.parametrize("si", DEEP)
def test_wide_conv_split_dgrad_with_addend_and_gate_against_fp64(si):
    """The data gradient as `alt_resnet._backward` calls it: (conv_transpose(dz, w) + addend) * (act > 0) in one launch, the
    zero-insert form at stride 2 (the 1x1 projection included), against fp64 per element."""
    n, h, w, cin, cout, ks, stride, pad = SHAPES[si]
    p = _problem(si)
    wb = ops.wide_pack_weights(p["w"], L.PACK_DGRAD, L.BF16X3)
    with L.f32_mma(L.MIL_DT_F32S):
        dx = ops.wide_conv(p["dz"], wb, cin, res=p["addend"], act=p["act"], **_dgrad_kw(si))
    assert tuple(dx.shape) == (n, h, w, cin)
    w64, dz64 = p["w"].double().cpu(), _nchw(p["dz"])
    ho, wo = dz64.shape[2:]
    opad = (h - ((ho - 1) * stride - 2 * pad + ks), w - ((wo - 1) * stride - 2 * pad + ks))
    lin = F.conv_transpose2d(dz64, w64, stride=stride, padding=pad, output_padding=opad).permute(0, 2, 3, 1)
    mag = F.conv_transpose2d(dz64.abs(), w64.abs(), stride=stride, padding=pad, output_padding=opad).permute(0, 2, 3, 1)
    assert tuple(lin.shape) == (n, h, w, cin)
    total = lin + p["addend"].double().cpu()
    gate = p["act"].cpu() > 0
    _within(dx, total * gate, REL * mag + 2.0 ** -23 * total.abs(), f"data gradient + addend, gated {SHAPES[si]}")
    off = dx.cpu()[~gate]
    assert off.numel() > dx.numel() // 4 and bool((off == 0).all())            # gated-off elements are exactly 0


# ---- 4c ---------------------------------------------------------------------------------------------------------------
def test_wide_conv_split_epilogue_reads_exact_fp32():
    n, h, w, cin, cout, ks, stride, pad = SHAPES[0]
    p = _problem(0)
    y0 = p["y"]
    gen = torch.Generator().manual_seed(11)
    res = torch.randn(tuple(y0.shape), generator=gen).cuda()
    act = torch.randn(tuple(y0.shape), generator=gen).cuda()
    wp = ops.wide_pack_weights(p["w"], L.PACK_FWD, L.BF16X3)
    with L.f32_mma(L.MIL_DT_F32S):
        y = ops.wide_conv(p["x"], wp, cout, ks=ks, stride=stride, pad=pad, res=res, act=act, relu=True)
    gate = (act > 0).float()
    torch.testing.assert_close(y, torch.relu(y0 + res) * gate, rtol=1e-6, atol=0.0)
    # the residual enters as exact fp32, not as its hi + lo reconstruction: where the two candidates differ and the
    # epilogue passes the value through, the output is the exact sum
    hi = res.to(torch.bfloat16).float()
    rec = hi + (res - hi).to(torch.bfloat16).float()
    exact, rounded = y0 + res, y0 + rec
    sel = (exact != rounded) & (exact > 0) & (act > 0)
    assert int(sel.sum()) > sel.numel() // 8
    assert torch.equal(y[sel], exact[sel])
    assert not torch.equal(y[sel], rounded[sel])


# ---- 4d ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [0, 1, 2] + DEEP)
def test_wide_wgrad_split_against_fp64(si):
    """SHAPES[9] (512 -> 512) has 128 (block, chunk) pairs and two tiles, SHAPES[8] 64 pairs and one: `run_wide_wgrad` clamps its
    slabs per pair (512 / pairs) to the tile count."""
    n, h, w, cin, cout, ks, stride, pad = SHAPES[si]
    p = _problem(si)
    with L.f32_mma(L.MIL_DT_F32S):
        dw, _ = ops.wide_wgrad(p["x"], p["dz"], cin, cout, ks=ks, stride=stride, pad=pad)
        dw2, _ = ops.wide_wgrad(p["x"], p["dz"], cin, cout, ks=ks, stride=stride, pad=pad)
        base = torch.randn((cout, cin, ks, ks), generator=torch.Generator().manual_seed(5)).cuda()
        acc = base.clone()
        ops.wide_wgrad(p["x"], p["dz"], cin, cout, ks=ks, stride=stride, pad=pad, out=acc)
    shape = (cout, cin, ks, ks)
    ref = torch.nn.grad.conv2d_weight(_nchw(p["x"]), shape, _nchw(p["dz"]), stride=stride, padding=pad)
    bound = REL * torch.nn.grad.conv2d_weight(_nchw(p["x"]).abs(), shape, _nchw(p["dz"]).abs(), stride=stride, padding=pad)
    _within(dw, ref, bound, f"weight gradient {SHAPES[si]}")
    assert torch.equal(dw, dw2)                       # slabs reduced in a fixed order
    assert torch.equal(acc, base + dw)                # accumulate: the same values onto a non-zero buffer


# ---- pipelined form ----------------------------------------------------------------------------------------------------
PLAIN = "1000000000"       # MIL_PF_MIN_TILES above any tile count: the plain forms (unset: the pipelined forms where the geometry fits)


def test_wide_conv_split_pipelined_form_is_bit_identical_to_plain(monkeypatch):
    """wide_conv_x3_pf_kernel (stride-1 and zero-insert launches) against wide_conv_kernel<F32S> on the same problems: 3x3 with
    two chunks and ragged tiles, 3x3 with one chunk and a ragged image group, 1x1, the zero-insert data gradient, and the
    full epilogue; the deep stride-1 shapes forward and as the gated data gradient with its addend, the deep zero-insert
    launches (3x3 and the 1x1 projection) bare and with addend and gate.  _problem() ran its stride-1 shapes on the pipelined
    form (checked against fp64 above).  SHAPES[9] and [10] run the plain kernel by their geometry either way (module
    docstring): the knob changes nothing there."""
    runs = []
    for si, (n, h, w, cin, cout, ks, stride, pad) in enumerate(SHAPES):
        p = _problem(si)
        if stride == 1:
            runs.append((p["x"], p["w"], L.PACK_FWD, cout, dict(ks=ks, stride=1, pad=pad), p["y"]))
        elif ks == 3 or si in DEEP:          # SHAPES[1] has no data gradient here: its 96 input channels are no multiple of 64
            runs.append((p["dz"], p["w"], L.PACK_DGRAD, cin, _dgrad_kw(si), None))
        if si in DEEP:
            runs.append((p["dz"], p["w"], L.PACK_DGRAD, cin, dict(_dgrad_kw(si), res=p["addend"], act=p["act"]), None))
    p = _problem(0)
    gen = torch.Generator().manual_seed(13)
    res, act = (torch.randn(tuple(p["y"].shape), generator=gen).cuda() for _ in range(2))
    runs.append((p["x"], p["w"], L.PACK_FWD, SHAPES[0][4], dict(ks=3, stride=1, pad=1, res=res, act=act, relu=True), None))
    x1 = p["x"]                                              # 1x1 stride 1 on the first shape's input
    w1 = torch.randn((128, 64, 1, 1), generator=gen).cuda() * 0.2
    runs.append((x1, w1, L.PACK_FWD, 128, dict(ks=1, stride=1, pad=0), None))
    assert len(runs) == 5 + 4 + 3 + 7           # deep: four stride-1 forwards, three bare zero-insert launches, seven gated gradients
    for x, w, mode, cout_x, kw, known in runs:
        wp = ops.wide_pack_weights(w, mode, L.BF16X3)
        with L.f32_mma(L.MIL_DT_F32S):
            monkeypatch.delenv("MIL_PF_MIN_TILES", raising=False)
            y_pf = ops.wide_conv(x, wp, cout_x, **kw)
            monkeypatch.setenv("MIL_PF_MIN_TILES", PLAIN)
            y_plain = ops.wide_conv(x, wp, cout_x, **kw)
        assert bool(torch.isfinite(y_pf).all())
        assert torch.equal(y_pf, y_plain), kw
        if known is not None:
            assert torch.equal(y_pf, known)


# ---- 4e ---------------------------------------------------------------------------------------------------------------
def _load(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    return z, tuple(int(v) for v in z["layers"]), int(z["num_classes"]), int(z["wseed"])


def _net(layers, num_classes, wseed, mode):
    net = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, list(layers), num_classes=num_classes, compute_dtype=mode)
    sd = orc.alt_seeded_state(layers, num_classes, wseed)
    assert list(sd.keys()) == list(net.state_dict().keys())
    net.load_state_dict(sd)
    return net.cuda()


@functools.lru_cache(maxsize=None)
def _x3_run(golden_dir, name):
    """One forward + backward of the BF16X3 net on a golden case, and the exact-fp32 features of the same net afterwards."""
    z, layers, nc, wseed = _load(golden_dir, name)
    net = _net(layers, nc, wseed, mil_amd.BF16X3)
    x = torch.from_numpy(z["x"]).cuda()
    feats = net(x)
    feats.backward(torch.from_numpy(z["dfeats"]).cuda())
    grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    net.compute_dtype = torch.float32                  # a live net re-packs for the new mode
    with torch.no_grad():
        f32_live = net(x).cpu()
    f32_fresh = _net(layers, nc, wseed, torch.float32)(x).detach().cpu()
    return dict(z=z, layers=layers, nc=nc, wseed=wseed, feats=feats.detach().cpu(), grads=grads, f32_live=f32_live,
                f32_fresh=f32_fresh)


@pytest.mark.parametrize("name", CASES)
def test_alt_resnet_bf16x3_features_match_golden_and_fp32(golden_dir, name):
    r = _x3_run(golden_dir, name)
    ref = torch.from_numpy(r["z"]["feats"])
    tol = 1e-4 * max(1.0, float(ref.abs().max()))
    err_g = float((r["feats"] - ref).abs().max())
    err_f = float((r["feats"] - r["f32_fresh"]).abs().max())
    print(f"{name}: features vs golden {err_g / max(1.0, float(ref.abs().max())):.2e}, vs exact fp32 "
          f"{err_f / max(1.0, float(ref.abs().max())):.2e} (of max(1, |ref|max))")
    assert err_g <= tol
    assert err_f <= tol


def test_alt_resnet_bf16x3_gradients_l1111_match_golden(golden_dir):
    r = _x3_run(golden_dir, "alt_l1111_n4_64")
    z = r["z"]
    norms = dict(zip([str(k) for k in z["gradnorm.names"]], z["gradnorm.l2"]))
    for k, g in r["grads"].items():
        got = float(g.double().norm())
        assert abs(got - norms[k]) <= 1e-3 * norms[k] + 1e-6, (k, got, norms[k])
    for k in ("conv1.weight", "layer2.0.downsample.0.weight", "fc.bias"):
        ref_g = torch.from_numpy(z["grad." + k])
        assert float((r["grads"][k] - ref_g).abs().max()) <= 1e-3 * float(ref_g.abs().max()), k


def test_alt_resnet_bf16x3_gradients_l2222_norms_and_direction(golden_dir):
    """On this case a 1e-5 perturbation already flips a ReLU / max-pool decision (two tiles), so single elements move by more
    than 1e-3 of the maximum; what holds is every parameter's gradient norm within the project's end-to-end fp32 bound of
    5e-3 and its direction (cosine >= 0.999) against the fp32 oracle gradient."""
    r = _x3_run(golden_dir, "alt_l2222_n2_96x80")
    z = r["z"]
    norms = dict(zip([str(k) for k in z["gradnorm.names"]], z["gradnorm.l2"]))
    sd = orc.alt_seeded_state(r["layers"], r["nc"], r["wseed"], requires_grad=True)
    orc.alt_backbone(sd, torch.from_numpy(z["x"]), r["layers"]).backward(torch.from_numpy(z["dfeats"]))
    worst_n, worst_c = 0.0, 1.0
    for k, g in r["grads"].items():
        got = float(g.double().norm())
        worst_n = max(worst_n, abs(got - norms[k]) / norms[k])
        a, b = g.double().flatten(), sd[k].grad.double().flatten()
        worst_c = min(worst_c, float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30)))
    print(f"alt_l2222_n2_96x80: worst gradient-norm deviation {worst_n:.2e}, lowest cosine {worst_c:.6f}")
    for k, g in r["grads"].items():
        got = float(g.double().norm())
        assert abs(got - norms[k]) <= 5e-3 * norms[k], (k, got, norms[k])
        a, b = g.double().flatten(), sd[k].grad.double().flatten()
        assert float(a @ b / (a.norm() * b.norm()).clamp_min(1e-30)) >= 0.999, k


# ---- 4f ---------------------------------------------------------------------------------------------------------------
def test_alt_resnet18_bf16x3_module_surface(golden_dir):
    net = mil_amd.alt_resnet.resnet18(num_classes=80, compute_dtype=mil_amd.BF16X3)
    assert net.compute_dtype == mil_amd.BF16X3
    assert list(net.state_dict().keys()) == [k for k, _ in orc.alt_state_dict_spec((2, 2, 2, 2), 80)]
    assert inspect.signature(mil_amd.alt_resnet.ResNet.__init__).parameters["compute_dtype"].default == torch.bfloat16   # default unchanged
    # compute_dtype set to torch.float32 on a live BF16X3 net: the next call gives the exact-fp32 features
    r = _x3_run(golden_dir, "alt_l1111_n4_64")
    assert torch.equal(r["f32_live"], r["f32_fresh"])
    assert not torch.equal(r["f32_live"], r["feats"])
    bad = mil_amd.alt_resnet.ResNet(layers=(1, 1, 1, 1), num_classes=8, compute_dtype=torch.float16).cuda()
    with pytest.raises(ValueError):
        bad(torch.zeros((1, 3, 32, 32), device="cuda"))
