"""-m gpu: feature inversion — `ops.stage_energy` / `stage_match`, `pixel_reg`, `pixel_shift` and `pixel_momentum_step` against their
numpy restatements (bit for bit where the output is elementwise, within a derived bound where it is a sum), the inversion's
gradient against fp64 on the encoder's own activation pattern, `mil_amd.FeatureInverter` and the regularised
`mil_amd.FeatureVisualizer` against the loops they replace, and the inverter's descent against the CPU oracle's.  Every output
buffer a kernel is handed is NaN-filled or 255-filled first."""
import functools
import os

import numpy as np
import pytest
import torch

import feature_inv_reference as ref
import feature_vis_reference as fv_ref
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
U = 2.0 ** -24                                   # the unit roundoff of fp32


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


def _buffer(values, misalign, dtype=torch.float32):
    """A contiguous device tensor holding `values`; misalign: its first element sits 4 bytes (uint8: 1 byte) off the 16-byte grid,
    which sends the kernels down their element-by-element paths."""
    flat = torch.empty(values.numel() + 4, dtype=dtype, device="cuda")
    view = flat[1:1 + values.numel()] if misalign else flat[:values.numel()]
    view = view.view(values.shape)
    view.copy_(values.to(dtype))
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


def _nan_like(shape, misalign=False):
    return _buffer(torch.full(shape, NAN), misalign)


# ---- 1. stage_energy and stage_match -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("hw", [(5, 7), (16, 16), (33, 37)], ids=["5x7", "16x16", "33x37"])
@pytest.mark.parametrize("c", [20, 40, 60, 80])
def test_stage_match_and_energy_against_numpy(ops, c, hw, dtype):
    """dz bit for bit (from the energy the device computed), the padding channels exactly zero; energy and loss against fp64.

    The bound.  A fixed-order fp32 sum of n non-negative terms, however it is bracketed, lies within n u sum|terms| of the exact sum
    of the terms (u = 2^-24), and the terms' own roundings — a difference and a product, 3 u each at most — and the at most ~60
    additions any one term passes through (a thread's chain, 6 butterfly steps, 4 waves, 16 slices) are far inside n >= 700 here.
    So |E - E64| <= n u E64 and |D - D64| <= n u D64.  loss = weight * (D / E) adds the relative error of E to that of D and three
    roundings — the fp32 weight, the quotient, the product — so loss / loss64 lies within (1 + u)^3 (1 + n u) / (1 - n u), which is
    1 + (2 n + 3) u to first order; the assertion uses the full expression."""
    h, w = hw
    gen = torch.Generator().manual_seed(2000 * c + 41 * h + w)
    a = torch.randn(3, h, w, cpad(c), generator=gen)
    a[torch.rand(a.shape, generator=gen) < 0.15] = 0.0                            # exact zeros: the branch rule is a strict > 0
    a[:, 0, 0, 0], a[:, 1, 0, 0], a[:, 2, 0, 0] = 0.0, -0.5, 0.5                  # a zero, a negative, a positive for certain
    a[:, 0, 0, c - 1], a[:, 1, 0, c - 1], a[:, 2, 0, c - 1] = 0.0, -0.5, 0.5
    tgt = torch.randn(3, h, w, cpad(c), generator=gen).abs() * torch.tensor([0.5, 1.0, 3.0]).view(3, 1, 1, 1)
    act, target = a.to(dtype).cuda(), tgt.to(dtype).cuda()                        # the padding channels hold values too: they do not count
    sa, st = act.float().cpu().numpy(), target.float().cpu().numpy()
    n = h * w * c
    energy = torch.full((3,), NAN, device="cuda")
    assert ops.stage_energy(target, c, energy=energy) is energy
    e64 = ref.stage_energy64(st, c)
    e_err = np.abs(energy.cpu().numpy().astype(np.float64) - e64)
    loss = torch.full((3,), NAN, device="cuda")
    dz = torch.full(act.shape, NAN, device="cuda").to(dtype)
    got = ops.stage_match(act, target, c, weight=0.1, energy=energy, loss=loss, dz=dz)
    assert got[0] is loss and got[1] is dz
    dz_ref = ref.stage_match_dz(sa, st, c, energy.cpu().numpy(), 0.1)
    assert _same(dz, torch.from_numpy(dz_ref).to(dtype))
    assert float(dz[..., :c].float().abs().max()) > 0.0
    assert cpad(c) == c or float(dz[..., c:].float().abs().max()) == 0.0         # (40 and 80 channels have no padding)
    l64 = 0.1 * ref.stage_distance64(sa, st, c) / e64
    l_err = np.abs(loss.cpu().numpy().astype(np.float64) - l64)
    l_bound = (1 + U) ** 3 * (1 + n * U) / (1 - n * U) - 1
    print(f"stage_match[c={c}, {h}x{w}, {dtype}]: |E - E64| / E64 {(e_err / e64).max():.2e} (bound {n * U:.2e}), "
          f"|loss - loss64| / loss64 {(l_err / l64).max():.2e} (bound {l_bound:.2e})")
    assert (e_err <= n * U * e64).all(), (e_err, n * U * e64)
    assert (l_err <= l_bound * l64).all(), (l_err, l64)
    assert _same(energy, torch.from_numpy(tree.stage_energy(st, c)))              # the summation tree itself
    assert _same(loss, torch.from_numpy(tree.stage_match_loss(sa, st, c, energy.cpu().numpy(), 0.1)))
    loss2, dz2 = ops.stage_match(act, target, c, weight=0.1)                      # fresh outputs, its own energy: the same bits
    assert _same(loss2, loss) and _same(dz2, dz) and _same(ops.stage_energy(target, c), energy)


# ---- 2. pixel_reg --------------------------------------------------------------------------------------------------------------
REG_SHAPES = [(1, 3, 5, 7), (2, 3, 33, 37), (3, 3, 64, 64), (1, 3, 1, 9), (1, 3, 6, 1)]
REG_WEIGHTS = [(0.0, 0.25), (0.125, 0.0), (0.3, 0.7)]


@pytest.mark.parametrize("alpha", [2, 6])
@pytest.mark.parametrize("shape", REG_SHAPES + [(1, 3, 96, 96)], ids=lambda s: "x".join(map(str, s)))
def test_pixel_reg_bit_for_bit(ops, shape, alpha):
    """Every shift and weight combination of one shape and alpha on one x (values outside [-1, 1]).  (1,3,5,7) sits 4 bytes off
    the 16-byte grid and ends in a short group; (2,3,33,37)'s second tile starts off the grid; (1,3,1,9) is on the grid with a
    short last group.

    terms.  n is the number of summed terms (3 H W powers; two squares per cell of the trimmed planes).  Each is >= 0, so the
    fixed-order fp32 sum lies within n u sum|terms| of the exact sum however it is bracketed, provided the terms' own roundings
    (alpha - 1 products; a difference, a square and the sum of two squares) plus the additions one term passes through stay below n:
    the tightest case is (1,3,6,1) — 18 terms, one group of 4 per workgroup then 5 slices: 4 + 5 additions and 5 products.
    Beside the bound, the terms bit for bit against the summation tree itself; (1,3,96,96) gives a thread a second group
    (432 groups per slice)."""
    _t, _c, H, W = shape
    misalign = shape == (1, 3, 5, 7)
    rng = np.random.default_rng(sum(shape) * 10 + alpha)
    x = rng.uniform(-1.8, 1.8, shape).astype(np.float32)
    g = rng.standard_normal(shape).astype(np.float32)
    g[0, 0, 0, 0] = -0.0                                                          # a signed zero survives the zero-weight path
    assert np.abs(x).max() > 1
    dx_, dg = _buffer(torch.from_numpy(x), misalign), _buffer(torch.from_numpy(g), misalign)
    kept = dx_.clone()
    t64 = ref.reg_terms64(x, alpha)
    t32 = torch.from_numpy(tree.reg_terms(x, alpha))
    n_terms = np.array([3 * H * W, 2 * 3 * (H - 1) * (W - 1)], dtype=np.float64)[:, None]
    for shift in [(0, 0), (-3, 5), (H, W), (H + 1, -W - 2)]:
        for aw, tw in REG_WEIGHTS + [(0.0, 0.0)]:
            want = ref.pixel_reg(x, g, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift)
            out = _nan_like(shape, misalign)
            terms = torch.full((2, shape[0]), NAN, device="cuda")
            assert ops.pixel_reg(dx_, dg, out, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift, terms=terms) is out
            assert _same(out, torch.from_numpy(want)), (shift, aw, tw)
            err = np.abs(terms.cpu().numpy().astype(np.float64) - t64)
            assert (err <= n_terms * U * t64).all(), (shift, aw, tw, err, n_terms * U * t64)
            assert _same(terms, t32), (shift, aw, tw)
            plain = ops.pixel_reg(dx_, dg, None, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift)      # without terms
            assert _same(plain, out)
            if shift[0] % H == 0 and shift[1] % W == 0:                          # the aliased form: out is g
                alias = _buffer(torch.from_numpy(g), misalign)
                assert ops.pixel_reg(dx_, alias, alias, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift) is alias
                assert _same(alias, out)
            else:
                with pytest.raises(ValueError, match="shift"):
                    ops.pixel_reg(dx_, dg, dg, alpha=alpha, alpha_weight=aw, tv_weight=tw, shift=shift)
    if min(H, W) == 1:
        assert np.all(t64[1] == 0) and float(terms[1].abs().max()) == 0.0        # no total variation in a single row or column
    assert _same(dx_, kept) and _same(dg, torch.from_numpy(g))                    # x and g are only read
    print(f"pixel_reg[{shape}, alpha={alpha}]: terms {terms.cpu().tolist()} against {t64.tolist()}")


# ---- 3. pixel_shift ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", REG_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pixel_shift_is_a_bit_copy_that_pixel_reg_undoes(ops, shape):
    _t, _c, H, W = shape
    misalign = shape == (1, 3, 5, 7)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)))
    bits = x.view(torch.int32)
    bits[0, 0, 0, 0], bits[0, 1, 0, 0], bits[0, 2, 0, 0] = 0x7FC01234, -0x7FFFFFFF - 1, 0x7F800001     # a NaN payload, -0, a signalling NaN
    dx_ = _buffer(x, misalign)
    assert _same(dx_, x)
    for shift in [(0, 0), (-3, 5), (1, 0), (0, -1), (H, W), (H + 1, -W - 2), (3 * H - 1, 2 * W + 1)]:
        out = _nan_like(shape, misalign)
        assert ops.pixel_shift(dx_, out, shift) is out
        assert _same(out, torch.from_numpy(ref.shift_copy(x.numpy().view(np.int32), shift).view(np.float32))), shift
        back = ops.pixel_reg(x=torch.zeros(shape, device="cuda"), g=out, out=_nan_like(shape, misalign), alpha_weight=0.0, tv_weight=0.0, shift=shift)
        assert _same(back, x), shift
        assert _same(ops.pixel_shift(dx_, None, shift), out)
    with pytest.raises(ValueError, match="overlaps"):
        ops.pixel_shift(dx_, dx_, (1, 1))


# ---- 4. pixel_momentum_step ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("project", ["none", "clamp", "u8"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 3, 33, 37), (3, 3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_pixel_momentum_step_bit_for_bit(ops, shape, project):
    """30 steps carried through on the device and in numpy fp32; x, the buffer and the bytes compared at steps 1, 2 and 30, with
    and without u8_out.  The shapes, the misaligned case and the zero patch of test_pixel_step_bit_for_bit."""
    rng = np.random.default_rng(sum(shape) + 11 * len(project))
    misalign = shape[0] == 1
    kw = dict(lr=6.0, momentum=0.9, weight_decay=1e-4, project=project)
    x = rng.uniform(-1, 1, shape).astype(np.float32)
    x[0, 0, :2, :3] = 0.0
    buf = np.zeros_like(x)
    dx_ = _buffer(torch.from_numpy(x), misalign)
    dbuf = _buffer(torch.zeros(shape), misalign)
    plain, plain_buf = dx_.clone(), torch.zeros(shape, device="cuda")             # the same steps without u8_out
    left = False
    for step in range(1, 31):
        g = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 0)).astype(np.float32)
        g[0, 0, :2, :3] = 0.0
        x, buf, codes = ref.momentum_step(x, g, buf, **kw)
        left = left or bool((np.abs(x) > 1).any())
        dg = _buffer(torch.from_numpy(g), misalign)
        u8 = _buffer(torch.full(shape, 255, dtype=torch.uint8), misalign, torch.uint8)
        assert ops.pixel_momentum_step(dx_, dg, dbuf, u8_out=u8, **kw) is dx_
        ops.pixel_momentum_step(plain, dg.clone(), plain_buf, **kw)
        if step in (1, 2, 30):
            assert _same(dx_, torch.from_numpy(x)), step
            assert _same(dbuf, torch.from_numpy(buf)), step
            assert torch.equal(u8.cpu(), torch.from_numpy(codes)), step
            assert _same(dg, torch.from_numpy(g))
    assert _same(plain, dx_) and _same(plain_buf, dbuf)
    assert project != "none" or left                                             # x did reach outside [-1, 1]
    if project != "u8":                                                          # (code 128 decodes to 1/255, not to 0)
        assert np.all(x[0, 0, :2, :3] == 0) and np.all(buf[0, 0, :2, :3] == 0)
    if project == "clamp":
        assert float(dx_.abs().max()) == 1.0
    if project == "u8":
        assert _same(dx_, torch.from_numpy(fv_ref.decode_table())[torch.from_numpy(codes).long()])


def test_the_first_momentum_step_is_the_plain_sgd_step(ops):
    """A zero buffer: torch's first step, which clones the gradient — x as `pixel_step(rule="sgd")` leaves it, buf = g + wd x."""
    gen = torch.Generator().manual_seed(3)
    x0, g = torch.randn(2, 3, 33, 37, generator=gen).cuda(), torch.randn(2, 3, 33, 37, generator=gen).cuda()
    a, b, buf = x0.clone(), x0.clone(), torch.zeros_like(x0)
    ops.pixel_momentum_step(a, g, buf, lr=100.0, momentum=0.9, weight_decay=1e-4)
    ops.pixel_step(b, g, None, rule="sgd", lr=100.0, weight_decay=1e-4)
    assert _same(a, b) and _same(buf, torch.from_numpy(g.cpu().numpy() + np.float32(1e-4) * x0.cpu().numpy()))


# ---- 5. the inversion's gradient on its own activation pattern -----------------------------------------------------------------
def _hip_patterns(saved):
    """Activation pattern of a HIP encoder run in the form `orc.backbone(patterns=...)` takes (as tests/test_gpu_feature_vis.py)."""
    widx = saved["widx"][..., :20].permute(0, 3, 1, 2).cpu()
    pat = {"stem_tap": (widx & 15).long(), "stem_pos": ((widx >> 4) & 1) == 0}
    names = [f"layer{li}.{b}" for li in range(1, 5) for b in range(3)]
    for name, (_xin, o1, out) in zip(names, saved["blocks"]):
        c = orc.STAGES[int(name[5]) - 1][1]
        pat[name + ".o1"] = (o1[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
        pat[name] = (out[..., :c].float() > 0).permute(0, 3, 1, 2).cpu()
    return pat


MATCH_GATES = {torch.float32: 1e-5, X3: 2e-4, torch.bfloat16: 4e-2}


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_inversion_gradient_on_its_own_activation_pattern(golden_dir, dtype, case):
    """d(sum_t loss_t)/d tiles through `stage_match` + `encoder_pixel_gradient` for every stage against fp64 autograd on the linear
    piece the HIP forward took, the targets being the HIP forward's own outputs for a second bag (so the fp64 loss has the very
    target the device matched): L2 error of dx relative to its norm within the gates of
    test_filter_gradient_on_its_own_activation_pattern — 1e-5 for fp32, 2e-4 for bf16x3, 4e-2 for bf16.  Unlike that test's
    one-channel seed this one is dense: in bf16 storage every element of dz carries a rounding of up to 2^-9, and the device's
    act - target is taken between bf16-rounded outputs while fp64 follows the unrounded ones.
    Measured on MI355X, layer1 / layer2 / layer3 / layer4 at 6x64x64: fp32 9.94e-7 / 1.84e-6 / 2.60e-6 / 3.82e-6; bf16x3 1.86e-5 /
    3.58e-5 / 4.41e-5 / 5.24e-5; bf16 1.35e-2 / 2.25e-2 / 2.62e-2 / 3.37e-2.  At 3x50x70: fp32 1.01e-6 / 1.82e-6 / 3.06e-6 / 3.92e-6;
    bf16x3 1.87e-5 / 3.17e-5 / 4.40e-5 / 4.98e-5; bf16 1.29e-2 / 2.05e-2 / 3.02e-2 / 3.47e-2 — three to 3.6 times the one-channel
    seed's figures, and the dense bf16 seed stays inside its gate."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    n, h, w = case
    x = synth_bag(n, h, w, 20260401)
    other = synth_bag(n, h, w, 20260402)
    wts = _weights(golden_dir)
    enc = _model(golden_dir, dtype).cnn.module
    st = L.storage_dtype(dtype)
    got, targets = {}, {}
    with L.f32_mma(L.mma_code(dtype)), torch.no_grad():
        _f, tsaved = encoder.encoder_forward(enc, other.cuda(), st)
        _feats, saved = encoder.encoder_forward(enc, x.cuda(), st)
        pat = _hip_patterns(saved)
        for stage, c in enumerate(encoder.STAGE_WIDTHS, 1):
            target = tsaved["blocks"][3 * stage - 1][2]
            _loss, dz = ops.stage_match(saved["blocks"][3 * stage - 1][2], target, c, weight=0.1)
            got[stage] = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)[0].double().cpu()
            targets[stage] = target[..., :c].double().permute(0, 3, 1, 2).cpu()
    sd64 = {k: torch.tensor(wts[k], dtype=torch.float64) for k, _s in orc.state_dict_spec()}
    x64 = x.double().requires_grad_()
    acts = {}
    orc.backbone(sd64, x64, acts=acts, patterns=pat)
    errs = []
    for stage, dx in got.items():
        t64 = targets[stage]
        loss = (0.1 * ((acts[f"layer{stage}"] - t64) ** 2).sum(dim=(1, 2, 3)) / (t64 ** 2).sum(dim=(1, 2, 3))).sum()
        (want,) = torch.autograd.grad(loss, x64, retain_graph=True)
        errs.append(float((dx - want).norm() / want.norm()))
    print(f"own-pattern inversion gradient [{dtype}, {case}]: layer1..4 " + " / ".join(f"{e:.2e}" for e in errs))
    assert all(e < MATCH_GATES[dtype] for e in errs), errs


# ---- 6. the classes equal their loops ------------------------------------------------------------------------------------------
def _manual_inversion(fi, tiles, stage, steps, shifts, seed):
    """The six ops by hand, with outputs of its own that are poisoned first."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    enc, mode, reg = fi.net, fi.net.compute_dtype, fi.regularizer
    st = L.storage_dtype(mode)
    c = encoder.STAGE_WIDTHS[stage - 1]
    x = (0.1 * torch.randn(tuple(tiles.shape), generator=torch.Generator().manual_seed(seed))).cuda()
    n = x.shape[0]
    buf = torch.zeros_like(x)
    trace = torch.full((steps, n), NAN, device="cuda")
    terms = torch.full((steps, 2, n), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    lr = fi.lr
    with L.f32_mma(L.mma_code(mode)), torch.no_grad():
        _f, tsaved = encoder.encoder_forward(enc, tiles.u8 if hasattr(tiles, "u8") else tiles, st, upto=stage)
        target = tsaved["blocks"][-1][2]
        energy = ops.stage_energy(target, c)
        for k in range(steps):
            xs = ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]) if reg.jitter else x
            _f, saved = encoder.encoder_forward(enc, xs, st, upto=stage)
            loss, dz = ops.stage_match(saved["blocks"][-1][2], target, c, weight=fi.weight, energy=energy)
            trace[k] = loss
            g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)
            g = ops.pixel_reg(x, g, torch.full_like(x, NAN), alpha=reg.alpha, alpha_weight=reg.alpha_weight, tv_weight=reg.tv_weight,
                              shift=shifts[k], terms=terms[k])
            ops.pixel_momentum_step(x, g, buf, lr=lr, momentum=fi.momentum, project=fi.project, u8_out=u8 if k == steps - 1 else None)
            if fi.lr_decay is not None and k % fi.lr_decay[0] == 0:
                lr *= fi.lr_decay[1]
    return x, u8, trace, terms


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_inverter_equals_the_loop_of_the_six_ops(golden_dir, dtype):
    import mil_amd
    model = _model(golden_dir, dtype)
    # 50x70 with jitter 3, the toolkit's decaying schedule, from bytes; regulariser weights large enough to reach the bits
    reg = mil_amd.PixelRegularizer(alpha=6, alpha_weight=1e-3, tv_weight=1e-3, jitter=3, seed=4)
    fi = mil_amd.FeatureInverter(model, lr=50.0, lr_decay=(2, 0.5), regularizer=reg, project="clamp")
    tiles = mil_amd.U8Tiles(_to_u8(synth_bag(3, 50, 70, 20260403)).cuda())
    res = fi.invert(tiles, "layer2", steps=4, seed=7)
    shifts = reg.shifts(4)
    assert any(s != (0, 0) for s in shifts)
    x, u8, trace, terms = _manual_inversion(fi, tiles, 2, 4, shifts, 7)
    assert isinstance(res, mil_amd.InversionResult) and isinstance(res.u8, mil_amd.U8Tiles)
    assert res.trace.shape == (4, 3) and res.terms.shape == (4, 2, 3) and bool(torch.isfinite(res.trace).all()) and bool(torch.isfinite(res.terms).all())
    assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace) and _same(res.terms, terms)
    again = fi.invert(tiles, "layer2", steps=4, seed=7)
    assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace) and _same(again.terms, res.terms)
    assert not _same(fi.invert(tiles, "layer2", steps=4, seed=8).x, res.x)
    assert _same(fi.invert(tiles.float(), "layer2", steps=4, seed=7).x, res.x)     # bytes or the fp32 stack they decode to
    # 64x64 without jitter, the defaults, on the bare encoder
    fb = mil_amd.FeatureInverter(model.cnn.module)
    f32 = synth_bag(3, 64, 64, 20260404).cuda()
    res = fb.invert(f32, "layer4", steps=3)
    x, u8, trace, terms = _manual_inversion(fb, f32, 4, 3, [(0, 0)] * 3, 0)
    assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace) and _same(res.terms, terms)
    again = fb.invert(f32, "layer4", steps=3)
    assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace) and _same(again.terms, res.terms)
    # distance: the loss of stage_match for the final image, and what the next step's trace row would hold
    d = fb.distance(res.x, f32, "layer4")
    assert d.shape == (3,) and d.dtype == torch.float32 and bool(torch.isfinite(d).all())
    assert _same(fb.invert(f32, "layer4", steps=4).trace[3], d)


def _manual_regularised_filters(fv, x, stage, chans, steps, kw, shifts):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    enc, mode, reg = fv.net, fv.net.compute_dtype, fv.regularizer
    st = L.storage_dtype(mode)
    c = encoder.STAGE_WIDTHS[stage - 1]
    ch = torch.tensor(chans, dtype=torch.int32).cuda()
    state = (torch.zeros_like(x), torch.zeros_like(x))
    trace = torch.full((steps, x.shape[0]), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(mode)), torch.no_grad():
        for k in range(steps):
            xs = ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]) if reg.jitter else x
            _f, saved = encoder.encoder_forward(enc, xs, st, upto=stage)
            j, dz = ops.stage_seed(saved["blocks"][-1][2], ch, c)
            trace[k] = j
            g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)
            g = ops.pixel_reg(x, g, torch.full_like(x, NAN), alpha=reg.alpha, alpha_weight=reg.alpha_weight, tv_weight=reg.tv_weight, shift=shifts[k])
            ops.pixel_step(x, g, state, step=k + 1, u8_out=u8 if k == steps - 1 else None, **kw)
    return x, u8, trace


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_regularised_feature_visualizer_equals_its_loops(golden_dir, dtype):
    import mil_amd
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    from mil_amd.head import head_apply
    from mil_amd.saliency import bag_setup
    model = _model(golden_dir, dtype)
    adam = dict(rule="adam", lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, project="none")
    chans = [0, 19, 39]
    # filters, 50x70 with jitter 3 and 64x64 without
    for size, reg in (((50, 70), mil_amd.PixelRegularizer(alpha=4, alpha_weight=1e-3, tv_weight=1e-3, jitter=3, seed=2)),
                      ((64, 64), mil_amd.PixelRegularizer(alpha_weight=1e-3, tv_weight=1e-3))):
        fv = mil_amd.FeatureVisualizer(model, regularizer=reg)
        res = fv.filters("layer2", channels=chans, size=size, steps=3, seed=4)
        start = torch.randint(150, 180, (3, 3) + size, generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
        x, u8, trace = _manual_regularised_filters(fv, mil_amd.U8Tiles(start.cuda()).float(), 2, chans, 3, adam, reg.shifts(3))
        assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace)
        again = fv.filters("layer2", channels=chans, size=size, steps=3, seed=4)
        assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace)
        plain = mil_amd.FeatureVisualizer(model).filters("layer2", channels=chans, size=size, steps=3, seed=4)
        assert not _same(plain.x, res.x)                                         # the regulariser does reach the image
    # regularizer=None: the class as it was
    a = mil_amd.FeatureVisualizer(model, regularizer=None).filters("layer2", channels=chans, size=(50, 70), steps=3, seed=4)
    b = mil_amd.FeatureVisualizer(model).filters("layer2", channels=chans, size=(50, 70), steps=3, seed=4)
    assert _same(a.x, b.x) and _same(a.u8.u8, b.u8.u8) and _same(a.trace, b.trace)
    ca = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8", regularizer=None).classes(2, 4, size=(64, 64), steps=2, seed=9)
    cb = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8").classes(2, 4, size=(64, 64), steps=2, seed=9)
    assert _same(ca.x, cb.x) and _same(ca.u8.u8, cb.u8.u8) and _same(ca.trace, cb.trace)
    # classes with a jittering regulariser
    reg = mil_amd.PixelRegularizer(alpha_weight=1e-3, tv_weight=1e-3, jitter=3, seed=6)
    fc = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="clamp", regularizer=reg)
    cres = fc.classes(2, 4, size=(50, 70), steps=3, seed=9)
    shifts = reg.shifts(3)
    enc, st = model.cnn.module, L.storage_dtype(dtype)
    x = mil_amd.U8Tiles(torch.randint(0, 256, (4, 3, 50, 70), generator=torch.Generator().manual_seed(9), dtype=torch.uint8).cuda()).float()
    layout, y, cw = bag_setup(model, 4, 2)
    trace = torch.full((3, 4), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(dtype)):
        for k in range(3):
            with torch.no_grad():
                feats, saved = encoder.encoder_forward(enc, ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]), st)
            H = feats.detach().requires_grad_(True)
            loss = head_apply(H, layout, y, None, cw, [p.detach() for p in model.head_weights()], None, direct=False)[0]
            (dH,) = torch.autograd.grad(loss.sum(), H)
            with torch.no_grad():
                trace[k] = -loss.detach()
                g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dH)
                g = ops.pixel_reg(x, g, torch.full_like(x, NAN), alpha=6, alpha_weight=1e-3, tv_weight=1e-3, shift=shifts[k])
                ops.pixel_step(x, g, None, rule="sgd", lr=6, weight_decay=0, step=k + 1, project="clamp", u8_out=u8 if k == 2 else None)
    assert _same(cres.x, x) and _same(cres.u8.u8, u8) and _same(cres.trace, trace)
    again = fc.classes(2, 4, size=(50, 70), steps=3, seed=9)
    assert _same(again.x, cres.x) and _same(again.u8.u8, cres.u8.u8) and _same(again.trace, cres.trace)


# ---- 7. it descends ------------------------------------------------------------------------------------------------------------
def _descent_inputs():
    tiles = synth_bag(3, 64, 64, 20260405)
    x0 = 0.1 * torch.randn(tuple(tiles.shape), generator=torch.Generator().manual_seed(0))
    return tiles, x0


@functools.lru_cache(maxsize=None)
def _oracle_descent(golden_dir, layer):
    """The toolkit's loop on the CPU oracle (fp32) at lr=100: (distance at the start, gain after 12 steps) per tile; computed once
    per layer and shared by the three modes."""
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    w = _weights(golden_dir)
    sd = {k: torch.tensor(w[k]) for k, _s in orc.state_dict_spec()}
    tiles, x0 = _descent_inputs()
    _x, trace = ref.oracle_invert_loop(orc, sd, tiles, x0, layer, 12, lr=100.0, momentum=0.9)
    return trace[0], trace[0] - trace[-1]


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("layer", ["layer1", "layer4"])
def test_inversion_descends_at_least_half_as_far_as_the_oracle(golden_dir, layer, dtype):
    """Golden weights, 3 tiles of 64x64, 12 steps at lr=100 and momentum 0.9 with the default regulariser from seed 0:
    distance(start) - distance(result) is at least half the gain of the same loop on the CPU oracle, per tile, and the oracle's
    gain is positive.  On the CPU the oracle falls from about 0.070 to 0.018 (layer1) and from 0.068 to about 0.005 (layer4).
    Measured on MI355X, the gain relative to the oracle's: within 0.04 % in fp32, 0.4 % in bf16x3, 1.1 % in bf16."""
    import mil_amd
    d0, gain = _oracle_descent(golden_dir, layer)
    tiles, x0 = _descent_inputs()
    fi = mil_amd.FeatureInverter(_model(golden_dir, dtype), lr=100.0, momentum=0.9)
    res = fi.invert(tiles, layer, steps=12, seed=0)
    start = fi.distance(x0, tiles, layer)
    assert _same(start, res.trace[0])                                            # the inverter did start from x0
    got = (start - fi.distance(res.x, tiles, layer)).cpu()
    print(f"descent[{layer}, {dtype}]: start {start.cpu().tolist()} (oracle {d0.tolist()}), gain {got.tolist()} (oracle {gain.tolist()})")
    assert bool((gain > 0).all()) and bool((got >= 0.5 * gain).all()), (got, gain)


# ---- 8. side effects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_inverter_leaves_the_model_as_it_found_it(golden_dir, dtype):
    import mil_amd
    net = _model(golden_dir, dtype)
    net.train()                                                                  # the flag is left alone, whatever it is
    marks = {k: torch.full_like(p, 0.5) if i % 2 else None for i, (k, p) in enumerate(net.named_parameters())}
    for k, p in net.named_parameters():
        p.grad = None if marks[k] is None else marks[k].clone()
    u8 = mil_amd.U8Tiles(_to_u8(synth_bag(3, 64, 64, 20260406)).cuda())
    before = u8.u8.clone()
    f32 = u8.float()
    kept = f32.clone()
    rng, rng_gpu = torch.get_rng_state(), torch.cuda.get_rng_state()
    reg = mil_amd.PixelRegularizer(jitter=2)
    fi = mil_amd.FeatureInverter(net, regularizer=reg)
    fi.invert(u8, "layer1", steps=2)
    fi.invert(f32, "layer4", steps=2)
    fi.distance(f32, u8, "layer3")
    fv = mil_amd.FeatureVisualizer(net, regularizer=reg)
    fv.filters("layer1", channels=[0, 7], size=(64, 64), steps=2)
    fv.dream(u8, "layer4", 41, steps=2)
    fv.classes(1, 4, size=(64, 64), steps=2)
    assert torch.equal(torch.get_rng_state(), rng) and torch.equal(torch.cuda.get_rng_state(), rng_gpu) and net.training
    assert torch.equal(u8.u8, before) and torch.equal(f32, kept)
    for k, p in net.named_parameters():
        assert (p.grad is None) if marks[k] is None else torch.equal(p.grad, marks[k]), k


def test_feature_inverter_with_flat_params_leaves_the_bucket_alone(golden_dir):
    import mil_amd
    net = _model(golden_dir, X3)
    flat = mil_amd.FlatParams(net)
    x = synth_bag(8, 64, 64, 20260407).cuda()
    flat.zero_grad()
    net(x, torch.tensor([0], device="cuda"))["loss"].backward()
    bucket = flat.flat_grad.clone()
    assert float(bucket.abs().max()) > 0
    reg = mil_amd.PixelRegularizer(jitter=2)
    mil_amd.FeatureInverter(net, regularizer=reg).invert(x[:3], "layer3", steps=2)
    fv = mil_amd.FeatureVisualizer(net, regularizer=reg)
    fv.filters("layer3", channels=[0, 31], size=(64, 64), steps=2)
    fv.classes(0, 4, size=(64, 64), steps=2)
    assert torch.equal(flat.flat_grad, bucket)
