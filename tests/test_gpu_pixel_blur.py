"""-m gpu: the Gaussian blur on the device — `ops.pixel_blur` bit for bit against its numpy restatement (tests/pixel_blur_reference.py)
for every edge rule, the radii 1, 4 and 16, shapes around the kernel's 64 x 64 tile and tensors on and off the 16-byte grid;
non-finite inputs; and `mil_amd.FeatureInverter` / `FeatureVisualizer` with the blur options of `mil_amd.PixelRegularizer` against
the hand-written loops of the ops.  Every output buffer a kernel is handed is NaN-filled first."""
import os

import numpy as np
import pytest
import torch

import pixel_blur_reference as ref
from fixture_inputs import synth_bag
from gpu_util import X3

pytestmark = pytest.mark.gpu

NAN = float("nan")
TILE = 64                                        # pixel_blur.hip: PB_TILE, the output tile of a workgroup
MODES = [torch.float32, X3, torch.bfloat16]
MODE_IDS = ["fp32", "bf16x3", "bf16"]
# 1x1: replicate and wrap only; 3x40: wrap with radius >= H, replicate; 5x7: reflect at its limit radius = H - 1 with radius 4;
# the tile exactly, the tile plus one in each dimension, two tiles minus one
SHAPES = [(1, 1), (3, 40), (5, 7), (33, 37), (50, 70), (64, 64), (TILE, TILE), (TILE + 1, TILE + 1), (2 * TILE - 1, 2 * TILE - 1)]
SHAPES = list(dict.fromkeys(SHAPES))
PLANES = (1, 6, 7)


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _bits(t):
    t = t.detach().contiguous().cpu()
    return t.view({4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _buffer(values, misalign):
    """A contiguous device tensor holding `values`; misalign: its first element sits 4 bytes off the 16-byte grid, which sends the
    kernel down its element-by-element paths."""
    flat = torch.empty(values.numel() + 4, dtype=torch.float32, device="cuda")
    view = flat[1:1 + values.numel()] if misalign else flat[:values.numel()]
    view = view.view(values.shape)
    view.copy_(values)
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


def _nan_like(shape, misalign=False):
    return _buffer(torch.full(shape, NAN), misalign)


def _planes(h, w, seed):
    """7 planes of h x w: values of mixed magnitude and sign, a signed zero and an exact zero patch."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((7, h, w)) * 10.0 ** rng.integers(-2, 3, (7, 1, 1))).astype(np.float32)
    x[0, 0, 0] = -0.0
    x[-1, : h // 2, : w // 2] = 0.0
    return x


# ---- 1. bit for bit against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("sigma", [0.25, 1.0, 4.0], ids=["r1", "r4", "r16"])
def test_pixel_blur_bit_for_bit(ops, sigma, edge):
    """One reference per shape (7 planes; a plane's output depends on that plane alone, so 1 and 6 planes are its first ones),
    compared for 1, 6 and 7 planes with x and out on the 16-byte grid and 4 bytes off it; the 6 planes also as a stack [2,3,H,W].
    Where reflect cannot take the shape (radius > min(H, W) - 1) the wrapper refuses it."""
    radius, taps = ops.gauss_taps(sigma)
    assert radius == {0.25: 1, 1.0: 4, 4.0: 16}[sigma]
    ran = 0
    for h, w in SHAPES:
        x = _planes(h, w, 100 * h + w)
        if edge == "reflect" and radius > min(h, w) - 1:
            with pytest.raises(ValueError, match="reflect"):
                ops.pixel_blur(torch.from_numpy(x).cuda(), sigma=sigma, edge=edge)
            continue
        want = torch.from_numpy(ref.pixel_blur(x, taps, edge))
        for planes in PLANES:
            for misalign in (False, True):
                dx_ = _buffer(torch.from_numpy(x[:planes]), misalign)
                out = _nan_like((planes, h, w), misalign)
                assert ops.pixel_blur(dx_, out, sigma=sigma, edge=edge) is out
                assert _same(out, want[:planes]), (h, w, planes, misalign)
                assert _same(dx_, torch.from_numpy(x[:planes]))                  # x is only read
                ran += 1
        stack = _buffer(torch.from_numpy(x[:6]).view(2, 3, h, w), False)
        got = ops.pixel_blur(stack, _nan_like((2, 3, h, w)), sigma=sigma, edge=edge)
        assert got.shape == (2, 3, h, w) and _same(got.view(6, h, w), want[:6])
        assert _same(ops.pixel_blur(stack, sigma=sigma, edge=edge), got)          # a fresh output; and a second call: the same bits
        one = ops.pixel_blur(torch.from_numpy(x[3]).cuda(), sigma=sigma, edge=edge)     # a single plane [H,W]
        assert _same(one, want[3])
    assert ran >= 6 * (len(SHAPES) - 3)
    if radius == 4:
        assert edge != "reflect" or ran == 6 * (len(SHAPES) - 2)                  # 5x7 did run: reflect at radius = H - 1
    if radius == 16 and edge == "wrap":
        assert ran == 6 * len(SHAPES)                                            # 1x1 and 3x40 too: radius >= n


def test_the_public_name_blurs_stacks_and_maps(ops):
    import mil_amd
    x = _planes(50, 70, 5)[:6]
    _r, taps = ops.gauss_taps(2.0)
    want = torch.from_numpy(ref.pixel_blur(x, taps, "reflect"))
    maps = torch.from_numpy(x).cuda()
    got = mil_amd.gaussian_blur(maps, 2.0)
    assert _same(got, want)
    out = _nan_like((2, 3, 50, 70))
    assert mil_amd.gaussian_blur(maps.view(2, 3, 50, 70), 2.0, out=out) is out and _same(out.view(6, 50, 70), want)
    assert _same(mil_amd.gaussian_blur(maps, 2.0, edge="wrap"), torch.from_numpy(ref.pixel_blur(x, taps, "wrap")))
    empty = mil_amd.gaussian_blur(maps[:0], 2.0)
    assert empty.shape == (0, 50, 70)


@pytest.mark.parametrize("edge", ref.EDGES)
def test_arbitrary_symmetric_taps(ops, edge):
    """The arithmetic is defined for any taps: signs, a zero, taps that do not sum to one, radius 1 .. 16 that no sigma gives."""
    rng = np.random.default_rng(17)
    for radius in (1, 2, 5, 7, 11, 16):
        taps = rng.uniform(-1.5, 1.5, radius + 1)
        taps[radius // 2] = 0.0
        for h, w in ((33, 37), (TILE + 1, TILE + 1)):
            x = _planes(h, w, radius)[:3]
            want = torch.from_numpy(ref.pixel_blur(x, taps, edge))
            for misalign in (False, True):
                out = _nan_like((3, h, w), misalign)
                ops.pixel_blur(_buffer(torch.from_numpy(x), misalign), out, taps=list(taps), edge=edge)
                assert _same(out, want), (radius, h, w, misalign)


@pytest.mark.parametrize("edge", ref.EDGES)
@pytest.mark.parametrize("sigma", [0.25, 1.0, 4.0], ids=["r1", "r4", "r16"])
def test_non_finite_inputs_spread_as_in_the_restatement(ops, sigma, edge):
    """One NaN and one +inf planted in each of two 33x37 planes, one of the pair next to a corner (within every radius of it), the
    other further down in the neighbouring column: the output's NaNs and infinities are where the restatement has them, and every
    finite output equals it bit for bit.  (Radius 16 under wrap reaches all 33 rows and 33 of the 37 columns from any one sample:
    the pair shares its columns but for one, so that three columns stay finite and one holds infinities without NaNs.)"""
    radius, taps = ops.gauss_taps(sigma)
    x = _planes(33, 37, 9)[:2]
    x[0, 1, 1] = np.nan
    x[0, 20, 2] = np.inf
    x[1, 31, 35] = np.inf
    x[1, 12, 34] = np.nan
    want = ref.pixel_blur(x, taps, edge)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).any()
    for misalign in (False, True):
        out = _nan_like((2, 33, 37), misalign)
        ops.pixel_blur(_buffer(torch.from_numpy(x), misalign), out, sigma=sigma, edge=edge)
        got = out.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
        assert np.array_equal(np.signbit(got[np.isinf(got)]), np.signbit(want[np.isinf(want)]))
        fin = np.isfinite(want)
        assert np.array_equal(got[fin].view(np.int32), want[fin].view(np.int32))


# ---- 2. the classes equal their loops ------------------------------------------------------------------------------------------
def _model(golden_dir, dtype):
    import mil_amd
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net.eval()


class _BlurCount:
    """`ops.TIMER` as a call counter: the labels of the `pixel_blur` launches, none other bracketed."""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        self.timer = self.ops.KernelTimer(lambda label: isinstance(label, tuple) and label[0] == "pixel_blur")
        self.kept, self.ops.TIMER = self.ops.TIMER, self.timer
        return self

    def __exit__(self, *exc):
        self.ops.TIMER = self.kept
        return False

    @property
    def n(self):
        return len(self.timer.spans)


def _start_of_step(ops, reg, x, k):
    """The image blur at the start of step k, into a poisoned stack of its own."""
    if reg.blur_sigma and k > 0 and k % reg.blur_every == 0:
        return ops.pixel_blur(x, torch.full_like(x, NAN), sigma=reg.blur_sigma, edge=reg.blur_edge)
    return x


def _regularised(ops, reg, x, g, shift, terms=None):
    g = ops.pixel_reg(x, g, torch.full_like(x, NAN), alpha=reg.alpha, alpha_weight=reg.alpha_weight, tv_weight=reg.tv_weight, shift=shift,
                      terms=terms)
    if reg.grad_blur_sigma:
        g = ops.pixel_blur(g, torch.full_like(x, NAN), sigma=reg.grad_blur_sigma, edge=reg.blur_edge)
    return g


def _manual_inversion(fi, tiles, stage, steps, seed):
    """The stated order by hand: [image blur] - [jittered copy] - forward - stage_match - pixel gradient - pixel_reg - [gradient
    blur] - momentum step; every output in a poisoned tensor of its own."""
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    enc, mode, reg = fi.net, fi.net.compute_dtype, fi.regularizer
    st = L.storage_dtype(mode)
    c = encoder.STAGE_WIDTHS[stage - 1]
    shifts = reg.shifts(steps)
    x = (0.1 * torch.randn(tuple(tiles.shape), generator=torch.Generator().manual_seed(seed))).cuda()
    n = x.shape[0]
    buf = torch.zeros_like(x)
    trace = torch.full((steps, n), NAN, device="cuda")
    terms = torch.full((steps, 2, n), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(mode)), torch.no_grad():
        _f, tsaved = encoder.encoder_forward(enc, tiles, st, upto=stage)
        target = tsaved["blocks"][-1][2]
        energy = ops.stage_energy(target, c)
        for k in range(steps):
            x = _start_of_step(ops, reg, x, k)
            xs = ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]) if reg.jitter else x
            _f, saved = encoder.encoder_forward(enc, xs, st, upto=stage)
            loss, dz = ops.stage_match(saved["blocks"][-1][2], target, c, weight=fi.weight, energy=energy)
            trace[k] = loss
            g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)
            g = _regularised(ops, reg, x, g, shifts[k], terms[k])
            ops.pixel_momentum_step(x, g, buf, lr=fi.lr, momentum=fi.momentum, project=fi.project, u8_out=u8 if k == steps - 1 else None)
    return x, u8, trace, terms


def _manual_filters(fv, x, stage, chans, steps):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    enc, mode, reg = fv.net, fv.net.compute_dtype, fv.regularizer
    st = L.storage_dtype(mode)
    c = encoder.STAGE_WIDTHS[stage - 1]
    shifts = reg.shifts(steps)
    ch = torch.tensor(chans, dtype=torch.int32).cuda()
    state = (torch.zeros_like(x), torch.zeros_like(x))
    trace = torch.full((steps, x.shape[0]), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(mode)), torch.no_grad():
        for k in range(steps):
            x = _start_of_step(ops, reg, x, k)
            xs = ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]) if reg.jitter else x
            _f, saved = encoder.encoder_forward(enc, xs, st, upto=stage)
            j, dz = ops.stage_seed(saved["blocks"][-1][2], ch, c)
            trace[k] = j
            g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dz=dz, stage=stage)
            g = _regularised(ops, reg, x, g, shifts[k])
            ops.pixel_step(x, g, state, rule="adam", lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8, project="none", step=k + 1,
                           u8_out=u8 if k == steps - 1 else None)
    return x, u8, trace


def _manual_classes(model, reg, x, label, steps):
    from mil_amd import _lib as L
    from mil_amd import encoder
    from mil_amd import ops
    from mil_amd.head import head_apply
    from mil_amd.saliency import bag_setup
    dtype = model.cnn.module.compute_dtype
    enc, st = model.cnn.module, L.storage_dtype(dtype)
    shifts = reg.shifts(steps)
    layout, y, cw = bag_setup(model, x.shape[0], label)
    trace = torch.full((steps, x.shape[0]), NAN, device="cuda")
    u8 = torch.full(x.shape, 255, dtype=torch.uint8, device="cuda")
    with L.f32_mma(L.mma_code(dtype)):
        for k in range(steps):
            with torch.no_grad():
                x = _start_of_step(ops, reg, x, k)
                xs = ops.pixel_shift(x, torch.full_like(x, NAN), shifts[k]) if reg.jitter else x
                feats, saved = encoder.encoder_forward(enc, xs, st)
            H = feats.detach().requires_grad_(True)
            loss = head_apply(H, layout, y, None, cw, [p.detach() for p in model.head_weights()], None, direct=False)[0]
            (dH,) = torch.autograd.grad(loss.sum(), H)
            with torch.no_grad():
                trace[k] = -loss.detach()
                g, _s = encoder.encoder_pixel_gradient(enc, saved, st, dfeats=dH)
                g = _regularised(ops, reg, x, g, shifts[k])
                ops.pixel_step(x, g, None, rule="sgd", lr=6, weight_decay=0, step=k + 1, project="u8", u8_out=u8 if k == steps - 1 else None)
    return x, u8, trace


BLURS = [dict(blur_sigma=1.0, blur_every=2), dict(grad_blur_sigma=0.5), dict(blur_sigma=1.0, blur_every=2, grad_blur_sigma=0.5)]
GEOMETRY = [((50, 70), 3, "wrap"), ((64, 64), 0, "reflect")]          # (size, jitter, blur_edge)
STEPS = 5


def _expected_launches(kw):
    return (2 if kw.get("blur_sigma") else 0) + (STEPS if kw.get("grad_blur_sigma") else 0)      # image blur at steps 2 and 4


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_inverter_with_blur_equals_the_loop_of_the_ops(golden_dir, dtype, ops):
    import mil_amd
    model = _model(golden_dir, dtype)
    for size, jitter, edge in GEOMETRY:
        tiles = synth_bag(3, size[0], size[1], 20260501).cuda()
        base = dict(alpha=6, alpha_weight=1e-3, tv_weight=1e-3, jitter=jitter, seed=4)
        plain = mil_amd.FeatureInverter(model, lr=50.0, regularizer=mil_amd.PixelRegularizer(**base), project="u8").invert(tiles, "layer2", steps=STEPS, seed=7)
        for kw in BLURS:
            reg = mil_amd.PixelRegularizer(**base, blur_edge=edge, **kw)
            fi = mil_amd.FeatureInverter(model, lr=50.0, regularizer=reg, project="u8")
            with _BlurCount(ops) as count:
                res = fi.invert(tiles, "layer2", steps=STEPS, seed=7)
            assert count.n == _expected_launches(kw), (count.n, kw)
            x, u8, trace, terms = _manual_inversion(fi, tiles, 2, STEPS, 7)
            assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace) and _same(res.terms, terms), (size, kw)
            assert bool(torch.isfinite(res.x).all()) and bool(torch.isfinite(res.trace).all()) and bool(torch.isfinite(res.terms).all())
            again = fi.invert(tiles, "layer2", steps=STEPS, seed=7)
            assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace) and _same(again.terms, res.terms)
            assert not _same(res.x, plain.x)                                     # the blur does reach the image
            # the u8 and x of a result are the ones the last step encoded: a blur never follows it
            assert _same(res.x, mil_amd.U8Tiles(res.u8.u8).float())
        # the options at their defaults, spelled out: no pixel_blur launch and the bits of a regulariser built without them
        off = mil_amd.PixelRegularizer(**base, blur_sigma=0.0, blur_every=2, grad_blur_sigma=0.0, blur_edge=edge)
        with _BlurCount(ops) as count:
            res = mil_amd.FeatureInverter(model, lr=50.0, regularizer=off, project="u8").invert(tiles, "layer2", steps=STEPS, seed=7)
        assert count.n == 0
        assert _same(res.x, plain.x) and _same(res.u8.u8, plain.u8.u8) and _same(res.trace, plain.trace) and _same(res.terms, plain.terms)


@pytest.mark.parametrize("dtype", MODES, ids=MODE_IDS)
def test_feature_visualizer_with_blur_equals_its_loops(golden_dir, dtype, ops):
    import mil_amd
    model = _model(golden_dir, dtype)
    chans = [0, 19, 39]
    for size, jitter, edge in GEOMETRY:
        base = dict(alpha=4, alpha_weight=1e-3, tv_weight=1e-3, jitter=jitter, seed=2)
        start = torch.randint(150, 180, (3, 3) + size, generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
        cstart = torch.randint(0, 256, (4, 3) + size, generator=torch.Generator().manual_seed(9), dtype=torch.uint8)
        pf = mil_amd.FeatureVisualizer(model, regularizer=mil_amd.PixelRegularizer(**base)).filters("layer2", channels=chans, size=size, steps=STEPS, seed=4)
        pc = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8", regularizer=mil_amd.PixelRegularizer(**base)).classes(
            2, 4, size=size, steps=STEPS, seed=9)
        for kw in BLURS:
            reg = mil_amd.PixelRegularizer(**base, blur_edge=edge, **kw)
            fv = mil_amd.FeatureVisualizer(model, regularizer=reg)
            with _BlurCount(ops) as count:
                res = fv.filters("layer2", channels=chans, size=size, steps=STEPS, seed=4)
            assert count.n == _expected_launches(kw), (count.n, kw)
            x, u8, trace = _manual_filters(fv, mil_amd.U8Tiles(start.cuda()).float(), 2, chans, STEPS)
            assert _same(res.x, x) and _same(res.u8.u8, u8) and _same(res.trace, trace), (size, kw)
            again = fv.filters("layer2", channels=chans, size=size, steps=STEPS, seed=4)
            assert _same(again.x, res.x) and _same(again.u8.u8, res.u8.u8) and _same(again.trace, res.trace)
            assert not _same(res.x, pf.x)
            fc = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8", regularizer=reg)
            with _BlurCount(ops) as count:
                cres = fc.classes(2, 4, size=size, steps=STEPS, seed=9)
            assert count.n == _expected_launches(kw), (count.n, kw)
            x, u8, trace = _manual_classes(model, reg, mil_amd.U8Tiles(cstart.cuda()).float(), 2, STEPS)
            assert _same(cres.x, x) and _same(cres.u8.u8, u8) and _same(cres.trace, trace), (size, kw)
            again = fc.classes(2, 4, size=size, steps=STEPS, seed=9)
            assert _same(again.x, cres.x) and _same(again.u8.u8, cres.u8.u8) and _same(again.trace, cres.trace)
            assert not _same(cres.x, pc.x)
        off = mil_amd.PixelRegularizer(**base, blur_sigma=0.0, blur_every=2, grad_blur_sigma=0.0, blur_edge=edge)
        with _BlurCount(ops) as count:
            res = mil_amd.FeatureVisualizer(model, regularizer=off).filters("layer2", channels=chans, size=size, steps=STEPS, seed=4)
            cres = mil_amd.FeatureVisualizer(model, "sgd", lr=6, weight_decay=0, project="u8", regularizer=off).classes(2, 4, size=size, steps=STEPS, seed=9)
        assert count.n == 0
        assert _same(res.x, pf.x) and _same(res.u8.u8, pf.u8.u8) and _same(res.trace, pf.trace)
        assert _same(cres.x, pc.x) and _same(cres.u8.u8, pc.u8.u8) and _same(cres.trace, pc.trace)
    # dream takes the same loop as filters: a blurred run from real tiles equals itself and differs from the plain one
    u8 = mil_amd.U8Tiles(start.cuda())
    reg = mil_amd.PixelRegularizer(blur_sigma=1.0, blur_every=2, grad_blur_sigma=0.5)
    fv = mil_amd.FeatureVisualizer(model, regularizer=reg)
    d = fv.dream(u8, "layer2", chans, steps=STEPS)
    x, du8, trace = _manual_filters(fv, u8.float(), 2, chans, STEPS)
    assert _same(d.x, x) and _same(d.u8.u8, du8) and _same(d.trace, trace)
    assert torch.equal(u8.u8.cpu(), start)                                       # the tiles are left untouched
