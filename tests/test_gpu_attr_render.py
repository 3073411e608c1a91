"""-m gpu: the attribution renderer on the device — `ops.map_quantile` (exact radix select), `ops.attr_render` and
`ops.cam_overlay` bit for bit against the numpy restatement of DESIGN.md section 3.41 (tests/attr_render_reference.py, which
tests/test_cpu_attr_render.py holds to np.percentile, Pillow and matplotlib), fed the same fp32 inputs; and
`mil_amd.AttributionRenderer` end to end on the golden weights."""
import functools
import os

import numpy as np
import pytest
import torch

import attr_render_reference as ref

pytestmark = pytest.mark.gpu

# 1x1; odd sizes with H W % 4 != 0; more than one 4096-pixel chunk per tile, odd tile count; the aligned vector path; and two
# sizes whose virtual index at q = 99 sits within one ulp of an integer (99 * 0.99, 100 * 0.99)
SHAPES = [(1, 3, 1, 1), (2, 3, 33, 37), (5, 3, 50, 70), (3, 3, 64, 64), (2, 3, 10, 10), (1, 3, 1, 101)]
KINDS = ["cubed", "half_zero", "ties", "constant"]
QS = (99.0, 50.0, 100.0, 0.5)
GROUPS = ("tile", "bag")


def _ids(s):
    return "x".join(map(str, s))


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


@functools.lru_cache(maxsize=None)
def _grad(shape, kind):
    """One fp32 gradient [T,3,H,W] on the CPU (numpy), made once and never changed."""
    rng = np.random.default_rng(hash((shape, KINDS.index(kind) if kind in KINDS else 9)) % (1 << 32))
    g = (rng.standard_normal(shape) ** 3).astype(np.float32)
    if kind == "half_zero":
        mask = rng.random(shape) < 0.5
        g[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
    elif kind == "ties":
        g = np.round(g * 2).astype(np.float32)
    elif kind == "constant":
        g[0] = np.float32(-0.375)                      # the first tile is constant, the others (if any) are not
    elif kind == "negative":
        g = -np.abs(g) - np.float32(1e-3)
    elif kind == "positive":
        g = np.abs(g) + np.float32(1e-3)
    g.setflags(write=False)
    return g


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _check_stats(got, values, q):
    stats, p = ref.quantile_stats(values, q)
    gs, gp = got.stats.cpu().numpy(), got.p.cpu().numpy()
    assert gs.shape == stats.shape and gp.shape == p.shape
    assert np.array_equal(_bits(gs), _bits(stats)), (q, gs, stats)
    assert np.array_equal(_bits(gp), _bits(p)), (q, gp, p)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_map_quantile_is_exact(ops, shape, kind):
    g = _grad(shape, kind)
    x = torch.from_numpy(g.copy()).cuda()
    m = x[:, 1].contiguous()                           # a [T,H,W] map: signed values, -0.0 among them
    for group in GROUPS:
        for q in QS:
            _check_stats(ops.map_quantile(x, q, group), ref.values_of(g, group), q)
            _check_stats(ops.map_quantile(m, q, group), ref.values_of(g[:, 1], group), q)
        _check_stats(ops.map_quantile(x, 100.0, group, raw=True), ref.values_of(g, group, raw=True), 100.0)
        _check_stats(ops.map_quantile(x, 99.0, group, raw=True), ref.values_of(g, group, raw=True), 99.0)


def _split_map(n_lo, n, lo_vals, hi_vals, seed):
    """n values, the n_lo smallest drawn from lo_vals and the others from hi_vals (every lo value below every hi value), shuffled."""
    rng = np.random.default_rng(seed)
    v = np.concatenate([rng.choice(lo_vals, n_lo), rng.choice(hi_vals, n - n_lo)]).astype(np.float32)
    rng.shuffle(v)
    return v


@pytest.mark.parametrize("where", ["top11", "low10", "mid11"])
def test_lo_and_hi_in_different_bins(ops, where):
    """s[lo] and s[hi] part ways in the first digit (their top 11 key bits differ), in the last one (only the lowest 10 differ)
    and in the middle one: the select carries two prefixes from there on."""
    t, h, w = 3, 50, 70                                # two histogram chunks per tile
    n = h * w
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -23)
    for q in (99.0, 50.0):
        lo, hi, _ = ref.ranks(n, q)
        assert hi == lo + 1
        if where == "top11":
            lo_vals, hi_vals = np.linspace(0.5, 0.99, 97, dtype=np.float32), np.linspace(1e10, 2e10, 89, dtype=np.float32)
        elif where == "low10":
            lo_vals, hi_vals = one + ulp * np.arange(0, 500, dtype=np.float32), one + ulp * np.arange(500, 1024, dtype=np.float32)
        else:
            lo_vals, hi_vals = one + ulp * np.arange(0, 1024, dtype=np.float32), one + ulp * np.arange(1024, 4096, dtype=np.float32)
        m = np.stack([_split_map(lo + 1, n, lo_vals, hi_vals, 11 * i + int(q)) for i in range(t)]).reshape(t, h, w)
        m[1] = -m[1][::-1]                             # the same split among negative keys (ascending order reversed)
        stats, _ = ref.quantile_stats(ref.values_of(m), q)
        klo, khi = _bits(stats[0, 2:3])[0], _bits(stats[0, 3:4])[0]
        assert klo != khi
        if where == "top11":
            assert klo >> 21 != khi >> 21
        elif where == "low10":
            assert klo >> 10 == khi >> 10
        else:
            assert klo >> 21 == khi >> 21 and klo >> 10 != khi >> 10
        x = torch.from_numpy(m).cuda()
        _check_stats(ops.map_quantile(x, q, "tile"), ref.values_of(m), q)
        assert np.array_equal(ops.attr_render(x, ops.map_quantile(x, q, "tile"), "grayscale").cpu().numpy(), ref.grayscale_bytes(m, q))
    # in the bag the two ranks fall where the three tiles' values interleave
    _check_stats(ops.map_quantile(x, 50.0, "bag"), ref.values_of(m, "bag"), 50.0)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_grayscale_bytes(ops, shape, kind):
    g = _grad(shape, kind)
    x = torch.from_numpy(g.copy()).cuda()
    m = x[:, 2].contiguous()
    for group in GROUPS:
        for q in (99.0, 50.0):
            got = ops.attr_render(x, ops.map_quantile(x, q, group), "grayscale")
            assert got.dtype == torch.uint8 and got.shape == (shape[0],) + shape[2:]
            assert np.array_equal(got.cpu().numpy(), ref.grayscale_bytes(g, q, group)), (group, q)
            got = ops.attr_render(m, ops.map_quantile(m, q, group), "grayscale")
            assert np.array_equal(got.cpu().numpy(), ref.grayscale_bytes(g[:, 2], q, group)), (group, q, "map")
    if kind == "constant":
        assert not ops.attr_render(x, ops.map_quantile(x, 99.0, "tile"), "grayscale")[0].any()


@pytest.mark.parametrize("kind", KINDS + ["negative", "positive"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_colour_and_pos_neg_bytes(ops, shape, kind):
    g = _grad(shape, kind)
    x = torch.from_numpy(g.copy()).cuda()
    for group in GROUPS:
        st = ops.map_quantile(x, 100.0, group, raw=True)
        col = ops.attr_render(x, st, "colour")
        assert col.dtype == torch.uint8 and col.shape == (shape[0],) + shape[2:] + (3,)
        assert np.array_equal(col.cpu().numpy(), ref.colour_bytes(g, group)), group
        pos, neg = ops.attr_render(x, st, "pos_neg")
        want_pos, want_neg = ref.pos_neg_bytes(g, group)
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(neg.cpu().numpy(), want_neg), group
        if kind == "negative":
            assert not pos.any() and bool(neg.any())
        if kind == "positive":
            assert not neg.any() and bool(pos.any())
    if kind == "constant":
        assert not ops.attr_render(x, ops.map_quantile(x, 100.0, "tile", raw=True), "colour")[0].any()


def test_unaligned_input_takes_the_scalar_path(ops):
    """A gradient that starts 4 bytes off the 16-byte grid (H W % 4 == 0, so only the pointer decides)."""
    shape = (3, 3, 64, 64)
    g = _grad(shape, "cubed")
    buf = torch.zeros(g.size + 1, dtype=torch.float32, device="cuda")
    buf[1:] = torch.from_numpy(g.copy()).cuda().view(-1)
    x = buf[1:].view(shape)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    st = ops.map_quantile(x, 99.0, "tile")
    _check_stats(st, ref.values_of(g), 99.0)
    assert np.array_equal(ops.attr_render(x, st, "grayscale").cpu().numpy(), ref.grayscale_bytes(g))
    st = ops.map_quantile(x, 100.0, "tile", raw=True)
    assert np.array_equal(ops.attr_render(x, st, "colour").cpu().numpy(), ref.colour_bytes(g))


def test_two_launches_give_the_same_bits(ops):
    g = _grad((5, 3, 50, 70), "ties")
    x = torch.from_numpy(g.copy()).cuda()
    for group in GROUPS:
        a, b = ops.map_quantile(x, 99.0, group), ops.map_quantile(x, 99.0, group)
        assert torch.equal(a.stats.view(torch.int32), b.stats.view(torch.int32)) and torch.equal(a.p.view(torch.int64), b.p.view(torch.int64))
        assert torch.equal(ops.attr_render(x, a, "grayscale"), ops.attr_render(x, b, "grayscale"))
        r = ops.map_quantile(x, 100.0, group, raw=True)
        assert torch.equal(ops.attr_render(x, r, "colour"), ops.attr_render(x, r, "colour"))
        for u, v in zip(ops.attr_render(x, r, "pos_neg"), ops.attr_render(x, r, "pos_neg")):
            assert torch.equal(u, v)


def test_non_finite_values_return(ops):
    """Where a NaN or an infinity sorts is documented, not a contract beyond: the calls return."""
    g = _grad((2, 3, 33, 37), "cubed").copy()
    g[0, 0, 0, :5] = (np.nan, np.inf, -np.inf, -np.nan, np.nan)
    g[1, 2, 3, 3] = np.inf
    x = torch.from_numpy(g).cuda()
    for group in GROUPS:
        st = ops.map_quantile(x, 99.0, group)
        out = ops.attr_render(x, st, "grayscale")
        st_raw = ops.map_quantile(x, 100.0, group, raw=True)
        col = ops.attr_render(x, st_raw, "colour")
        pos, neg = ops.attr_render(x, st_raw, "pos_neg")
        torch.cuda.synchronize()
        assert out.shape == (2, 33, 37) and col.shape == pos.shape == neg.shape == (2, 33, 37, 3)
        assert st.stats.shape == ((2, 4) if group == "tile" else (1, 4))


@pytest.mark.parametrize("hw", [(33, 37), (64, 64)], ids=_ids)
def test_overlay_against_the_restatement(ops, hw):
    import mil_amd
    h, w = hw
    rng = np.random.default_rng(h * 100 + w)
    tiles = rng.integers(0, 256, (3, 3, h, w), dtype=np.uint8)
    amap = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    amap.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attr_render.npz"))
    u8 = mil_amd.U8Tiles(torch.from_numpy(tiles).cuda())
    dmap = torch.from_numpy(amap).cuda()
    for name in ("hsv", "viridis"):
        lut = golden["lut_" + name]
        for alpha, a in ((0.4, 102), (0.0, 0), (1.0, 255)):
            r = mil_amd.AttributionRenderer(cmap=name, alpha=alpha)
            assert r.alpha_byte == a
            heat, on = r.overlay(u8, dmap)
            want_heat, want_on = ref.overlay_bytes(tiles, amap, lut, a)
            assert heat.dtype == on.dtype == torch.uint8 and heat.shape == on.shape == (3, h, w, 3)
            assert np.array_equal(heat.cpu().numpy(), want_heat) and np.array_equal(on.cpu().numpy(), want_on), (name, a)
    # a table of the caller's own
    own = torch.from_numpy(rng.integers(0, 256, (256, 3), dtype=np.uint8))
    heat, on = mil_amd.AttributionRenderer(cmap=own, alpha=0.5).overlay(u8, dmap)
    want_heat, want_on = ref.overlay_bytes(tiles, amap, own.numpy(), 127)
    assert np.array_equal(heat.cpu().numpy(), want_heat) and np.array_equal(on.cpu().numpy(), want_on)


def test_renderer_end_to_end_on_the_golden_weights(golden_dir):
    """4 tiles of 64x64 through TileSaliency and the renderer: every picture equals the restatement applied to the same device
    gradient copied to the host."""
    import mil_amd
    from fixture_inputs import synth_bag
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    net = mil_amd.Attention(3, compute_dtype=torch.bfloat16)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    net.eval()
    x = synth_bag(4, 64, 64, 20261020)
    u8 = mil_amd.U8Tiles(((x * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).cuda())
    grad = mil_amd.TileSaliency(net).input_gradient(u8, 1)
    assert grad.shape == (4, 3, 64, 64) and grad.dtype == torch.float32
    g = grad.cpu().numpy()
    assert np.isfinite(g).all() and g.min() < 0 < g.max()
    for normalize in GROUPS:
        r = mil_amd.AttributionRenderer(normalize=normalize)
        gray = r.grayscale(grad)
        assert np.array_equal(gray.cpu().numpy(), ref.grayscale_bytes(g, 99.0, normalize))
        assert int(gray.max()) == 255
        _check_stats(r.stats(grad), ref.values_of(g, normalize), 99.0)
        assert np.array_equal(r.colour(grad).cpu().numpy(), ref.colour_bytes(g, normalize))
        pos, neg = r.pos_neg(grad)
        want_pos, want_neg = ref.pos_neg_bytes(g, normalize)
        assert np.array_equal(pos.cpu().numpy(), want_pos) and np.array_equal(neg.cpu().numpy(), want_neg)
        heat, on = r.overlay(u8, gray)
        want_heat, want_on = ref.overlay_bytes(u8.u8.cpu().numpy(), gray.cpu().numpy(), r.table.numpy(), 102)
        assert np.array_equal(heat.cpu().numpy(), want_heat) and np.array_equal(on.cpu().numpy(), want_on)
    # a map: the saliency map of the same bag
    sal = mil_amd.TileSaliency(net).maps(u8, 1)
    assert sal.shape == (4, 64, 64)
    assert np.array_equal(mil_amd.AttributionRenderer().grayscale(sal).cpu().numpy(), ref.grayscale_bytes(sal.cpu().numpy()))
