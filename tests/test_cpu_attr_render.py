"""CPU (-m "not gpu"): the contract of the attribution renderer without a GPU — the numpy restatement
(tests/attr_render_reference.py) against np.percentile on fp64, against Pillow's and matplotlib's recorded tables and against
the bytes the toolkit's literal expressions gave (tests/golden/attr_render.npz, written by make_attr_render_golden.py); the
degenerate rules; the status codes of `mil_map_quantile`, `mil_attr_render` and `mil_cam_overlay` (decided before any GPU
call); the argument errors of the wrappers and of `AttributionRenderer`; the colour tables the package carries."""
import ctypes
import os

import numpy as np
import pytest
import torch

import attr_render_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
QS = (99.0, 50.0, 100.0, 0.5)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "attr_render.npz"))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_restatement_equals_numpy_percentile_on_fp64_bit_for_bit():
    rng = np.random.default_rng(341)
    sizes = [1, 2, 3, 7, 100, 101, 33 * 37, 50 * 70, 64 * 64]
    for trial in range(200):
        n = sizes[trial % len(sizes)]
        v = (rng.standard_normal(n) ** 3 * 10.0 ** rng.integers(-8, 4)).astype(np.float32)
        if trial % 5 == 1:
            v = np.round(v * 4)
        if trial % 5 == 2:
            v[rng.random(n) < 0.5] = 0.0
        v = v + np.float32(0.0)                       # -0.0 counts as +0.0 (np.round makes some)
        for q in QS:
            stats, p = ref.quantile_stats(v[None], q)
            want = np.percentile(v.astype(np.float64), q)
            assert _bits(p)[0] == _bits(np.float64(want)), (n, q, float(p[0]), float(want))
            lo, hi, t = ref.ranks(n, q)
            s = np.sort(v)
            assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1 and 0.0 <= t < 1.0
            assert stats[0].tolist() == [s[0], s[-1], s[lo], s[hi]]
    # q = 100 is the maximum itself, and an fp32 maximum survives the fp64 round trip
    stats, p = ref.quantile_stats(np.array([[3.0, -1.0, 2.5]], np.float32), 100.0)
    assert stats[0].tolist() == [-1.0, 3.0, 3.0, 3.0] and p[0] == 3.0
    # zeros of either sign are one value, returned as +0.0
    stats, p = ref.quantile_stats(np.array([[-0.0, -0.0, 0.0, -0.0]], np.float32), 50.0)
    assert not np.signbit(stats).any() and not np.signbit(p).any()


def test_virtual_index_within_one_ulp_of_an_integer():
    """n = 100 and 101 at q = 99: 99 * 0.99 and 100 * 0.99 in fp64.  Whatever side of the integer the product falls on, the
    restatement is numpy's (the test above); here: the two shapes the GPU suite uses do sit on such a boundary."""
    for n in (100, 101):
        lo, hi, t = ref.ranks(n, 99.0)
        exact = (n - 1) * 99 / 100
        assert abs((lo + float(t)) - exact) <= 2 * np.spacing(exact)
        print(f"n = {n}: lo {lo} hi {hi} t {float(t)!r}")
    assert ref.ranks(101, 99.0)[0] in (98, 99)


def test_composite_and_colour_tables_equal_pillow_and_matplotlib(golden):
    src = np.arange(256, dtype=np.uint8)[:, None].repeat(256, 1)
    dst = np.arange(256, dtype=np.uint8)[None, :].repeat(256, 0)
    alphas = golden["comp_alphas"].tolist()
    assert 102 in alphas and len(alphas) >= 3
    for a, table in zip(alphas, golden["comp_tables"]):
        assert np.array_equal(ref.composite(src, dst, a), table), a
    assert np.array_equal(ref.composite(src, dst, 0), dst) and np.array_equal(ref.composite(src, dst, 255), src)
    assert golden["lut_hsv"][:3].tolist() == [[255, 0, 0], [255, 5, 0], [255, 11, 0]]
    heat, on = ref.overlay_bytes(golden["ov_tile"][None], golden["ov_map"][None], golden["lut_hsv"], int(0.4 * 255))
    assert np.array_equal(heat[0], golden["ov_heat"]) and np.array_equal(on[0], golden["ov_on"])


def test_the_package_carries_matplotlibs_tables(golden):
    import mil_amd
    from mil_amd import attr_render
    assert attr_render.CMAPS == ("hsv", "jet", "viridis")
    for name in attr_render.CMAPS:
        assert np.array_equal(attr_render.colour_table(name).numpy(), golden["lut_" + name]), name
    r = mil_amd.AttributionRenderer()
    assert (r.percentile, r.normalize, r.alpha_byte) == (99.0, "tile", 102)
    assert np.array_equal(r.table.numpy(), golden["lut_hsv"])
    own = torch.arange(768, dtype=torch.int32).remainder(251).to(torch.uint8).view(256, 3)
    assert torch.equal(mil_amd.AttributionRenderer(cmap=own).table, own)
    # the package does not import matplotlib
    lines = [ln.strip() for ln in open(attr_render.__file__).read().splitlines()]
    assert not [ln for ln in lines if ln.startswith(("import matplotlib", "from matplotlib"))]


def _regular(golden):
    """Indices of the recorded gradients on which every literal expression of the toolkit is defined: both signs present and
    not constant (elsewhere it divides by zero or by a number of the wrong sign)."""
    g = golden["grads"]
    return [i for i in range(len(g)) if g[i].min() < 0 < g[i].max()]


def test_bytes_against_the_toolkits_literal_expressions(golden):
    g = golden["grads"]
    reg = _regular(golden)
    assert len(reg) >= 12
    mixed = [i for i in range(len(g)) if g[i].min() != g[i].max()]
    # grayscale: the toolkit's literal line runs np.percentile on fp32 (a version-dependent fp32 lerp); the contract takes the
    # percentile of the same values in fp64.  At most one level apart, on at most 1e-3 of the bytes.
    mine = ref.grayscale_bytes(g[mixed]).astype(np.int32)
    lit = golden["gray_bytes"][mixed].astype(np.int32)
    diff = np.abs(mine - lit)
    print(f"grayscale against the literal toolkit line: {int((diff != 0).sum())} of {diff.size} bytes differ, max {int(diff.max())}")
    assert diff.max() <= 1 and (diff != 0).sum() <= 1e-3 * diff.size
    # colour: the toolkit's own fp32 arithmetic
    assert np.array_equal(ref.colour_bytes(g[mixed]), golden["colour_bytes"][mixed])
    # positive / negative: pos = max(0, g) / max lies in [0, 1] with 0 (an element <= 0) and 1 (max / max) both attained, so the
    # second normalisation of save_gradient_images subtracts 0 and divides by 1: an identity.  The same for the negative part.
    pos, neg = ref.pos_neg_bytes(g[reg])
    assert np.array_equal(pos, golden["pos_bytes"][reg]) and np.array_equal(neg, golden["neg_bytes"][reg])
    for i in reg:
        for part in (np.maximum(np.float32(0), g[i]) / g[i].max(), np.maximum(np.float32(0), -g[i]) / -g[i].min()):
            assert part.min() == 0 and part.max() == 1
            again = part - part.min()
            again /= again.max()
            assert np.array_equal(again, part)


def test_degenerate_rules(golden):
    const = np.full((1, 3, 5, 7), 0.25, np.float32)
    assert not ref.grayscale_bytes(const).any() and not ref.colour_bytes(const).any()
    assert not ref.grayscale_bytes(const[:, 0]).any()
    pos, neg = ref.pos_neg_bytes(const)
    assert int(pos.min()) == 255 and not neg.any()                      # g / max = 1 everywhere; no negative value
    pos, neg = ref.pos_neg_bytes(-const)
    assert not pos.any() and int(neg.min()) == 255
    pos, neg = ref.pos_neg_bytes(np.zeros_like(const))
    assert not pos.any() and not neg.any()
    # p == min without a constant tile: 99 % of the values are the minimum
    x = np.zeros((1, 20, 20), np.float32)
    x[0, 0, :3] = 1.0
    stats, p = ref.quantile_stats(ref.values_of(x), 99.0)
    assert p[0] == 0.0 == stats[0, 0] and stats[0, 1] == 1.0 and not ref.grayscale_bytes(x).any()
    # the bag's range is one range: a bright tile dims the others
    two = np.stack([np.linspace(0, 1, 64, dtype=np.float32).reshape(8, 8), np.linspace(0, 4, 64, dtype=np.float32).reshape(8, 8)])
    assert ref.grayscale_bytes(two, 100.0, "tile")[0].max() == 255 and ref.grayscale_bytes(two, 100.0, "bag")[0].max() == 63
    # the recorded one-signed gradients: the part that does not exist is zeros
    g = golden["grads"]
    for i in range(len(g)):
        pos, neg = ref.pos_neg_bytes(g[i:i + 1])
        if g[i].max() <= 0:
            assert not pos.any()
        if g[i].min() >= 0:
            assert not neg.any()


def test_status_codes_are_decided_before_any_gpu_call():
    import mil_amd
    from mil_amd import _lib as L
    lib = mil_amd.lib()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)
    header = open(os.path.join(os.path.dirname(HERE), "include", "mil_hip.h")).read()
    for name in ("mil_map_quantile_workspace", "mil_map_quantile", "mil_attr_render", "mil_cam_overlay"):
        assert name in L.EXPORTS and hasattr(lib, name) and ("int " + name + "(") in header
    assert lib.mil_abi_version() == 2
    need = ctypes.c_size_t(0)
    assert lib.mil_map_quantile_workspace(ctypes.byref(need), 3, 0) == 0 and need.value == 3 * 4104 * 4
    assert lib.mil_map_quantile_workspace(ctypes.byref(need), 3, 1) == 0 and need.value == 16 * 4104 * 4
    assert "#define MIL_QUANTILE_WS_WORDS 4104" in header and "#define MIL_QUANTILE_BAG_TABLES 16" in header
    assert lib.mil_map_quantile_workspace(None, 3, 0) == 1 and lib.mil_map_quantile_workspace(ctypes.byref(need), 0, 0) == 1
    assert lib.mil_map_quantile_workspace(ctypes.byref(need), 3, 2) == 1
    # mil_map_quantile(x, n, channels, H, W, q, bag, workspace, workspace_bytes, stats, p, stream)
    mq = lib.mil_map_quantile
    big = 1 << 40
    assert mq(None, 1, 3, 8, 8, 99.0, 0, p, big, p, p, None) == 1
    assert mq(p, 1, 3, 8, 8, 99.0, 0, None, big, p, p, None) == 1
    assert mq(p, 1, 3, 8, 8, 99.0, 0, p, big, None, p, None) == 1
    assert mq(p, 1, 3, 8, 8, 99.0, 0, p, big, p, None, None) == 1
    assert mq(p, 0, 3, 8, 8, 99.0, 0, p, big, p, p, None) == 1                     # an empty bag has no statistics
    assert mq(p, 0, 3, 8, 8, 99.0, 1, p, big, p, p, None) == 1
    assert mq(p, -1, 3, 8, 8, 99.0, 0, p, big, p, p, None) == 1
    assert mq(p, 1, 3, 0, 8, 99.0, 0, p, big, p, p, None) == 1
    assert mq(p, 1, 3, 8, -1, 99.0, 0, p, big, p, p, None) == 1
    for ch in (0, 2, 4):
        assert mq(p, 1, ch, 8, 8, 99.0, 0, p, big, p, p, None) == 1
    for bag in (-1, 2):
        assert mq(p, 1, 3, 8, 8, 99.0, bag, p, big, p, p, None) == 1
    for q in (0.0, -1.0, 100.5, float("nan"), float("inf")):
        assert mq(p, 1, 3, 8, 8, q, 0, p, big, p, p, None) == 1
    assert mq(p, 2, 3, 8, 8, 99.0, 0, p, 2 * 4104 * 4 - 1, p, p, None) == 1       # a workspace one byte short
    assert mq(p, 2, 3, 8, 8, 99.0, 1, p, 16 * 4104 * 4 - 1, p, p, None) == 1
    assert mq(p, 1, 1, 1 << 16, 1 << 16, 99.0, 0, p, big, p, p, None) == 2
    assert mq(p, 1, 1, 1 << 15, (1 << 15) + 1, 99.0, 0, p, big, p, p, None) == 2   # a tile of more than 2^30 values
    assert mq(p, 2, 1, 1 << 15, 1 << 15, 99.0, 1, p, big, p, p, None) == 2         # a bag of 2^31 values
    # mil_attr_render(x, n, channels, H, W, mode, bag, stats, p, out0, out1, stream)
    ar = lib.mil_attr_render
    assert ar(None, 1, 3, 8, 8, 0, 0, p, p, p, None, None) == 1
    assert ar(p, 1, 3, 8, 8, 0, 0, None, p, p, None, None) == 1
    assert ar(p, 1, 3, 8, 8, 0, 0, p, p, None, None, None) == 1
    assert ar(p, 1, 3, 8, 8, 0, 0, p, None, p, None, None) == 1                    # grayscale reads the percentile
    assert ar(p, 1, 3, 8, 8, 2, 0, p, p, p, None, None) == 1                       # positive / negative writes two images
    assert ar(p, 1, 2, 8, 8, 0, 0, p, p, p, None, None) == 1
    for mode in (1, 2):
        assert ar(p, 1, 1, 8, 8, mode, 0, p, p, p, p, None) == 1                   # colour needs the three channels
    for mode in (-1, 3):
        assert ar(p, 1, 3, 8, 8, mode, 0, p, p, p, p, None) == 1
    assert ar(p, 1, 3, 8, 8, 0, 2, p, p, p, None, None) == 1
    assert ar(p, -1, 3, 8, 8, 0, 0, p, p, p, None, None) == 1
    assert ar(p, 1, 3, 0, 8, 0, 0, p, p, p, None, None) == 1
    assert ar(p, 1, 3, 8, 0, 0, 0, p, p, p, None, None) == 1
    assert ar(p, 1, 3, 1 << 16, 1 << 16, 0, 0, p, p, p, None, None) == 2
    for mode, ch in ((0, 3), (0, 1), (1, 3), (2, 3)):
        assert ar(p, 0, ch, 8, 8, mode, 0, p, p, p, p, None) == 0                  # nothing to do: no launch
    # mil_cam_overlay(tiles, map, lut, alpha, n, H, W, heat, on_image, stream)
    co = lib.mil_cam_overlay
    assert co(None, p, p, 102, 1, 8, 8, p, p, None) == 1
    assert co(p, None, p, 102, 1, 8, 8, p, p, None) == 1
    assert co(p, p, None, 102, 1, 8, 8, p, p, None) == 1
    assert co(p, p, p, 102, 1, 8, 8, None, None, None) == 1
    for a in (-1, 256):
        assert co(p, p, p, a, 1, 8, 8, p, p, None) == 1
    assert co(p, p, p, 102, -1, 8, 8, p, p, None) == 1
    assert co(p, p, p, 102, 1, 0, 8, p, p, None) == 1
    assert co(p, p, p, 102, 1, 8, 0, p, p, None) == 1
    assert co(p, p, p, 102, 1, 1 << 16, 1 << 16, p, p, None) == 2
    assert co(p, p, p, 102, 0, 8, 8, p, None, None) == 0 and co(p, p, p, 0, 0, 8, 8, None, p, None) == 0


def test_argument_errors_come_before_any_launch():
    import mil_amd
    from mil_amd import ops
    assert "AttributionRenderer" in mil_amd.__all__
    R = mil_amd.AttributionRenderer
    for bad in (0, -1, 100.5, float("nan")):
        with pytest.raises(ValueError, match="percentile"):
            R(percentile=bad)
    with pytest.raises(ValueError, match="normalize"):
        R(normalize="slide")
    with pytest.raises(ValueError, match="cmap"):
        R(cmap="magma")
    with pytest.raises(ValueError, match="cmap"):
        R(cmap=torch.zeros(256, 3))
    with pytest.raises(ValueError, match="cmap"):
        R(cmap=torch.zeros(255, 3, dtype=torch.uint8))
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            R(alpha=bad)
    assert R(alpha=0.0).alpha_byte == 0 and R(alpha=1.0).alpha_byte == 255 and R(alpha=0.5).alpha_byte == 127
    r = R()
    g, m = torch.zeros(2, 3, 8, 8), torch.zeros(2, 8, 8)
    for call in (r.stats, r.grayscale):
        with pytest.raises(ValueError, match="fp32"):
            call(g.double())
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(2, 4, 8, 8))
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(8, 8))
        with pytest.raises(ValueError, match="empty"):
            call(torch.zeros(0, 3, 8, 8))
        with pytest.raises(ValueError, match="CUDA"):                              # valid arguments on the CPU: no kernel for them
            call(g)
        with pytest.raises(ValueError, match="CUDA"):
            call(m)
    for call in (r.colour, r.pos_neg):
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(m)
        with pytest.raises(ValueError, match="empty"):
            call(torch.zeros(0, 3, 8, 8))
        with pytest.raises(ValueError, match="fp32"):
            call(g.half())
        with pytest.raises(ValueError, match="CUDA"):
            call(g)
    tiles = mil_amd.U8Tiles(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))
    mu8 = torch.zeros(2, 8, 8, dtype=torch.uint8)
    with pytest.raises(ValueError, match="U8Tiles"):
        r.overlay(g, mu8)
    with pytest.raises(ValueError, match="map_u8"):
        r.overlay(tiles, m)
    with pytest.raises(ValueError, match="map_u8"):
        r.overlay(tiles, mu8[:1])
    with pytest.raises(ValueError, match="map_u8"):
        r.overlay(tiles, torch.zeros(2, 8, 9, dtype=torch.uint8))
    with pytest.raises(ValueError, match="empty"):
        r.overlay(mil_amd.U8Tiles(torch.zeros(0, 3, 8, 8, dtype=torch.uint8)), torch.zeros(0, 8, 8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="CUDA"):
        r.overlay(tiles, mu8)
    # the wrappers
    with pytest.raises(ValueError, match="q must"):
        ops.map_quantile(g, 0.0)
    with pytest.raises(ValueError, match="group"):
        ops.map_quantile(g, 99.0, "slide")
    with pytest.raises(ValueError, match="mode"):
        ops.attr_render(g, None, "gray")
    with pytest.raises(ValueError, match="stats"):
        ops.attr_render(g, None, "grayscale")
    st = ops.MapStats(torch.zeros(1, 4), torch.zeros(1, dtype=torch.float64), "tile")
    with pytest.raises(ValueError, match="stats"):                                 # one group for two tiles
        ops.attr_render(g, st, "grayscale")
    with pytest.raises(ValueError, match="lut"):
        ops.cam_overlay(tiles, mu8, torch.zeros(256, 3), 102)
    with pytest.raises(ValueError, match="alpha_byte"):
        ops.cam_overlay(tiles, mu8, r.table, 256)
    with pytest.raises(ValueError, match="alpha_byte"):
        ops.cam_overlay(tiles, mu8, r.table, 101.5)
