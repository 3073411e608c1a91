"""-m gpu: the small kernels around the convolutions (`csrc/pointwise.hip`, `csrc/optim.hip`) against the fp64 references of
tests/pointwise_reference.py, element by element inside the derived bounds of that file (`err <= bound`, nothing max-normalised,
no tolerance taken from a kernel's output), at the channel counts, slopes and launch sizes both encoders run them at and at the
edges of their tiling: one-pixel maps, maps one pixel either side of the LDS staging chunk, the 512-thread launch, C < CP, row
counts around the 64-row slices of the weight gradient, a parameter count that wraps Adam's grid-stride loop.  The winner records
of the max-pool (tap in bits 0-3, "winner <= 0" in bit 4, which three backward kernels consume) are compared bit by bit.

Output buffers the tests allocate themselves start as NaN and must be finite afterwards.  tests/test_cpu_pointwise_bounds.py shows
on the same inputs that correct fp32 arithmetic stays inside these bounds and that six typical defects do not."""
import ctypes

import numpy as np
import pytest
import torch

import pointwise_reference as R

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _lib():
    from mil_amd import _lib as L
    return L


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def host(t):
    return t.detach().float().cpu().numpy()


def nans(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


def inside(got, ref, bound, what):
    """Asserts err <= bound for every element and returns the largest err / bound (0 where the error is 0)."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape == np.shape(bound), (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    worst = float(r.max(initial=0.0))
    i = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    assert bool((err <= bound).all()), f"{what}: err / bound = {worst:.3g} at {i}: got {got[i]!r}, want {ref[i]!r} +- {bound[i]:.3g}"
    return worst


def report(case, **ratios):
    print(f"\n{case}: largest err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ---- max-pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slope", R.MAXPOOL_SLOPES)
@pytest.mark.parametrize("kind", R.MAXPOOL_KINDS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", R.MAXPOOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_maxpool_records_and_gradient(ops, shape, dtype, kind, slope):
    n, c, h, w = shape
    bf16 = dtype == torch.bfloat16
    x, gy = R.maxpool_inputs(shape, kind, bf16)
    y_ref, tap, neg = R.maxpool(x)
    y, widx_g = ops.maxpool_fwd(dev(x, dtype))
    y, widx = host(y), widx_g.cpu().numpy()
    assert y.shape == y_ref.shape and widx.dtype == np.uint8 and widx.shape == tap.shape
    assert np.array_equal(y.astype(np.float64), y_ref)                               # bit-equal (a maximum is one of its inputs)
    assert np.array_equal(widx & 15, tap)                                            # first maximum in (ky, kx) scan order
    assert np.array_equal(((widx >> 4) & 1)[..., :c].astype(bool), neg[..., :c])     # winner <= 0
    assert not (widx >> 5).any()
    assert not y[..., c:].any()
    ratios = {}
    for use_mask in (True, False):
        gx_ref, bound = R.maxpool_bwd(gy, tap, neg, slope, use_mask, (h, w), bf16)
        gx = host(ops.maxpool_bwd(dev(gy, dtype), widx_g, (h, w), lrelu_mask=use_mask, slope=slope))
        ratios["gx" if use_mask else "gx_nomask"] = inside(gx, gx_ref, bound, f"gx use_mask={use_mask}")
        assert not gx[..., c:].any()
    report(f"maxpool {shape} {kind} slope {slope} {'bf16' if bf16 else 'fp32'}", **ratios)


# ---- pool + fc -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", R.POOLFC_CASES, ids=lambda s: "-".join(map(str, s)))
def test_avgpool_fc_forward_and_data_gradient(ops, case, dtype):
    n, h, w, c, cp, nf, has_bias = case
    bf16, slope = dtype == torch.bfloat16, R.poolfc_slope(case)
    x, wfc, bias, df = R.poolfc_inputs(case, bf16)
    xg, wg, dfg = dev(x, dtype), dev(wfc), dev(df)
    bg = dev(bias) if has_bias else None
    pooled_ref, pooled_bound, feats_ref, feats_bound = R.avgpool_fc_fwd(x, wfc, bias, c)
    pooled, feats = ops.avgpool_fc_fwd(xg, wg, c, bias=bg)
    ratios = dict(pooled=inside(host(pooled), pooled_ref, pooled_bound, "pooled"),
                  feats=inside(host(feats), feats_ref, feats_bound, "feats"))
    pooled2, feats2 = ops.avgpool_fc_fwd(xg, wg, c, bias=bg)
    assert torch.equal(pooled, pooled2) and torch.equal(feats, feats2)
    for masked in (True, False):
        dz_ref, bound = R.avgpool_fc_bwd(df, wfc, x, c, slope, masked, bf16)
        outs = [ops.avgpool_fc_bwd_data(dfg, wg, pooled, xg, masked=masked, slope=slope) for _ in range(2)]
        if masked:
            outs.append(ops.avgpool_fc_bwd(dfg, wg, pooled, xg, c, slope=slope)[0])
        assert all(torch.equal(outs[0], o) for o in outs[1:])                        # a second launch, and both entry points
        dz = host(outs[0])
        ratios["dz" if masked else "dz_nomask"] = inside(dz, dz_ref, bound, f"dz masked={masked}")
        assert dz.shape == x.shape and not dz[..., c:].any()
    report(f"pool+fc {case} {'bf16' if bf16 else 'fp32'}", **ratios)


# ---- fc weight gradient ----------------------------------------------------------------------------------------------------------
def _two_stage(dfg, pooled, dw, db, accumulate):
    """mil_fc_wgrad on test-owned outputs, as ops.avgpool_fc_bwd calls it."""
    L = _lib()
    n, nf = dfg.shape
    c = pooled.shape[1]
    need = ctypes.c_size_t(0)
    L.check(L.lib().mil_fc_wgrad_workspace(ctypes.byref(need), n, c, nf), "mil_fc_wgrad_workspace")
    ws = nans(((need.value + 3) // 4,))
    L.check(L.lib().mil_fc_wgrad(dfg.data_ptr(), pooled.data_ptr(), dw.data_ptr(), L.ptr(db), ws.data_ptr(), ws.numel() * 4,
                                 n, c, nf, 1 if accumulate else 0, L.stream_ptr()), "mil_fc_wgrad")


def _one_wave(dfg, wg, pooled, act, dw, db, accumulate):
    """The ABI path include/mil_hip.h documents: mil_avgpool_fc_bwd with a non-null dwfc (one wave per output element)."""
    L = _lib()
    n, nf = dfg.shape
    c = pooled.shape[1]
    dz = nans(act.shape)
    L.check(L.lib().mil_avgpool_fc_bwd(dfg.data_ptr(), wg.data_ptr(), pooled.data_ptr(), act.data_ptr(), dz.data_ptr(),
                                       dw.data_ptr(), L.ptr(db), n, 1, c, c, nf, 1 if accumulate else 0, 0.1,
                                       L.dt_code(torch.float32), L.stream_ptr()), "mil_avgpool_fc_bwd")
    assert bool(torch.isfinite(dz).all())


def _fcw_check(ops, c, nf, n, with_bias, accumulate):
    df, pooled_in, prev_w, prev_b = R.fcw_inputs(c, nf, n)
    dfg, wg = dev(df), dev(prev_w)
    act = dev(pooled_in.reshape(n, 1, 1, c))
    pooled, _ = ops.avgpool_fc_fwd(act, wg, c)                   # the kernel's own pooled (a one-pixel map: the map itself)
    assert np.array_equal(host(pooled), pooled_in)
    dw_ref, dw_bound, db_ref, db_bound = R.fc_wgrad(df, host(pooled), prev_w if accumulate else None,
                                                    prev_b if accumulate else None)
    got, ratios = {}, {}
    for name in ("two_stage", "one_wave"):
        dw = dev(prev_w) if accumulate else nans((nf, c))
        db = (dev(prev_b) if accumulate else nans((nf,))) if with_bias else None
        if name == "two_stage":
            _two_stage(dfg, pooled, dw, db, accumulate)
        else:
            _one_wave(dfg, wg, pooled, act, dw, db, accumulate)
        ratios[name + " dw"] = inside(host(dw), dw_ref, dw_bound, name + " dW")
        if with_bias:
            ratios[name + " db"] = inside(host(db), db_ref, db_bound, name + " dbias")
        got[name] = (host(dw), host(db) if with_bias else None)
    # both are inside the bound around the same reference, so they agree inside twice the bound
    assert bool((np.abs(got["two_stage"][0].astype(np.float64) - got["one_wave"][0]) <= 2 * dw_bound).all())
    if with_bias:
        assert bool((np.abs(got["two_stage"][1].astype(np.float64) - got["one_wave"][1]) <= 2 * db_bound).all())
    report(f"fc_wgrad C {c} NF {nf} n {n} bias {with_bias} accumulate {accumulate}", **ratios)


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("n", R.FCW_N)
@pytest.mark.parametrize("shape", R.FCW_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_fc_wgrad(ops, shape, n, with_bias, accumulate):
    _fcw_check(ops, shape[0], shape[1], n, with_bias, accumulate)


@pytest.mark.parametrize("accumulate", [False, True], ids=["fresh", "accumulate"])
def test_fc_wgrad_largest_nf_at_512_channels(ops, accumulate):
    """64 rows of [dfeats | pooled | 1] fill the 160 KiB of LDS exactly at NF = 127."""
    _fcw_check(ops, 512, R.FCW_MAX_NF_AT_512, 65, True, accumulate)


def test_fc_wgrad_refuses_the_next_nf_without_a_launch():
    L = _lib()
    c, nf, n = 512, R.FCW_MAX_NF_AT_512 + 1, 65
    dfg, pooled = dev(np.ones((n, nf), np.float32)), dev(np.ones((n, c), np.float32))
    dw, db = nans((nf, c)), nans((nf,))
    with pytest.raises(L.MilLibraryError, match="unsupported"):
        _two_stage(dfg, pooled, dw, db, False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all()) and bool(torch.isnan(db).all())


def test_avgpool_fc_bwd_wrapper_refuses_half_an_accumulation_target(ops):
    """want_bias with only one of out / out_bias used to add the bias gradient to uninitialised memory."""
    n, c, nf = 2, 64, 10
    args = (dev(np.ones((n, nf), np.float32)), dev(np.ones((nf, c), np.float32)), dev(np.ones((n, c), np.float32)),
            dev(np.ones((n, 1, 1, c), np.float32)), c)
    with pytest.raises(ValueError, match="both out and out_bias"):
        ops.avgpool_fc_bwd(*args, slope=0.0, out=nans((nf, c)), want_bias=True)
    with pytest.raises(ValueError, match="both out and out_bias"):
        ops.avgpool_fc_bwd(*args, slope=0.0, out_bias=nans((nf,)), want_bias=True)
    # both given: both accumulate; neither: both fresh
    dw0, db0 = dev(np.full((nf, c), 2.0, np.float32)), dev(np.full(nf, 3.0, np.float32))
    _, dw, db = ops.avgpool_fc_bwd(*args, slope=0.0, out=dw0, want_bias=True, out_bias=db0)
    assert dw is dw0 and db is db0 and bool((dw == 2.0 + n).all()) and bool((db == 3.0 + n).all())
    _, dw, db = ops.avgpool_fc_bwd(*args, slope=0.0, want_bias=True)
    assert bool((dw == float(n)).all()) and bool((db == float(n)).all())


# ---- Adam ------------------------------------------------------------------------------------------------------------------------
_ADAM_INPUTS = {}


def _adam_inputs(n):
    if n not in _ADAM_INPUTS:
        _ADAM_INPUTS[n] = R.adam_inputs(n)
    return _ADAM_INPUTS[n]


@pytest.mark.parametrize("step", R.ADAM_STEPS)
@pytest.mark.parametrize("wd_scale", R.ADAM_WD_SCALE, ids=lambda s: f"wd{s[0]:g}-scale{s[1]:.3g}")
@pytest.mark.parametrize("n", R.ADAM_N)
def test_adam_step(n, wd_scale, step):
    """One step from a given state, called as FlatAdam.step calls it."""
    L = _lib()
    wd, scale = wd_scale
    p, g, m, v = _adam_inputs(n)
    hyper = dict(R.ADAM_HYPER, weight_decay=wd, grad_scale=scale, step=step)
    ref = R.adam_step(p, g, m, v, **hyper)
    pg, gg, mg, vg = dev(p), dev(g), dev(m), dev(v)
    L.check(L.lib().mil_adam_step(pg.data_ptr(), gg.data_ptr(), mg.data_ptr(), vg.data_ptr(), n, hyper["lr"], hyper["beta1"],
                                  hyper["beta2"], hyper["eps"], wd, step, scale, L.stream_ptr()), "mil_adam_step")
    got = dict(m=host(mg), v=host(vg), p=host(pg))
    assert np.array_equal(host(gg), g)
    ratios = {k: inside(got[k], ref[k], ref[k + "_bound"], f"new {k}") for k in "mvp"}
    if n >= 255:
        assert got["p"][R.ADAM_SPECIAL["all0"]] == 0.0                                # nothing to update from: exactly 0
        if wd == 0.0:
            assert got["p"][R.ADAM_SPECIAL["gmv0"]] == p[R.ADAM_SPECIAL["gmv0"]]
    report(f"adam n {n} wd {wd} scale {scale:.3g} step {step}", **ratios)
