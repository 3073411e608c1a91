"""The bounds of tests/pointwise_reference.py, checked in both directions without a GPU, on the inputs of every case of
tests/test_gpu_pointwise.py:

  * a plain fp32 numpy restatement of each operation (sums in pixel / row order, one rounding per operation, fp32 `pow`) stays
    inside its bound — if it needed more than the factor 2 the derivation would be wrong;
  * six deliberately wrong restatements each leave the bound on at least one of those cases — so a kernel with that defect
    fails the GPU test.

The largest err / bound per operation is printed (`pytest -s`); DESIGN.md section 3.37 records them."""
import numpy as np
import pytest

import pointwise_reference as R

f32 = np.float32


def ratio(got, ref, bound):
    """max err / bound, element by element: 0 where the error is 0, inf where an error meets a zero bound."""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    assert not np.isnan(r).any()
    return float(r.max())


# ---- fp32 restatements (wrong=...: the deliberately wrong ones) -------------------------------------------------------------------
def maxpool32(x, wrong=None):
    n, h, w, c = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = np.empty((n, ho, wo, c), f32)
    tap = np.empty((n, ho, wo, c), np.uint8)
    for oy in range(ho):
        for ox in range(wo):
            best, bi = np.full((n, c), -np.inf, f32), np.zeros((n, c), np.uint8)
            for ky in range(3):
                for kx in range(3):
                    iy, ix = 2 * oy - 1 + ky, 2 * ox - 1 + kx
                    if not (0 <= iy < h and 0 <= ix < w):
                        continue
                    v = x[:, iy, ix, :]
                    take = (v >= best) if wrong == "last_max" else (v > best)
                    best, bi = np.where(take, v, best), np.where(take, np.uint8(ky * 3 + kx), bi)
            y[:, oy, ox], tap[:, oy, ox] = best, bi
    return y, tap, (y < 0) if wrong == "strict_neg" else (y <= 0)


def maxpool_bwd32(gy, tap, neg, slope, use_mask, in_hw, bf16):
    n, ho, wo, c = gy.shape
    h, w = in_hw
    gx = np.zeros((n, h, w, c), f32)
    f = np.where(neg, f32(slope), f32(1)) if use_mask else np.ones(gy.shape, f32)
    for oy in range(ho):
        for ox in range(wo):
            for k in range(9):
                iy, ix = 2 * oy - 1 + k // 3, 2 * ox - 1 + k % 3
                if 0 <= iy < h and 0 <= ix < w:
                    sel = tap[:, oy, ox] == k
                    gx[:, iy, ix] += np.where(sel, gy[:, oy, ox] * f[:, oy, ox], f32(0))
    assert gx.dtype == f32
    return R.to_bf16(gx) if bf16 else gx


def poolfc_fwd32(x, wfc, bias, c, wrong=None):
    n, cp = x.shape[0], x.shape[-1]
    x = x.reshape(n, -1, cp)
    hw, pch = x.shape[1], 4096 // cp
    s = np.zeros((n, c), f32)
    for i in range(hw):
        if wrong == "drop_chunk_last" and i % pch == pch - 1:
            continue
        s += x[:, i, :c]
    pooled = s / f32(hw)
    acc = np.zeros((n, wfc.shape[0]), f32) if bias is None else np.tile(bias, (n, 1))
    for i in range(c):
        acc += pooled[:, i:i + 1] * wfc[None, :, i]
    assert pooled.dtype == f32 and acc.dtype == f32
    return pooled, acc


def poolfc_bwd32(df, wfc, act, c, slope, masked, bf16):
    n, cp = act.shape[0], act.shape[-1]
    hw = int(np.prod(act.shape[1:-1]))
    g = np.zeros((n, c), f32)
    for o in range(wfc.shape[0]):
        g += df[:, o:o + 1] * wfc[o][None, :]
    g /= f32(hw)
    g = g.reshape((n,) + (1,) * (act.ndim - 2) + (c,))
    dz = np.zeros(act.shape, f32)
    dz[..., :c] = g * (np.where(act[..., :c] > 0, f32(1), f32(slope)) if masked else f32(1))
    return R.to_bf16(dz) if bf16 else dz


def fcw32(df, pooled, prev_w=None, prev_b=None, wrong=None):
    n, nf = df.shape
    dw, db = np.zeros((nf, pooled.shape[1]), f32), np.zeros(nf, f32)
    for t in range(n):
        if wrong == "drop_row_63" and t % 64 == 63:
            continue
        dw += df[t][:, None] * pooled[t][None, :]
        db += df[t]
    if prev_w is not None:
        dw = prev_w + dw
    if prev_b is not None:
        db = prev_b + db
    assert dw.dtype == f32 and db.dtype == f32
    return dw, db


def adam32(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale, wrong=None):
    lr, b1, b2, eps, wd, s = (f32(a) for a in (lr, beta1, beta2, eps, weight_decay, grad_scale))
    gi = (g + wd * p) * s if wrong == "scale_after_decay" else g * s + wd * p
    m2 = b1 * m + (f32(1) - b1) * gi
    v2 = b2 * v + (f32(1) - b2) * gi * gi
    bc1 = f32(1) - np.power(b1, f32(step))
    bc2 = f32(1) - np.power(b2, f32(step))
    denom = np.sqrt(v2) / (bc2 if wrong == "bc2_not_sqrt" else np.sqrt(bc2)) + eps
    p2 = p - (lr / bc1) * (m2 / denom)
    assert all(a.dtype == f32 for a in (m2, v2, p2)) and isinstance(bc1, f32) and isinstance(bc2, f32)
    return m2, v2, p2


# ---- the checks ------------------------------------------------------------------------------------------------------------------
def _maxpool_cases():
    for shape in R.MAXPOOL_SHAPES:
        for kind in R.MAXPOOL_KINDS:
            for bf16 in (False, True):
                yield shape, kind, bf16


def _maxpool_bwd_ratio(gy, tap, neg, ref_tap, ref_neg, in_hw, bf16):
    worst = 0.0
    for slope in R.MAXPOOL_SLOPES:
        for use_mask in (True, False):
            want, bound = R.maxpool_bwd(gy, ref_tap, ref_neg, slope, use_mask, in_hw, bf16)
            worst = max(worst, ratio(maxpool_bwd32(gy, tap, neg, slope, use_mask, in_hw, bf16), want, bound))
    return worst


def test_maxpool_restatement_stays_inside():
    worst = 0.0
    for shape, kind, bf16 in _maxpool_cases():
        x, gy = R.maxpool_inputs(shape, kind, bf16)
        y, tap, neg = R.maxpool(x)
        y32, tap32, neg32 = maxpool32(x)
        assert np.array_equal(y32.astype(np.float64), y) and np.array_equal(tap32, tap) and np.array_equal(neg32, neg)
        assert tap.max() <= 8
        worst = max(worst, _maxpool_bwd_ratio(gy, tap32, neg32, tap, neg, shape[2:], bf16))
    print(f"\nmaxpool_bwd: largest err / bound of the fp32 restatement {worst:.3f}")
    assert worst <= 1.0


def test_maxpool_inputs_have_the_edges_they_promise():
    ties = zeros_won = negative_won = 0
    for shape, kind, bf16 in _maxpool_cases():
        x, _ = R.maxpool_inputs(shape, kind, bf16)
        c = shape[1]
        y, tap, neg = R.maxpool(x[..., :c])
        _, tap_last, _ = maxpool32(x[..., :c], wrong="last_max")
        ties += int((tap_last != tap).sum())
        zeros_won += int((y == 0).sum())
        negative_won += int((y < 0).sum())
        assert float(np.abs(x[..., c:]).max(initial=0.0)) == 0.0
    assert ties > 100 and zeros_won > 100 and negative_won > 0


@pytest.mark.parametrize("wrong", ["last_max", "strict_neg"])
def test_wrong_maxpool_records_leave_the_bounds(wrong):
    record_differs = gradient_leaves = 0
    for shape, kind, bf16 in _maxpool_cases():
        x, gy = R.maxpool_inputs(shape, kind, bf16)
        c = shape[1]
        y, tap, neg = R.maxpool(x)
        _, tap_w, neg_w = maxpool32(x, wrong=wrong)
        record_differs += int(not (np.array_equal(tap_w, tap) and np.array_equal(neg_w[..., :c], neg[..., :c])))
        gradient_leaves += int(_maxpool_bwd_ratio(gy, tap_w, neg_w, tap, neg, shape[2:], bf16) > 1.0)
    print(f"\n{wrong}: the record differs on {record_differs} cases, the gradient leaves its bound on {gradient_leaves}")
    assert record_differs > 0 and gradient_leaves > 0


def _poolfc_cases():
    for case in R.POOLFC_CASES:
        for bf16 in (False, True):
            yield case, bf16


def test_pool_fc_restatement_stays_inside():
    worst = dict(pooled=0.0, feats=0.0, dz=0.0)
    for case, bf16 in _poolfc_cases():
        c, slope = case[3], R.poolfc_slope(case)
        x, wfc, bias, df = R.poolfc_inputs(case, bf16)
        assert (x[..., :c] == 0).any()
        pooled, pb, feats, fb = R.avgpool_fc_fwd(x, wfc, bias, c)
        p32, f32_ = poolfc_fwd32(x, wfc, bias, c)
        worst["pooled"] = max(worst["pooled"], ratio(p32, pooled, pb))
        worst["feats"] = max(worst["feats"], ratio(f32_, feats, fb))
        for masked in (True, False):
            dz, db = R.avgpool_fc_bwd(df, wfc, x, c, slope, masked, bf16)
            worst["dz"] = max(worst["dz"], ratio(poolfc_bwd32(df, wfc, x, c, slope, masked, bf16), dz, db))
    print("\npool + fc: largest err / bound of the fp32 restatement " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_pooled_sum_that_drops_a_chunks_last_pixel_leaves_the_bound():
    left = []
    for case, bf16 in _poolfc_cases():
        n, h, w, c, cp = case[:5]
        x, wfc, bias, _ = R.poolfc_inputs(case, bf16)
        pooled, pb, feats, fb = R.avgpool_fc_fwd(x, wfc, bias, c)
        p32, f32_ = poolfc_fwd32(x, wfc, bias, c, wrong="drop_chunk_last")
        if ratio(p32, pooled, pb) > 1.0 and ratio(f32_, feats, fb) > 1.0:
            left.append((h * w, cp))
    assert (52, 80) in left and (9, 512) in left, left          # hw = PCH + 1 at both channel counts


def _fcw_cases():
    for c, nf in R.FCW_SHAPES + [(512, R.FCW_MAX_NF_AT_512)]:
        for n in (R.FCW_N if nf != R.FCW_MAX_NF_AT_512 else [65]):
            yield c, nf, n


def test_fc_wgrad_restatement_stays_inside():
    worst = dict(dw=0.0, db=0.0)
    for c, nf, n in _fcw_cases():
        df, pooled, prev_w, prev_b = R.fcw_inputs(c, nf, n)
        for acc in (False, True):
            dw, dwb, db, dbb = R.fc_wgrad(df, pooled, prev_w if acc else None, prev_b if acc else None)
            dw32, db32 = fcw32(df, pooled, prev_w if acc else None, prev_b if acc else None)
            worst["dw"], worst["db"] = max(worst["dw"], ratio(dw32, dw, dwb)), max(worst["db"], ratio(db32, db, dbb))
    print("\nfc_wgrad: largest err / bound of the fp32 restatement " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_fc_wgrad_that_drops_row_63_leaves_the_bound():
    for c, nf, n in _fcw_cases():
        df, pooled, prev_w, prev_b = R.fcw_inputs(c, nf, n)
        for acc in (False, True):
            dw, dwb, db, dbb = R.fc_wgrad(df, pooled, prev_w if acc else None, prev_b if acc else None)
            dw32, db32 = fcw32(df, pooled, prev_w if acc else None, prev_b if acc else None, wrong="drop_row_63")
            # every case with a 64th row notices, in both outputs; the others have no such row
            assert (ratio(dw32, dw, dwb) > 1.0) == (n >= 64) and (ratio(db32, db, dbb) > 1.0) == (n >= 64), (c, nf, n, acc)


def _adam_cases(sizes=R.ADAM_N):
    for n in sizes:
        for wd, scale in R.ADAM_WD_SCALE:
            for step in R.ADAM_STEPS:
                yield n, dict(R.ADAM_HYPER, weight_decay=wd, grad_scale=scale, step=step)


def test_adam_restatement_stays_inside():
    worst = dict(m=0.0, v=0.0, p=0.0)
    vs_u_p = 0.0
    for n, hyper in _adam_cases():
        p, g, m, v = R.adam_inputs(n)
        ref = R.adam_step(p, g, m, v, **hyper)
        got = dict(zip("mvp", adam32(p, g, m, v, **hyper)))
        for k in "mvp":
            worst[k] = max(worst[k], ratio(got[k], ref[k], ref[k + "_bound"]))
        assert np.isfinite(ref["p_bound"]).all()
        # the figure the docstring of adam_step quotes: against u |p| + the update's bound
        vs_u_p = max(vs_u_p, ratio(got["p"], ref["p"], R.U * np.abs(p) + ref["update_bound"]))
        if n >= 255:
            assert got["p"][R.ADAM_SPECIAL["all0"]] == 0.0 and ref["p_bound"][R.ADAM_SPECIAL["all0"]] == 0.0
    print("\nadam_step: largest err / bound of the fp32 restatement " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items())
          + f"; p against u |p| + update bound {vs_u_p:.3f}")
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("wrong", ["scale_after_decay", "bc2_not_sqrt"])
def test_wrong_adam_leaves_the_bound(wrong):
    left = []
    for n, hyper in _adam_cases(sizes=[255, 257]):
        p, g, m, v = R.adam_inputs(n)
        ref = R.adam_step(p, g, m, v, **hyper)
        got = dict(zip("mvp", adam32(p, g, m, v, wrong=wrong, **hyper)))
        if ratio(got["p"], ref["p"], ref["p_bound"]) > 1.0:
            left.append((n, hyper["weight_decay"], hyper["step"]))
    print(f"\n{wrong}: p leaves its bound on {len(left)} of 30 cases")
    if wrong == "scale_after_decay":      # only visible with a decay and a scale
        assert left and all(wd > 0 for _, wd, _ in left) and len(left) == 20
    else:                                 # sqrt(1 - b2^t) != 1 - b2^t at every step count used
        assert len(left) == 30


def test_bf16_rounding_helper_is_round_to_nearest_even():
    import torch
    x = np.random.default_rng(0).standard_normal(4096).astype(f32) * f32(37.0)
    x[:4] = [1.00390625, 1.01171875, 0.0, -1.00390625]                 # two ties (down to even, up to even), zero, a negative tie
    assert np.array_equal(R.to_bf16(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())


def test_avgpool_fc_bwd_wrapper_refuses_half_an_accumulation_target():
    """want_bias with only one of out / out_bias used to add the bias gradient to uninitialised memory."""
    import torch
    from mil_amd import ops
    n, c, nf = 2, 8, 3
    args = (torch.zeros(n, nf), torch.zeros(nf, c), torch.zeros(n, c), torch.zeros(n, 1, 1, c), c)
    with pytest.raises(ValueError, match="both out and out_bias"):
        ops.avgpool_fc_bwd(*args, out=torch.zeros(nf, c), want_bias=True)
    with pytest.raises(ValueError, match="both out and out_bias"):
        ops.avgpool_fc_bwd(*args, out_bias=torch.zeros(nf), want_bias=True)
