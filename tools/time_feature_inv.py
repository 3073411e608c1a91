#!/usr/bin/env python3
"""Times one feature-inversion step on one GPU: `FeatureInverter.invert` at `layer4` for `--tiles` tiles of
`--size`^2 (default 256 of 256^2), in bf16 and bf16x3, the loop written out as the class runs it:

  (i)   the whole step with jitter (six groups of launches) and without (five), `--steps` steps between one pair of device events
        and nothing synchronising in between, as the class runs them;
  (ii)  the same loop with the three new elementwise stages written in torch: `torch.roll` for the jitter and its way back, the
        regulariser gradient and the two norms as tensor expressions, the momentum step as `mul_` / `add_`;
  (iii) each of the new launches alone — `pixel_shift`, `pixel_reg` (with and without terms, aliased and not),
        `pixel_momentum_step`, `stage_match` — with its algorithmic bytes (every tensor read or written once) at the median;
  (iv)  beside them, the `filters("layer4")` step of `tools/time_feature_vis.py` for 80 tiles on the same box;
  (v)   the Gaussian blur: `pixel_blur` alone on the 3 `--tiles` planes at sigma 1.0 and 4.0 for each edge
        rule, beside the torch form it replaces (`F.pad` plus two grouped `F.conv2d`) and `pixel_shift`, the pure copy through a
        comparable gather; and the `invert` and `filters("layer4")` steps without jitter with the image blur (sigma 1 every 2
        steps), with the gradient blur (sigma 1 every step), with both and with neither.

`--warmup` untimed and `--reps` timed repetitions, medians.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L  # noqa: E402
from mil_amd import encoder, ops  # noqa: E402

HBM_PEAK_TBPS = 8.0
ALPHA, AW, TW, LR, MO, WEIGHT = 6, 1e-7, 1e-8, 100.0, 0.9, 0.1


def timed(f, warmup, reps, per=1):
    out = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1) / per)
    return out


def summary(v, moved=None):
    r = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if moved is not None:
        tbps = moved / r["median_ms"] / 1e9
        r.update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
    return r


def torch_reg(x, g, shift, terms):
    """The regulariser stage as tensor expressions: the gradient moved back, the two gradients added, the two norms summed."""
    if shift != (0, 0):
        g = torch.roll(g, (-shift[0], -shift[1]), (2, 3))
    g.add_(x.pow(ALPHA - 1), alpha=AW * ALPHA)
    own = x[..., :-1, :-1]
    dd, dr = own - x[..., 1:, :-1], own - x[..., :-1, 1:]
    s = torch.zeros_like(x)
    s[..., :-1, :-1] += dd + dr
    s[..., 1:, :-1] -= dd
    s[..., :-1, 1:] -= dr
    g.add_(s, alpha=2 * TW)
    terms[0] = x.pow(ALPHA).sum(dim=(1, 2, 3))
    terms[1] = (dd * dd + dr * dr).sum(dim=(1, 2, 3))
    return g


TORCH_PAD = {"reflect": "reflect", "replicate": "replicate", "wrap": "circular"}


def torch_blur(x, full, edge):
    """The torch form of `ops.pixel_blur`: the padded stack, then one grouped convolution along W and one along H."""
    c, r = x.shape[1], (full.numel() - 1) // 2
    p = torch.nn.functional.pad(x, (r, r, r, r), mode=TORCH_PAD[edge])
    p = torch.nn.functional.conv2d(p, full.view(1, 1, 1, -1).expand(c, 1, 1, -1), groups=c)
    return torch.nn.functional.conv2d(p, full.view(1, 1, -1, 1).expand(c, 1, -1, 1), groups=c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_feature_inv.py needs a GPU")
    s, n = a.size, a.tiles
    res = {"size": s, "tiles": n, "steps_per_timing": a.steps, "reps": a.reps}
    run = lambda f, moved=None, per=1: summary(timed(f, a.warmup, a.reps, per), moved)      # noqa: E731
    gen = torch.Generator("cuda").manual_seed(1)
    tiles = mil_amd.U8Tiles(torch.randint(0, 256, (n, 3, s, s), device="cuda", generator=gen, dtype=torch.uint8))
    x0 = 0.1 * torch.randn((n, 3, s, s), device="cuda", generator=gen)
    g0 = torch.randn(x0.shape, device="cuda", generator=gen) * 1e-3
    nel = x0.numel()
    shifts = mil_amd.PixelRegularizer(jitter=4, seed=0).shifts(a.steps)
    # (iii) the new launches alone
    k = {}
    x, buf, out, xs = x0.clone(), torch.zeros_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    terms = torch.empty((2, n), device="cuda")
    k["pixel_shift"] = run(lambda: ops.pixel_shift(x, xs, (3, -2)), 8 * nel)
    k["pixel_reg_shifted_terms"] = run(lambda: ops.pixel_reg(x, g0, out, alpha=ALPHA, alpha_weight=AW, tv_weight=TW, shift=(3, -2), terms=terms), 12 * nel)
    k["pixel_reg_shifted"] = run(lambda: ops.pixel_reg(x, g0, out, alpha=ALPHA, alpha_weight=AW, tv_weight=TW, shift=(3, -2)), 12 * nel)
    ga = g0.clone()
    k["pixel_reg_aliased_terms"] = run(lambda: ops.pixel_reg(x, ga, ga, alpha=ALPHA, alpha_weight=AW, tv_weight=TW, terms=terms), 12 * nel)
    k["pixel_momentum_step"] = run(lambda: ops.pixel_momentum_step(x, g0, buf, lr=1e-3, momentum=MO), 20 * nel)
    tt = torch.empty((2, n), device="cuda")
    gt = g0.clone()
    k["torch_roll"] = run(lambda: torch.roll(x, (3, -2), (2, 3)), 8 * nel)
    k["torch_reg_shifted_terms"] = run(lambda: torch_reg(x, gt, (3, -2), tt))
    bt = torch.zeros_like(x0)
    k["torch_momentum"] = run(lambda: x.add_(bt.mul_(MO).add_(g0), alpha=-1e-3), 40 * nel)
    res["launches_alone"] = k
    # (v) the blur alone: 8 bytes per element of compulsory traffic
    b = {"planes": 3 * n, "pixel_shift": k["pixel_shift"]}
    for sigma in (1.0, 4.0):
        radius, half = ops.gauss_taps(sigma)
        full = torch.tensor(list(half[:0:-1]) + list(half), dtype=torch.float32, device="cuda")
        for edge in ops.BLUR_EDGES:
            b[f"pixel_blur_sigma{sigma:g}_{edge}"] = run(lambda: ops.pixel_blur(x, xs, sigma=sigma, edge=edge), 8 * nel)
            b[f"torch_pad_conv2d_sigma{sigma:g}_{edge}"] = run(lambda: torch_blur(x, full, edge), 8 * nel)
            b[f"max_abs_difference_sigma{sigma:g}_{edge}"] = float((ops.pixel_blur(x, xs, sigma=sigma, edge=edge) - torch_blur(x, full, edge)).abs().max())
        b[f"radius_sigma{sigma:g}"] = radius
    res["blur_alone"] = b
    del x, buf, out, xs, ga, gt, bt
    for name, mode in (("bf16", torch.bfloat16), ("bf16x3", L.BF16X3)):
        st = L.storage_dtype(mode)
        torch.manual_seed(2)
        net = mil_amd.Attention(3, compute_dtype=mode).eval().cnn.module
        c = encoder.STAGE_WIDTHS[3]
        r = {}
        with torch.no_grad(), L.f32_mma(L.mma_code(mode)):
            target = encoder.encoder_forward(net, tiles.u8, st, upto=4)[1]["blocks"][-1][2]
            energy = ops.stage_energy(target, c)
            x, buf, out, xs = x0.clone(), torch.zeros_like(x0), torch.empty_like(x0), torch.empty_like(x0)
            trace = torch.empty((a.steps, n), device="cuda")
            terms = torch.empty((a.steps, 2, n), device="cuda")
            box = {}

            def grad(src, i):
                saved = encoder.encoder_forward(net, src, st, upto=4)[1]
                box["act"] = saved["blocks"][-1][2]
                dz = ops.stage_match(box["act"], target, c, weight=WEIGHT, energy=energy, loss=trace[i])[1]
                return encoder.encoder_pixel_gradient(net, saved, st, dz=dz, stage=4)[0]

            def hip_loop(jitter):
                for i in range(a.steps):
                    sh = shifts[i] if jitter else (0, 0)
                    g = grad(ops.pixel_shift(x, xs, sh) if jitter else x, i)
                    g = ops.pixel_reg(x, g, out if jitter else g, alpha=ALPHA, alpha_weight=AW, tv_weight=TW, shift=sh, terms=terms[i])
                    ops.pixel_momentum_step(x, g, buf, lr=LR, momentum=MO)

            def torch_loop(jitter):
                for i in range(a.steps):
                    sh = shifts[i] if jitter else (0, 0)
                    g = grad(torch.roll(x, sh, (2, 3)) if jitter else x, i)
                    g = torch_reg(x, g, sh, terms[i])
                    x.add_(buf.mul_(MO).add_(g), alpha=-LR)

            def core_loop():
                for i in range(a.steps):
                    grad(x, i)

            for label, f in (("hip_jitter", lambda: hip_loop(True)), ("hip_no_jitter", lambda: hip_loop(False)),
                             ("torch_jitter", lambda: torch_loop(True)), ("torch_no_jitter", lambda: torch_loop(False)),
                             ("forward_match_backward_only", core_loop)):
                x.copy_(x0)
                buf.zero_()
                r[label] = run(f, per=a.steps)
            r["stage_match"] = run(lambda: ops.stage_match(box["act"], target, c, weight=WEIGHT, energy=energy),
                                   3 * box["act"].numel() * box["act"].element_size())
            # (iv) the filters step for 80 tiles
            xf = mil_amd.U8Tiles(tiles.u8[:80].clone()).float()
            ch = torch.arange(80, dtype=torch.int32, device="cuda")
            state = (torch.zeros_like(xf), torch.zeros_like(xf))

            def filters_loop():
                for _ in range(a.steps):
                    saved = encoder.encoder_forward(net, xf, st, upto=4)[1]
                    dz = ops.stage_seed(saved["blocks"][-1][2], ch, c)[1]
                    g = encoder.encoder_pixel_gradient(net, saved, st, dz=dz, stage=4)[0]
                    ops.pixel_step(xf, g, state, rule="adam", lr=0.1, weight_decay=1e-6, step=3)
            r["filters_80_tiles"] = run(filters_loop, per=a.steps)
            # (v) the steps with the blurs, without jitter: two stacks that swap at an image blur, the spare one takes the blurred gradient
            def blur_steps(first, second, step, image, grad):
                cur = [first, second]
                for i in range(a.steps):
                    if image and i > 0 and i % 2 == 0:
                        ops.pixel_blur(cur[0], cur[1], sigma=1.0)
                        cur.reverse()
                    g = step(cur[0], i)
                    if grad:
                        g = ops.pixel_blur(g, cur[1], sigma=1.0)
                    yield cur[0], g

            def invert_step(xc, i):
                g = grad(xc, i)
                return ops.pixel_reg(xc, g, g, alpha=ALPHA, alpha_weight=AW, tv_weight=TW, terms=terms[i])

            def filters_step(xc, i):
                saved = encoder.encoder_forward(net, xc, st, upto=4)[1]
                dz = ops.stage_seed(saved["blocks"][-1][2], ch, c)[1]
                return encoder.encoder_pixel_gradient(net, saved, st, dz=dz, stage=4)[0]

            def invert_blur(image, grad_):
                for xc, g in blur_steps(x, xs, invert_step, image, grad_):
                    ops.pixel_momentum_step(xc, g, buf, lr=LR, momentum=MO)

            xf2 = torch.empty_like(xf)

            def filters_blur(image, grad_):
                for xc, g in blur_steps(xf, xf2, filters_step, image, grad_):
                    ops.pixel_step(xc, g, state, rule="adam", lr=0.1, weight_decay=1e-6, step=3)

            for label, image, grad_ in (("neither", False, False), ("image_blur", True, False), ("gradient_blur", False, True), ("both", True, True)):
                x.copy_(x0)
                buf.zero_()
                r["invert_step_" + label] = run(lambda: invert_blur(image, grad_), per=a.steps)
                r["filters_80_tiles_step_" + label] = run(lambda: filters_blur(image, grad_), per=a.steps)
        res[name] = r
        del net, x, buf, out, xs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
