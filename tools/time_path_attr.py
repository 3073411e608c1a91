#!/usr/bin/env python3
"""Times integrated gradients and SmoothGrad on one GPU, by default 256 tiles of 256 x 256, per compute
mode (bf16, bf16x3 and the exact fp32 mode):

  (i)   the three kernels alone: `ops.path_point` from fp32 and from uint8 tiles, without and with noise; `ops.stem_dgrad_acc`
        next to `ops.stem_dgrad` (dstem random, half its elements zero, as the pool backward leaves it); `ops.attr_finish`
        making the attributions, a map, and a map with the per-tile sums.  Algorithmic bytes (every tensor read or written
        once) at the median, as a fraction of the 8 TB/s HBM peak the project prices against;
  (ii)  one integrated-gradients step and one SmoothGrad step through the new path: `ops.path_point` into a reused buffer, the
        encoder forward and backward with `dx_acc`;
  (iii) the same steps composed in torch, as they would be written without this feature: `base + a * (x - base)` (or
        `x + sigma * randn_like(x)`), `TileSaliency.input_gradient`, `acc.add_(dx, alpha=w)` — the yardstick;
  (iv)  peak device memory of (ii) and (iii) above what is resident before the step (tiles, model, accumulator).

Device events around each route, `--warmup` untimed and `--reps` timed repetitions, medians.  Prints one JSON line.  A report, not
a test."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L  # noqa: E402
from mil_amd import ops  # noqa: E402
from mil_amd.saliency import bag_setup, bag_step  # noqa: E402

HBM_PEAK_TBPS = 8.0


def timed(f, warmup, reps):
    out = []
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            out.append(e0.elapsed_time(e1))
    return out


def summary(v, moved=None):
    r = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if moved is not None:
        tbps = moved / r["median_ms"] / 1e9
        r.update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
    return r


def peak_above_resident(f):
    """Peak allocated bytes during f() above what was allocated when it was called."""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - before


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_path_attr.py needs a GPU")
    t, s = a.tiles, a.size
    h2 = (s + 1) // 2
    res = {"tiles": t, "size": s, "reps": a.reps}
    gen = torch.Generator("cuda").manual_seed(1)
    u8 = mil_amd.U8Tiles(torch.randint(0, 256, (t, 3, s, s), device="cuda", generator=gen, dtype=torch.uint8))
    x = u8.float()
    nel = x.numel()
    base = (1.0, 0.9, 0.8)
    out = torch.empty_like(x)
    rng = torch.stack((x.amin(), x.amax()))
    run = lambda f, moved=None: summary(timed(f, a.warmup, a.reps), moved)      # noqa: E731
    k = {"path_point_f32": run(lambda: ops.path_point(x, 0.375, base, out=out), 8 * nel),
         "path_point_u8": run(lambda: ops.path_point(u8, 0.375, base, out=out), 5 * nel),
         "path_point_f32_noise": run(lambda: ops.path_point(x, 1.0, 0.0, noise_level=0.15, value_range=rng, seed=1, sample=3, out=out), 8 * nel),
         "path_point_u8_noise": run(lambda: ops.path_point(u8, 1.0, 0.0, noise_level=0.15, value_range=rng, seed=1, sample=3, out=out), 5 * nel),
         "attr_finish_attr_f32": run(lambda: ops.attr_finish(out, x, base), 12 * nel),
         "attr_finish_map_u8": run(lambda: ops.attr_finish(out, u8, base, want_attr=False, want_map=True), 5 * nel + 4 * nel // 3),
         "attr_finish_map_sums_u8": run(lambda: ops.attr_finish(out, u8, base, want_attr=False, want_map=True, want_sums=True), 5 * nel + 4 * nel // 3),
         "attr_finish_grad_map": run(lambda: ops.attr_finish(out, None, 0.0, want_attr=False, want_map=True, map_mode="grad_max"), 4 * nel + 4 * nel // 3)}
    res["kernels"] = k
    wt = torch.randn(20, 3, 7, 7, device="cuda", generator=gen) / 147 ** 0.5
    for name, mode in (("bf16", torch.bfloat16), ("bf16x3", L.BF16X3), ("fp32", torch.float32)):
        st = L.storage_dtype(mode)
        r = {}
        with L.f32_mma(L.mma_code(mode)):
            wp, _ = ops.pack_weights(wt, None, L.PACK_STEM_DGRAD, st)
            dstem = torch.randn(t, h2, h2, 24, device="cuda", generator=gen)
            dstem = (dstem * (torch.rand(dstem.shape, device="cuda", generator=gen) < 0.5)).to(st)
            dstem[..., 20:] = 0
            acc = torch.zeros_like(x)
            db = dstem.numel() * dstem.element_size()
            r["stem_dgrad"] = run(lambda: ops.stem_dgrad(dstem, wp, (s, s), dx=out), db + 4 * nel)
            r["stem_dgrad_acc"] = run(lambda: ops.stem_dgrad_acc(dstem, wp, (s, s), acc, 0.25), db + 8 * nel)
            del dstem
        torch.manual_seed(2)
        model = mil_amd.Attention(3, compute_dtype=mode).eval()
        sal = mil_amd.TileSaliency(model)
        setup = bag_setup(model, t, 1)
        acc.zero_()

        def ig_fused():
            ops.path_point(u8, 0.375, base, out=out)
            bag_step(model, setup, out, dx_acc=(acc, 0.25))

        def sg_fused():
            ops.path_point(u8, 1.0, 0.0, noise_level=0.15, value_range=rng, seed=1, sample=3, out=out)
            bag_step(model, setup, out, dx_acc=(acc, 0.25))

        b4 = torch.tensor(base, device="cuda").view(1, 3, 1, 1)
        sigma = 0.15 * (rng[1] - rng[0])

        def ig_torch():
            xf = u8.float()
            acc.add_(sal.input_gradient(b4 + 0.375 * (xf - b4), 1), alpha=0.25)

        def sg_torch():
            xf = u8.float()
            acc.add_(sal.input_gradient(xf + sigma * torch.randn_like(xf), 1), alpha=0.25)

        for key, f in (("ig_step_fused", ig_fused), ("ig_step_torch", ig_torch), ("sg_step_fused", sg_fused), ("sg_step_torch", sg_torch)):
            r[key] = run(f)
            r[key]["peak_bytes_above_resident"] = peak_above_resident(f)
        r["input_gradient"] = run(lambda: sal.input_gradient(x, 1))
        res[name] = r
        del model, sal, acc
    print(json.dumps(res))


if __name__ == "__main__":
    main()
