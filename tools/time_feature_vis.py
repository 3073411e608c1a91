#!/usr/bin/env python3
"""Times one activation-maximisation step on one GPU: `filters("layer4")` — 80 tiles — and
`filters("layer2")` — 40 tiles — of 256 x 256, in bf16 and bf16x3:

  (i)   the step split into its four parts: the truncated forward, `ops.stage_seed`, `encoder_pixel_gradient`, `ops.pixel_step`
        (Adam, no projection), each between device events of its own, and the whole step between one pair;
  (ii)  the same backward with `want_wgrad=True` forced (the walk of `encoder_stage_gradient` / `encoder_backward`: every
        weight-gradient launch, results dropped), to show what the skipped launches were worth;
  (iii) `ops.pixel_step` alone per rule and projection, with and without the byte output: algorithmic bytes (every tensor read or
        written once) at the median, as a fraction of the 8 TB/s HBM peak the project prices against.

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_feature_vis.py needs a GPU")
    s = a.size
    res = {"size": s, "reps": a.reps}
    run = lambda f, moved=None: summary(timed(f, a.warmup, a.reps), moved)      # noqa: E731
    gen = torch.Generator("cuda").manual_seed(1)
    x = mil_amd.U8Tiles(torch.randint(150, 180, (80, 3, s, s), device="cuda", generator=gen, dtype=torch.uint8)).float()
    g = torch.randn(x.shape, device="cuda", generator=gen) * 1e-3
    m, v, u8 = torch.zeros_like(x), torch.zeros_like(x), torch.empty(x.shape, dtype=torch.uint8, device="cuda")
    nel = x.numel()
    k = {}
    for rule, state, words in (("sgd", None, 3), ("adam", (m, v), 7)):
        for project in ops.PIXEL_PROJECTIONS:
            for out in (None, u8):
                xx = x.clone()
                k[f"{rule}_{project}" + ("_u8out" if out is not None else "")] = run(
                    lambda: ops.pixel_step(xx, g, state, rule=rule, lr=0.1, weight_decay=1e-6, step=3, project=project, u8_out=out),
                    (4 * words + (1 if out is not None else 0)) * nel)
    res["pixel_step_80_tiles"] = k
    del g, m, v, u8
    for name, mode in (("bf16", torch.bfloat16), ("bf16x3", L.BF16X3)):
        st = L.storage_dtype(mode)
        torch.manual_seed(2)
        net = mil_amd.Attention(3, compute_dtype=mode).eval().cnn.module
        r = {}
        for stage in (4, 2):
            c = encoder.STAGE_WIDTHS[stage - 1]
            xs = x[:c].clone()
            ch = torch.arange(c, dtype=torch.int32, device="cuda")
            state = (torch.zeros_like(xs), torch.zeros_like(xs))
            obj = torch.empty(c, device="cuda")
            box = {}

            def fwd():
                box["saved"] = encoder.encoder_forward(net, xs, st, upto=stage)[1]

            def seed():
                box["dz"] = ops.stage_seed(box["saved"]["blocks"][-1][2], ch, c, objective=obj)[1]

            def bwd():
                box["g"] = encoder.encoder_pixel_gradient(net, box["saved"], st, dz=box["dz"], stage=stage)[0]

            def bwd_with_wgrad():
                saved = box["saved"]
                bw = encoder._Backward(net, saved, st, False, True)
                dz = box["dz"]
                with bw.reductions(dz.device):
                    for below in reversed(net.stages()[:stage]):
                        dz = encoder._stage_backward(bw, below, dz)
                    dstem = encoder._stem_backward(bw, dz)
                if dstem is None:
                    dstem = ops.maxpool_bwd(dz, saved["widx"], saved["stem_hw"])
                box["g"] = ops.stem_dgrad(dstem, net.stem_dgrad_packed(st), saved["tile_hw"])[0]

            def step():
                ops.pixel_step(xs, box["g"], state, rule="adam", lr=0.1, weight_decay=1e-6, step=3)

            def whole():
                fwd(); seed(); bwd(); step()

            with torch.no_grad(), L.f32_mma(L.mma_code(mode)):
                fwd(); seed(); bwd()
                r[f"layer{stage}"] = {"tiles": c, "forward": run(fwd), "stage_seed": run(seed), "backward": run(bwd),
                                      "backward_with_wgrad": run(bwd_with_wgrad), "pixel_step": run(step), "step": run(whole)}
        res[name] = r
        del net
    print(json.dumps(res))


if __name__ == "__main__":
    main()
