#!/usr/bin/env python3
"""Times the wide encoder (`alt_resnet`, bf16) on one GPU for its three feeds, by default 2048 tiles of
256 x 256 and the resnet18 depths:

  (i)  the stem forward alone — one launch of `stem_fwd_fused_kernel<4, ...>` per call: `ops.stem_fwd_fused` on the fp32 stack (as
       the encoder calls it: the space-to-depth copy is written for the backward), the same with `keep_s2d=False` (what the two
       other feeds are bit-equal to), `ops.stem_fwd_fused_u8` on the bytes, `ops.stem_fwd_fused_xs` on the space-to-depth tensor,
       and `ops.stem_s2d_u8` (what the uint8 feed adds to the backward);
  (ii) a full step — `net(feed)` and `feats.backward(dfeats)` — for the fp32 tensor, `U8Tiles` and `S2dTiles`.

Device events around each call, `--warmup` untimed and `--reps` / `--step-reps` timed repetitions; within a repetition the routes
run one after the other, so that whatever else the machine is doing is shared between them.  The algorithmic bytes of (i) are one
read of the input form plus the pooled map and the winner records (plus the space-to-depth copy where one is written); the rate is
printed next to the 8 TB/s HBM peak.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import alt_resnet as alt, ops  # noqa: E402

HBM_PEAK_TBPS = 8.0


def timed_round_robin(routes, warmup, reps):
    """{name: [ms per timed repetition]}: every repetition runs every route once, in the order given."""
    out = {k: [] for k in routes}
    for it in range(warmup + reps):
        for k, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                out[k].append(e0.elapsed_time(e1))
    return out


def summary(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
            "spread": round((max(v) - min(v)) / med, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=2048)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--layers", type=int, nargs=4, default=[2, 2, 2, 2])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step-reps", type=int, default=6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_wide_feed.py needs a GPU")
    t, r = a.tiles, a.resolution
    torch.manual_seed(1)
    net = alt.ResNet(alt.BasicBlock, a.layers, num_classes=80, compute_dtype=torch.bfloat16).cuda()
    u8 = torch.empty((t, 3, r, r), dtype=torch.uint8, device="cuda")
    u8.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(2))
    handle = mil_amd.U8Tiles(u8)
    x = handle.float()
    xs = ops.stem_s2d_u8(u8, torch.bfloat16)
    wp, bp = alt._packed_stem(net, torch.bfloat16)

    def need(v):
        if v is None:
            sys.exit(f"no fused 64-channel stem at {t} x {r} x {r}")
        return v

    stem = {
        "stem_fp32_keep_s2d": lambda: need(ops.stem_fwd_fused(x, wp, bp, 64, slope=0.0)),
        "stem_fp32": lambda: need(ops.stem_fwd_fused(x, wp, bp, 64, slope=0.0, keep_s2d=False)),
        "stem_u8": lambda: need(ops.stem_fwd_fused_u8(u8, wp, bp, 64, slope=0.0)),
        "stem_s2d": lambda: need(ops.stem_fwd_fused_xs(xs, wp, bp, 64, slope=0.0)),
        "s2d_from_u8": lambda: ops.stem_s2d_u8(u8, torch.bfloat16),
    }
    # the three forward forms agree bit for bit at the size that is timed
    ref = stem["stem_fp32"]()[1:]
    for k in ("stem_u8", "stem_s2d"):
        got = stem[k]()
        if not (torch.equal(got[0].view(torch.int16), ref[0].view(torch.int16)) and torch.equal(got[1], ref[1])):
            sys.exit(f"{k} differs from the fp32 feed")
    del ref, got
    times = timed_round_robin(stem, a.warmup, a.reps)

    dfeats = torch.randn((t, 80), generator=torch.Generator("cuda").manual_seed(3), device="cuda")

    def step(feed):
        def run():
            for p in net.parameters():
                p.grad = None
            net(feed).backward(dfeats)
        return run

    steps = {"step_fp32": step(x), "step_u8": step(handle), "step_s2d": step(mil_amd.S2dTiles(xs))}
    times.update(timed_round_robin(steps, min(a.warmup, 2), a.step_reps))

    h2 = r // 2
    hp = (h2 - 1) // 2 + 1
    out_bytes = t * hp * hp * 64 * 3                       # bf16 pooled map + 1-byte winner records
    x_bytes, u8_bytes, xs_bytes = t * 3 * r * r * 4, t * 3 * r * r, t * h2 * h2 * 32
    moved_by = {"stem_fp32_keep_s2d": x_bytes + xs_bytes + out_bytes, "stem_fp32": x_bytes + out_bytes, "stem_u8": u8_bytes + out_bytes,
                "stem_s2d": xs_bytes + out_bytes, "s2d_from_u8": u8_bytes + xs_bytes}
    res = {"tiles": t, "resolution": r, "layers": a.layers, "reps": a.reps, "step_reps": a.step_reps,
           "peak_memory_GiB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    for k, v in times.items():
        res[k] = summary(v)
        if k in moved_by:
            moved = moved_by[k]
            tbps = moved / statistics.median(v) / 1e9
            res[k].update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
    for k in ("u8", "s2d"):
        res[f"stem_{k}_over_fp32"] = round(res[f"stem_{k}"]["median_ms"] / res["stem_fp32"]["median_ms"], 4)
        res[f"stem_{k}_over_fp32_keep_s2d"] = round(res[f"stem_{k}"]["median_ms"] / res["stem_fp32_keep_s2d"]["median_ms"], 4)
        res[f"step_{k}_over_fp32"] = round(res[f"step_{k}"]["median_ms"] / res["step_fp32"]["median_ms"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
