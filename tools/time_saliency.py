#!/usr/bin/env python3
"""Times tile saliency on one GPU, by default 256 tiles of 256 x 256:

  (i)   `ops.stem_dgrad` alone, per compute mode (bf16 and bf16x3; --fp32 adds the exact mode): the launch that writes
        dx [T,3,H,W], and the one with the fused epilogue that writes sal [T,H,W] only.  dstem is random with half its elements
        zero, as the pool backward leaves it;
  (ii)  `ops.maxpool_bwd`, the launch in front of it (what produces dstem);
  (iii) a whole `TileSaliency.maps()` call ("gradient") and a whole `input_gradient()` call, random weights.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The kernel's algorithmic bytes are one read
of dstem plus one write of dx (or sal); their rate at the median is printed next to the 8 TB/s HBM peak the project prices
against.  Prints one JSON line.  A report, not a test."""
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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fp32", action="store_true", help="also time the exact-fp32 mode")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_saliency.py needs a GPU")
    t, s = a.tiles, a.size
    h2 = (s + 1) // 2
    hp = (h2 - 1) // 2 + 1
    res = {"tiles": t, "size": s, "reps": a.reps}
    gen = torch.Generator("cuda").manual_seed(1)
    wt = torch.randn(20, 3, 7, 7, device="cuda", generator=gen) / 147 ** 0.5
    modes = [("bf16", torch.bfloat16), ("bf16x3", L.BF16X3)] + ([("fp32", torch.float32)] if a.fp32 else [])
    for name, mode in modes:
        st = L.storage_dtype(mode)
        with L.f32_mma(L.mma_code(mode)):
            wp, _ = ops.pack_weights(wt, None, L.PACK_STEM_DGRAD, st)
            dstem = torch.randn(t, h2, h2, 24, device="cuda", generator=gen)
            dstem = (dstem * (torch.rand(dstem.shape, device="cuda", generator=gen) < 0.5)).to(st)
            dstem[..., 20:] = 0
            gy = torch.randn(t, hp, hp, 24, device="cuda", generator=gen).to(st)
            widx = torch.randint(0, 9, (t, hp, hp, 24), device="cuda", generator=gen).to(torch.uint8)
            dx = torch.empty(t, 3, s, s, device="cuda")
            sal = torch.empty(t, s, s, device="cuda")
            r = {"stem_dgrad_dx": summary(timed(lambda: ops.stem_dgrad(dstem, wp, (s, s), dx=dx), a.warmup, a.reps)),
                 "stem_dgrad_sal": summary(timed(lambda: ops.stem_dgrad(dstem, wp, (s, s), reduce="max_abs", sal=sal), a.warmup, a.reps)),
                 "maxpool_bwd": summary(timed(lambda: ops.maxpool_bwd(gy, widx, (h2, h2)), a.warmup, a.reps))}
        for key, out_bytes in (("stem_dgrad_dx", dx.numel() * 4), ("stem_dgrad_sal", sal.numel() * 4)):
            moved = dstem.numel() * dstem.element_size() + out_bytes
            tbps = moved / r[key]["median_ms"] / 1e9
            r[key].update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
        del dstem, gy, widx, dx, sal
        torch.manual_seed(2)
        model = mil_amd.Attention(3, compute_dtype=mode).eval()
        tiles = torch.randn(t, 3, s, s, device="cuda", generator=gen).clamp_(-1, 1)
        ts = mil_amd.TileSaliency(model)
        r["maps_gradient"] = summary(timed(lambda: ts.maps(tiles, 1), a.warmup, a.reps))
        r["input_gradient"] = summary(timed(lambda: ts.input_gradient(tiles, 1), a.warmup, a.reps))
        with torch.no_grad():
            r["forward_only"] = summary(timed(lambda: model(tiles, torch.tensor([1])), a.warmup, a.reps))
        res[name] = r
        del model, ts, tiles
    print(json.dumps(res))


if __name__ == "__main__":
    main()
