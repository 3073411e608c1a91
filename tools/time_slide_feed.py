#!/usr/bin/env python3
"""Times the three ways to turn kept windows of a resident slide into uint8 tiles, on one GPU:

  (i)   `TilePreprocessor.from_slide(slide, coords, out="u8")` — the windows are read where they lie;
  (ii)  the copy loop of `RoiSelector.select` (roi_select.py: one `copy_` per kept window into a [T,S,S,3] stack) followed by
        `prep(rois, out="u8")` — the route before from_slide existed;
  (iii) `prep(rois, out="u8")` alone on the already gathered stack.

The slide's row pitch is deliberately no multiple of 16, so (i) takes the unaligned staging; (i) / (iii) is its price.  Device
events around each route, the three routes alternating inside every repetition; prints one JSON line with the median, the
smallest and the largest time of each route and the bytes each has to move.  A report, not a test: nothing is asserted but
that the three routes return the same bytes."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, default=8, help="windows per axis (default 8: 64 windows)")
    ap.add_argument("--roi", type=int, default=1200)
    ap.add_argument("--res", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--train", action="store_true", help="the train chain (Pad, crop, flips) instead of the flat one")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_slide_feed.py needs a GPU")
    s, r, g = a.roi, a.res, a.grid
    h, w = g * s + 100, g * s + 111
    assert (3 * w) % 16, "the row pitch must not be a multiple of 16"
    slide = torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
    coords = [(13 + s * i, 13 + s * j) for j in range(g) for i in range(g)]
    n = len(coords)
    prep = mil_amd.TilePreprocessor(s, r)
    params = prep.draw_params(n, torch.Generator().manual_seed(2)) if a.train else None

    def gather():
        rois = torch.empty((n, s, s, 3), dtype=torch.uint8, device=slide.device)
        for j, (y, x) in enumerate(coords):
            rois[j].copy_(slide[y:y + s, x:x + s])
        return rois

    stack = gather()
    routes = {
        "from_slide": lambda: prep.from_slide(slide, coords, params, out="u8"),
        "gather_then_prep": lambda: prep(gather(), params, out="u8"),
        "prep_on_stack": lambda: prep(stack, params, out="u8"),
    }
    want = routes["prep_on_stack"]().u8
    for name, f in routes.items():
        assert torch.equal(f().u8, want), name
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for name, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    win, out = n * s * s * 3, n * 3 * r * r
    moved = {"from_slide": win + out, "gather_then_prep": 3 * win + out, "prep_on_stack": win + out}
    res = {"windows": n, "roi": s, "res": r, "row_pitch": 3 * w, "chain": "train" if a.train else "flat", "reps": a.reps}
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                  "bytes": moved[k], "GBps_at_median": round(moved[k] / statistics.median(v) / 1e6, 1)}
    res["from_slide_over_gather_then_prep"] = round(res["from_slide"]["median_ms"] / res["gather_then_prep"]["median_ms"], 3)
    res["from_slide_over_prep_on_stack"] = round(res["from_slide"]["median_ms"] / res["prep_on_stack"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
