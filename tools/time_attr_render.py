#!/usr/bin/env python3
"""Times the attribution renderer on one GPU, by default 256 tiles of 256 x 256:

  (i)   `ops.map_quantile` of a gradient [T,3,H,W] at q = 99 (three histogram + select passes), per tile and per bag, of a map
        [T,H,W], and the one-pass q = 100 form on the raw gradient that colour and positive / negative use;
  (ii)  `ops.attr_render` in each mode and `ops.cam_overlay`, the pointwise launches;
  (iii) whole `AttributionRenderer.grayscale()` / `colour()` / `pos_neg()` / `overlay()` calls;
  (iv)  what a user writes without them: `torch.quantile(gray.view(T,-1), 0.99, dim=1)` plus torch pointwise ops on the
        device, for the grayscale picture and for the colour picture.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of a route (every
pass reads its input once, a picture is written once) and their rate at the median are printed next to the 8 TB/s HBM peak the
project prices against.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
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


def summary(v, moved=None):
    r = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    if moved is not None:
        tbps = moved / r["median_ms"] / 1e9
        r.update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
    return r


def torch_grayscale(grad):
    t = grad.shape[0]
    gray = grad.abs().sum(1)
    flat = gray.view(t, -1)
    p = torch.quantile(flat, 0.99, dim=1).view(t, 1, 1)
    mn = flat.amin(1).view(t, 1, 1)
    return (((gray - mn) / (p - mn)).clamp_(0, 1) * 255).to(torch.uint8)


def torch_colour(grad):
    t = grad.shape[0]
    flat = grad.view(t, -1)
    mn, mx = flat.amin(1).view(t, 1, 1, 1), flat.amax(1).view(t, 1, 1, 1)
    return (((grad - mn) / (mx - mn)) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_attr_render.py needs a GPU")
    t, s = a.tiles, a.size
    gen = torch.Generator("cuda").manual_seed(1)
    grad = torch.randn(t, 3, s, s, device="cuda", generator=gen) ** 3 * 1e-4
    amap = grad.abs().amax(1)
    tiles = mil_amd.U8Tiles(torch.randint(0, 256, (t, 3, s, s), device="cuda", generator=gen, dtype=torch.uint8))
    gbytes, mbytes, px = grad.numel() * 4, amap.numel() * 4, t * s * s
    w, n = a.warmup, a.reps
    res = {"tiles": t, "size": s, "reps": n}
    res["map_quantile_q99_tile"] = summary(timed(lambda: ops.map_quantile(grad, 99.0, "tile"), w, n), 3 * gbytes)
    res["map_quantile_q99_bag"] = summary(timed(lambda: ops.map_quantile(grad, 99.0, "bag"), w, n), 3 * gbytes)
    res["map_quantile_q99_tile_map"] = summary(timed(lambda: ops.map_quantile(amap, 99.0, "tile"), w, n), 3 * mbytes)
    res["map_quantile_q100_raw"] = summary(timed(lambda: ops.map_quantile(grad, 100.0, "tile", raw=True), w, n), gbytes)
    st = ops.map_quantile(grad, 99.0, "tile")
    st_raw = ops.map_quantile(grad, 100.0, "tile", raw=True)
    res["attr_render_grayscale"] = summary(timed(lambda: ops.attr_render(grad, st, "grayscale"), w, n), gbytes + px)
    res["attr_render_colour"] = summary(timed(lambda: ops.attr_render(grad, st_raw, "colour"), w, n), gbytes + 3 * px)
    res["attr_render_pos_neg"] = summary(timed(lambda: ops.attr_render(grad, st_raw, "pos_neg"), w, n), gbytes + 6 * px)
    r = mil_amd.AttributionRenderer()
    gray = r.grayscale(grad)
    lut = r.table.cuda()
    res["cam_overlay"] = summary(timed(lambda: ops.cam_overlay(tiles, gray, lut, 102), w, n), 3 * px + px + 6 * px)
    res["renderer_grayscale"] = summary(timed(lambda: r.grayscale(grad), w, n), 4 * gbytes + px)
    res["renderer_colour"] = summary(timed(lambda: r.colour(grad), w, n), 2 * gbytes + 3 * px)
    res["renderer_pos_neg"] = summary(timed(lambda: r.pos_neg(grad), w, n), 2 * gbytes + 6 * px)
    res["renderer_overlay"] = summary(timed(lambda: r.overlay(tiles, gray), w, n), 10 * px)
    try:                                                   # (torch.quantile refuses inputs it finds too large)
        res["torch_grayscale"] = summary(timed(lambda: torch_grayscale(grad), w, n))
        res["torch_quantile_only"] = summary(timed(lambda: torch.quantile(amap.view(t, -1), 0.99, dim=1), w, n))
        diff = (torch_grayscale(grad).int() - gray.int()).abs()
        res["torch_grayscale_vs_renderer"] = {"bytes_differing": int((diff != 0).sum()), "max_levels": int(diff.max()), "bytes": diff.numel()}
    except RuntimeError as e:
        res["torch_grayscale"] = {"error": str(e).splitlines()[0]}
    res["torch_colour"] = summary(timed(lambda: torch_colour(grad), w, n))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
