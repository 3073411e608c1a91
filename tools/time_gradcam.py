#!/usr/bin/env python3
"""Times Grad-CAM on one GPU, by default 256 tiles of 256 x 256, for `layer4` (8x8 maps of 80
channels) and `layer1` (64x64 maps of 20 channels of 24 stored), per compute mode (bf16 and bf16x3; --fp32 adds the exact mode):

  (i)   `ops.grad_cam` alone on random tensors of the stage's shape: the launch that writes raw only, the one that writes the
        bytes only, and the one with a given range (the second launch of normalize="bag");
  (ii)  a whole `TileGradCam.raw()` call and a whole `maps()` call in both normalisations, random weights;
  (iii) for scale, a whole `TileSaliency.maps()` call ("gradient") and an eval forward of the same bag.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The kernel's algorithmic bytes are one read
of act, one of grad and one write of the output; their rate at the median is printed next to the 8 TB/s HBM peak the project
prices against.  Prints one JSON line.  A report, not a test."""
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
WIDTHS = {"layer1": 20, "layer2": 40, "layer3": 60, "layer4": 80}


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


def stage_hw(size, layer):
    """Edge of the stage's maps for square tiles of `size`: the stem and the pool halve it, then every stage but the first."""
    s = (size + 1) // 2
    s = (s - 1) // 2 + 1
    for _ in range(int(layer[-1]) - 1):
        s = (s - 1) // 2 + 1
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--layers", default="layer4,layer1")
    ap.add_argument("--fp32", action="store_true", help="also time the exact-fp32 mode")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_gradcam.py needs a GPU")
    t, s = a.tiles, a.size
    res = {"tiles": t, "size": s, "reps": a.reps}
    gen = torch.Generator("cuda").manual_seed(1)
    modes = [("bf16", torch.bfloat16), ("bf16x3", L.BF16X3)] + ([("fp32", torch.float32)] if a.fp32 else [])
    for name, mode in modes:
        st = L.storage_dtype(mode)
        torch.manual_seed(2)
        model = mil_amd.Attention(3, compute_dtype=mode).eval()
        tiles = torch.randn(t, 3, s, s, device="cuda", generator=gen).clamp_(-1, 1)
        r = {}
        for layer in a.layers.split(","):
            c, m = WIDTHS[layer], stage_hw(s, layer)
            cs = ops.cpad(c)
            act = torch.randn(t, m, m, cs, device="cuda", generator=gen).to(st)
            grad = torch.randn(t, m, m, cs, device="cuda", generator=gen).to(st)
            rng = torch.tensor([0.0, 2.0], device="cuda")
            k = {"map_hw": m, "channels": c,
                 "kernel_raw": summary(timed(lambda: ops.grad_cam(act, grad, c, (s, s), want_map=False), a.warmup, a.reps)),
                 "kernel_map": summary(timed(lambda: ops.grad_cam(act, grad, c, (s, s), want_raw=False), a.warmup, a.reps)),
                 "kernel_map_range": summary(timed(lambda: ops.grad_cam(act, grad, c, (s, s), value_range=rng, want_raw=False),
                                                   a.warmup, a.reps))}
            read = 2 * act.numel() * act.element_size()
            for key, out_bytes in (("kernel_raw", t * m * m * 4), ("kernel_map", t * s * s), ("kernel_map_range", t * s * s)):
                tbps = (read + out_bytes) / k[key]["median_ms"] / 1e9
                k[key].update(algorithmic_bytes=read + out_bytes, TBps_at_median=round(tbps, 3),
                              fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4))
            del act, grad
            cam = mil_amd.TileGradCam(model, layer=layer)
            k["raw"] = summary(timed(lambda: cam.raw(tiles, 1), a.warmup, a.reps))
            k["maps_tile"] = summary(timed(lambda: cam.maps(tiles, 1), a.warmup, a.reps))
            k["maps_bag"] = summary(timed(lambda: cam.maps(tiles, 1, normalize="bag"), a.warmup, a.reps))
            r[layer] = k
        ts = mil_amd.TileSaliency(model)
        r["saliency_maps_gradient"] = summary(timed(lambda: ts.maps(tiles, 1), a.warmup, a.reps))
        with torch.no_grad():
            r["forward_only"] = summary(timed(lambda: model(tiles, torch.tensor([1])), a.warmup, a.reps))
        res[name] = r
        del model, ts, tiles
    print(json.dumps(res))


if __name__ == "__main__":
    main()
