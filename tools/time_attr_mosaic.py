#!/usr/bin/env python3
"""Times the slide mosaic of per-tile attribution maps on one GPU, by default 2000 windows of
1200 x 1200 at scale 16 with maps uint8 [2000,256,256] on a synthetic slide (blocks of 75 x 75: the ratio 256/75).

  (i)   `mil_attr_mosaic` alone — the launch, with every argument already on the device;
  (ii)  `AttributionMosaic.render` — the host side of a call (refusals, uploads, the white canvas), the tissue thumbnail launch
        (`mil_heatmap_render`) and (i);
  (iii) for comparison, the same picture composed in torch on the device from the same thumbnail: adaptive average pooling of
        the maps in fp32, a table lookup and a float blend scattered into the canvas.  Its bytes may differ from (i)'s by a
        level; the count of differing bytes is reported.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of (i) are the maps
read once plus, per owned pixel, three bytes of tissue read and six bytes written; its rate is printed next to DESIGN.md's
measured stream-copy bandwidth of the box (6.22 TB/s).  `--maps 64` (footprints of one map pixel and less) and `--scale 1200`
(one output pixel per window: the wave-per-pixel form) time the other regimes.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L  # noqa: E402

STREAM_COPY_TBPS = 6.22


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grid", type=int, nargs=2, default=(40, 50), help="windows per axis (default 40 50: 2000 windows)")
    ap.add_argument("--roi", type=int, default=1200)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--maps", type=int, default=256, help="side of a map")
    ap.add_argument("--alpha", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_attr_mosaic.py needs a GPU")
    s, d, (gy, gx), hm = a.roi, a.scale, a.grid, a.maps
    n = s // d
    h, w = gy * s + 2 * d, gx * s + 2 * d + 5
    slide = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    slide.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(1))
    coords = np.asarray([(d + 3 + s * i, d + 5 + s * j) for i in range(gy) for j in range(gx)], dtype=np.int64)
    t = len(coords)
    maps = torch.empty((t, hm, hm), dtype=torch.uint8, device="cuda")
    maps.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(2))
    r = mil_amd.AttributionMosaic(s, d, alpha=a.alpha)
    lib = L.lib()

    # (i): the launch alone, on the thumbnail (ii) composites on
    ht, wt = h // d, w // d
    none = torch.full((4, t), -1, dtype=torch.int16)
    thumb = mil_amd.AttentionMapRenderer(s, d).render_into(torch.full((5, ht, wt, 3), 255, dtype=torch.uint8, device="cuda"), slide,
                                                           coords, none)[0].clone()
    pos = torch.from_numpy(coords // d).to(torch.int32).cuda()
    lut = r.table.cuda()
    heat, tissue = torch.full((ht, wt, 3), 255, dtype=torch.uint8, device="cuda"), thumb.clone()

    def launch():
        L.check(lib.mil_attr_mosaic(maps.data_ptr(), 1, t, hm, hm, n, pos.data_ptr(), lut.data_ptr(), r.alpha_byte, 0, heat.data_ptr(),
                                    tissue.data_ptr(), ht, wt, L.stream_ptr()), "mil_attr_mosaic")

    # (iii): torch on the device
    ar = torch.arange(n, device="cuda")
    oy = (pos[:, 0].long()[:, None, None] + ar[None, :, None]).expand(t, n, n)
    ox = (pos[:, 1].long()[:, None, None] + ar[None, None, :]).expand(t, n, n)
    lutf, al = lut.float(), float(r.alpha_byte)

    def composed():
        v = torch.nn.functional.adaptive_avg_pool2d(maps.float().unsqueeze(1), n).squeeze(1)
        src = lutf[(v + 0.5).floor().clamp_(0, 255).long()]
        out_heat = torch.full((ht, wt, 3), 255, dtype=torch.uint8, device="cuda")
        out_tissue = thumb.clone()
        out_heat[oy, ox] = src.to(torch.uint8)
        blend = (src * al + thumb[oy, ox].float() * (255.0 - al)) / 255.0
        out_tissue[oy, ox] = (blend + 0.5).floor().clamp_(0, 255).to(torch.uint8)
        return out_heat, out_tissue

    times = {"launch": timed(launch, a.warmup, a.reps),
             "render": timed(lambda: r.render(slide, coords, maps), a.warmup, a.reps),
             "torch_composed": timed(composed, a.warmup, a.reps)}
    tissue.copy_(thumb)
    launch()
    got = r.render(slide, coords, maps)
    assert torch.equal(got[0], heat) and torch.equal(got[1], tissue)
    th, tt = composed()
    owned_bytes = t * n * n * 3
    moved = t * hm * hm + t * n * n * 9
    res = {"windows": t, "roi": s, "scale": d, "maps": [t, hm, hm], "block": n, "out_shape": [2, ht, wt, 3],
           "form": "wave" if (-(-hm // n)) ** 2 >= 64 else "thread", "algorithmic_bytes": moved, "warmup": a.warmup, "reps": a.reps,
           "torch_bytes_that_differ": {"heat": int((th != heat).sum()), "on_tissue": int((tt != tissue).sum()), "of": owned_bytes},
           "torch_largest_difference": int(max((th.int() - heat.int()).abs().max(), (tt.int() - tissue.int()).abs().max()))}
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    tbps = moved / statistics.median(times["launch"]) / 1e9
    res["launch"]["TBps_at_median"] = round(tbps, 3)
    res["launch"]["fraction_of_stream_copy"] = round(tbps / STREAM_COPY_TBPS, 3)
    res["torch_composed_over_launch"] = round(res["torch_composed"]["median_ms"] / res["launch"]["median_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
