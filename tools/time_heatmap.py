#!/usr/bin/env python3
"""Times the attention heat-map render of a resident slide on one GPU, by default at the reference's
ceiling: 2500 windows of 1200 x 1200 at scale 16 on a synthetic slide.

  (i)   `mil_heatmap_render` alone — the launch, with every argument already on the device;
  (ii)  `AttentionMapRenderer.render` — (i) plus the host side of a call (indices, refusals, uploads, the white canvas);
  (iii) for comparison, what the picture costs without the kernel: `SlideBag.rois(all)` (the [T,S,S,3] stack the reference's
        create_map takes) followed by torch average pooling to the same thumbnail scale, in slices of `--pool-chunk` windows.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions of (i) and (ii), `--compare-reps` of (iii).
The algorithmic bytes of (i) are T*S*S*3 read + 5*Ht*Wt*3 written; its rate is printed next to DESIGN.md's measured stream-copy
bandwidth of the box (6.22 TB/s).  Prints one JSON line.  A report, not a test: nothing is asserted but that panel 0 without
rectangles agrees with the pooled stack to rounding."""
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
from mil_amd import heatmap as hm  # noqa: E402

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
    ap.add_argument("--grid", type=int, default=50, help="windows per axis (default 50: 2500 windows)")
    ap.add_argument("--roi", type=int, default=1200)
    ap.add_argument("--scale", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--compare-reps", type=int, default=2)
    ap.add_argument("--pool-chunk", type=int, default=50)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_heatmap.py needs a GPU")
    s, d, g = a.roi, a.scale, a.grid
    h, w = g * s + 2 * d, g * s + 2 * d + 5
    assert (3 * w) % 16, "the row pitch must not be a multiple of 16"
    slide = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    slide.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(1))
    coords = np.asarray([(d + 3 + s * i, d + 5 + s * j) for j in range(g) for i in range(g)], dtype=np.int64)
    t = len(coords)
    gen = torch.Generator().manual_seed(2)
    a1, fterm = torch.rand(3, t, generator=gen), torch.randn(t, 80, generator=gen)
    r = mil_amd.AttentionMapRenderer(s, d)
    bag = mil_amd.SlideBag(slide, s, coords=coords)

    # (i): the launch alone
    ht, wt = h // d, w // d
    canvas = torch.full((5, ht, wt, 3), 255, dtype=torch.uint8, device="cuda")
    cc = torch.from_numpy(coords)
    off = ((cc[:, 0] * w + cc[:, 1]) * 3).cuda()
    pos = (cc // d).to(torch.int32).cuda()
    jidx, fidx = hm.attention_indices(a1).cuda(), hm.feature_indices(fterm).cuda()
    jet, vir = torch.from_numpy(hm.JET105.copy()).cuda(), torch.from_numpy(hm.VIRIDIS256.copy()).cuda()
    lib = L.lib()

    def launch():
        L.check(lib.mil_heatmap_render(slide.data_ptr(), slide.numel(), off.data_ptr(), 3 * w, t, s, d, pos.data_ptr(),
                                       jidx.data_ptr(), fidx.data_ptr(), jet.data_ptr(), vir.data_ptr(), 16, 77, 230,
                                       canvas.data_ptr(), ht, wt, L.stream_ptr()), "mil_heatmap_render")

    def pooled():
        out = torch.empty((t, s // d, s // d, 3), dtype=torch.float32, device="cuda")
        for i in range(0, t, a.pool_chunk):
            rois = bag.rois(np.arange(i, min(i + a.pool_chunk, t)))
            out[i:i + len(rois)] = torch.nn.functional.avg_pool2d(rois.permute(0, 3, 1, 2).float(), d).permute(0, 2, 3, 1)
        return out

    times = {"launch": timed(launch, a.warmup, a.reps),
             "render": timed(lambda: r.render(slide, coords, a1, fterm), a.warmup, a.reps),
             "rois_then_avg_pool": timed(pooled, 1, a.compare_reps)}
    plain = r.render_into(torch.zeros_like(canvas), slide, coords, torch.full((4, t), -1, dtype=torch.int16))
    y, x = int(pos[-1, 0]), int(pos[-1, 1])
    n = s // d
    assert float((plain[0, y:y + n, x:x + n].float() - pooled()[-1]).abs().max()) <= 0.5 + 1e-3

    moved = t * s * s * 3 + 5 * ht * wt * 3
    res = {"windows": t, "roi": s, "scale": d, "row_pitch": 3 * w, "out_shape": [5, ht, wt, 3], "algorithmic_bytes": moved,
           "reps": a.reps, "compare_reps": a.compare_reps}
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    tbps = moved / statistics.median(times["launch"]) / 1e9
    res["launch"]["TBps_at_median"] = round(tbps, 3)
    res["launch"]["fraction_of_stream_copy"] = round(tbps / STREAM_COPY_TBPS, 3)
    res["rois_then_avg_pool_over_render"] = round(res["rois_then_avg_pool"]["median_ms"] / res["render"]["median_ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
