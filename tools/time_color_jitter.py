#!/usr/bin/env python3
"""Times the colour jitter of a bag of uint8 tiles on one GPU, by default 500 tiles of 300 x 300 with
the full four-op chain in per-tile random order, beside the pre-processing call it follows:

  (i)   `mil_color_jitter_u8` alone — the two launches and the workspace memset, every argument already on the device; also
        with one op at a time (what each op costs) and with the chain without contrast (no pass A work);
  (ii)  `ColorJitter.apply` — (i) plus the host side of a call (parameter checks, three uploads, the workspace);
  (iii) `TilePreprocessor.from_slide(..., out="u8")` for as many 1200 x 1200 windows of a synthetic slide: the call whose output
        the jitter reads and writes.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of (i) are one read
and one write of the tile stack (pass A's second read comes on top where contrast is active); its rate is printed next to the
8 TB/s HBM peak.  Prints one JSON line.  A report, not a test."""
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

HBM_PEAK_TBPS = 8.0


def timed(f, warmup, reps, before=None):
    out = []
    for it in range(warmup + reps):
        if before is not None:
            before()                      # untimed: every repetition jitters the same bytes
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
    ap.add_argument("--tiles", type=int, default=500)
    ap.add_argument("--resolution", type=int, default=300)
    ap.add_argument("--roi", type=int, default=1200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_color_jitter.py needs a GPU")
    t, r, s = a.tiles, a.resolution, a.roi
    jit = mil_amd.ColorJitter(brightness=0.2, contrast=0.1, saturation=0.05, hue=0.02)
    gen = torch.Generator().manual_seed(1)
    p = jit.draw_params(t, gen)
    src = torch.empty((t, 3, r, r), dtype=torch.uint8, device="cuda")
    src.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(2))
    work = src.clone()
    lsum = torch.empty(t, dtype=torch.int32, device="cuda")
    factors, shift = p.factors.cuda(), p.hue_shift.cuda()
    lib = L.lib()

    def launcher(order):
        order = order.cuda()

        def launch():
            L.check(lib.mil_color_jitter_u8(work.data_ptr(), order.data_ptr(), factors.data_ptr(), shift.data_ptr(),
                                            lsum.data_ptr(), t, r, L.stream_ptr()), "mil_color_jitter_u8")
        return launch

    def only(op):
        o = torch.full((t, 4), -1, dtype=torch.int32)
        o[:, 0] = op
        return o

    no_contrast = p.order.clone()
    no_contrast[no_contrast == 1] = -1
    routes = {"launch_full_chain": launcher(p.order), "launch_without_contrast": launcher(no_contrast),
              "launch_brightness_only": launcher(only(0)), "launch_contrast_only": launcher(only(1)),
              "launch_saturation_only": launcher(only(2)), "launch_hue_only": launcher(only(3)),
              "launch_no_op": launcher(only(-1))}

    def restore():
        work.copy_(src)

    times = {k: timed(f, a.warmup, a.reps, restore) for k, f in routes.items()}
    handle = mil_amd.U8Tiles(work)
    times["apply"] = timed(lambda: jit.apply(handle, p), a.warmup, a.reps, restore)

    # (iii): the pre-processing call for as many windows of a synthetic slide (pitch no multiple of 16)
    g = int(np.ceil(np.sqrt(t)))
    h, w = g * s + 3, g * s + 7
    slide = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
    slide.view(-1).random_(0, 256, generator=torch.Generator("cuda").manual_seed(3))
    coords = np.asarray([(1 + s * i, 5 + s * j) for j in range(g) for i in range(g)], dtype=np.int64)[:t]
    prep = mil_amd.TilePreprocessor(s, r)
    pp = prep.draw_params(t, gen)
    times["from_slide_u8"] = timed(lambda: prep.from_slide(slide, coords, pp, out="u8"), a.warmup, a.reps)
    times["from_slide_u8_jitter"] = timed(lambda: prep.from_slide(slide, coords, pp, out="u8", jitter=p), a.warmup, a.reps)

    moved = 2 * t * 3 * r * r
    res = {"tiles": t, "resolution": r, "roi": s, "algorithmic_bytes": moved, "reps": a.reps}
    for k, v in times.items():
        res[k] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    tbps = moved / statistics.median(times["launch_full_chain"]) / 1e9
    res["launch_full_chain"]["TBps_at_median"] = round(tbps, 3)
    res["launch_full_chain"]["fraction_of_hbm_peak"] = round(tbps / HBM_PEAK_TBPS, 4)
    res["jitter_over_from_slide"] = round(res["launch_full_chain"]["median_ms"] / res["from_slide_u8"]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
