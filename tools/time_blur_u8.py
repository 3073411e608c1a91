#!/usr/bin/env python3
"""Times Pillow's Gaussian blur for uint8 tiles on one GPU:

  (i)   `mil_gaussian_blur_u8` alone on 500 tiles of 300 x 300 and on 256 tiles of 256 x 256, at sigma 0.5, 2 and 8 (box radius
        0, 1 and 7: the three halo sizes), every argument already on the device; `mil_amd.gaussian_blur_u8`, which adds the host
        side of a call (the sigmas to six integers per tile, their upload, the output's allocation); beside them the two in-place
        passes the blur follows in the train chain, the stain map and the colour jitter, on the same 500 tiles;
  (ii)  `TilePreprocessor.from_slide` on `--windows` windows of a resident slide, with and without `blur=`.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of (i) are one read and
one write of the stack; its rate is printed next to the 8 TB/s HBM peak.  Prints one JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L, ops  # noqa: E402
from mil_amd import color_jitter as cj, stain as st  # noqa: E402

HBM_PEAK_TBPS = 8.0
SIGMAS = (0.5, 2.0, 8.0)


def timed(f, warmup, reps, before=None):
    out = []
    for it in range(warmup + reps):
        if before is not None:
            before()
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
    ap.add_argument("--windows", type=int, default=256)
    ap.add_argument("--roi-size", type=int, default=1200)
    ap.add_argument("--resolution", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_blur_u8.py needs a GPU")
    lib = L.lib()
    res = {"reps": a.reps, "library": os.path.basename(mil_amd.LIB_PATH)}
    g = torch.Generator(device="cuda").manual_seed(1)

    # (i) the launch alone
    for t, r in ((500, 300), (256, 256)):
        src = torch.randint(0, 256, (t, 3, r, r), dtype=torch.uint8, device="cuda", generator=g)
        dst = torch.empty_like(src)
        tiles = mil_amd.U8Tiles(src)
        moved = 2 * src.numel()
        for sigma in SIGMAS:
            p = ops.box_blur_params([sigma] * t).cuda()
            v = timed(lambda: L.check(lib.mil_gaussian_blur_u8(src.data_ptr(), dst.data_ptr(), p.data_ptr(), 3 * t, 3, r, r, L.stream_ptr()),
                                      "mil_gaussian_blur_u8"), a.warmup, a.reps)
            row = summary(v)
            row["box_radius"] = int(p[0, 0])
            row["TBps_at_median"] = round(moved / statistics.median(v) / 1e9, 3)
            row["fraction_of_hbm_peak"] = round(row["TBps_at_median"] / HBM_PEAK_TBPS, 4)
            res[f"launch_{t}x{r}_sigma{sigma:g}"] = row
            res[f"call_{t}x{r}_sigma{sigma:g}"] = summary(timed(lambda: mil_amd.gaussian_blur_u8(tiles, sigma), a.warmup, a.reps))
        # sigmas as the augmentation draws them: half the tiles untouched, the rest in [0.1, 2]
        drawn = mil_amd.GaussianBlurU8((0.1, 2.0), 0.5).draw_params(t, torch.Generator().manual_seed(2))
        p = ops.box_blur_params(drawn).cuda()
        res[f"launch_{t}x{r}_drawn"] = summary(timed(lambda: L.check(lib.mil_gaussian_blur_u8(
            src.data_ptr(), dst.data_ptr(), p.data_ptr(), 3 * t, 3, r, r, L.stream_ptr()), "mil_gaussian_blur_u8"), a.warmup, a.reps))
        if (t, r) == (500, 300):
            # the two passes it sits next to, on the same stack (they work in place; the bytes do not change their time much)
            sj = mil_amd.StainJitter(0.05, 0.01)
            aff = sj.affine(sj.draw_params(t, torch.Generator().manual_seed(1)))
            work = mil_amd.U8Tiles(src.clone())
            res["stain_apply_500x300"] = summary(timed(lambda: st.apply_stain(work, aff), a.warmup, a.reps))
            jit = mil_amd.ColorJitter(0.2, 0.1, 0.05, 0.02)
            jp = jit.draw_params(t, torch.Generator().manual_seed(3))
            res["color_jitter_apply_500x300"] = summary(timed(lambda: cj.apply_jitter(work, jp), a.warmup, a.reps))
            del work
        del src, dst, tiles

    # (ii) the chain on a resident slide
    n, s = a.windows, a.roi_size
    side = int(np.ceil(np.sqrt(n)))
    slide = torch.randint(0, 256, (side * s, side * s, 3), dtype=torch.uint8, device="cuda", generator=g)
    coords = np.asarray([(i // side * s, i % side * s) for i in range(n)], dtype=np.int64)
    prep = mil_amd.TilePreprocessor(s, a.resolution, pad=100, device="cuda")
    params = prep.draw_params(n, torch.Generator().manual_seed(4))
    sig = mil_amd.GaussianBlurU8((0.1, 2.0), 0.5).draw_params(n, torch.Generator().manual_seed(5))
    res["from_slide"] = {"windows": n, "roi_size": s, "resolution": a.resolution,
                         "without_blur": summary(timed(lambda: prep.from_slide(slide, coords, params, "u8"), a.warmup, a.reps)),
                         "with_blur": summary(timed(lambda: prep.from_slide(slide, coords, params, "u8", blur=sig), a.warmup, a.reps))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
