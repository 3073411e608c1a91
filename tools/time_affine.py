#!/usr/bin/env python3
"""Times the affine augmentation on one GPU:

  (i)   the `U8Tiles` path, by default 500 tiles of 300 x 300 with one random matrix per tile (rotation by any angle, scale
        0.8-1.25, shear +-5 degrees, translation up to a tenth of the tile): the `mil_affine_u8` launch alone, every argument
        already on the device; `RandomAffine.apply`, which adds the host side of a call (checks, the upload of the matrices, the
        output allocation); and the launch with quarter turns only (integer matrices: the taps coincide);
  (ii)  the slide path, by default 500 windows of 1200 x 1200 at random places of a 30000 x 30000 slide (2.7 GB: byte offsets
        beyond 2^31), resized to 300 x 300: one `ops.affine_windows_u8` call on a chunk of AFFINE_CHUNK windows;
        `TilePreprocessor.from_slide(..., affine=m)` as a whole; and beside it the existing `from_slide` call for the same windows
        without `affine`.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes of a transform are one
read of as many source pixels as it writes and one write (the four taps of neighbouring pixels share cache lines); the rate is
printed next to the 8 TB/s HBM peak.  The arithmetic is fp64 (about 55 instructions per pixel, none an FMA).  Prints one
JSON line.  A report, not a test."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import _lib as L, ops  # noqa: E402
from mil_amd import preprocess as pp  # noqa: E402

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=500)
    ap.add_argument("--resolution", type=int, default=300)
    ap.add_argument("--windows", type=int, default=500)
    ap.add_argument("--roi-size", type=int, default=1200)
    ap.add_argument("--slide", type=int, default=30000, help="side of the square slide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_affine.py needs a GPU")
    lib = L.lib()
    times = {}
    aug = mil_amd.RandomAffine(180, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5, fill=(255, 255, 255))
    turns = mil_amd.RandomAffine(0, quarter_turns=True)

    # (i) planar tiles
    t, r = a.tiles, a.resolution
    src = torch.randint(0, 256, (t, 3, r, r), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    m = aug.draw_params(t, r, torch.Generator().manual_seed(1))
    mq = turns.draw_params(t, r, torch.Generator().manual_seed(1))
    md, mqd = m.cuda(), mq.cuda()
    fill = ops.affine_fill(aug.fill)

    def launch(mat):
        return lambda: L.check(lib.mil_affine_u8(src.data_ptr(), 3 * r * r, r, 1, r * r, r, r, dst.data_ptr(), 1, r * r, r, r,
                                                 mat.data_ptr(), fill, t, L.stream_ptr()), "mil_affine_u8")

    times["tiles_launch"] = timed(launch(md), a.warmup, a.reps)
    times["tiles_launch_quarter_turns"] = timed(launch(mqd), a.warmup, a.reps)
    handle = mil_amd.U8Tiles(src)
    times["tiles_apply"] = timed(lambda: aug.apply(handle, m), a.warmup, a.reps)
    del dst, handle, src

    # (ii) slide windows
    n, s, side = a.windows, a.roi_size, a.slide
    slide = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(2)
    coords = torch.randint(0, side - s + 1, (n, 2), generator=g)
    mw = aug.draw_params(n, s, g)
    prep = mil_amd.TilePreprocessor(s, r, pad=100, device="cuda")
    params = prep.draw_params(n, g)
    k = min(n, pp.AFFINE_CHUNK)
    times["windows_affine_one_chunk"] = timed(lambda: ops.affine_windows_u8(slide, coords[:k], mw[:k], aug.fill, s), a.warmup, a.reps)
    times["from_slide_with_affine"] = timed(lambda: prep.from_slide(slide, coords, params, "u8", affine=mw, affine_fill=aug.fill),
                                            a.warmup, a.reps)
    times["from_slide_without_affine"] = timed(lambda: prep.from_slide(slide, coords, params, "u8"), a.warmup, a.reps)

    res = {"tiles": t, "resolution": r, "windows": n, "roi_size": s, "slide_bytes": slide.numel(), "chunk": k, "reps": a.reps,
           "library": os.path.basename(mil_amd.LIB_PATH)}
    for key, v in times.items():
        res[key] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for key, moved in (("tiles_launch", 2 * t * 3 * r * r), ("tiles_launch_quarter_turns", 2 * t * 3 * r * r),
                       ("windows_affine_one_chunk", 2 * k * 3 * s * s)):
        tbps = moved / statistics.median(times[key]) / 1e9
        res[key].update(algorithmic_bytes=moved, TBps_at_median=round(tbps, 3), fraction_of_hbm_peak=round(tbps / HBM_PEAK_TBPS, 4),
                        Gpixel_per_s=round(moved / 6 / statistics.median(times[key]) / 1e6, 2))
    res["affine_over_plain_from_slide"] = round(res["from_slide_with_affine"]["median_ms"] / res["from_slide_without_affine"]["median_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
