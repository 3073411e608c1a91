#!/usr/bin/env python3
"""Times the elastic deformation fused into the affine resampling on one GPU, each route beside the
matching route of the affine transform alone (the rows of tools/time_affine.py), in one session:

  (i)   the `U8Tiles` path, by default 500 tiles of 300 x 300 with one random matrix per tile (rotation by any angle, scale
        0.8-1.25, shear +-5 degrees, translation up to a tenth of the tile) and one control lattice of 8 x 8 cells per tile
        (magnitude 4 pixels, clipped at 8): the `mil_affine_elastic_u8` launch alone, every argument already on the device,
        beside the `mil_affine_u8` launch on the same tiles and matrices; the same launch with lattices of zeros (the affine
        transform's bytes through the elastic kernel); `ElasticDeform.apply` with the host side of a call;
  (ii)  the slide path, by default 500 windows of 1200 x 1200 at random places of a 30000 x 30000 slide (2.7 GB), resized to
        300 x 300: one `ops.elastic_windows_u8` call on a chunk of AFFINE_CHUNK windows beside `ops.affine_windows_u8` on the same
        chunk; `TilePreprocessor.from_slide(..., affine=m, elastic=c)` as a whole beside `from_slide(..., affine=m)`.

Device events around each route, `--warmup` untimed and `--reps` timed repetitions.  The algorithmic bytes are those of the affine
transform (one read of as many source pixels as are written, one write); the lattice and the tables are a few KB per tile.
Prints one JSON line.  A report, not a test."""
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
    ap.add_argument("--cells", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_elastic.py needs a GPU")
    lib = L.lib()
    times = {}
    aug = mil_amd.RandomAffine(180, translate=(0.1, 0.1), scale=(0.8, 1.25), shear=5, fill=(255, 255, 255))
    deform = mil_amd.ElasticDeform(4.0, cells=a.cells, fill=(255, 255, 255))
    g8 = a.cells + 3

    # (i) planar tiles
    t, r = a.tiles, a.resolution
    src = torch.randint(0, 256, (t, 3, r, r), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    m = aug.draw_params(t, r, torch.Generator().manual_seed(1))
    c = deform.draw_params(t, r, torch.Generator().manual_seed(3))
    md, cd, zd = m.cuda(), c.cuda(), torch.zeros_like(c).cuda()
    iy, wy = (x.cuda() for x in ops.elastic_tables(r, a.cells))
    fill = ops.affine_fill(aug.fill)

    def affine_launch():
        L.check(lib.mil_affine_u8(src.data_ptr(), 3 * r * r, r, 1, r * r, r, r, dst.data_ptr(), 1, r * r, r, r, md.data_ptr(), fill, t,
                                  L.stream_ptr()), "mil_affine_u8")

    def elastic_launch(lat):
        return lambda: L.check(lib.mil_affine_elastic_u8(src.data_ptr(), 3 * r * r, r, 1, r * r, r, r, dst.data_ptr(), 1, r * r, r, r,
                                                         md.data_ptr(), fill, t, lat.data_ptr(), g8, g8, iy.data_ptr(), wy.data_ptr(),
                                                         iy.data_ptr(), wy.data_ptr(), L.stream_ptr()), "mil_affine_elastic_u8")

    times["tiles_affine_launch"] = timed(affine_launch, a.warmup, a.reps)
    times["tiles_elastic_launch"] = timed(elastic_launch(cd), a.warmup, a.reps)
    times["tiles_elastic_launch_zero_lattice"] = timed(elastic_launch(zd), a.warmup, a.reps)
    handle = mil_amd.U8Tiles(src)
    times["tiles_elastic_apply"] = timed(lambda: deform.apply(handle, c, m), a.warmup, a.reps)
    del dst, handle, src

    # (ii) slide windows
    n, s, side = a.windows, a.roi_size, a.slide
    slide = torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, device="cuda")
    g = torch.Generator().manual_seed(2)
    coords = torch.randint(0, side - s + 1, (n, 2), generator=g)
    mw = aug.draw_params(n, s, g)
    prep = mil_amd.TilePreprocessor(s, r, pad=100, device="cuda")
    params = prep.draw_params(n, g)
    cw = deform.draw_params(n, s, g)
    k = min(n, pp.AFFINE_CHUNK)
    times["windows_affine_one_chunk"] = timed(lambda: ops.affine_windows_u8(slide, coords[:k], mw[:k], aug.fill, s), a.warmup, a.reps)
    times["windows_elastic_one_chunk"] = timed(lambda: ops.elastic_windows_u8(slide, coords[:k], mw[:k], cw[:k], aug.fill, s),
                                               a.warmup, a.reps)
    times["from_slide_with_affine"] = timed(lambda: prep.from_slide(slide, coords, params, "u8", affine=mw, affine_fill=aug.fill),
                                            a.warmup, a.reps)
    times["from_slide_with_affine_and_elastic"] = timed(
        lambda: prep.from_slide(slide, coords, params, "u8", affine=mw, affine_fill=aug.fill, elastic=cw), a.warmup, a.reps)

    res = {"tiles": t, "resolution": r, "windows": n, "roi_size": s, "cells": a.cells, "slide_bytes": slide.numel(), "chunk": k,
           "reps": a.reps, "library": os.path.basename(mil_amd.LIB_PATH)}
    for key, v in times.items():
        res[key] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for key, pixels in (("tiles_affine_launch", t * r * r), ("tiles_elastic_launch", t * r * r),
                        ("tiles_elastic_launch_zero_lattice", t * r * r), ("windows_affine_one_chunk", k * s * s),
                        ("windows_elastic_one_chunk", k * s * s)):
        res[key].update(algorithmic_bytes=6 * pixels, Gpixel_per_s=round(pixels / statistics.median(times[key]) / 1e6, 2))
    for num, den in (("tiles_elastic_launch", "tiles_affine_launch"), ("windows_elastic_one_chunk", "windows_affine_one_chunk"),
                     ("from_slide_with_affine_and_elastic", "from_slide_with_affine")):
        res[num + "_over_affine"] = round(res[num]["median_ms"] / res[den]["median_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
