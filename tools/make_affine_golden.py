#!/usr/bin/env python3
"""Writes tests/golden/affine_u8.npz, the fixture of the affine tests, with Pillow itself (the tests read it; Pillow need not be
installed where they run).  torchvision is not needed: what its PIL backend asks of Pillow for `RandomAffine` / `RandomRotation`
is asked of Pillow here,

    Image.fromarray(img).transform((ow, oh), Image.AFFINE, m, Image.BILINEAR, fillcolor=fill)

with m from torchvision's inverse-matrix formula (`mil_amd.affine_matrix`) or an exact quarter turn.

  p17_*   three planar tiles of 17 x 23 (h x w) random bytes, random angle / scale / shear / translation, fill 0
  p33_*   ONE tile of 33 x 33 under five maps: identity, the three quarter turns, a map that lands wholly outside; fill (1, 2, 3)
  p64_*   ONE tile of 64 x 64 under two random maps; fill (255, 255, 255)
  slide, coords, win_m, win_fill, win_out
          a slide of 70 x 90 (H x W) and six windows of 24 pixels — the four slide corners and two inside — rotated by up to 45
          degrees about their centres in WINDOW coordinates; Pillow transforms the whole slide with the window's origin added to
          a2 (col) and a5 (row): the corners leave the slide (fill), the inner windows read their neighbourhood
  *_in uint8 [k,3,h,w], *_m float64 [n,6] (tile i of n uses source i mod k), *_fill uint8 [3], *_out uint8 [n,3,h,w] Pillow's bytes;
  win_out uint8 [6,24,24,3].  The 33, 64 and slide sources hold multiples of 17 only, so that the file stays small.

    python tools/make_affine_golden.py          (written with Pillow 12.2.0)
"""
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mil_amd  # noqa: E402

WIN = 24


def pillow(img, m, out_hw, fill):
    """uint8 [H,W,3] through Pillow -> uint8 [oh,ow,3]."""
    oh, ow = out_hw
    out = Image.fromarray(np.ascontiguousarray(img), "RGB").transform((ow, oh), Image.AFFINE, tuple(float(v) for v in m),
                                                                      Image.BILINEAR, fillcolor=tuple(int(v) for v in fill))
    return np.asarray(out)


def planar(tiles, ms, fill):
    k = len(tiles)
    return np.stack([np.moveaxis(pillow(np.moveaxis(tiles[i % k], 0, -1), m, tiles.shape[2:], fill), -1, 0) for i, m in enumerate(ms)])


def random_matrix(rng, h, w):
    return mil_amd.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))),
                                 rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


def main():
    rng = np.random.default_rng(20262)
    z = {}
    t17 = rng.integers(0, 256, (3, 3, 17, 23), dtype=np.uint8)
    m17 = np.array([random_matrix(rng, 17, 23) for _ in range(3)])
    z.update(p17_in=t17, p17_m=m17, p17_fill=np.zeros(3, np.uint8), p17_out=planar(t17, m17, (0, 0, 0)))
    t33 = (rng.integers(0, 16, (1, 3, 33, 33)) * 17).astype(np.uint8)
    m33 = np.array([mil_amd.quarter_turn_matrix(k, 33) for k in range(4)] + [[1.0, 0.0, 40.0, 0.0, 1.0, -7.5]])
    z.update(p33_in=t33, p33_m=m33, p33_fill=np.array([1, 2, 3], np.uint8), p33_out=planar(t33, m33, (1, 2, 3)))
    t64 = (rng.integers(0, 16, (1, 3, 64, 64)) * 17).astype(np.uint8)
    m64 = np.array([random_matrix(rng, 64, 64) for _ in range(2)])
    z.update(p64_in=t64, p64_m=m64, p64_fill=np.full(3, 255, np.uint8), p64_out=planar(t64, m64, (255, 255, 255)))

    slide = (rng.integers(0, 16, (70, 90, 3)) * 17).astype(np.uint8)
    coords = np.array([(0, 0), (0, 90 - WIN), (70 - WIN, 0), (70 - WIN, 90 - WIN), (20, 30), (23, 41)], np.int64)
    angles = [45.0, -30.0, 17.5, 200.0, 45.0, -8.0]
    wm = np.array([mil_amd.affine_matrix((WIN * 0.5, WIN * 0.5), a, (0, 0), 1.0, (0.0, 0.0)) for a in angles])
    fill = np.array([255, 255, 255], np.uint8)
    wout = []
    for (r, c), m in zip(coords, wm):
        mm = m.copy()
        mm[2] = mm[2] + np.float64(c)
        mm[5] = mm[5] + np.float64(r)
        wout.append(pillow(slide, mm, (WIN, WIN), fill))
    z.update(slide=slide, coords=coords, win_m=wm, win_fill=fill, win_out=np.stack(wout))
    for k in ("p17", "p33", "p64"):
        print(k, z[k + "_out"].shape, "bytes that differ from the source:",
              int((z[k + "_out"] != z[k + "_in"][np.arange(len(z[k + "_m"])) % len(z[k + "_in"])]).sum()))
    print("windows: fill pixels per window", [(w == 255).all(axis=-1).sum() for w in wout])
    path = os.path.join(ROOT, "tests", "golden", "affine_u8.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
