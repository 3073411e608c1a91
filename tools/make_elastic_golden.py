#!/usr/bin/env python3
"""Writes tests/golden/elastic_u8.npz, the fixture of the elastic-deformation tests, from the numpy restatement of the byte
contract (tests/elastic_reference.py).  No library computes these bytes: the fixture pins the restatement
(tests/test_cpu_elastic.py) and the kernel (tests/test_gpu_elastic.py) to one recorded state of it, and the CPU tests tie the
restatement to Pillow (zero lattices) and to scipy (identity matrix) separately.

  p17_*   three planar tiles of 17 x 23 (h x w) random bytes, cells (3, 2): random angle / scale / shear / translation and a
          lattice clip(1.5 * randn, -2, 2); fill 0
  p33_*   ONE tile of 33 x 33, cells 4, under three maps: the identity with a random lattice, a random map with a random
          lattice, a random map with a lattice of zeros (the affine transform's bytes); fill (1, 2, 3)
  slide, coords, win_m, win_ctrl, win_fill, win_out
          a slide of 70 x 90 (H x W) and four windows of 24 pixels, cells 4 — two slide corners and two inside — rotated about
          their centres in WINDOW coordinates and deformed with lattices clip(3 * randn, -6, 6) while reading the whole slide: the
          corners leave the slide (fill), the inner windows read their neighbourhood
  *_in uint8 [k,3,h,w], *_m float64 [n,6] (tile i of n uses source i mod k), *_ctrl float64 [n,2,gy+3,gx+3], *_fill uint8 [3],
  *_out uint8 [n,3,h,w]; win_out uint8 [4,24,24,3].  The 33 and slide sources hold multiples of 17 only, so that the file stays
  small.

    python tools/make_elastic_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import affine_reference as ar  # noqa: E402
import elastic_reference as er  # noqa: E402

WIN = 24


def random_matrix(rng, h, w):
    return ar.affine_matrix((w * 0.5, h * 0.5), rng.uniform(-180, 180), (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))),
                            rng.uniform(0.5, 2.0), (rng.uniform(-20, 20), rng.uniform(-20, 20)))


def lattice(rng, n, gy, gx, sigma, clip):
    return np.clip(sigma * rng.standard_normal((n, 2, gy + 3, gx + 3)), -clip, clip)


def main():
    rng = np.random.default_rng(20263)
    z = {}
    t17 = rng.integers(0, 256, (3, 3, 17, 23), dtype=np.uint8)
    m17 = np.array([random_matrix(rng, 17, 23) for _ in range(3)])
    c17 = lattice(rng, 3, 3, 2, 1.5, 2.0)
    z.update(p17_in=t17, p17_m=m17, p17_ctrl=c17, p17_fill=np.zeros(3, np.uint8), p17_out=er.transform_planar(t17, m17, c17, None, 0))
    t33 = (rng.integers(0, 16, (1, 3, 33, 33)) * 17).astype(np.uint8)
    m33 = np.array([list(er.IDENTITY), random_matrix(rng, 33, 33), random_matrix(rng, 33, 33)])
    c33 = lattice(rng, 3, 4, 4, 1.5, 2.0)
    c33[2] = 0.0
    z.update(p33_in=t33, p33_m=m33, p33_ctrl=c33, p33_fill=np.array([1, 2, 3], np.uint8),
             p33_out=er.transform_planar(t33[[0, 0, 0]], m33, c33, None, (1, 2, 3)))

    slide = (rng.integers(0, 16, (70, 90, 3)) * 17).astype(np.uint8)
    coords = np.array([(0, 0), (70 - WIN, 90 - WIN), (20, 30), (23, 41)], np.int64)
    wm = np.array([ar.affine_matrix((WIN * 0.5, WIN * 0.5), a, (0, 0), 1.0, (0.0, 0.0)) for a in (45.0, 200.0, -30.0, 17.5)])
    wc = lattice(rng, 4, 4, 4, 3.0, 6.0)
    fill = np.array([255, 255, 255], np.uint8)
    wout = er.slide_windows(slide, coords, wm, wc, WIN, fill)
    z.update(slide=slide, coords=coords, win_m=wm, win_ctrl=wc, win_fill=fill, win_out=wout)
    print("p33: tile 2 (zero lattice) equals the affine restatement:",
          bool(np.array_equal(z["p33_out"][2], np.moveaxis(ar.transform(np.moveaxis(t33[0], 0, -1), m33[2], None, (1, 2, 3)), -1, 0))))
    print("windows: fill pixels per window", [int((w == 255).all(axis=-1).sum()) for w in wout])
    path = os.path.join(ROOT, "tests", "golden", "elastic_u8.npz")
    np.savez_compressed(path, **z)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
