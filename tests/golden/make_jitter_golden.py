#!/usr/bin/env python3
"""Fixture of the colour-jitter tests, produced by Pillow itself (the tests read it; Pillow need not be installed where they
run).  torchvision is not needed: what its PIL backend asks of Pillow for `ColorJitter` (RoiBuilder.py:200) is asked of Pillow
here, op by op, in the order `ColorJitter.forward` applies `fn_idx`:

    adjust_brightness   ImageEnhance.Brightness(img).enhance(f)
    adjust_contrast     ImageEnhance.Contrast(img).enhance(f)
    adjust_saturation   ImageEnhance.Color(img).enhance(f)
    adjust_hue          h, s, v = img.convert("HSV").split(); h = (h + shift) mod 256; merge("HSV", ...).convert("RGB")
                        with shift = int(hue_factor * 255) mod 256 (torchvision adds np.uint8(hue_factor * 255) to a uint8 array)

  jitter_chain.npz   per group g in (19, 32, 2, 1): in_g uint8 [T,3,g,g] planar tiles, order_g int32 [T,4] (op codes 0 brightness,
                     1 contrast, 2 saturation, 3 hue; -1 = no op), factors_g float32 [T,3], shift_g int32 [T], out_g = Pillow's bytes
      19   24 tiles of random bytes, one per order of the four ops (19 * 19 is odd: the planes of a tile are misaligned)
      32   8 special tiles: constant, black, white, grey (s == 0) pixels, factors exactly 1.0, 0.0 and 2.0 (the clip branch), hue
           shifts 0 and 251, one / two / three ops switched off
      2, 1 two 2 x 2 tiles and one 1 x 1 tile

    python tests/golden/make_jitter_golden.py          (written with Pillow 12.2.0)
"""
import itertools
import os

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))


def pillow_jitter(tile, order, factors, shift):
    """One planar uint8 [3,R,R] tile through Pillow; the factors are the float32 values the fixture stores."""
    img = Image.fromarray(np.ascontiguousarray(np.moveaxis(tile, 0, -1)), "RGB")
    fb, fc, fs = (float(np.float32(f)) for f in factors)
    for op in order:
        if op == 0:
            img = ImageEnhance.Brightness(img).enhance(fb)
        elif op == 1:
            img = ImageEnhance.Contrast(img).enhance(fc)
        elif op == 2:
            img = ImageEnhance.Color(img).enhance(fs)
        elif op == 3:
            h, s, v = img.convert("HSV").split()
            nh = ((np.asarray(h).astype(np.int64) + int(shift)) % 256).astype(np.uint8)
            img = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
        else:
            assert op == -1, op
    return np.ascontiguousarray(np.moveaxis(np.asarray(img), -1, 0))


def draw(rng, n):
    """Factors in the ranges of the reference's line (0.2, 0.1, 0.05) and the shifts of hue = 0.02."""
    f = np.stack([rng.uniform(0.8, 1.2, n), rng.uniform(0.9, 1.1, n), rng.uniform(0.95, 1.05, n)], axis=1).astype(np.float32)
    shift = np.array([int(h * 255) % 256 for h in rng.uniform(-0.02, 0.02, n)], dtype=np.int32)
    return f, shift


def group_19(rng):
    order = np.array(list(itertools.permutations(range(4))), dtype=np.int32)
    tiles = rng.integers(0, 256, (24, 3, 19, 19), dtype=np.uint8)
    f, shift = draw(rng, 24)
    shift[:4] = [0, 251, 255, 5]
    return tiles, order, f, shift


def group_32(rng):
    def noise():
        return rng.integers(0, 256, (3, 32, 32), dtype=np.uint8)

    const = np.empty((3, 32, 32), np.uint8)
    const[0], const[1], const[2] = 77, 130, 200
    grey = noise()
    mask = rng.random((32, 32)) < 0.5
    grey[1][mask], grey[2][mask] = grey[0][mask], grey[0][mask]                 # s == 0 on half of the pixels
    rows = [
        (const, (1, 0, 2, 3), (1.2, 0.9, 1.05), 251),
        (np.zeros((3, 32, 32), np.uint8), (3, 2, 1, 0), (0.8, 1.1, 0.95), 0),
        (np.full((3, 32, 32), 255, np.uint8), (0, 1, 3, 2), (1.2, 1.1, 1.05), 5),
        (grey, (3, -1, -1, -1), (1.0, 1.0, 1.0), 0),                            # three ops off; the HSV round trip alone
        (noise(), (2, 0, 1, 3), (1.0, 1.0, 1.0), 251),                          # factors exactly 1
        (noise(), (2, 1, -1, -1), (1.0, 0.0, 0.0), 0),                          # factors 0: grey, then the mean; two ops off
        (noise(), (1, 2, 0, -1), (2.0, 2.0, 2.0), 0),                           # the clip branch; hue off
        (grey.copy(), (0, -1, 3, 1), (0.85, 1.07, 1.0), 128),                   # a gap in the order; saturation off
    ]
    return (np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], np.int32), np.array([r[2] for r in rows], np.float32),
            np.array([r[3] for r in rows], np.int32))


def group_small(rng, n, size, orders):
    tiles = rng.integers(0, 256, (n, 3, size, size), dtype=np.uint8)
    f, shift = draw(rng, n)
    return tiles, np.array(orders, np.int32), f, shift


def main():
    rng = np.random.default_rng(20261)
    groups = {"19": group_19(rng), "32": group_32(rng), "2": group_small(rng, 2, 2, [(0, 1, 2, 3), (3, 1, 0, 2)]),
              "1": group_small(rng, 1, 1, [(2, 3, 1, 0)])}
    arrays = {}
    for g, (tiles, order, f, shift) in groups.items():
        out = np.stack([pillow_jitter(t, o, ff, s) for t, o, ff, s in zip(tiles, order, f, shift)])
        assert out.shape == tiles.shape and out.dtype == np.uint8
        arrays.update({f"in_{g}": tiles, f"order_{g}": order, f"factors_{g}": f, f"shift_{g}": shift, f"out_{g}": out})
        print(g, tiles.shape, "changed bytes:", int((out != tiles).sum()), "of", tiles.size)
    np.savez_compressed(os.path.join(HERE, "jitter_chain.npz"), **arrays)


if __name__ == "__main__":
    main()
