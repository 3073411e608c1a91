"""Writes tests/golden/gaussian_blur_u8.npz: the bytes Pillow's `ImageFilter.GaussianBlur` wrote for a few small images, so that the
kernel and the numpy restatement can be held against Pillow where no Pillow is installed.  Run from the repository root:

    python tests/golden/make_blur_u8_golden.py

Per case `<name>`: `<name>_in` (uint8 [H,W,3] for RGB, [H,W] for L), `<name>_sigmas` (float64 [k,2] of (sx, sy), Pillow's tuple radius)
and `<name>_out` (uint8 [k, ...], one blurred image per row of sigmas).  `pillow_version` records the library that wrote them."""
import os

import numpy as np
import PIL
from PIL import Image, ImageFilter

HERE = os.path.dirname(os.path.abspath(__file__))

# (name, height, width, bands, [(sx, sy), ...])
CASES = [
    ("rgb_70x67", 70, 67, 3, [(8.0, 8.0)]),
    ("rgb_33x47", 33, 47, 3, [(0.3, 0.3), (1.4, 1.4), (4.0, 4.0), (1.4, 4.0)]),
    ("l_64x64", 64, 64, 1, [(1.0, 1.0), (8.0, 8.0), (4.0, 0.0)]),
    ("l_5x3", 5, 3, 1, [(0.3, 0.3), (8.0, 8.0)]),
]


def make_input(rng, h, w, bands):
    """Uniform noise with a flat 0 region, a flat 255 region and a horizontal ramp: saturation at both ends, and borders that
    differ from what lies beside them, so the clamp shows."""
    img = rng.integers(0, 256, (h, w, bands), dtype=np.uint8)
    img[: h // 3, : w // 2] = 0
    img[: h // 3, w // 2:] = 255
    img[h - max(h // 4, 1):] = np.linspace(0, 255, w).astype(np.uint8)[None, :, None]
    img[h // 2, :] = rng.integers(0, 256, (w, bands), dtype=np.uint8)
    return img if bands == 3 else img[..., 0]


def main():
    rng = np.random.default_rng(20261021)
    out = {"pillow_version": np.asarray(PIL.__version__)}
    for name, h, w, bands, sigmas in CASES:
        img = make_input(rng, h, w, bands)
        pil = Image.fromarray(img)
        assert pil.mode == ("RGB" if bands == 3 else "L")
        out[name + "_in"] = img
        out[name + "_sigmas"] = np.asarray(sigmas, dtype=np.float64)
        out[name + "_out"] = np.stack([np.asarray(pil.filter(ImageFilter.GaussianBlur(s))) for s in sigmas])
    path = os.path.join(HERE, "gaussian_blur_u8.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
