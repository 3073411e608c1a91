"""Writes tests/golden/gradcam_lanczos.npz: what Pillow and numpy themselves return for the two steps of the Grad-CAM
post-processing that `mil_grad_cam` restates (recorded with Pillow 12.2.0, numpy as installed).

  pairs            int [P,4]: (h, w, H, W) of every resize case
  rand_i, bin_i    uint8 [h,w]: a random map and a map of 0 / 255 only, case i.  The tables of the largest supported map,
                   128 -> 512, are exercised one axis at a time (128x128 -> 512x8 and -> 8x512): the full 512x512 results
                   would be most of the file
  rand_out_i, bin_out_i   uint8 [H,W]: Image.fromarray(map).resize((W, H), Image.LANCZOS)  (LANCZOS is what the toolkit's
                          Image.ANTIALIAS named)
  cam_i            float32 [h,w] maps in [0,1] (among them exact k/255 values and values next to them)
  cam_u8_i         np.uint8(cam_i * 255), gradcam.py:87

Only Pillow and numpy are imported.  Run from the repository root: python tests/golden/make_gradcam_golden.py"""
import os

import numpy as np
import PIL
from PIL import Image

PAIRS = [(8, 8, 256, 256), (2, 3, 50, 70), (1, 1, 32, 32), (10, 10, 300, 300), (64, 64, 256, 256), (16, 16, 512, 512),
         (1, 2, 33, 37), (13, 18, 50, 70), (7, 9, 50, 70), (128, 128, 512, 8), (128, 128, 8, 512), (16, 16, 16, 16), (64, 48, 16, 24)]


def resize(img, H, W):
    return np.asarray(Image.fromarray(img).resize((W, H), Image.LANCZOS))


if __name__ == "__main__":
    rng = np.random.default_rng(20260301)
    data = {"pairs": np.array(PAIRS, dtype=np.int32), "pillow_version": np.array(PIL.__version__)}
    for i, (h, w, H, W) in enumerate(PAIRS):
        rand = rng.integers(0, 256, (h, w), dtype=np.uint8)
        binary = (rng.integers(0, 2, (h, w)) * 255).astype(np.uint8)
        data[f"rand_{i}"], data[f"rand_out_{i}"] = rand, resize(rand, H, W)
        data[f"bin_{i}"], data[f"bin_out_{i}"] = binary, resize(binary, H, W)
    k = np.arange(256, dtype=np.float32) / np.float32(255)
    cams = [rng.random((13, 18), dtype=np.float32), np.stack([k, np.nextafter(k, np.float32(0)), np.nextafter(k, np.float32(2))]),
            (rng.random((64, 64), dtype=np.float32) ** 4).astype(np.float32)]
    for i, cam in enumerate(cams):
        cam = np.clip(cam, 0, 1).astype(np.float32)
        data[f"cam_{i}"], data[f"cam_u8_{i}"] = cam, np.uint8(cam * 255)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gradcam_lanczos.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes; Pillow", PIL.__version__)
