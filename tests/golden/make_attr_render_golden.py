"""Writes tests/golden/attr_render.npz: what matplotlib, Pillow and the literal expressions of the saliency toolkit's
misc_functions.py (pytorch-cnn-visualizations-master/src) make of small inputs — the recorded side of
tests/test_cpu_attr_render.py.  Imports numpy, Pillow and matplotlib only; run it by hand, the tests read the file.

  lut_<name>        uint8 [256,3]: (matplotlib.colormaps[name](np.arange(256, dtype=np.uint8)) * 255).astype(np.uint8), RGB
  comp_alphas       the alpha bytes of the composite tables
  comp_tables       uint8 [len(comp_alphas),256,256]: Image.alpha_composite of a source byte (row) with that alpha over an
                    opaque destination byte (column); the output alpha is asserted to be 255 everywhere
  grads             fp32 [N,3,H,W]: small gradients (cubed normals, half zeros, ties, a constant one, one-signed ones)
  gray_bytes        uint8 [N,H,W]: convert_to_grayscale + format_np_output on the fp32 gradient, literally
  colour_bytes      uint8 [N,H,W,3]: save_gradient_images + format_np_output
  pos_bytes, neg_bytes  uint8 [N,H,W,3]: get_positive_negative_saliency, each through save_gradient_images (both normalisations)
  ov_tile, ov_map   uint8 [3,H,W] planar tile and uint8 [H,W] map of one overlay case
  ov_heat, ov_on    uint8 [H,W,3]: apply_colormap_on_image(tile, map, 'hsv'), the RGB of its two images
  versions          numpy, Pillow and matplotlib that wrote the file
"""
import os

import matplotlib
import numpy as np
import PIL
from PIL import Image

CMAPS = ("hsv", "jet", "viridis")
ALPHAS = (102, 127, 254)
N, H, W = 24, 23, 27


def lut(name):
    return (matplotlib.colormaps[name](np.arange(256, dtype=np.uint8)) * 255).astype(np.uint8)[:, :3]


def composite_table(alpha):
    src = np.zeros((256, 256, 4), np.uint8)
    src[..., :3] = np.arange(256, dtype=np.uint8)[:, None, None]
    src[..., 3] = alpha
    dst = np.zeros((256, 256, 4), np.uint8)
    dst[..., :3] = np.arange(256, dtype=np.uint8)[None, :, None]
    dst[..., 3] = 255
    out = np.asarray(Image.alpha_composite(Image.fromarray(dst, "RGBA"), Image.fromarray(src, "RGBA")))
    assert (out[..., 3] == 255).all() and (out[..., 0] == out[..., 1]).all() and (out[..., 0] == out[..., 2]).all()
    return out[..., 0].copy()


def gradients():
    rng = np.random.default_rng(20261020)
    out = []
    for i in range(N):
        g = rng.standard_normal((3, H, W)).astype(np.float32) ** 3 * np.float32(10.0 ** rng.integers(-6, 2))
        kind = i % 6
        if kind == 1:                                      # half of the elements exactly zero, some of them -0.0
            mask = rng.random((3, H, W)) < 0.5
            g[mask] = np.where(rng.random(int(mask.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        elif kind == 2:                                    # heavy ties
            g = np.round(rng.standard_normal((3, H, W)) * 3).astype(np.float32)
        elif kind == 3 and i == 3:                         # a constant gradient
            g[:] = np.float32(0.25)
        elif kind == 4:
            g = np.abs(g) + np.float32(1e-3) if i % 12 == 4 else -np.abs(g) - np.float32(1e-3)
        out.append(g)
    return np.stack(out)


def format_bytes(a):
    """format_np_output of a [C,H,W] array with values in [0,1] (C = 1 or 3): repeat, transpose, multiply, truncate."""
    if a.shape[0] == 1:
        a = np.repeat(a, 3, axis=0)
    a = a.transpose(1, 2, 0)
    assert np.max(a) <= 1 or np.isnan(np.max(a))
    return (a * 255).astype(np.uint8)


def toolkit_gray(g):
    gray = np.sum(np.abs(g), axis=0)
    im_max = np.percentile(gray, 99)
    im_min = np.min(gray)
    gray = np.clip((gray - im_min) / (im_max - im_min), 0, 1)
    return format_bytes(np.expand_dims(gray, axis=0))[..., 0]


def toolkit_colour(g):
    g = g - g.min()
    g /= g.max()
    return format_bytes(g)


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    data = {"versions": np.array([np.__version__, PIL.__version__, matplotlib.__version__])}
    for name in CMAPS:
        data["lut_" + name] = lut(name)
    data["comp_alphas"] = np.array(ALPHAS, np.int32)
    data["comp_tables"] = np.stack([composite_table(a) for a in ALPHAS])
    grads = gradients()
    data["grads"] = grads
    with np.errstate(all="ignore"):
        data["gray_bytes"] = np.stack([toolkit_gray(g) for g in grads])
        data["colour_bytes"] = np.stack([toolkit_colour(g) for g in grads])
        pos = [np.maximum(0, g) / g.max() for g in grads]
        neg = [np.maximum(0, -g) / -g.min() for g in grads]
        data["pos_bytes"] = np.stack([toolkit_colour(p) for p in pos])
        data["neg_bytes"] = np.stack([toolkit_colour(n) for n in neg])
    rng = np.random.default_rng(7)
    tile = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    amap = rng.integers(0, 256, (H, W), dtype=np.uint8)
    amap.flat[:256] = np.arange(256, dtype=np.uint8)          # every table row
    org = Image.fromarray(tile.transpose(1, 2, 0).copy(), "RGB")
    no_trans = matplotlib.colormaps["hsv"](amap)
    heat = no_trans.copy()
    heat[:, :, 3] = 0.4
    heat = Image.fromarray((heat * 255).astype(np.uint8))
    no_trans = Image.fromarray((no_trans * 255).astype(np.uint8))
    on = Image.alpha_composite(Image.new("RGBA", org.size), org.convert("RGBA"))
    on = np.asarray(Image.alpha_composite(on, heat))
    assert (on[..., 3] == 255).all()
    data.update(ov_tile=tile, ov_map=amap, ov_heat=np.asarray(no_trans)[..., :3].copy(), ov_on=on[..., :3].copy())
    np.savez_compressed(os.path.join(here, "attr_render.npz"), **data)
    print({k: (v.shape, str(v.dtype)) for k, v in data.items()})


if __name__ == "__main__":
    main()
