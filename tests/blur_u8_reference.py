"""The numpy restatement of `mil_gaussian_blur_u8` (include/mil_hip.h), written from the header's text and from nothing else: the six
integers of an item from its sigmas in fp32, and the box pass in uint32.  It imports no Pillow; tests/test_cpu_blur_u8.py holds it
against Pillow bit for bit, tests/test_gpu_blur_u8.py holds the kernel against it."""
import math

import numpy as np

MAX_BOX = 7                     # MIL_BLUR_U8_MAX_BOX
ONE = 1 << 24


def box_params(sigma):
    """(r, ww, fw) of one axis for a sigma >= 0, in fp32 as the header writes it (sqrt and floor in double, cast back)."""
    f32 = np.float32
    radius = f32(sigma)
    sigma2 = f32(f32(radius * radius) / f32(3))
    L = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(L) - 1.0) / 2.0))
    a = f32(f32(f32(f32(2) * l) + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(f32(f32(16777216) / f32(f32(fr * f32(2)) + f32(1))))
    fw = (ONE - (2 * r + 1) * ww) // 2
    return r, ww, fw


def item_params(sigma_x, sigma_y=None):
    """The six integers (r_x, ww_x, fw_x, r_y, ww_y, fw_y) of one item."""
    return box_params(sigma_x) + box_params(sigma_x if sigma_y is None else sigma_y)


def params_array(sigmas):
    """int32 [n,6] for a list of sigmas, each a number or an (sx, sy) pair."""
    rows = [item_params(*s) if isinstance(s, (tuple, list)) else item_params(s) for s in sigmas]
    return np.asarray(rows, dtype=np.int32).reshape(-1, 6)


def box_pass(a, axis, r, ww, fw):
    """One pass along `axis` of a uint8 array: out[x] = (ww * sum_{k=-r..r} in[c(x+k)] + fw * (in[c(x-r-1)] + in[c(x+r+1)])
    + 2^23) >> 24 with the index clamped to the line, in uint32."""
    a = np.moveaxis(np.asarray(a, dtype=np.uint8), axis, -1)
    n = a.shape[-1]
    x = np.arange(n)
    v = a.astype(np.uint32)

    def at(k):
        return v[..., np.clip(x + k, 0, n - 1)]

    s = np.zeros(v.shape, dtype=np.uint32)
    for k in range(-r, r + 1):
        s += at(k)
    with np.errstate(over="raise"):
        acc = np.uint32(ww) * s + np.uint32(fw) * (at(-r - 1) + at(r + 1)) + np.uint32(1 << 23)
    out = (acc >> np.uint32(24)).astype(np.uint8)
    assert int((acc >> np.uint32(24)).max(initial=0)) <= 255
    return np.moveaxis(out, -1, axis)


def blur_plane(plane, p):
    """One plane [H,W] through three passes along W with p[0:3], then three along H with p[3:6]."""
    out = np.asarray(plane, dtype=np.uint8)
    for _ in range(3):
        out = box_pass(out, 1, int(p[0]), int(p[1]), int(p[2]))
    for _ in range(3):
        out = box_pass(out, 0, int(p[3]), int(p[4]), int(p[5]))
    return out


def gaussian_blur_u8(planes, params, planes_per_item):
    """uint8 [P,H,W] with int [P / planes_per_item, 6]: plane p takes row p // planes_per_item."""
    planes = np.asarray(planes, dtype=np.uint8)
    params = np.asarray(params).reshape(-1, 6)
    assert planes.ndim == 3 and planes.shape[0] == params.shape[0] * planes_per_item
    out = np.empty_like(planes)
    for p in range(planes.shape[0]):
        out[p] = blur_plane(planes[p], params[p // planes_per_item])
    return out


def blur_image(img, sigma):
    """An image [H,W] (`L`) or [H,W,3] (`RGB`) as Pillow's `img.filter(ImageFilter.GaussianBlur(sigma))` writes it; sigma a number
    or (sx, sy)."""
    p = item_params(*sigma) if isinstance(sigma, (tuple, list)) else item_params(sigma)
    img = np.asarray(img, dtype=np.uint8)
    if img.ndim == 2:
        return blur_plane(img, p)
    return np.stack([blur_plane(img[..., c], p) for c in range(img.shape[2])], axis=-1)
