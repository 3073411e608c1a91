"""Restatements of the feature-inversion kernels (csrc/feature_inv.hip and the momentum rule of csrc/feature_vis.hip) in numpy,
with the operation order of include/mil_hip.h: every product, quotient, sum and difference is one correctly rounded operation of
the arrays' dtype — fp32 for the comparison with the device (bit for bit), fp64 for the comparison with torch.autograd and
torch.optim (tests/test_cpu_feature_inv.py).

The toolkit itself (pytorch-cnn-visualizations-master/src of the reference) cannot run here: it imports torchvision.  What is
restated, by its lines:
  inverted_representation.py:21-26   alpha_norm: ((x.view(-1)) ** alpha).sum()
  inverted_representation.py:28-38   total_variation_norm: to_check = x[:, :-1, :-1], one_bottom = x[:, 1:, :-1], one_right =
                                     x[:, :-1, 1:]; (((to_check - one_bottom) ** 2 + (to_check - one_right) ** 2) ** (beta / 2)).sum()
  inverted_representation.py:40-48   euclidian_loss: ((target - org) ** 2).sum() / (org ** 2).sum()
  inverted_representation.py:64-114  opt_img = 1e-1 * randn; SGD([opt_img], lr=1e4, momentum=0.9); 201 steps of
                                     loss = 1e-1 * euclidian_loss + 1e-7 * alpha_norm(opt_img, 6) + 1e-8 * total_variation_norm(opt_img, 2);
                                     lr *= 1/10 after every step i with i % 40 == 0
`oracle_invert_loop` is that loop on `oracle.mil_oracle.backbone(..., acts=...)` with `torch.optim.SGD`, a batch of tiles at once
(every term is a sum over tiles of per-tile terms, so the batch is the toolkit's loop run once per image)."""
import numpy as np
import torch

from feature_vis_reference import LEAK, decode_table, encode


def stage_energy64(target, c):
    """E_t in fp64 for target [T,h,w,cp] holding the STORED values."""
    return (np.asarray(target, dtype=np.float64)[..., :c] ** 2).sum(axis=(1, 2, 3))


def stage_distance64(act, target, c):
    d = np.asarray(act, dtype=np.float64)[..., :c] - np.asarray(target, dtype=np.float64)[..., :c]
    return (d * d).sum(axis=(1, 2, 3))


def stage_match_dz(act, target, c, energy, weight, slope=LEAK):
    """dz like act for arrays of one dtype holding the STORED values and energy [T] of that dtype:
    (((2 weight) / E_t) * (act - target)) * (act > 0 ? 1 : slope) in the real channels, zero in the padding.  (A bf16 tensor's dz
    is this one rounded to bf16.)"""
    dt = act.dtype.type
    n, h, w, cp = act.shape
    assert cp == (c + 7) // 8 * 8 and target.dtype == act.dtype and energy.dtype == act.dtype
    scale = (dt(2) * dt(weight)) / energy
    a = act[..., :c]
    dz = np.zeros_like(act)
    dz[..., :c] = (scale[:, None, None, None] * (a - target[..., :c])) * np.where(a > 0, dt(1), dt(slope)).astype(act.dtype)
    return dz


def shift_copy(x, shift):
    """mil_pixel_shift: out[t,c,i,j] = x[t,c,(i - dy) mod H,(j - dx) mod W]."""
    return np.roll(x, (shift[0], shift[1]), axis=(2, 3))


def tv_stencil(x):
    """S of mil_pixel_reg: half the gradient of the total variation, its three contributions added in the header's order."""
    s = np.zeros_like(x)
    own = x[:, :, :-1, :-1]
    s[:, :, :-1, :-1] += (own - x[:, :, 1:, :-1]) + (own - x[:, :, :-1, 1:])
    s[:, :, 1:, :-1] += x[:, :, 1:, :-1] - own                  # the term of the cell above
    s[:, :, :-1, 1:] += x[:, :, :-1, 1:] - own                  # the term of the cell to the left
    return s


def pixel_reg(x, g, *, alpha, alpha_weight, tv_weight, shift=(0, 0)):
    """mil_pixel_reg's out for arrays of one dtype."""
    dt = x.dtype.type
    out = np.roll(g, (-shift[0], -shift[1]), axis=(2, 3))       # out[i, j] = g[(i + dy) mod H, (j + dx) mod W]
    if alpha_weight != 0:
        p = x.copy()
        for _ in range(alpha - 2):
            p = p * x
        out = out + (dt(alpha_weight) * dt(alpha)) * p
    if tv_weight != 0:
        out = out + (dt(2) * dt(tv_weight)) * tv_stencil(x)
    return out


def reg_terms64(x, alpha):
    """(sum x^alpha, total variation) per tile in fp64, [2,T], and the sums of the terms' magnitudes (the same: every term is >= 0)."""
    x = np.asarray(x, dtype=np.float64)
    own = x[:, :, :-1, :-1]
    tv = ((own - x[:, :, 1:, :-1]) ** 2 + (own - x[:, :, :-1, 1:]) ** 2).sum(axis=(1, 2, 3))
    return np.stack([(x ** alpha).sum(axis=(1, 2, 3)), tv])


def momentum_step(x, g, buf, *, lr, momentum=0.9, weight_decay=0.0, project="none"):
    """mil_pixel_momentum_step on arrays of one dtype: (x, buf, codes) as new arrays."""
    dt = x.dtype.type
    gd = g + dt(weight_decay) * x
    buf = dt(momentum) * buf + gd
    xn = x - dt(lr) * buf
    if project == "clamp":
        xn = np.where(xn < -1, dt(-1), np.where(xn > 1, dt(1), xn)).astype(x.dtype)
    elif project == "u8":
        xn = decode_table()[encode(xn.astype(np.float32))].astype(x.dtype)
    else:
        assert project == "none"
    return xn, buf, encode(xn.astype(np.float32))


def torch_alpha_norm(x, alpha):
    return (x.reshape(-1) ** alpha).sum()


def torch_tv_norm(x, beta=2):
    """total_variation_norm on a stack [T,3,H,W]: the toolkit's slices on the last two axes."""
    to_check, one_bottom, one_right = x[..., :-1, :-1], x[..., 1:, :-1], x[..., :-1, 1:]
    return (((to_check - one_bottom) ** 2 + (to_check - one_right) ** 2) ** (beta / 2)).sum()


def oracle_invert_loop(orc, sd, tiles, x0, layer, steps, *, lr, momentum=0.9, weight=0.1, alpha=6, alpha_weight=1e-7, tv_weight=1e-8):
    """inverted_representation.py's loop on the CPU oracle, constant lr.  Returns (final x, trace [steps + 1, T]): the weighted
    distance at the start of every step and of the final image."""
    with torch.no_grad():
        acts = {}
        orc.backbone(sd, tiles, acts=acts)
        target = acts[layer]
        energy = (target ** 2).sum(dim=(1, 2, 3))
    x = x0.clone().requires_grad_()
    opt = torch.optim.SGD([x], lr=lr, momentum=momentum)
    trace = []

    def distance():
        acts = {}
        orc.backbone(sd, x, acts=acts)
        return weight * ((acts[layer] - target) ** 2).sum(dim=(1, 2, 3)) / energy
    for _ in range(steps):
        opt.zero_grad()
        d = distance()
        (d.sum() + alpha_weight * torch_alpha_norm(x, alpha) + tv_weight * torch_tv_norm(x)).backward()
        opt.step()
        trace.append(d.detach())
    with torch.no_grad():
        trace.append(distance())
    return x.detach(), torch.stack(trace)
