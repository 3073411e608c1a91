"""Restatements of the activation-maximisation kernels (csrc/feature_vis.hip) in numpy, with the operation order of
include/mil_hip.h: every product, quotient, sum and difference is one correctly rounded operation of the arrays' dtype — fp32
for the comparison with the device (bit for bit), fp64 for the comparison with torch.optim (tests/test_cpu_feature_vis.py).

The toolkit itself (pytorch-cnn-visualizations-master/src of the reference) cannot run here: it imports torchvision.  What is
restated, by its lines:
  cnn_layer_visualization.py:38-60  random image uniform(150, 180), Adam([image], lr=0.1, weight_decay=1e-6), 30 steps of
                                    loss = -mean(conv_output of the selected filter); loss.backward(); optimizer.step()
  deep_dream.py:44-66               the same loss from a real image (SGD, lr=12, weight_decay=1e-4, 250 steps)
  generate_class_specific_samples.py:39-66   SGD([image], lr=6) on -output[0, class], the image re-created as bytes
                                    (recreate_image) and re-processed every step
  misc_functions.py:173-192         recreate_image: un-normalise, clip to [0, 1], np.round(x * 255) — at this project's mean and
                                    std of 0.5 that is round(clip(x / 2 + 0.5, 0, 1) * 255)
`oracle_filter_loop` is the whole loop of the first on `oracle.mil_oracle.backbone(..., acts=...)` with `torch.optim`."""
import numpy as np
import torch

LEAK = np.float32(0.1)


def decode_table():
    """The 256 fp32 values `U8Tiles.float()` looks up: ((u / 255) - 0.5) / 0.5 in IEEE fp32."""
    u = np.arange(256, dtype=np.float32)
    return ((u / np.float32(255)) - np.float32(0.5)) / np.float32(0.5)


def encode(x):
    """uint8 codes of an fp32 array: rint(clip(x / 2 + 0.5, 0, 1) * 255), half to even (np.round); a NaN encodes as 0."""
    x = np.asarray(x, dtype=np.float32)
    y = x * np.float32(0.5) + np.float32(0.5)
    y = np.where(y > 0, np.where(y > 1, np.float32(1), y), np.float32(0)).astype(np.float32)
    return np.round(y * np.float32(255)).astype(np.uint8)


def stage_seed(act, channels, c, slope=LEAK):
    """(J64 [T] fp64, dz fp32 like act) for act [T,h,w,cp] fp32 holding the STORED values: J64 the fp64 mean of each tile's
    channel, dz = (-(1/(h w))) * (act > 0 ? 1 : slope) at the tile's channel — 1/(h w) one fp32 division, the product one fp32
    multiplication — and zero elsewhere.  (A bf16 tensor's dz is this one rounded to bf16.)"""
    act = np.asarray(act, dtype=np.float32)
    n, h, w, cp = act.shape
    assert cp == (c + 7) // 8 * 8
    neg_inv = -(np.float32(1) / np.float32(h * w))
    dz = np.zeros_like(act)
    j64 = np.zeros(n, dtype=np.float64)
    for t in range(n):
        a = act[t, :, :, channels[t]]
        j64[t] = a.astype(np.float64).mean()
        dz[t, :, :, channels[t]] = neg_inv * np.where(a > 0, np.float32(1), np.float32(slope)).astype(np.float32)
    return j64, dz


def step_scalars(lr, weight_decay, betas, eps, step, dtype=np.float32):
    """(lr, wd, beta1, 1 - beta1, beta2, 1 - beta2, bc1, sqrt(bc2), eps): formed in double, rounded once to `dtype`."""
    b1, b2 = float(betas[0]), float(betas[1])
    vals = (lr, weight_decay, b1, 1.0 - b1, b2, 1.0 - b2, 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5, eps)
    return tuple(dtype(v) for v in vals)


def pixel_step(x, g, m, v, *, rule, lr, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, step=1, project="none", table=None):
    """One step on arrays of one dtype (fp32: the kernel's bits; fp64: torch.optim's formula).  Returns (x, m, v, codes) as new
    arrays; m and v pass through for rule="sgd"; codes = encode(x) of the value returned."""
    dt = x.dtype.type
    lr, wd, b1, omb1, b2, omb2, bc1, sbc2, eps = step_scalars(lr, weight_decay, betas, eps, step, dt)
    gd = g + wd * x
    if rule == "sgd":
        xn = x - lr * gd
    else:
        m = b1 * m + omb1 * gd
        v = b2 * v + (omb2 * gd) * gd
        denom = np.sqrt(v) / sbc2 + eps
        xn = x - ((lr / bc1) * m) / denom
    if project == "clamp":
        xn = np.where(xn < -1, dt(-1), np.where(xn > 1, dt(1), xn)).astype(dt)
    elif project == "u8":
        xn = (decode_table() if table is None else table)[encode(xn.astype(np.float32))].astype(dt)
    else:
        assert project == "none"
    return xn, m, v, encode(xn.astype(np.float32))


def oracle_filter_loop(orc, sd, x0, layer, channels, steps, *, lr=0.1, weight_decay=1e-6, betas=(0.9, 0.999), eps=1e-8):
    """cnn_layer_visualization.py's loop on the CPU oracle: one image per channel in one batch, torch.optim.Adam on the stack
    (element-wise, so the batch is the toolkit's loop run once per image).  Returns (final x, trace [steps + 1, T]): the
    objective J_t = mean of channel channels[t] of `layer`'s output at the start of every step, and of the final image."""
    x = x0.clone().requires_grad_()
    opt = torch.optim.Adam([x], lr=lr, weight_decay=weight_decay, betas=betas, eps=eps)
    idx = torch.arange(x.shape[0])
    ch = torch.as_tensor(list(channels))
    trace = []

    def objective():
        acts = {}
        orc.backbone(sd, x, acts=acts)
        return acts[layer][idx, ch].mean(dim=(1, 2))
    for _ in range(steps):
        opt.zero_grad()
        j = objective()
        (-j.sum()).backward()
        opt.step()
        trace.append(j.detach())
    with torch.no_grad():
        trace.append(objective())
    return x.detach(), torch.stack(trace)
