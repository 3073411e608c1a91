#!/usr/bin/env python3
"""Times what it costs to watch the encoder's layers, on one GPU, on the eval forward of the benchmark
shape (8 bags x 256 tiles at 256x256 by default) in bf16 and in the default (bf16x3) mode:

  off      no summary attached
  stages   `ActivationSummary(taps="stages")`  (6 tensors, two launches behind the encoder pass)
  blocks   `ActivationSummary(taps="blocks")`  (27 tensors, two launches)
  hooks    the route without the device summaries: forward hooks on the modules of the "stages" taps, each computing finite
           count / sum / min / max with torch on the NCHW fp32 copy it is handed (results left on the device)

and, on their own: the two statistics launches on 27 tensors of the shapes the forward keeps, against the bytes they must read
and the stream-copy rate of the box (`mil_stream_copy`, 1 GiB); `parameter_stats` on the flat bucket (+ its one copy to the host)
against 65 x 2 torch reductions with `.item()`.

Device events around each route, the routes alternating inside every repetition; prints one JSON line with the median, the
smallest and the largest time of each.  A report, not a test: nothing is asserted but that the routes return the same features
where the same kernels ran."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402
from mil_amd import summary  # noqa: E402


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


class _ShapeProbe:
    """Stands where a summary would: records shape, dtype and real width of every tensor the encoder hands over."""

    def __init__(self, widths):
        self.widths, self.shapes = widths, None

    def observe(self, pool, blocks, pooled, feats):
        ts = [pool] + [t for _x, o1, out in blocks for t in (o1, out)] + [pooled, feats]
        self.shapes = [(tuple(t.shape), t.dtype, w) for t, w in zip(ts, self.widths)]


def _torch_stats_hook(store):
    def hook(mod, inp, out):
        store.append((torch.isfinite(out).sum(), out.sum(dtype=torch.float64), out.min(), out.max()))
    return hook


def time_mode(mode, a):
    dtype = {"bf16": torch.bfloat16, "bf16x3": mil_amd.BF16X3}[mode]
    net = mil_amd.Attention(3, compute_dtype=dtype).eval()
    enc = net.cnn.module
    gen = torch.Generator("cuda").manual_seed(1)
    x = torch.rand((a.bags * a.tiles, 3, a.res, a.res), device="cuda", generator=gen) * 2 - 1
    sizes, labels = [a.tiles] * a.bags, torch.zeros(a.bags, dtype=torch.long)
    s_stages = mil_amd.ActivationSummary(net, taps="stages")
    enc.activation_summary = None
    s_blocks = mil_amd.ActivationSummary(net, taps="blocks")
    enc.activation_summary = None
    probe = _ShapeProbe(s_blocks._widths)
    hooked = [enc.maxpool, enc.layer1, enc.layer2, enc.layer3, enc.layer4, enc.fc]
    kept = []

    def forward(attach=None, hooks=False):
        enc.activation_summary = attach
        handles = [m.register_forward_hook(_torch_stats_hook(kept)) for m in hooked] if hooks else []
        try:
            with torch.no_grad():
                return net.forward_bags((x, sizes), labels)[0]["Fterm"]
        finally:
            enc.activation_summary = None
            for h in handles:
                h.remove()
            kept.clear()

    routes = {"off": lambda: forward(), "stages": lambda: forward(s_stages), "blocks": lambda: forward(s_blocks),
              "hooks": lambda: forward(hooks=True)}
    want = routes["off"]()
    assert torch.equal(routes["stages"](), want) and torch.equal(routes["blocks"](), want)
    forward(probe)
    shapes = probe.shapes
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for name, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {k: _stat(v) for k, v in times.items()}
    for k in ("stages", "blocks", "hooks"):
        res[k]["over_off_ms"] = round(res[k]["median_ms"] - res["off"]["median_ms"], 4)
        res[k]["over_off_share"] = round(res[k]["median_ms"] / res["off"]["median_ms"] - 1, 4)
    first = s_blocks.first_nonfinite()
    res["first_nonfinite"] = first
    s_stages.close()
    s_blocks.close()
    del net, x
    torch.cuda.empty_cache()
    return res, shapes


def time_launches(shapes, a):
    """The two launches alone on tensors of the given shapes, beside a 1 GiB stream copy."""
    gen = torch.Generator("cuda").manual_seed(2)
    tensors = [((torch.rand(shape, device="cuda", generator=gen) - 0.3).to(dt), w) for shape, dt, w in shapes]
    entries = [summary._entry(t) for t in tensors]
    nbytes = sum(t.numel() * t.element_size() for t, _w in tensors)
    table, out = summary._StatsTable(), torch.empty((len(entries), 8), dtype=torch.float64, device="cuda")
    n16 = 1 << 30
    src, dst = torch.empty(n16, dtype=torch.uint8, device="cuda").random_(), torch.empty(n16, dtype=torch.uint8, device="cuda")
    lib = mil_amd.lib()
    routes = {"stats": lambda: table.run(entries, out),
              "copy": lambda: lib.mil_stream_copy(dst.data_ptr(), src.data_ptr(), n16, torch.cuda.current_stream().cuda_stream)}
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for name, f in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            if it >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = {k: _stat(v) for k, v in times.items()}
    res["stats"].update(tensors=len(entries), bytes_read=nbytes, GBps_at_median=round(nbytes / res["stats"]["median_ms"] / 1e6, 1))
    res["copy"].update(bytes_moved=2 * n16, GBps_at_median=round(2 * n16 / res["copy"]["median_ms"] / 1e6, 1))
    res["stats"]["ms_at_copy_rate"] = round(nbytes / (res["copy"]["GBps_at_median"] * 1e6), 4)
    return res


def time_parameters(a):
    net = mil_amd.Attention(3)
    flat = mil_amd.FlatParams(net)
    params = list(net.parameters())

    def ours():
        names, st = mil_amd.parameter_stats(flat)
        return st.cpu()

    def torch_items():
        return [(p.mean().item(), p.max().item()) for p in params]

    routes = {"parameter_stats": ours, "torch_item_reductions": torch_items}
    times = {k: [] for k in routes}
    for it in range(a.warmup + a.reps):
        for name, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    res = {k: _stat(v) for k, v in times.items()}
    res["parameters"], res["floats"] = len(params), flat.numel
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bags", type=int, default=8)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--res", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--modes", default="bf16,bf16x3")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_layer_summary.py needs a GPU")
    res = {"bags": a.bags, "tiles": a.tiles, "res": a.res, "reps": a.reps, "warmup": a.warmup}
    for mode in a.modes.split(","):
        res[mode], shapes = time_mode(mode, a)
        res[mode]["launches_alone"] = time_launches(shapes, a)
    res["parameters"] = time_parameters(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
