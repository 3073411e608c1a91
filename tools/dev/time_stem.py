"""Times the fused stem forward / backward alone (2048 tiles @256x256 by default):
`python tools/dev/time_stem.py [bf16|bf16x3] [n] [size] [fp32|u8] [rounds]`.
The feed is the form the tiles are handed over in: fp32 [n,3,H,W] (mil_stem_fwd_fused / mil_stem_bwd_fused_nchw) or uint8
(mil_stem_fwd_fused_u8 / mil_stem_bwd_fused_u8); both feeds time the SAME tiles (random bytes, decoded for the fp32 feed).
Each line is one round of 20 launches; with rounds > 1 a median / min / max line follows.
With MIL_LIB_PATH=<stamp build> the instrumented kernels print their phase shares."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import mil_amd  # noqa: E402
from mil_amd import _lib as L, ops  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "bf16"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
size = int(sys.argv[3]) if len(sys.argv) > 3 else 256
feed = sys.argv[4] if len(sys.argv) > 4 else "fp32"
rounds = int(sys.argv[5]) if len(sys.argv) > 5 else 1
if feed not in ("fp32", "u8"):
    raise SystemExit("feed must be fp32 or u8")
dt = torch.bfloat16 if mode == "bf16" else torch.float32
code = L.MIL_DT_F32S if mode == "bf16x3" else L.MIL_DT_F32
g = torch.Generator(device="cuda").manual_seed(1)
u8 = torch.randint(0, 256, (n, 3, size, size), generator=g, device="cuda", dtype=torch.uint8)
x = u8 if feed == "u8" else mil_amd.U8Tiles(u8).float()
if feed == "fp32":
    del u8
wt = torch.randn((20, 3, 7, 7), generator=g, device="cuda") * 0.08
b = torch.randn((20,), generator=g, device="cuda") * 0.1
with L.f32_mma(code):
    wp, bp = ops.pack_weights(wt, b, L.PACK_STEM, dt)

    def fwd():
        if feed == "u8":
            return ops.stem_fwd_fused_u8(x, wp, bp, 24, dtype=dt)
        return ops.stem_fwd_fused(x, wp, bp, 24, dtype=dt, keep_s2d=False)[1:]

    pool, widx = fwd()
    gp = torch.randn(pool.shape[:3] + (20,), generator=g, device="cuda").to(dt)

    def bwd():
        return ops.stem_bwd_fused_u8(x, gp, widx) if feed == "u8" else ops.stem_bwd_fused_nchw(x, gp, widx)

    for name, fn in (("stem_fwd", fwd), ("stem_bwd", bwd)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        reps = 20
        us = []
        for _ in range(rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / reps * 1e3)
            print(f"{mode} {feed} {name}: {us[-1]:.1f} us per launch ({n} tiles @{size})", flush=True)
        if rounds > 1:
            print(f"{mode} {feed} {name}: median {statistics.median(us):.1f} us, min {min(us):.1f}, max {max(us):.1f} over {rounds} rounds "
                  f"({n} tiles @{size})", flush=True)
