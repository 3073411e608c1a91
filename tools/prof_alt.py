"""alt_resnet.ResNet(BasicBlock,[3,3,3,3]) forward+backward on 256 tiles @256x256 (the bench's alt_resnet_path step) in one
compute mode (bf16, fp32 or bf16x3).  Under a profiler it is the traced workload:
    rocprofv3 --kernel-trace --stats -d out -- python3 tools/prof_alt.py [steps] [mode]
on its own it also prints the time per step from device events around `steps` steps after three warm-up steps:
    python3 tools/prof_alt.py 10 bf16x3"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mil_amd  # noqa: E402

MODES = {"bf16": torch.bfloat16, "fp32": torch.float32, "bf16x3": mil_amd.BF16X3}
WARMUP = 3

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 4
mode = sys.argv[2] if len(sys.argv) > 2 else "bf16"
if mode not in MODES:
    sys.exit(f"mode must be one of {sorted(MODES)}, got {mode}")
torch.manual_seed(77)
net = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, [3, 3, 3, 3], num_classes=80, compute_dtype=MODES[mode]).cuda()
gen = torch.Generator(device="cuda").manual_seed(5)
x = torch.randn((256, 3, 256, 256), generator=gen, device="cuda").clamp_(-1.0, 1.0)
dfe = torch.randn((256, 80), generator=gen, device="cuda")


def step():
    for p in net.parameters():
        p.grad = None
    net(x).backward(dfe)


for _ in range(WARMUP):
    step()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(steps):
    step()
e1.record()
torch.cuda.synchronize()
print(f"alt_resnet [3,3,3,3] 256 tiles @256x256 {mode}: {e0.elapsed_time(e1) / steps:.2f} ms per step ({steps} steps after {WARMUP} warm-up)")
