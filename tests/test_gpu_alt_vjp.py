"""-m gpu: the wide encoder's (`alt_resnet`) vector-Jacobian product against fp64 ON THE LINEAR PIECE IT TOOK, in every compute
mode — the wide counterpart of tests/test_gpu_configs.py::test_encoder_gradients_on_its_own_activation_pattern.

A ReLU / max-pool network is piecewise linear; two correct evaluations differ in the branch of the few elements whose
pre-activation is within rounding of zero, and one flipped element moves every upstream gradient by more than any kernel's
arithmetic does.  That is why the golden tests of this encoder can only hold gradient norms to 1e-3..5e-3 (and a cosine), which
a layer with one split-product cross term missing (6e-3..7.5e-3 of its output's root-sum-square, one layer of eighteen) passes.
Here the fp64 oracle (`orc.alt_backbone(patterns=)`) runs on the activation pattern the HIP forward itself took — pool winners
and stem gate from the winner records, both ReLU gates of every block from the tensors the forward saved — so the kernels'
arithmetic is all that is left, and the narrow encoder's tolerances (26 layers; this one has at most 18) are ceilings:

    mode      features (max error / max magnitude)    every parameter gradient (L2 error / fp64 norm)
    fp32      2e-6                                     1e-5
    BF16X3    2e-5                                     2e-4      ~10x a correct split per layer (2e-5), ~30x below one dropped term
    bf16      1e-2                                     4e-2      both with the gather-GEMM kernels and with GATHER_GEMM off

Measured on MI355X (features / worst gradient), case a then case b:
    fp32      7.0e-7 / 9.9e-7,  1.0e-6 / 1.5e-6 (conv1.weight)
    BF16X3    1.1e-5 / 1.2e-5,  5.0e-6 / 1.8e-5 (layer1.0.conv2.weight)
    bf16      6.7e-3 / 7.5e-3,  5.5e-3 / 8.6e-3 with the gather-GEMM kernels; 6.7e-3 / 7.5e-3,  5.1e-3 / 8.7e-3 with
              GATHER_GEMM off (channel-blocked kernels only)
The kernels reduce in a fixed order (no atomics): these figures repeat run to run.
"""
import pytest
import torch

from mil_amd import _lib as L, alt_resnet
from oracle import mil_oracle as orc

pytestmark = pytest.mark.gpu

NUM_CLASSES = 24
# layers, tiles, tile height, width, seed
CASES = {
    "a-l1111-4x64x64": ((1, 1, 1, 1), 4, 64, 64, 20261001),      # maps 16, 8, 4, 2: many images per tile
    "b-l2222-3x96x80": ((2, 2, 2, 2), 3, 96, 80, 20261002),      # maps 24x20, 12x10, 6x5, 3x3: odd, ragged, identity blocks at
}                                                                # every width, a ragged last image group
# mode, GATHER_GEMM, (feature ceiling, gradient ceiling)
MODES = {
    "fp32": (torch.float32, True, (2e-6, 1e-5)),
    "bf16x3": (L.BF16X3, True, (2e-5, 2e-4)),
    "bf16-gather": (torch.bfloat16, True, (1e-2, 4e-2)),
    "bf16-blocked": (torch.bfloat16, False, (1e-2, 4e-2)),
}


def _hip_patterns(saved, layers):
    """Activation pattern of an `alt_resnet._forward` run in the form `orc.alt_backbone(patterns=...)` takes."""
    widx = saved["widx"][..., :64].permute(0, 3, 1, 2).cpu()
    pat = {"stem_tap": (widx & 15).long(), "stem_pos": ((widx >> 4) & 1) == 0}
    names = [f"layer{li}.{b}" for li, depth in enumerate(layers, start=1) for b in range(depth)]
    assert len(names) == len(saved["blocks"])
    for name, blk in zip(names, saved["blocks"]):
        o1, out = blk[1], blk[2]
        pat[name + ".o1"] = (o1.float() > 0).permute(0, 3, 1, 2).cpu()
        pat[name] = (out.float() > 0).permute(0, 3, 1, 2).cpu()
    return pat


@pytest.mark.parametrize("mode_id", list(MODES))
@pytest.mark.parametrize("case_id", list(CASES))
def test_wide_encoder_gradients_on_its_own_activation_pattern(case_id, mode_id):
    layers, n, h, w, seed = CASES[case_id]
    mode, gather, (ftol, gtol) = MODES[mode_id]
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 3, h, w), generator=gen) * 2 - 1
    dfe = torch.randn((n, NUM_CLASSES), generator=gen)
    sd = orc.alt_seeded_state(layers, NUM_CLASSES, seed + 1)
    was = alt_resnet.GATHER_GEMM[0]
    alt_resnet.GATHER_GEMM[0] = gather
    try:
        net = alt_resnet.ResNet(alt_resnet.BasicBlock, list(layers), num_classes=NUM_CLASSES, compute_dtype=mode)
        net.load_state_dict(sd)
        net = net.cuda()
        with L.f32_mma(L.mma_code(mode)), torch.no_grad():
            feats, saved = alt_resnet._forward(net, x.cuda(), mode)
            pat = _hip_patterns(saved, layers)
            grads = alt_resnet._backward(net, saved, dfe.cuda())
        torch.cuda.synchronize()
    finally:
        alt_resnet.GATHER_GEMM[0] = was
    names = [k for k, _s in orc.alt_state_dict_spec(layers, NUM_CLASSES)]
    assert len(names) == len(grads)
    sd64 = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    f64 = orc.alt_backbone(sd64, x.double(), layers, patterns=pat)
    f64.backward(dfe.double())
    ferr = float((feats.double().cpu() - f64.detach()).abs().max() / f64.detach().abs().max())
    errs = {}
    for k, g in zip(names, grads):
        g64 = sd64[k].grad
        assert tuple(g.shape) == tuple(g64.shape), k
        errs[k] = float((g.double().cpu() - g64).norm() / g64.norm())
    worst = sorted(errs, key=errs.get, reverse=True)[:3]
    print(f"alt own-pattern VJP [{case_id}, {mode_id}]: features {ferr:.2e}; worst gradients " +
          ", ".join(f"{k} {errs[k]:.2e}" for k in worst))
    assert bool(torch.isfinite(feats).all())
    assert ferr < ftol, ferr
    for k, e in errs.items():
        assert e < gtol, (k, e)
