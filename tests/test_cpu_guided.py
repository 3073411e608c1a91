"""CPU (-m "not gpu"): guided backpropagation — the restated rule of tests/guided_reference.py against the toolkit's expression
and against the oracle, the host-side checks of the four new entry points, and the argument errors of the wrappers and of
`mil_amd.TileGuidedBackprop` / `mil_amd.TileGuidedGradCam`, which come before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import guided_reference as gref
from fixture_inputs import synth_bag
from oracle import mil_oracle as orc


def test_guided_leaky_backward_is_the_toolkits_hook():
    """guided_backprop.py:41-50: (out > 0) * clamp(grad, min=0), non-negative; clamp=False: the ReLU derivative on the pattern."""
    g = torch.Generator().manual_seed(3)
    v = torch.randn(4, 7, 9, 5, dtype=torch.float64, generator=g).requires_grad_()
    grad = torch.randn(4, 7, 9, 5, dtype=torch.float64, generator=g)
    y = gref.GuidedLeaky.apply(v, v.detach() > 0)
    assert torch.equal(y, torch.nn.functional.leaky_relu(v, orc.LEAK))
    y.backward(grad)
    want = (y.detach() > 0) * torch.clamp(grad, min=0)
    assert torch.equal(v.grad, want) and float(v.grad.min()) >= 0 and float(v.grad.max()) > 0
    assert int((v.grad != grad * torch.where(v.detach() > 0, 1.0, orc.LEAK)).sum()) > v.numel() // 2      # not the plain derivative
    v2 = v.detach().clone().requires_grad_()
    gref.GuidedLeaky.apply(v2, v2.detach() > 0, False).backward(grad)
    assert torch.equal(v2.grad, (v2.detach() > 0) * grad)


def test_unclamped_reference_is_the_oracles_gradient_with_slope_zero(golden_dir, monkeypatch):
    """With the clamp removed the rule is a ReLU's derivative at every activation: on one pattern, the input gradient of the
    reference equals that of `orc.backbone(patterns=)` with the slope set to 0 (the forward values differ, the linear map of the
    backward does not).  The clamped gradient differs from both, and is what reaches the pixels through non-negative gates."""
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    sd = {k: torch.tensor(w[k], dtype=torch.float64) for k, _s in orc.state_dict_spec()}
    x = synth_bag(2, 33, 37, 20260207).double()
    pat = gref.oracle_patterns(sd, x)
    dfe = torch.randn(2, 80, dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    # the pattern reproduces the un-patterned forward: the reference's forward is the network's
    assert torch.allclose(gref.backbone(sd, x, pat), orc.backbone(sd, x), rtol=1e-12, atol=1e-14)

    def grad_of(fn):
        xg = x.clone().requires_grad_()
        fn(xg).backward(dfe)
        return xg.grad
    unclamped = grad_of(lambda xg: gref.backbone(sd, xg, pat, clamp=False))
    guided = grad_of(lambda xg: gref.backbone(sd, xg, pat))
    plain = grad_of(lambda xg: orc.backbone(sd, xg, patterns=pat))
    monkeypatch.setattr(orc, "LEAK", 0.0)
    relu = grad_of(lambda xg: orc.backbone(sd, xg, patterns=pat))
    assert float((unclamped - relu).norm() / relu.norm()) < 1e-12
    assert float(guided.norm()) > 0 and float((guided - plain).norm() / guided.norm()) > 0.1
    assert float((guided - relu).norm() / guided.norm()) > 0.1


def test_guided_entry_points_check_their_arguments_on_the_host():
    """Status codes decided before any GPU call (1: MIL_ERR_ARG, 2: MIL_ERR_UNSUPPORTED, 0 where there is nothing to do)."""
    import mil_amd
    lib = mil_amd.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    # mil_conv_dgrad_rule(x, wpack, bias, res, act, y, n, H, W, cin_p, Ho, Wo, cout_p, ks, stride, pad, zins, lrelu, slope, rule, dtype, stream)
    cr = lib.mil_conv_dgrad_rule
    assert cr(p, p, None, None, None, p, 1, 8, 8, 24, 8, 8, 24, 3, 1, 1, 0, 0, 0.1, 1, 1, None) == 1      # rule 1 without act
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 24, 3, 1, 1, 0, 0, 0.1, 2, 1, None) == 1         # rule outside {0, 1}
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 24, 3, 1, 1, 0, 0, 0.1, -1, 1, None) == 1
    assert cr(None, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 24, 3, 1, 1, 0, 0, 0.1, 1, 1, None) == 1
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 24, 3, 1, 1, 0, 0, 0.1, 1, 2, None) == 1         # the dense-gradient codes are no storage type here
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 24, 5, 1, 1, 0, 0, 0.1, 1, 1, None) == 1
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 8, 8, 40, 3, 1, 1, 0, 0, 0.1, 1, 1, None) == 2         # a forward shape: not a data gradient of the walk
    assert cr(p, p, None, None, p, p, 1, 8, 8, 24, 4, 4, 24, 3, 2, 1, 0, 0, 0.1, 0, 1, None) == 2         # stride 2 without zero-insert
    # mil_maxpool_bwd_guided(gy, widx, gx, n, H, W, cp, dtype, stream)
    mp = lib.mil_maxpool_bwd_guided
    assert mp(p, p, None, 1, 8, 8, 24, 1, None) == 1
    assert mp(p, p, p, 1, 8, 8, 20, 1, None) == 1
    assert mp(p, p, p, 1, 8, 8, 24, 3, None) == 1
    assert mp(p, p, p, 1, 0, 8, 24, 1, None) == 1
    assert mp(p, p, p, 0, 8, 8, 24, 1, None) == 0
    # mil_avgpool_fc_bwd_data_guided(dfeats, wfc, act, dz, n, hw, cp, c, nf, dtype, stream)
    ap = lib.mil_avgpool_fc_bwd_data_guided
    assert ap(p, p, None, p, 1, 4, 80, 80, 80, 1, None) == 1                                                # the gate needs act
    assert ap(p, p, p, p, 1, 4, 84, 80, 80, 1, None) == 1
    assert ap(p, p, p, p, 1, 4, 72, 80, 80, 1, None) == 1
    assert ap(p, p, p, p, 1, 0, 80, 80, 80, 1, None) == 1
    assert ap(p, p, p, p, 1, 4, 80, 80, 80, 3, None) == 1
    assert ap(p, p, p, p, 0, 4, 80, 80, 80, 0, None) == 0
    # mil_stem_dgrad_gated(dstem, wpack, gate, dx, n, H, W, dtype, stream): its siblings' rules
    sg = lib.mil_stem_dgrad_gated
    assert sg(p, p, None, p, 1, 32, 32, 1, None) == 1
    assert sg(p, p, p, None, 1, 32, 32, 1, None) == 1
    assert sg(None, p, p, p, 1, 32, 32, 1, None) == 1
    assert sg(p, p, p, p, 1, 0, 32, 1, None) == 1
    assert sg(p, p, p, p, -1, 32, 32, 1, None) == 1
    assert sg(p, p, p, p, 1, 32, 32, 2, None) == 1
    assert sg(p, p, p, p, 0, 32, 32, 3, None) == 0
    assert sg(p, p, p, p, 1, 40000, 40000, 0, None) == 2                                                    # one image's dstem beyond a buffer descriptor
    assert lib.mil_abi_version() == 2


def test_ops_wrappers_refuse_bad_rule_and_gate_arguments():
    from mil_amd import ops
    d = torch.zeros(2, 16, 16, 24)
    with pytest.raises(ValueError, match="gate"):
        ops.stem_dgrad(d, d, (32, 32), reduce="max_abs", gate=torch.zeros(2, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="gate"):                                     # nor with a caller's sal: it would not be written
        ops.stem_dgrad(d, d, (32, 32), sal=torch.zeros(2, 32, 32), gate=torch.zeros(2, 32, 32, dtype=torch.uint8))
    with pytest.raises(ValueError, match="act is required"):
        ops.conv_dgrad_rule(d, d, 24, ks=3, pad=1, rule=1)
    for bad in (2, -1, "guided", None, True):
        with pytest.raises(ValueError, match="rule"):
            ops.conv_dgrad_rule(d, d, 24, ks=3, pad=1, rule=bad, act=d)
        with pytest.raises(ValueError, match="rule"):
            ops.maxpool_bwd(d, torch.zeros(2, 16, 16, 24, dtype=torch.uint8), (32, 32), rule=bad)
        with pytest.raises(ValueError, match="rule"):
            ops.avgpool_fc_bwd_data(torch.zeros(2, 80), torch.zeros(80, 80), torch.zeros(2, 80), torch.zeros(2, 2, 2, 80), rule=bad)
    with pytest.raises(ValueError, match="zero_insert"):
        ops.conv_dgrad_rule(d, d, 24, ks=3, pad=1, rule=0, zero_insert=True)
    with pytest.raises(ValueError, match="stride-2"):
        ops.conv_dgrad_rule(d, d, 24, ks=3, pad=1, rule=0, zero_insert=True, out_hw=(30, 32))
    with pytest.raises(ValueError, match="wpack"):                                   # a CPU tensor is refused before any launch
        ops.conv_dgrad_rule(d, d, 24, ks=3, pad=1, rule=0)
    with pytest.raises(ValueError, match="lrelu_mask"):
        ops.maxpool_bwd(d, torch.zeros(2, 16, 16, 24, dtype=torch.uint8), (32, 32), lrelu_mask=False, rule=1)
    with pytest.raises(ValueError, match="masked"):
        ops.avgpool_fc_bwd_data(torch.zeros(2, 80), torch.zeros(80, 80), torch.zeros(2, 80), torch.zeros(2, 2, 2, 80), masked=False, rule=1)


def test_encoder_pixel_gradient_refuses_unknown_rules_and_gate_with_a_reduction():
    import mil_amd
    from mil_amd.encoder import encoder_pixel_gradient
    net = mil_amd.Attention(3, device="cpu").cnn.module
    dfe = torch.zeros(2, 80)
    gate = torch.zeros(2, 32, 32, dtype=torch.uint8)
    with pytest.raises(ValueError, match="rule"):
        encoder_pixel_gradient(net, {}, torch.float32, dfeats=dfe, rule="deconvnet")
    with pytest.raises(ValueError, match="gate"):
        encoder_pixel_gradient(net, {}, torch.float32, dfeats=dfe, rule="guided", gate=gate, dx_reduce="max_abs")
    with pytest.raises(ValueError, match="gate"):
        encoder_pixel_gradient(net, {}, torch.float32, dfeats=dfe, gate=gate, dx_acc=(torch.zeros(2, 3, 32, 32), 1.0))


def test_guided_classes_argument_errors_come_before_any_launch():
    import mil_amd
    assert "TileGuidedBackprop" in mil_amd.__all__ and "TileGuidedGradCam" in mil_amd.__all__
    model = mil_amd.Attention(3, device="cpu")
    gb = mil_amd.TileGuidedBackprop(model)
    cam = mil_amd.TileGuidedGradCam(model)
    assert cam.layer == "layer4" and mil_amd.TileGuidedGradCam(model, 2).layer == "layer2"
    x = torch.zeros(4, 3, 32, 32)
    s2d = mil_amd.S2dTiles(torch.zeros(4, 16, 16, 16, dtype=torch.bfloat16))
    for call in (gb.gradients, gb.maps, cam.gradients):
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(3, 32, 32), 0)
        with pytest.raises(ValueError, match="S2dTiles"):
            call(s2d, 0)
        for label in (3, -1):
            with pytest.raises(ValueError, match="label"):
                call(x, label)
        with pytest.raises(ValueError, match="U8Tiles"):
            call(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), 0)
        with pytest.raises(RuntimeError, match="AMD GPU"):                          # valid arguments reach the device check
            call(x, 1)
    with pytest.raises(ValueError, match="normalize"):
        cam.gradients(x, 0, normalize="slide")
    with pytest.raises(ValueError, match="layer"):
        mil_amd.TileGuidedGradCam(model, "layer5")
    # filters: layer, tiles, then the channels — one per tile or one for all, inside the stage's width
    with pytest.raises(ValueError, match="layer"):
        gb.filters(x, "stem", 0)
    with pytest.raises(ValueError, match="S2dTiles"):
        gb.filters(s2d, "layer2", 0)
    with pytest.raises(ValueError, match=r"\[0, 40\)"):
        gb.filters(x, "layer2", 40)
    with pytest.raises(ValueError, match=r"\[0, 20\)"):
        gb.filters(x, "layer1", [0, 1, 2, -1])
    with pytest.raises(ValueError, match="3 channels for 4 tiles"):
        gb.filters(x, "layer2", [0, 1, 2])
    with pytest.raises(RuntimeError, match="AMD GPU"):
        gb.filters(x, "layer2", [0, 1, 2, 39])
    for cls in (mil_amd.TileGuidedBackprop, mil_amd.TileGuidedGradCam):
        with pytest.raises(ValueError, match="Attention"):
            cls(model.cnn.module)
        wide = mil_amd.Attention(3, device="cpu")
        wide.cnn.module = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, (1, 1, 1, 1), num_classes=80)
        with pytest.raises(ValueError, match="wide encoder"):
            cls(wide)
