"""CPU (-m "not gpu"): the host side of tile saliency — the packing mode of the stem's data-gradient filter, the argument
checks of `mil_stem_dgrad` (status codes, decided before any GPU call) and the argument errors of `mil_amd.TileSaliency`, which
are raised before anything is launched."""
import ctypes

import pytest
import torch


def test_stem_dgrad_pack_mode_is_for_the_stem_filter_only():
    import mil_amd
    from mil_amd import _lib as L
    lib = mil_amd.lib()
    assert L.PACK_STEM_DGRAD == 4
    n = ctypes.c_size_t(0)
    assert lib.mil_packed_weight_elems(ctypes.byref(n), 20, 3, 7, 4) == 0
    assert n.value == 12 * 1 * 64 * 8                  # 16 taps x 3 groups of 8 channels = 48 k-groups = 12 k-steps, one column tile
    assert lib.mil_packed_weight_elems(ctypes.byref(n), 40, 40, 3, 4) == 2
    assert lib.mil_packed_weight_elems(ctypes.byref(n), 64, 3, 7, 4) == 2          # alt_resnet's stem: no such kernel
    job = (ctypes.c_char * lib.mil_pack_job_bytes())()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    assert lib.mil_pack_job_fill(ctypes.addressof(job), p, None, p, None, 40, 40, 3, 4, 1) == 2
    assert lib.mil_pack_job_fill(ctypes.addressof(job), p, None, p, None, 20, 3, 7, 4, 1) == 0
    assert lib.mil_pack_conv_weights(p, None, p, None, 40, 40, 3, 4, 1, None) == 2       # decided before the launch
    assert lib.mil_pack_conv_weights(p, None, p, None, 20, 3, 7, 5, 1, None) == 1        # no mode 5


def test_stem_dgrad_argument_errors_are_status_codes():
    import mil_amd
    lib = mil_amd.lib()
    one = ctypes.c_float(0)
    p = ctypes.addressof(one)
    assert lib.mil_stem_dgrad(None, None, None, None, 1, 32, 32, 0, 1, None) == 1
    assert lib.mil_stem_dgrad(p, p, None, None, 1, 32, 32, 0, 1, None) == 1        # both outputs null
    assert lib.mil_stem_dgrad(p, p, None, None, 1, 32, 32, 1, 1, None) == 1
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 32, 32, 2, 1, None) == 1              # reduce outside {0, 1}
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 32, 32, -1, 1, None) == 1
    assert lib.mil_stem_dgrad(p, p, None, p, 1, 32, 32, 0, 1, None) == 1           # reduce = 0 writes dx
    assert lib.mil_stem_dgrad(p, p, p, None, 1, 32, 32, 1, 1, None) == 1           # reduce = 1 writes sal
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 0, 32, 0, 1, None) == 1
    assert lib.mil_stem_dgrad(p, p, p, p, -1, 32, 32, 0, 1, None) == 1
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 32, 32, 0, 2, None) == 1              # the dense-gradient codes are no storage type here
    assert lib.mil_stem_dgrad(p, p, p, p, 0, 32, 32, 0, 1, None) == 0              # nothing to do: no launch
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 40000, 40000, 0, 0, None) == 2        # one image's dstem beyond a buffer descriptor
    assert lib.mil_abi_version() == 2


def test_tile_saliency_argument_errors_come_before_any_launch():
    import mil_amd
    assert "TileSaliency" in mil_amd.__all__
    model = mil_amd.Attention(3, device="cpu")
    sal = mil_amd.TileSaliency(model)
    x = torch.zeros(4, 3, 32, 32)
    for call in (sal.input_gradient, sal.maps):
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(3, 32, 32), 0)                                        # wrong rank
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(4, 1, 32, 32), 0)
        with pytest.raises(ValueError, match="S2dTiles"):
            call(mil_amd.S2dTiles(torch.zeros(4, 16, 16, 16, dtype=torch.bfloat16)), 0)
        for label in (3, -1):
            with pytest.raises(ValueError, match="label"):
                call(x, label)
        with pytest.raises(ValueError, match="U8Tiles"):
            call(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), 0)                   # bytes come wrapped
    with pytest.raises(ValueError, match="method"):
        sal.maps(x, 0, method="guided")
    with pytest.raises(ValueError, match="method"):
        sal.maps(torch.zeros(3, 32, 32), 7, method="guided")                       # the method is looked at first
    # valid arguments reach the device check: no kernel without a GPU, no silent CPU path
    with pytest.raises(RuntimeError, match="AMD GPU"):
        sal.input_gradient(x, 1)
    with pytest.raises(ValueError, match="Attention"):
        mil_amd.TileSaliency(model.cnn.module)
    wide = mil_amd.Attention(3, device="cpu")
    wide.cnn.module = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, (1, 1, 1, 1), num_classes=80)
    with pytest.raises(ValueError, match="wide encoder"):
        mil_amd.TileSaliency(wide)


def test_ops_stem_dgrad_checks_shapes_on_the_host():
    from mil_amd import ops
    d = torch.zeros(2, 16, 16, 24)
    with pytest.raises(ValueError, match="reduce"):
        ops.stem_dgrad(d, d, (32, 32), reduce="sum")
    with pytest.raises(ValueError, match="dstem"):
        ops.stem_dgrad(torch.zeros(16, 16, 24), d, (32, 32))
    with pytest.raises(ValueError, match="dstem"):                                  # a CPU tensor is refused before any launch
        ops.stem_dgrad(d, d, (32, 32))


def test_attribution_classes_share_one_module_and_keep_their_own_wording():
    import mil_amd
    from mil_amd import attribution, feature_vis, gradcam, path_attr, saliency
    for name in ("bag_setup", "bag_step", "check_tiles", "device_tiles"):
        assert getattr(saliency, name) is getattr(attribution, name), name
        assert getattr(path_attr, name) is getattr(attribution, name), name
    assert gradcam.LAYERS is feature_vis.LAYERS is attribution.LAYERS
    model = mil_amd.Attention(3, compute_dtype=torch.float32, device="cpu")
    s2d = mil_amd.S2dTiles(torch.zeros(4, 16, 16, 16, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="S2dTiles feed the bf16 compute mode only"):
        mil_amd.TileGradCam(model)._check(s2d, 0)
    with pytest.raises(ValueError, match="S2dTiles hold bf16-rounded .*: saliency takes the fp32 stack or U8Tiles"):
        saliency.check_tiles(model, s2d, 0, "saliency")
    with pytest.raises(ValueError, match="S2dTiles hold bf16-rounded .*: feature visualisation takes the fp32 stack or U8Tiles"):
        mil_amd.FeatureVisualizer(model).dream(s2d, "layer1", 0)
    assert mil_amd.TileGradCam(model, layer=2).layer == "layer2"                    # the shared layer -> stage mapping takes 1..4 too
