"""CPU (-m "not gpu"): activation maximisation without a GPU — the optimiser formulas of `mil_pixel_step` (the numpy restatement
in fp64 against torch.optim), the byte encode / decode round trip, and every argument check of `mil_amd.FeatureVisualizer`,
`ops.stage_seed` and `ops.pixel_step`, which fire on CPU tensors before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import feature_vis_reference as ref


@pytest.mark.parametrize("wd", [0.0, 1e-6, 1e-4])
@pytest.mark.parametrize("rule", ["adam", "sgd"])
def test_the_restated_step_is_torch_optim_in_fp64(rule, wd):
    """30 steps with random gradients: the restatement in fp64 and torch.optim in fp64 agree within 1e-12 (relative to the
    largest value).  The two write the moment update differently (lerp / addcmul); nothing else separates them.  The fp32
    kernel is held to the same code bit for bit (tests/test_gpu_feature_vis.py)."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (2, 3, 9, 7))
    p = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    lr = 0.1 if rule == "adam" else 6.0
    opt = (torch.optim.Adam([p], lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8) if rule == "adam" else
           torch.optim.SGD([p], lr=lr, weight_decay=wd))
    m, v = np.zeros_like(x), np.zeros_like(x)
    for step in range(1, 31):
        g = rng.standard_normal(x.shape) * 10.0 ** rng.integers(-6, 1)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        x, m, v, _codes = ref.pixel_step(x, g, m, v, rule=rule, lr=lr, weight_decay=wd, step=step)
        want = p.detach().numpy()
        assert np.abs(x - want).max() <= 1e-12 * np.abs(want).max(), (step, np.abs(x - want).max())
    if rule == "adam":
        st = opt.state[p]
        assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 * np.abs(m).max()
        assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(v).max()


def test_encode_inverts_decode_for_all_256_codes():
    import mil_amd
    tab = ref.decode_table()
    assert np.array_equal(ref.encode(tab), np.arange(256, dtype=np.uint8))
    u = torch.arange(256, dtype=torch.uint8).view(1, 1, 16, 16).expand(1, 3, 16, 16).contiguous()
    assert np.array_equal(mil_amd.U8Tiles(u).float()[0, 0].reshape(-1).numpy(), tab)          # the table the kernel is handed
    assert np.array_equal(mil_amd.U8Tiles.decode_table("cpu").numpy(), tab)
    lib_tab = np.zeros(256, dtype=np.float32)
    assert mil_amd.lib().mil_u8_decode_table(lib_tab.ctypes.data_as(ctypes.c_void_p)) == 0
    assert np.array_equal(lib_tab, tab)
    # the ends clip, a NaN encodes as 0, and 0.0 — x / 2 + 0.5 = 0.5, times 255 = 127.5 exactly — goes to the EVEN code
    assert ref.encode(np.float32([-3.0, -1.0, 1.0, 7.0, np.nan, 0.0])).tolist() == [0, 0, 255, 255, 0, 128]


def test_entry_points_return_status_codes_without_a_gpu():
    import mil_amd
    lib = mil_amd.lib()
    assert lib.mil_stage_seed(None, None, None, None, None, 1, 8, 8, 24, 20, 0.1, 1, None) == 1
    one = ctypes.c_void_p(16)
    assert lib.mil_stage_seed(one, one, one, one, one, -1, 8, 8, 24, 20, 0.1, 1, None) == 1
    assert lib.mil_stage_seed(one, one, one, one, one, 1, 0, 8, 24, 20, 0.1, 1, None) == 1
    assert lib.mil_stage_seed(one, one, one, one, one, 1, 8, 8, 20, 20, 0.1, 1, None) == 1             # cp not a multiple of 8
    assert lib.mil_stage_seed(one, one, one, one, one, 1, 8, 8, 24, 25, 0.1, 1, None) == 1             # c > cp
    assert lib.mil_stage_seed(one, one, one, one, one, 1, 8, 8, 24, 20, 0.1, 3, None) == 1             # no such storage
    assert lib.mil_stage_seed(one, one, one, one, one, 1, 4096, 4096, 24, 20, 0.1, 1, None) == 2       # h w = 2^24
    assert lib.mil_stage_seed(one, one, one, one, one, 0, 8, 8, 24, 20, 0.1, 1, None) == 0             # nothing to do
    f9 = (0.1, 0.0, 0.9, 0.1, 0.999, 0.001, 0.1, 0.03, 1e-8)
    assert lib.mil_pixel_step(None, None, None, None, None, None, 16, 0, 0, *f9, None) == 1
    assert lib.mil_pixel_step(one, one, None, None, None, None, 16, 2, 0, *f9, None) == 1                 # rule
    assert lib.mil_pixel_step(one, one, None, None, None, None, 16, 0, 3, *f9, None) == 1                 # project
    assert lib.mil_pixel_step(one, one, None, None, None, None, 16, 1, 0, *f9, None) == 1                 # adam without moments
    assert lib.mil_pixel_step(one, one, one, one, None, None, 16, 1, 0, *(f9[:6] + (0.0,) + f9[7:]), None) == 1   # bc1 == 0
    assert lib.mil_pixel_step(one, one, None, None, None, None, 16, 0, 2, *f9, None) == 1                 # "u8" without the table
    assert lib.mil_pixel_step(one, one, None, None, None, None, 16, 0, 0, *((float("nan"),) + f9[1:]), None) == 1
    assert lib.mil_pixel_step(one, one, None, None, None, None, 0, 0, 0, *f9, None) == 0


def test_wrapper_argument_checks_fire_on_cpu_tensors():
    import mil_amd  # noqa: F401
    from mil_amd import ops
    act = torch.zeros(2, 5, 7, 24)
    ch = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA"):
        ops.stage_seed(act, ch, 20)
    with pytest.raises(ValueError, match="stored"):
        ops.stage_seed(act, ch, 30)
    with pytest.raises(ValueError, match="stored"):
        ops.stage_seed(act, ch, 0)
    with pytest.raises(ValueError, match=r"\[T,h,w,cp\]"):
        ops.stage_seed(act[0], ch, 20)
    with pytest.raises(ValueError):
        ops.stage_seed(act.to(torch.float16), ch, 20)
    x = torch.zeros(2, 3, 5, 7)
    with pytest.raises(ValueError, match="CUDA"):
        ops.pixel_step(x, x.clone(), (x.clone(), x.clone()))
    with pytest.raises(ValueError, match="rule"):
        ops.pixel_step(x, x, None, rule="momentum")
    with pytest.raises(ValueError, match="project"):
        ops.pixel_step(x, x, None, rule="sgd", project="tanh")
    with pytest.raises(ValueError, match="state"):
        ops.pixel_step(x, x, None, rule="adam")
    with pytest.raises(ValueError, match="state"):
        ops.pixel_step(x, x, (x, x), rule="sgd")
    with pytest.raises(ValueError, match="step"):
        ops.pixel_step(x, x, None, rule="sgd", step=0)
    with pytest.raises(ValueError, match="betas"):
        ops.pixel_step(x, x, (x, x), betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="weight_decay"):
        ops.pixel_step(x, x, None, rule="sgd", weight_decay=-1.0)
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        ops.pixel_step(x[:, :2], x, None, rule="sgd")


def test_feature_visualizer_argument_checks_fire_without_a_gpu():
    import mil_amd
    model = mil_amd.Attention(3, device="cpu")
    fv = mil_amd.FeatureVisualizer(model)
    assert (fv.optimizer, fv.lr, fv.weight_decay, fv.betas, fv.eps, fv.project) == ("adam", 0.1, 1e-6, (0.9, 0.999), 1e-8, "none")
    bare = mil_amd.FeatureVisualizer(model.cnn.module, "sgd", lr=6, weight_decay=0, project="u8")
    with pytest.raises(ValueError, match="Attention"):
        mil_amd.FeatureVisualizer(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="wide encoder"):
        mil_amd.FeatureVisualizer(mil_amd.alt_resnet.ResNet(layers=(1, 1, 1, 1), num_classes=8))
    for kw in (dict(optimizer="rmsprop"), dict(project="tanh"), dict(betas=(0.9,)), dict(betas=(0.9, 1.0)), dict(weight_decay=-1),
               dict(eps=-1.0), dict(lr=float("nan"))):
        with pytest.raises(ValueError):
            mil_amd.FeatureVisualizer(model, **kw)
    tiles = torch.zeros(2, 3, 32, 32)
    bad_calls = [
        lambda: fv.filters("layer5"),
        lambda: fv.filters(0),
        lambda: fv.filters("layer1", channels=[20]),
        lambda: fv.filters("layer2", channels=[-1]),
        lambda: fv.filters("layer2", channels=[]),
        lambda: fv.filters("layer2", channels=[1.5]),
        lambda: fv.filters("layer1", size=(0, 32)),
        lambda: fv.filters("layer1", size=32),
        lambda: fv.filters("layer1", steps=0),
        lambda: fv.filters("layer1", steps=2.5),
        lambda: fv.filters("layer1", init=(180, 150)),
        lambda: fv.filters("layer1", init=(0, 257)),
        lambda: fv.dream(tiles, "layer1", [0]),                                  # one channel per tile
        lambda: fv.dream(tiles, "layer1", None),
        lambda: fv.dream(tiles, "layer1", 20),
        lambda: fv.dream(tiles[:, :2], "layer1", 0),
        lambda: fv.dream(tiles.to(torch.uint8), "layer1", 0),
        lambda: fv.dream(mil_amd.S2dTiles(torch.zeros((2, 16, 16, 16), dtype=torch.bfloat16)), "layer1", 0),
        lambda: fv.dream(tiles[:0], "layer1", 0),
        lambda: fv.dream(tiles, "layer1", 0, steps=0),
        lambda: fv.objective(tiles, "layer9", 0),
        lambda: fv.objective(tiles, "layer3", [0, 60]),
        lambda: fv.classes(3, 4),
        lambda: fv.classes(-1, 4),
        lambda: fv.classes(1.0, 4),
        lambda: fv.classes(1, 1),                                                # the head's batch norm refuses a single tile
        lambda: fv.classes(1, 4, size=(32,)),
        lambda: fv.classes(1, 4, steps=0),
        lambda: fv.classes(1, 4, init=(5, 5)),
        lambda: bare.classes(1, 4),                                              # the bare encoder has no head
    ]
    for i, call in enumerate(bad_calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {i} was accepted")
    # a well-formed call gets as far as the device check: the model is on the CPU
    for call in (lambda: fv.filters("layer1", channels=[0], size=(32, 32), steps=1), lambda: fv.dream(tiles, 2, 0, steps=1),
                 lambda: fv.objective(mil_amd.U8Tiles(tiles.to(torch.uint8)), "layer4", [0, 79]), lambda: fv.classes(2, 4, size=(32, 32), steps=1)):
        with pytest.raises(RuntimeError, match="AMD GPU"):
            call()


def test_encoder_plumbing_argument_checks():
    import mil_amd
    from mil_amd import encoder
    net = mil_amd.Attention(3, device="cpu").cnn.module
    with pytest.raises(ValueError, match="upto"):
        encoder.encoder_forward(net, torch.zeros(1, 3, 32, 32), torch.float32, upto=5)
    saved = {"blocks": [(None, None, torch.zeros(1, 8, 8, 24))] * 3}
    with pytest.raises(ValueError, match="either"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32)
    with pytest.raises(ValueError, match="either"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dz=torch.zeros(1), stage=1, dfeats=torch.zeros(1, 80))
    with pytest.raises(ValueError, match="stage"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dz=torch.zeros(1, 8, 8, 24), stage=0)
    with pytest.raises(ValueError, match="stopped below"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dz=torch.zeros(1, 4, 4, 40), stage=2)
    with pytest.raises(ValueError, match="like the output"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dz=torch.zeros(1, 8, 8, 20), stage=1)
    with pytest.raises(ValueError, match="whole forward"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dfeats=torch.zeros(1, 80))
    with pytest.raises(ValueError, match="no stage"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dfeats=torch.zeros(1, 80), stage=4)
    with pytest.raises(ValueError, match="dx_acc"):
        encoder.encoder_pixel_gradient(net, saved, torch.float32, dz=torch.zeros(1, 8, 8, 24), stage=1, dx_reduce="max_abs", dx_acc=(None, 1.0))
