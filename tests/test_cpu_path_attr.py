"""CPU (-m "not gpu"): the host side of integrated gradients and SmoothGrad — the Philox4x32-10 / Box-Muller definition of
`mil_path_point`'s noise (known answers, moments), the status codes of `mil_path_point`, `mil_stem_dgrad_acc` and
`mil_attr_finish` (decided before any GPU call) and the argument errors of the wrappers and of the two classes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import path_attr_reference as ref


def test_philox_restatement_reproduces_the_known_answers():
    for counter, key, want in ref.KNOWN_ANSWERS:
        got = tuple(int(v) for v in ref.philox4x32_10(counter, key))
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    # arrays go through the same arithmetic as scalars
    cs = np.array([k[0] for k in ref.KNOWN_ANSWERS], dtype=np.uint64).T
    ks = np.array([k[1] for k in ref.KNOWN_ANSWERS], dtype=np.uint64).T
    got = np.stack(ref.philox4x32_10(cs, ks), 1)
    assert got.tolist() == [list(k[2]) for k in ref.KNOWN_ANSWERS]


def test_noise_moments_of_seed_0_sample_0():
    """CLT bounds on the fixed sequence the tests and the defaults use: |mean| <= 5 / sqrt(N), |var - 1| <= 5 sqrt(2 / N)."""
    n = 2 * 3 * 64 * 64
    z = ref.normals(n, seed=0, sample=0)
    mean, var = float(z.mean()), float(z.var())
    print(f"noise of seed 0, sample 0, N = {n}: mean {mean:.3e} (bound {5 / n ** 0.5:.3e}), var - 1 {var - 1:.3e} (bound {5 * (2 / n) ** 0.5:.3e})")
    assert bool(np.isfinite(z).all())
    assert abs(mean) <= 5 / n ** 0.5
    assert abs(var - 1) <= 5 * (2 / n) ** 0.5
    # another sample or seed is another sequence; a prefix does not depend on the length asked for
    assert not np.array_equal(ref.normals(64, 0, 1), z[:64]) and not np.array_equal(ref.normals(64, 1, 0), z[:64])
    assert np.array_equal(ref.normals(61, 0, 0), z[:61])


def test_the_pinned_seed_gives_u1_equal_to_one():
    r = ref.philox4x32_10((0, 0, 0, 0), (ref.SEED_WITH_U1_ONE, 0))
    assert int(r[0]) >> 8 == 0xffffff
    z = ref.normals(4, seed=ref.SEED_WITH_U1_ONE)
    assert z[0] == 0 and z[1] == 0 and z[2] != 0


def test_status_codes_are_decided_before_any_gpu_call():
    import mil_amd
    from mil_amd import _lib as L
    lib = mil_amd.lib()
    one = (ctypes.c_float * 4)()
    p = ctypes.addressof(one)
    for name in ("mil_path_point", "mil_stem_dgrad_acc", "mil_attr_finish"):
        assert name in L.EXPORTS
    # mil_path_point(tiles, is_u8, out, b0, b1, b2, alpha, noise_level, range, seed, sample, n, H, W, stream)
    pp = lib.mil_path_point
    assert pp(None, 0, p, 0, 0, 0, .5, 0, None, 0, 0, 1, 8, 8, None) == 1
    assert pp(p, 0, None, 0, 0, 0, .5, 0, None, 0, 0, 1, 8, 8, None) == 1
    assert pp(p, 2, p, 0, 0, 0, .5, 0, None, 0, 0, 1, 8, 8, None) == 1            # neither fp32 nor uint8
    assert pp(p, 0, p, 0, 0, 0, .5, 0, None, 0, 0, -1, 8, 8, None) == 1
    assert pp(p, 0, p, 0, 0, 0, .5, 0, None, 0, 0, 1, 0, 8, None) == 1
    assert pp(p, 0, p, 0, 0, 0, .5, 0, None, 0, 0, 1, 8, -3, None) == 1
    assert pp(p, 0, p, 0, 0, 0, .5, -0.1, None, 0, 0, 1, 8, 8, None) == 1         # a negative noise level
    assert pp(p, 0, p, 0, 0, 0, .5, float("nan"), None, 0, 0, 1, 8, 8, None) == 1
    assert pp(p, 0, p, 0, 0, 0, float("nan"), 0, None, 0, 0, 1, 8, 8, None) == 1
    assert pp(p, 0, p, 0, 0, 0, .5, 0, None, 0, 0, 1, 1 << 16, 1 << 16, None) == 2
    assert pp(p, 0, p, 0, 0, 0, .5, 0, None, 0, 0, 0, 8, 8, None) == 0            # nothing to do: no launch
    assert pp(p, 1, p, 1, 1, 1, .5, 0.2, None, 2 ** 64 - 1, 2 ** 32 - 1, 0, 8, 8, None) == 0
    # mil_stem_dgrad_acc(dstem, wpack, acc, scale, n, H, W, dtype, stream)
    da = lib.mil_stem_dgrad_acc
    assert da(None, p, p, 1.0, 1, 32, 32, 1, None) == 1
    assert da(p, None, p, 1.0, 1, 32, 32, 1, None) == 1
    assert da(p, p, None, 1.0, 1, 32, 32, 1, None) == 1
    assert da(p, p, p, 1.0, -1, 32, 32, 1, None) == 1
    assert da(p, p, p, 1.0, 1, 0, 32, 1, None) == 1
    assert da(p, p, p, 1.0, 1, 32, -1, 1, None) == 1
    for bad in (2, 4, 5, -1):                                                      # the dense-gradient codes are no storage type here
        assert da(p, p, p, 1.0, 1, 32, 32, bad, None) == 1
    for dt in (0, 1, 3):
        assert da(p, p, p, 1.0, 0, 32, 32, dt, None) == 0
    assert da(p, p, p, 1.0, 1, 40000, 40000, 0, None) == 2
    # mil_stem_dgrad still refuses a `reduce` outside {0, 1}: the accumulating form is a symbol of its own
    assert lib.mil_stem_dgrad(p, p, p, p, 1, 32, 32, 2, 1, None) == 1
    # mil_attr_finish(acc, tiles, is_u8, b0, b1, b2, attr, map, map_mode, tile_sum, ws, n, H, W, stream)
    af = lib.mil_attr_finish
    assert af(None, p, 0, 0, 0, 0, p, None, 0, None, None, 1, 8, 8, None) == 1
    assert af(p, p, 0, 0, 0, 0, None, None, 0, None, None, 1, 8, 8, None) == 1     # no output
    assert af(p, None, 0, 0, 0, 0, p, None, 2, None, None, 1, 8, 8, None) == 1     # attr reads the tiles
    assert af(p, None, 0, 0, 0, 0, None, p, 0, None, None, 1, 8, 8, None) == 1     # so do map modes 0 and 1
    assert af(p, None, 0, 0, 0, 0, None, p, 1, None, None, 1, 8, 8, None) == 1
    assert af(p, None, 0, 0, 0, 0, None, None, 2, p, p, 1, 8, 8, None) == 1        # and the sums
    assert af(p, p, 0, 0, 0, 0, None, None, 0, p, None, 1, 8, 8, None) == 1        # sums without their workspace
    for bad in (-1, 3):
        assert af(p, p, 0, 0, 0, 0, p, p, bad, None, None, 1, 8, 8, None) == 1     # a bad map mode
    assert af(p, p, 3, 0, 0, 0, p, None, 0, None, None, 1, 8, 8, None) == 1
    assert af(p, p, 0, 0, 0, 0, p, None, 0, None, None, -1, 8, 8, None) == 1
    assert af(p, p, 0, 0, 0, 0, p, None, 0, None, None, 1, 0, 8, None) == 1
    assert af(p, p, 0, 0, 0, 0, p, None, 0, None, None, 1, 8, 0, None) == 1
    assert af(p, p, 0, 0, 0, 0, p, None, 0, None, None, 1, 1 << 15, 1 << 15, None) == 2
    assert af(p, p, 0, 0, 0, 0, p, p, 1, p, p, 0, 8, 8, None) == 0                 # nothing to do: no launch
    assert af(p, None, 0, 0, 0, 0, None, p, 2, None, None, 0, 8, 8, None) == 0     # the gradient's own map needs no tiles
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mil_hip.h")
    assert L.ATTR_SLICES == 32 and "#define MIL_ATTR_SLICES 32" in open(header).read()
    # the three slice counts: the header, _lib.py, the one place the kernels define them, and the tree's numpy restatement
    import glob
    import slice_sum_reference as tree
    csrc = glob.glob(os.path.join(os.path.dirname(header), "..", "*_amd", "csrc"))[0]
    for name, value in (("ATTR", L.ATTR_SLICES), ("SEED", L.SEED_SLICES), ("REG", L.REG_SLICES)):
        line = f"#define MIL_{name}_SLICES {value}"
        assert line in open(header).read() and getattr(tree, f"{name}_SLICES") == value
        sources = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cuh")))
        assert [os.path.basename(f) for f in sources if line in open(f).read()] == ["slice_sum.cuh"]


def test_wrappers_check_their_arguments_on_the_host():
    import mil_amd
    from mil_amd import encoder, ops
    x = torch.zeros(2, 3, 8, 8)
    with pytest.raises(ValueError, match="base"):
        ops.path_point(x, 0.5, (0.0, 1.0))
    with pytest.raises(ValueError, match="noise_level"):
        ops.path_point(x, 0.5, 0.0, noise_level=-1.0)
    with pytest.raises(ValueError, match="seed"):
        ops.path_point(x, 0.5, 0.0, seed=-1)
    with pytest.raises(ValueError, match="sample"):
        ops.path_point(x, 0.5, 0.0, sample=1 << 32)
    with pytest.raises(ValueError, match="U8Tiles"):
        ops.path_point(torch.zeros(2, 3, 8, 8, dtype=torch.uint8), 0.5, 0.0)
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        ops.path_point(torch.zeros(3, 8, 8), 0.5, 0.0)
    with pytest.raises(ValueError, match="tiles"):                                 # a CPU tensor is refused before any launch
        ops.path_point(x, 0.5, 0.0)
    with pytest.raises(ValueError, match="tiles"):
        ops.path_point(mil_amd.U8Tiles(torch.zeros(2, 3, 8, 8, dtype=torch.uint8)), 0.5, 0.0)
    with pytest.raises(ValueError, match="map_mode"):
        ops.attr_finish(x, x, 0.0, want_map=True, map_mode="mean")
    with pytest.raises(ValueError, match="nothing"):
        ops.attr_finish(x, x, 0.0, want_attr=False)
    with pytest.raises(ValueError, match="acc"):
        ops.attr_finish(torch.zeros(2, 8, 8), x, 0.0)
    with pytest.raises(ValueError, match="acc"):
        ops.attr_finish(x, x, 0.0)                                                  # CPU tensors
    d = torch.zeros(2, 4, 4, 24)
    with pytest.raises(ValueError, match="dstem"):
        ops.stem_dgrad_acc(torch.zeros(4, 4, 24), d, (8, 8), x, 1.0)
    with pytest.raises(ValueError, match="dstem"):
        ops.stem_dgrad_acc(d, d, (8, 8), x, 1.0)
    # dx_acc and dx_reduce exclude each other, and the accumulator is a data gradient: decided before anything else is looked at
    with pytest.raises(ValueError, match="dx_acc"):
        encoder.encoder_backward(None, None, None, None, want_dx=True, dx_reduce="max_abs", dx_acc=(x, 1.0))
    with pytest.raises(ValueError, match="dx_acc"):
        encoder.encoder_backward(None, None, None, None, want_dx=False, dx_acc=(x, 1.0))


def test_class_argument_errors_come_before_any_launch():
    import mil_amd
    for name in ("TileIntegratedGradients", "TileSmoothGrad"):
        assert name in mil_amd.__all__
    model = mil_amd.Attention(3, device="cpu")
    IG, SG = mil_amd.TileIntegratedGradients, mil_amd.TileSmoothGrad
    with pytest.raises(ValueError, match="rule"):
        IG(model, rule="trapezoid")
    for steps in (0, -2, 2.5):
        with pytest.raises(ValueError, match="steps"):
            IG(model, steps=steps)
    for n in (0, -1, 1.5):
        with pytest.raises(ValueError, match="n must"):
            SG(model, n=n)
    with pytest.raises(ValueError, match="noise_level"):
        SG(model, noise_level=-0.1)
    for baseline in ((0.0, 1.0), (0.0,) * 4, []):
        with pytest.raises(ValueError, match="base"):
            IG(model, baseline=baseline)
    with pytest.raises(ValueError, match="baseline"):
        IG(model, baseline="pink")
    assert IG(model, baseline="white").baseline == (1.0, 1.0, 1.0) and IG(model, baseline="black").baseline == (-1.0,) * 3
    assert IG(model, baseline="grey").baseline == IG(model).baseline == (0.0, 0.0, 0.0)
    assert IG(model, baseline=(0.1, 0.2, 0.3)).baseline == (0.1, 0.2, 0.3)
    # the two rules: alphas in double, midpoint weights add up to 1, the toolkit's to (m + 1) / m
    mid, tk = IG(model, steps=4).path(), IG(model, steps=4, rule="toolkit").path()
    assert [a for a, _ in mid] == [0.125, 0.375, 0.625, 0.875] and [w for _, w in mid] == [0.25] * 4
    assert [a for a, _ in tk] == [0.0, 0.25, 0.5, 0.75, 1.0] and [w for _, w in tk] == [0.25] * 5
    wide = mil_amd.Attention(3, device="cpu")
    wide.cnn.module = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, (1, 1, 1, 1), num_classes=80)
    for cls in (IG, SG):
        with pytest.raises(ValueError, match="wide encoder"):
            cls(wide)
        with pytest.raises(ValueError, match="Attention"):
            cls(model.cnn.module)
    x = torch.zeros(4, 3, 32, 32)
    ig, sg = IG(model, steps=2), SG(model, n=2)
    for call in (ig.gradients, ig.attributions, ig.maps, ig.completeness, sg.gradients, sg.maps):
        with pytest.raises(ValueError, match="S2dTiles"):
            call(mil_amd.S2dTiles(torch.zeros(4, 16, 16, 16, dtype=torch.bfloat16)), 0)
        with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
            call(torch.zeros(3, 32, 32), 0)
        with pytest.raises(ValueError, match="label"):
            call(x, 3)
        with pytest.raises(ValueError, match="U8Tiles"):
            call(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), 0)
        with pytest.raises(RuntimeError, match="AMD GPU"):                          # valid arguments: no kernel without a GPU
            call(x, 1)
    with pytest.raises(ValueError, match="reduce"):
        ig.maps(x, 0, reduce="mean")
