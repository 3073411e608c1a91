"""CPU (-m "not gpu"): the host side of Grad-CAM — the Lanczos coefficient tables of `mil_resample_coeffs` against Pillow's own
results (through the numpy restatement of tests/gradcam_reference.py and tests/golden/gradcam_lanczos.npz), the bilinear tables
against `mil_resize_coeffs`, the status codes `mil_grad_cam` decides before any GPU call, and the argument errors of
`mil_amd.TileGradCam`, which need no device either."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gradcam_reference as ref

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 2
LANCZOS, BILINEAR = 1, 2


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "gradcam_lanczos.npz"))


def _tables(in_size, out_size, filt=LANCZOS):
    import mil_amd  # noqa: F401
    from mil_amd import ops
    ks, bounds, kk = ops.resample_tables(in_size, out_size, filt, "cpu")
    assert tuple(kk.shape) == (out_size, ks) and tuple(bounds.shape) == (out_size, 2)
    return bounds.numpy(), kk.numpy()


def test_lanczos_tables_reproduce_pillow_byte_for_byte(golden):
    pairs = golden["pairs"]
    assert len(pairs) >= 12
    for i, (h, w, H, W) in enumerate(map(tuple, pairs.tolist())):
        ytab, xtab = _tables(h, H), _tables(w, W)
        for kind in ("rand", "bin"):
            src, want = golden[f"{kind}_{i}"], golden[f"{kind}_out_{i}"]
            got = ref.resize_u8(src[None], ytab, xtab, H, W)[0]
            assert want.shape == (H, W) and np.array_equal(got, want), (kind, h, w, H, W, int((got != want).sum()))


def test_lanczos_tables_have_negative_lobes_and_sum_to_one():
    bounds, kk = _tables(8, 256)
    assert kk.shape[1] == 7 and int(kk.min()) < 0                                 # support 3 -> ksize 7; the filter's side lobes
    assert np.abs(kk.sum(1) - (1 << 22)).max() <= kk.shape[1]                      # normalised, up to the roundings
    assert (bounds[:, 0] >= 0).all() and (bounds[:, 0] + bounds[:, 1] <= 8).all() and (bounds[:, 1] >= 1).all()
    down_b, down_k = _tables(64, 16)                                              # support 3 * scale = 12 -> ksize 25
    assert down_k.shape[1] == 25 and (down_b[:, 0] + down_b[:, 1] <= 64).all()
    for b, k in ((bounds, kk), (down_b, down_k)):                                 # nothing behind a row's count
        assert all(not k[i, b[i, 1]:].any() for i in range(len(k)))


def test_quantisation_restatement_is_numpys(golden):
    for i in range(3):
        cam, want = golden[f"cam_{i}"], golden[f"cam_u8_{i}"]
        lo, hi = np.float32(0), np.float32(1)
        got = ref.quantise(cam[None], value_range=(lo, hi))[0]                    # (cam - 0) / (1 - 0) is exact
        assert np.array_equal(got, want)
    const = np.full((1, 4, 5), 3.5, dtype=np.float32)
    assert not ref.quantise(const).any()                                           # where the toolkit divides by zero


@pytest.mark.parametrize("sizes", [(300, 256), (1200, 300), (50, 80), (7, 7), (1, 32), (120, 32)], ids=lambda s: f"{s[0]}to{s[1]}")
def test_bilinear_tables_are_mil_resize_coeffs(sizes):
    import mil_amd
    lib = mil_amd.lib()
    s, r = sizes
    ks_old, ks_new = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.mil_resize_plan(s, r, ctypes.byref(ks_old)) == OK and lib.mil_resample_plan(s, r, BILINEAR, ctypes.byref(ks_new)) == OK
    assert ks_old.value == ks_new.value
    b_old, b_new = np.full((r, 2), -1, np.int32), np.full((r, 2), -2, np.int32)
    k_old, k_new = np.full((r, ks_old.value), -1, np.int32), np.full((r, ks_old.value), -2, np.int32)
    assert lib.mil_resize_coeffs(s, r, b_old.ctypes.data, k_old.ctypes.data) == OK
    assert lib.mil_resample_coeffs(s, r, BILINEAR, b_new.ctypes.data, k_new.ctypes.data) == OK
    assert np.array_equal(b_old, b_new) and np.array_equal(k_old, k_new) and int(k_new.min()) >= 0


def test_resample_argument_errors():
    import mil_amd
    lib = mil_amd.lib()
    ks = ctypes.c_int(0)
    buf = np.zeros(4096, np.int32)
    p = buf.ctypes.data
    assert lib.mil_resample_plan(8, 256, LANCZOS, ctypes.byref(ks)) == OK and ks.value == 7
    assert lib.mil_resample_plan(0, 256, LANCZOS, ctypes.byref(ks)) == ERR_ARG
    assert lib.mil_resample_plan(8, 0, LANCZOS, ctypes.byref(ks)) == ERR_ARG
    assert lib.mil_resample_plan(8, 256, 0, ctypes.byref(ks)) == ERR_ARG
    assert lib.mil_resample_plan(8, 256, 3, ctypes.byref(ks)) == ERR_ARG
    assert lib.mil_resample_plan(8, 256, LANCZOS, None) == ERR_ARG
    assert lib.mil_resample_coeffs(8, 16, LANCZOS, p, p) == OK
    assert lib.mil_resample_coeffs(-1, 16, LANCZOS, p, p) == ERR_ARG
    assert lib.mil_resample_coeffs(8, 0, LANCZOS, p, p) == ERR_ARG
    assert lib.mil_resample_coeffs(8, 16, 7, p, p) == ERR_ARG
    assert lib.mil_resample_coeffs(8, 16, LANCZOS, None, p) == ERR_ARG
    assert lib.mil_resample_coeffs(8, 16, LANCZOS, p, None) == ERR_ARG


def test_grad_cam_argument_errors_are_status_codes():
    """Every status here is decided on the host, before any GPU call: the pointers are never followed."""
    import mil_amd
    lib = mil_amd.lib()
    buf = (ctypes.c_char * 64)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def call(act=p, grad=p, n=1, h=8, w=8, c=80, cs=80, dtype=1, offset=1.0, rng=None, yb=p, yk=p, yks=7, xb=p, xk=p, xks=7, raw=p,
             out=p, H=256, W=256):
        return lib.mil_grad_cam(act, grad, n, h, w, c, cs, dtype, offset, rng, yb, yk, yks, xb, xk, xks, raw, out, H, W, None)
    assert call(act=None) == ERR_ARG and call(grad=None) == ERR_ARG
    assert call(raw=None, out=None) == ERR_ARG                                     # both outputs null
    for name in ("yb", "yk", "xb", "xk"):                                          # out without one of its tables
        assert call(**{name: None}) == ERR_ARG
    assert call(n=-1) == ERR_ARG
    assert call(h=0) == ERR_ARG and call(w=0) == ERR_ARG and call(H=0) == ERR_ARG and call(W=0) == ERR_ARG
    assert call(c=0) == ERR_ARG and call(c=81) == ERR_ARG                          # c < 1, c > cs
    assert call(c=20, cs=20) == ERR_ARG and call(c=20, cs=28) == ERR_ARG           # cs % 8 != 0
    assert call(yks=3) == ERR_ARG and call(xks=9) == ERR_ARG                       # not mil_resample_plan's
    assert call(dtype=2) == ERR_ARG and call(dtype=4) == ERR_ARG and call(dtype=-1) == ERR_ARG
    for dtype in (0, 1, 3):
        assert call(n=0, dtype=dtype) == OK                                        # nothing to do: no launch
    assert call(n=0, out=None, yb=None, yk=None, xb=None, xk=None, yks=0, xks=0) == OK     # raw alone needs no table
    assert call(n=0, raw=None, c=20, cs=24) == OK
    # beyond the 160 KB of LDS: 256x256 maps; 128x128 -> 1024x1024 (its strip)
    assert call(h=256, w=256, H=512, W=512, c=20, cs=24, out=None) == ERR_UNSUPPORTED
    assert call(h=128, w=128, H=1024, W=1024, c=20, cs=24) == ERR_UNSUPPORTED
    assert call(act=p + 4) == ERR_UNSUPPORTED                                      # off the 16-byte grid


def test_ops_grad_cam_checks_shapes_on_the_host():
    from mil_amd import ops
    a = torch.zeros(2, 8, 8, 24)
    with pytest.raises(ValueError, match="one dtype"):
        ops.grad_cam(a, a.bfloat16(), 20, (64, 64))
    with pytest.raises(ValueError, match="one dtype"):
        ops.grad_cam(a, torch.zeros(2, 8, 8, 40), 20, (64, 64))
    with pytest.raises(ValueError, match="neither"):
        ops.grad_cam(a, a, 20, (64, 64), want_raw=False, want_map=False)
    with pytest.raises(ValueError, match="act"):                                    # a CPU tensor is refused before any launch
        ops.grad_cam(a, a, 20, (64, 64))


def test_tile_grad_cam_argument_errors():
    import mil_amd
    with pytest.raises(ValueError, match="Attention"):
        mil_amd.TileGradCam(torch.nn.Linear(2, 2))
    assert "TileGradCam" in mil_amd.__all__
    net = mil_amd.Attention(3, compute_dtype=torch.float32, device="cpu")
    with pytest.raises(ValueError, match="Attention"):
        mil_amd.TileGradCam(net.cnn.module)
    wide = mil_amd.Attention(3, device="cpu")
    wide.cnn.module = mil_amd.alt_resnet.ResNet(mil_amd.alt_resnet.BasicBlock, (1, 1, 1, 1), num_classes=80)
    with pytest.raises(ValueError, match="wide encoder"):
        mil_amd.TileGradCam(wide)
    with pytest.raises(ValueError, match="layer"):
        mil_amd.TileGradCam(net, layer="layer5")
    with pytest.raises(ValueError, match="layer"):
        mil_amd.TileGradCam(net, layer="conv1")
    cam = mil_amd.TileGradCam(net)
    assert cam.layer == "layer4" and cam.stage == 4 and mil_amd.TileGradCam(net, layer="layer2").stage == 2
    x = torch.zeros(4, 3, 32, 32)
    for bad in (-1, 3, 7):
        with pytest.raises(ValueError, match="label"):
            cam.raw(x, bad)
    with pytest.raises(ValueError, match="tiles"):
        cam.raw([x], 0)
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        cam.raw(torch.zeros(4, 1, 32, 32), 0)
    with pytest.raises(ValueError, match=r"\[T,3,H,W\]"):
        cam.maps(torch.zeros(3, 32, 32), 0)
    with pytest.raises(ValueError, match="floating point"):
        cam.raw(torch.zeros(4, 3, 32, 32, dtype=torch.uint8), 0)
    with pytest.raises(ValueError, match="empty"):
        cam.maps(torch.zeros(0, 3, 32, 32), 0)
    with pytest.raises(ValueError, match="normalize"):
        cam.maps(x, 0, normalize="slide")
    with pytest.raises(ValueError, match="bf16"):                                  # this model computes in fp32
        cam.raw(mil_amd.S2dTiles(torch.zeros(4, 16, 16, 16, dtype=torch.bfloat16)), 0)
    with pytest.raises(RuntimeError, match="AMD GPU"):                             # checked arguments, no device: nothing ran
        cam.raw(x, 0)
    assert all(p.grad is None for p in net.parameters())
