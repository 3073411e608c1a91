"""-m gpu: the uint8 tile feed (csrc/u8_feed.cuh) against the fp32 feed on the decoded tensor.  Both sides run the same
arithmetic on the same 256 values, so every comparison between the two feeds is bit for bit (torch.equal / np.array_equal);
only the end-to-end case against the CPU oracles carries a tolerance — the 1e-3 gate the default compute mode is held to."""
import os

import numpy as np
import pytest
import torch

import mil_amd
from fixture_inputs import prep_inputs
from oracle import preprocess_oracle as po

pytestmark = pytest.mark.gpu
LEAK = 0.1
PREP_CASES = ["prep_s120_r32_train", "prep_s100_r37_flat", "prep_s50_r80_train", "prep_s1200_r300_train"]
MODES = [mil_amd.BF16X3, torch.bfloat16, torch.float32]


@pytest.fixture(scope="module")
def ops():
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _lib():
    from mil_amd import _lib as L
    return L


def _decode(u8):
    return mil_amd.U8Tiles(u8).float()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32 if t.dtype == torch.float32 else t.dtype)


def _tiles(n, h, w, seed, zero_image=True):
    """Random uint8 tiles; image 0 is all code 0 (decodes to -1 everywhere): a wrong padding value then shows in every border
    pixel of that image instead of in some."""
    u = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    if zero_image:
        u[0] = 0
    return u.cuda()


# ---- 4. the pre-processor's uint8 output -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PREP_CASES)
def test_preprocess_u8_output_decodes_to_the_fp32_output_and_the_golden(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    rois = torch.from_numpy(prep_inputs(z)).cuda()
    train, res, pad, roi = bool(int(z["train"])), int(z["res"]), int(z["pad"]), int(z["roi"])
    prep = mil_amd.TilePreprocessor(roi, res, pad=pad)
    params = torch.from_numpy(z["params"]) if train else None
    h = prep(rois, params, out="u8")
    assert isinstance(h, mil_amd.U8Tiles) and h.u8.dtype == torch.uint8 and h.u8.is_cuda
    f32 = prep(rois, params)
    assert tuple(h.shape) == tuple(f32.shape)
    assert torch.equal(_bits(h.float()), _bits(f32))
    want = z["out"] if "out" in z.files else np.stack([po.to_tensor_normalize(u) for u in z["out_u8"]])
    assert np.array_equal(h.float().cpu().numpy(), want)
    if "out_u8" in z.files:                                          # Pillow's own bytes
        assert np.array_equal(h.u8.cpu().numpy(), z["out_u8"].transpose(0, 3, 1, 2))
    with pytest.raises(ValueError):
        prep(rois, params, out="bytes")


# ---- 5. stem_s2d from uint8 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 37, 51), (2, 50, 70)])
def test_stem_s2d_u8_equals_stem_s2d_of_the_decoded_tensor(ops, shape, dtype):
    u = _tiles(*shape, seed=17)
    got, want = ops.stem_s2d_u8(u, dtype), ops.stem_s2d(_decode(u), dtype)
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))


# ---- 6. fused forward --------------------------------------------------------------------------------------------------------
def _stem_weights(ops, mode, seed):
    L = _lib()
    g = torch.Generator().manual_seed(seed)
    wt = (torch.randn(20, 3, 7, 7, generator=g) * 0.08).cuda()
    b = (torch.randn(20, generator=g) * 0.1).cuda()
    dt = torch.bfloat16 if mode == "bf16" else torch.float32
    return ops.pack_weights(wt, b, L.PACK_STEM, dt) + (dt,)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 36, 44), (5, 300, 300), (4, 256, 256)])
def test_stem_forward_u8_equals_the_fp32_feed_tiled(ops, shape, mode, monkeypatch):
    L = _lib()
    monkeypatch.setenv("MIL_STEM_WALK", "0")
    u = _tiles(*shape, seed=23 + shape[1])
    with L.f32_mma(L.MIL_DT_F32S if mode == "bf16x3" else L.MIL_DT_F32):
        wp, bp, dt = _stem_weights(ops, mode, 5)
        got = ops.stem_fwd_fused_u8(u, wp, bp, 24, dtype=dt)
        want = ops.stem_fwd_fused(_decode(u), wp, bp, 24, dtype=dt, keep_s2d=False)
    assert got is not None and want is not None
    (pool, widx), (_xs, pool_f, widx_f) = got, want
    torch.cuda.synchronize()
    assert torch.equal(_bits(pool), _bits(pool_f)), float((pool.float() - pool_f.float()).abs().max())
    assert torch.equal(widx, widx_f), int((widx != widx_f).sum())


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_stem_forward_u8_row_walk_equals_tiled_and_the_fp32_feed(ops, mode, monkeypatch):
    L = _lib()
    u = _tiles(8, 256, 256, seed=29)
    with L.f32_mma(L.MIL_DT_F32S if mode == "bf16x3" else L.MIL_DT_F32):
        wp, bp, dt = _stem_weights(ops, mode, 6)
        monkeypatch.setenv("MIL_STEM_WALK", "1")
        walk = ops.stem_fwd_fused_u8(u, wp, bp, 24, dtype=dt)
        walk_f = ops.stem_fwd_fused(_decode(u), wp, bp, 24, dtype=dt, keep_s2d=False)
        monkeypatch.setenv("MIL_STEM_WALK", "0")
        tiled = ops.stem_fwd_fused_u8(u, wp, bp, 24, dtype=dt)
    torch.cuda.synchronize()
    assert walk is not None and tiled is not None and walk_f is not None
    for a, b in ((walk, tiled), (walk, walk_f[1:])):
        assert torch.equal(_bits(a[0]), _bits(b[0])), float((a[0].float() - b[0].float()).abs().max())
        assert torch.equal(a[1], b[1]), int((a[1] != b[1]).sum())


def test_stem_forward_u8_refuses_what_the_fused_kernels_cannot_do(ops):
    L = _lib()
    wp, bp, dt = _stem_weights(ops, "bf16", 7)
    assert ops.stem_fwd_fused_u8(_tiles(2, 50, 70, seed=1), wp, bp, 24) is None            # W % 4 != 0
    assert ops.stem_fwd_fused_u8(_tiles(2, 33, 64, seed=1), wp, bp, 24) is None            # odd H
    assert ops.stem_fwd_fused_u8(_tiles(2, 64, 64, seed=1), wp, bp, 24, dtype=torch.float32) is None       # exact fp32: no fused stem
    with pytest.raises(ValueError):
        ops.stem_fwd_fused_u8(_decode(_tiles(2, 64, 64, seed=1)), wp, bp, 24)


# ---- 7. fused backward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("shape", [(3, 64, 64), (2, 36, 44), (5, 300, 300), (4, 256, 256)])
def test_stem_backward_u8_equals_the_fp32_feed(ops, shape, mode, dense, monkeypatch):
    """All four dtype codes (bf16 / split precision x padded / dense pooled gradient), tiled form on both sides (the bf16 row walk
    sums in another order), accumulate 0 and 1."""
    L = _lib()
    monkeypatch.setenv("MIL_STEM_WALK", "0")
    u = _tiles(*shape, seed=31 + shape[2])
    x = _decode(u)
    with L.f32_mma(L.MIL_DT_F32S if mode == "bf16x3" else L.MIL_DT_F32):
        wp, bp, dt = _stem_weights(ops, mode, 8)
        pool, widx = ops.stem_fwd_fused_u8(u, wp, bp, 24, dtype=dt)
        gp = torch.randn(pool.shape[:3] + (20 if dense else 24,), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda").to(dt)
        if not dense:
            gp[..., 20:] = 0
        got = ops.stem_bwd_fused_u8(u, gp, widx)
        want = ops.stem_bwd_fused_nchw(x, gp, widx)
        assert got is not None and want is not None
        torch.cuda.synchronize()
        assert torch.equal(_bits(got[0]), _bits(want[0])), float((got[0] - want[0]).abs().max())
        assert torch.equal(_bits(got[1]), _bits(want[1])), float((got[1] - want[1]).abs().max())
        assert float(got[0].abs().max()) > 0
        # accumulate = 1: into existing gradients
        acc_u = (torch.full((20, 3, 7, 7), 0.25, device="cuda"), torch.full((20,), -0.5, device="cuda"))
        acc_f = (acc_u[0].clone(), acc_u[1].clone())
        ops.stem_bwd_fused_u8(u, gp, widx, out=acc_u)
        ops.stem_bwd_fused_nchw(x, gp, widx, out=acc_f)
        torch.cuda.synchronize()
        assert torch.equal(_bits(acc_u[0]), _bits(acc_f[0])) and torch.equal(_bits(acc_u[1]), _bits(acc_f[1]))
        assert not torch.equal(acc_u[0], got[0])


def test_stem_backward_u8_keeps_the_tiled_form_where_the_fp32_feed_walks(ops, monkeypatch):
    """The bf16 row-walk backward reads fp32 tiles only: with the walk forced on, the uint8 feed still runs the tiled kernel (its
    result does not move), and agrees with the fp32 feed's row walk to fp32 summation order."""
    L = _lib()
    u = _tiles(4, 64, 256, seed=37)
    wp, bp, dt = _stem_weights(ops, "bf16", 9)
    pool, widx = ops.stem_fwd_fused_u8(u, wp, bp, 24, dtype=dt)
    gp = torch.randn(pool.shape, generator=torch.Generator(device="cuda").manual_seed(6), device="cuda").to(dt)
    gp[..., 20:] = 0
    monkeypatch.setenv("MIL_STEM_WALK", "0")
    dw_t, db_t = ops.stem_bwd_fused_u8(u, gp, widx)
    monkeypatch.setenv("MIL_STEM_WALK", "1")
    dw_w, db_w = ops.stem_bwd_fused_u8(u, gp, widx)
    dw_f, db_f = ops.stem_bwd_fused_nchw(_decode(u), gp, widx)
    torch.cuda.synchronize()
    assert torch.equal(dw_t, dw_w) and torch.equal(db_t, db_w)
    assert float((dw_f - dw_t).abs().max()) <= 2e-5 * float(dw_t.abs().max())              # the bound the two fp32-feed forms are held to
    assert float((db_f - db_t).abs().max()) <= 2e-5 * float(db_t.abs().max())


# ---- 8. model level ----------------------------------------------------------------------------------------------------------
def _net(golden_dir, mode, train=False):
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    net = mil_amd.Attention(3, compute_dtype=mode)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()})
    return net.train() if train else net.eval()


def _run(golden_dir, mode, feed, sizes, labels, train=False, rng=None, setup=None):
    net = _net(golden_dir, mode, train)
    if rng is not None:
        net.rng_override = rng
    if setup is not None:
        setup(net)
    outs = net.forward_bags(feed if sizes is None else (feed, sizes), labels)
    outs.loss.sum().backward()
    torch.cuda.synchronize()
    return ([{k: v.detach().clone() for k, v in o.items()} for o in outs],
            {k: p.grad.detach().clone() for k, p in net.named_parameters()})


def _same(run_a, run_b):
    assert len(run_a[0]) == len(run_b[0])
    for oa, ob in zip(run_a[0], run_b[0]):
        assert list(oa) == list(ob)
        for k in oa:
            assert torch.equal(oa[k], ob[k]), k
    assert list(run_a[1]) == list(run_b[1])
    for k, g in run_a[1].items():
        assert torch.equal(g, run_b[1][k]), k


@pytest.mark.parametrize("mode", MODES, ids=["bf16x3", "bf16", "f32"])
def test_model_on_u8tiles_equals_the_fp32_tensor_eval_ragged_bags(golden_dir, mode, monkeypatch):
    monkeypatch.setenv("MIL_PF_MIN_TILES", "1")
    h = mil_amd.U8Tiles(_tiles(24, 128, 128, seed=41))
    sizes, labels = [14, 10], torch.tensor([2, 0])
    ref = _run(golden_dir, mode, h.float(), sizes, labels)
    _same(_run(golden_dir, mode, h, sizes, labels), ref)
    # list form, and a handle that still lives on the host (moved as uint8)
    _same(_run(golden_dir, mode, [h[:14], h[14:]], None, labels), ref)
    host = mil_amd.U8Tiles(h.u8.cpu())
    _same(_run(golden_dir, mode, host, sizes, labels), ref)
    # keep_s2d = True: the library keeps its own copy of what the backward re-reads
    def keep(net):
        net.cnn.module.keep_s2d = True
    _same(_run(golden_dir, mode, h, sizes, labels, setup=keep), _run(golden_dir, mode, h.float(), sizes, labels, setup=keep))
    with pytest.raises(ValueError):                                  # one kind of feed per call
        _net(golden_dir, mode).forward_bags([h[:14], h.float()[14:]], labels)


@pytest.mark.parametrize("mode", MODES, ids=["bf16x3", "bf16", "f32"])
def test_model_on_u8tiles_equals_the_fp32_tensor_train_subsample(golden_dir, mode):
    h = mil_amd.U8Tiles(_tiles(20, 128, 128, seed=43))
    rng = {"indices": torch.tensor([3, 0, 7, 9]), "keep_mask": (torch.rand(8, 80, generator=torch.Generator().manual_seed(1)) > 0.2).to(torch.uint8)}
    labels = torch.tensor([1, 2])
    ref = _run(golden_dir, mode, [h.float()[:10], h.float()[10:]], None, labels, train=True, rng=rng)
    _same(_run(golden_dir, mode, [h[:10], h[10:]], None, labels, train=True, rng=rng), ref)
    _same(_run(golden_dir, mode, h, [10, 10], labels, train=True, rng=rng), ref)             # (x_all, sizes) form: split per bag


@pytest.mark.parametrize("mode", MODES, ids=["bf16x3", "bf16", "f32"])
def test_model_on_u8tiles_equals_the_fp32_tensor_unfused_fallback(golden_dir, mode):
    """50 x 70 tiles: W % 4 != 0, so neither feed has a fused stem — mil_stem_s2d_u8 feeds the three-call chain, forward and backward."""
    h = mil_amd.U8Tiles(_tiles(9, 50, 70, seed=47))
    sizes, labels = [5, 4], torch.tensor([0, 1])
    _same(_run(golden_dir, mode, h, sizes, labels), _run(golden_dir, mode, h.float(), sizes, labels))


@pytest.mark.parametrize("mode", MODES, ids=["bf16x3", "bf16", "f32"])
def test_hook_on_conv1_sees_the_decoded_tensor(golden_dir, mode):
    h = mil_amd.U8Tiles(_tiles(6, 64, 64, seed=53))
    seen = {}

    def setup_for(key):
        def setup(net):
            net.cnn.module.conv1.register_forward_hook(lambda m, i, o: seen.__setitem__(key, (i[0].detach().clone(), o.detach().clone())))
        return setup
    labels = torch.tensor([1])
    _same(_run(golden_dir, mode, h, [6], labels, setup=setup_for("u8")), _run(golden_dir, mode, h.float(), [6], labels, setup=setup_for("f32")))
    xin, out = seen["u8"]
    assert xin.dtype == torch.float32 and tuple(xin.shape) == (6, 3, 64, 64) and torch.equal(xin, h.float())
    assert tuple(out.shape) == (6, 20, 32, 32) and torch.equal(out, seen["f32"][1])


# ---- 9. the default-constructed module, end to end against the CPU oracles ---------------------------------------------------
def test_default_module_fed_by_the_u8_preprocessor_is_inside_the_reference_tolerance(golden_dir):
    """uint8 ROIs -> TilePreprocessor(out="u8") -> mil_amd.Attention(3).eval() against preprocess_oracle.finalize_tile ->
    mil_oracle.attention_forward: the keys and the 1e-3 gate of test_default_constructed_module_is_inside_the_reference_tolerance."""
    from oracle import mil_oracle as orc
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    rng = np.random.default_rng(5)
    n, roi, res, pad = 6, 160, 64, 20
    rois_np = rng.integers(0, 256, (n, roi, roi, 3), dtype=np.uint8)
    prep = mil_amd.TilePreprocessor(roi, res, pad=pad)
    params = prep.draw_params(n, torch.Generator().manual_seed(2))
    h = prep(torch.from_numpy(rois_np).cuda(), params, out="u8")
    net = mil_amd.Attention(3)
    assert net.compute_dtype == mil_amd.BF16X3
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()})
    net.eval()
    y = torch.tensor([1])
    out = net(h, y)
    x_ref = torch.from_numpy(np.stack([po.finalize_tile(rois_np[t], res, params[t].numpy(), pad=pad) for t in range(n)]))
    assert np.array_equal(h.float().cpu().numpy(), x_ref.numpy())
    with torch.no_grad():
        ref = orc.attention_forward(orc.load_state(w), x_ref, y)
    for k in ("Mterm", "Aterm", "y_pred", "loss", "wROIs", "Bterm"):
        err = float((out[k].detach().cpu().double() - ref[k].detach().double().reshape(out[k].shape)).abs().max())
        print(f"u8 end to end: {k} max abs err {err:.3e}")
        assert err < 1e-3, (k, err)
    assert int(out["y_pred_hat"]) == int(ref["y_pred_hat"])


# ---- 10. what holds for the fp32 tensor holds for the handle -------------------------------------------------------------------
def test_in_place_change_between_forward_and_backward_raises(golden_dir):
    h = mil_amd.U8Tiles(_tiles(6, 64, 64, seed=59, zero_image=False))
    net = _net(golden_dir, mil_amd.BF16X3)
    out = net(h, torch.tensor([1]))
    h.u8.add_(1)
    with pytest.raises(RuntimeError, match="modified in place"):
        out["loss"].backward()
    # keep_s2d = True: the library's own copy — the caller may do as it likes
    net = _net(golden_dir, mil_amd.BF16X3)
    net.cnn.module.keep_s2d = True
    out = net(h, torch.tensor([1]))
    h.u8.add_(1)
    out["loss"].backward()
    assert net.cnn.module.conv1.weight.grad is not None


def test_s2dtiles_are_still_refused_outside_bf16_mode(golden_dir, ops):
    xs = mil_amd.S2dTiles(ops.stem_s2d(_decode(_tiles(4, 64, 64, seed=61)), torch.bfloat16))
    for mode in (torch.float32, mil_amd.BF16X3):
        with pytest.raises(ValueError):
            _net(golden_dir, mode)(xs, torch.tensor([1]))
    out = _net(golden_dir, torch.bfloat16)(xs, torch.tensor([1]))
    assert torch.isfinite(out["loss"])


@pytest.mark.parametrize("mode", MODES, ids=["bf16x3", "bf16", "f32"])
def test_forward_tile_parallel_takes_a_u8tiles_slice(golden_dir, mode):
    """Without an initialised process group gather_features returns the local features: the same dict as forward."""
    h = mil_amd.U8Tiles(_tiles(8, 64, 64, seed=67))
    net = _net(golden_dir, mode)
    y = torch.tensor([2])
    a, b, c = net.forward_tile_parallel(h, y), net(h, y), net.forward_tile_parallel(h.float(), y)
    for k in b:
        assert torch.equal(a[k].detach(), b[k].detach()), k
        assert torch.equal(a[k].detach(), c[k].detach()), k
    enc = net.cnn.module
    assert torch.equal(enc(h).detach(), enc(h.float()).detach())                            # ResNet.forward takes the handle too
