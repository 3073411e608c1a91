"""-m gpu: the one-launch backward of a stage-entry block (mil_conv_entry_bwd, bf16, the 20 -> 40 and 40 -> 60 channel entries) against the
two launches it replaces and against fp64.

  * dx is held to `torch.equal` with ops.conv_dgrad_s2 (same parity-class arithmetic), padded and dense layout;
  * dW1, db1, dWproj are held to a DERIVED bound against an fp64 CPU computation from the same bf16 inputs.  A product of two
    bf16 values is exact in fp32, so all of an element's error is summation error: K products summed in fp32 in any order
    (MFMA k-steps, the workgroup's tile walk, the slab reduction) are within (K - 1) * u * sum_q |a_q * b_q| of the exact sum,
    u = 2^-24, and every store of a rounded result (the final one; with accumulate=1 the addition onto the caller's value)
    adds u * |value stored|.  K = the number of summed pixels, n * h * w.  The bound is evaluated per element in fp64.
    ops.conv_wgrad_pair is held to the same bound on the same inputs, so a wrong bound is noticed.
  * On the launcher's own grid the weight gradients are also `torch.equal` to ops.conv_wgrad_pair's: same tiles, same
    workgroups, same k-step order — which is what keeps a training run on this kernel on the trajectory of the two launches.
"""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import cpad, round_to, to_nhwc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
# channel pair, n, H, W, grid cap (MIL_RES_GRID_CAP; None: the launcher's own grid).  The 40 -> 60 kernel works on 16x16-pixel
# tiles, the 20 -> 40 kernel on tiles 32 pixels wide and 16 high, and only on maps with a side above 16 pixels
CASES = [
    ((40, 60), 1, 16, 16, None),      # one tile, all four borders
    ((40, 60), 3, 32, 32, 5),         # interior tile seams, odd image count; 12 tiles on 5 workgroups: accumulators carry across tiles
    ((40, 60), 2, 19, 19, None),      # odd maps, ragged tiles (10x10 dz maps)
    ((20, 40), 1, 16, 32, None),      # one tile, all four borders
    ((20, 40), 3, 32, 32, 4),         # a seam in the tile row and between tile rows; 6 tiles on 4 workgroups
    ((20, 40), 3, 32, 32, None),      # the same on the launcher's own grid
    ((20, 40), 2, 19, 19, None),      # odd maps, ragged tiles in both directions
    ((20, 40), 2, 40, 70, None),      # three tiles per row, the last one ragged; three tile rows
]


@pytest.fixture(scope="module")
def ops():
    import mil_amd  # noqa: F401
    from mil_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _inputs(CIN, COUT, n, H, W, seed):
    dt = torch.bfloat16
    g = torch.Generator().manual_seed(seed)
    h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = round_to(torch.randn(n, CIN, H, W, generator=g), dt)                    # both signs: the mask takes both branches
    dz1 = round_to(torch.randn(n, COUT, h, w, generator=g), dt)
    dz2 = round_to(torch.randn(n, COUT, h, w, generator=g), dt)
    w1 = round_to(torch.randn(COUT, CIN, 3, 3, generator=g) / (9 * CIN) ** 0.5, dt)
    wp = round_to(torch.randn(COUT, CIN, 1, 1, generator=g) / CIN ** 0.5, dt)
    return x, dz1, dz2, w1, wp


def _fp64_reference(x, dz1, dz2):
    """(value, sum of |products|) in fp64 of dW1 [co,ci,3,3], db1 [co], dWproj [co,ci,1,1], and K."""
    CIN = x.shape[1]
    n, co, h, w = dz1.shape
    xd, z1, z2 = x.double(), dz1.double().reshape(n, co, h * w), dz2.double().reshape(n, co, h * w)
    cols = F.unfold(xd, 3, padding=1, stride=2)                                  # [n, ci*9, h*w], row = ci*9 + ky*3 + kx
    ctr = xd[:, :, ::2, ::2].reshape(n, CIN, h * w)
    ref = {
        "dw3": (torch.einsum("nkl,ncl->ck", cols, z1).reshape(co, CIN, 3, 3), torch.einsum("nkl,ncl->ck", cols.abs(), z1.abs()).reshape(co, CIN, 3, 3)),
        "db3": (z1.sum(dim=(0, 2)), z1.abs().sum(dim=(0, 2))),
        "dw1": (torch.einsum("nkl,ncl->ck", ctr, z2).reshape(co, CIN, 1, 1), torch.einsum("nkl,ncl->ck", ctr.abs(), z2.abs()).reshape(co, CIN, 1, 1)),
    }
    return ref, n * h * w


def _check_bound(name, got, ref, K, prior=None):
    """|got - exact| <= (K - 1) u sum|a b| + u |exact|, plus u |prior + exact| for the accumulating store."""
    val, mag = ref
    want = val if prior is None else prior.double() + val
    bound = (K - 1) * U * mag + U * val.abs()
    if prior is not None:
        bound = bound + U * want.abs()
    err = (got.double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{name}: max |err| {float(err.max()):.3e}, max err/bound {worst:.3e} (K = {K})")
    assert bool((err <= bound).all()), (name, float(err.max()), worst)


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0][0]}-{c[0][1]}-{c[1]}x{c[2]}x{c[3]}" + (f"-cap{c[4]}" if c[4] else ""))
def test_entry_backward_one_launch(ops, case, accumulate, monkeypatch):
    from mil_amd import _lib as L
    (CIN, COUT), n, H, W, cap = case
    monkeypatch.setenv("MIL_ENTRY_BWD", "1")
    if cap is not None:
        monkeypatch.setenv("MIL_RES_GRID_CAP", str(cap))
    dt = torch.bfloat16
    x, dz1, dz2, w1, wp = _inputs(CIN, COUT, n, H, W, 700 + H + CIN)
    ref, K = _fp64_reference(x, dz1, dz2)
    ws2, _ = ops.pack_weights(w1.cuda(), wp.cuda(), L.PACK_DGRAD_S2, dt)
    d1, d2, xin = to_nhwc(dz1, dt), to_nhwc(dz2, dt), to_nhwc(x, dt)
    g = torch.Generator().manual_seed(9)
    prior = [torch.randn(s, generator=g) for s in ((COUT, CIN, 3, 3), (COUT,), (COUT, CIN, 1, 1))] if accumulate else None

    def outs():
        return tuple(p.cuda().clone() for p in prior) if accumulate else None

    fused = ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT, out=outs())
    assert fused is not None
    dx, dw3, db3, dw1, _ws = fused
    # dx: the data-gradient kernel's result bit for bit, padded and dense, masked and bare
    want_dx = ops.conv_dgrad_s2(d1, d2, ws2, cpad(CIN), (H, W), act=xin)
    assert want_dx is not None and torch.equal(dx, want_dx)
    if CIN == 20:                                           # dense gradient layout: the 20-channel stage's only
        dense = ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT, dense_cx=CIN, out=outs())
        want_dense = ops.conv_dgrad_s2(d1, d2, ws2, cpad(CIN), (H, W), act=xin, dense_cx=CIN)
        assert dense is not None and dense[0].shape[-1] == CIN and torch.equal(dense[0], want_dense)
    else:
        assert ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT, dense_cx=CIN) is None
        dense = fused
    bare = ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT, masked=False, out=outs())
    assert torch.equal(bare[0], ops.conv_dgrad_s2(d1, d2, ws2, cpad(CIN), (H, W)))
    # weight gradients: the derived fp64 bound, in every variant of the call
    for tag, res in (("fused", fused), ("fused-dense", dense), ("fused-bare", bare)):
        for k, (name, got) in enumerate(zip(("dw3", "db3", "dw1"), res[1:4])):
            _check_bound(f"{tag} {name}", got, ref[name], K, prior[k] if accumulate else None)
        assert all(torch.equal(a, b) for a, b in zip(res[1:4], fused[1:4]))         # dx's layout and mask do not touch them
    # the two-launch pair on the same inputs meets the same bound (so a wrong bound is noticed)
    two = ops.conv_wgrad_pair(xin, d1, d2, CIN, COUT, out=outs())
    assert two is not None
    for k, (name, got) in enumerate(zip(("dw3", "db3", "dw1"), two[:3])):
        _check_bound(f"pair {name}", got, ref[name], K, prior[k] if accumulate else None)
    if cap is None:                                         # the launcher's own grid: the pair kernel's sums bit for bit
        assert all(torch.equal(a, b) for a, b in zip(fused[1:4], two[:3]))
    # fixed summation order: a second run gives the same bits
    again = ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT, out=outs())
    assert all(torch.equal(a, b) for a, b in zip(again[:4], fused[:4]))
    # forced off: no such kernel, the caller takes the two launches
    monkeypatch.setenv("MIL_ENTRY_BWD", "0")
    assert ops.conv_entry_bwd(d1, d2, ws2, xin, CIN, COUT) is None


def test_entry_backward_declines_what_it_does_not_own(ops, monkeypatch):
    """Other channel pairs, maps without 16x16 tiles and other dtypes return None (the caller's two launches), also forced on."""
    from mil_amd import _lib as L
    monkeypatch.setenv("MIL_ENTRY_BWD", "1")
    dt = torch.bfloat16
    for cin, cout, n, H, W in ((60, 80, 2, 16, 16), (40, 60, 4, 8, 8), (20, 40, 2, 16, 16)):      # (20 -> 40 on 16x16 maps: the pair kernel sums other tiles there)
        g = torch.Generator().manual_seed(5)
        w1 = torch.randn(cout, cin, 3, 3, generator=g)
        wp = torch.randn(cout, cin, 1, 1, generator=g)
        ws2, _ = ops.pack_weights(w1.cuda(), wp.cuda(), L.PACK_DGRAD_S2, dt)
        h, w = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        d = torch.zeros((n, h, w, cpad(cout)), dtype=dt, device="cuda")
        xin = torch.zeros((n, H, W, cpad(cin)), dtype=dt, device="cuda")
        assert ops.conv_entry_bwd(d, d, ws2, xin, cin, cout) is None
    d = torch.zeros((1, 8, 8, 40), dtype=torch.float32, device="cuda")
    assert ops.conv_entry_bwd(d, d, ws2, torch.zeros((1, 16, 16, 24), dtype=torch.float32, device="cuda"), 20, 40) is None


@pytest.mark.parametrize("size", [64, 128])
def test_both_paths_agree_through_the_model(golden_dir, size, monkeypatch):
    """The whole model, 2 bags x 8 tiles, with MIL_ENTRY_BWD=0 and =1: every forward output and EVERY parameter gradient bit for
    bit, conv1.weight, conv1.bias and downsample.0.weight of the entry blocks included (no looser bound is needed for them: the
    kernel sums in the pair kernel's order).  64x64 tiles: the entries run on maps of at most 16 / 8 pixels, where the kernel
    declines — the two runs are the same launches; 128x128 tiles: the 40 -> 60 entry on 16x16 maps and the 20 -> 40 entry on
    32x32 maps take the one launch."""
    import numpy as np
    import os
    import mil_amd
    from mil_amd import ops
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    gen = torch.Generator(device="cuda").manual_seed(77)
    x = torch.randn((16, 3, size, size), generator=gen, device="cuda").clamp_(-1, 1)
    labels = torch.tensor([1, 2])
    seen = []
    real = ops.conv_entry_bwd

    def recording(dz1, dz2, wpack, xin, cin, cout, **kw):
        res = real(dz1, dz2, wpack, xin, cin, cout, **kw)
        if res is not None:
            seen.append((cin, cout))
        return res

    monkeypatch.setattr(ops, "conv_entry_bwd", recording)
    res = {}
    for forced in ("0", "1"):
        monkeypatch.setenv("MIL_ENTRY_BWD", forced)
        net = mil_amd.Attention(3, compute_dtype=torch.bfloat16)
        net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
        net.eval()
        outs = net.forward_bags((x, [8, 8]), labels)
        torch.stack([o["loss"] for o in outs]).sum().backward()
        torch.cuda.synchronize()
        res[forced] = ([{k: o[k].detach().clone() for k in ("Aterm", "Mterm", "Fterm", "loss", "y_pred")} for o in outs],
                       {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None})
    assert seen == ([(40, 60), (20, 40)] if size == 128 else [])          # forced on: one launch each, last entry first
    for o0, o1 in zip(res["0"][0], res["1"][0]):
        for k in o0:
            assert torch.equal(o0[k], o1[k]), k
    assert len(res["0"][1]) > 60
    for k, g0 in res["0"][1].items():
        assert torch.equal(g0, res["1"][1][k]), k
