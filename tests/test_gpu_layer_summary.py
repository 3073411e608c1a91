"""-m gpu: the device summaries (csrc/tensor_stats.hip, mil_amd.summary) against numpy fp64 on the host copy of the same bits.

Bounds.  Counts, min, max and the element count are EQUAL.  A sum of n finite fp64 terms taken in ANY order is within
(n - 1) * 2^-53 * sum|x| * (1 + O(n 2^-53)) of the exact sum; `math.fsum` is the correctly rounded exact sum (one more 2^-53
relative).  The tests hold sum and sum of squares to n * 2^-52 * sum|x| and n * 2^-52 * sum x^2: that bound with one factor of
two for the reference's own rounding.  It is not a measured tolerance.  (Squares of fp32 / bf16 values are exact in fp64.)"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
F32, BF16 = 0, 1
NAN, INF = float("nan"), float("inf")


# ---- reference ---------------------------------------------------------------------------------------------------------------------
def _ref(real):
    """fp64 record of the REAL elements (any shape) of a host array."""
    v = np.asarray(real, np.float64).reshape(-1)
    f = v[np.isfinite(v)]
    n = int(f.size)
    return {"n": n, "sum": math.fsum(f), "sumsq": math.fsum(f * f), "abs": math.fsum(np.abs(f)),
            "min": float(f.min()) if n else INF, "max": float(f.max()) if n else -INF,
            "neg": int((f < 0).sum()), "bad": int(v.size - n), "total": int(v.size)}


def _check(rec, ref, what=""):
    rec = [float(x) for x in rec]
    print(f"{what}: n={ref['n']} sum err {abs(rec[1] - ref['sum']):.3e} (bound {ref['n'] * EPS * ref['abs']:.3e}) "
          f"sumsq err {abs(rec[2] - ref['sumsq']):.3e} (bound {ref['n'] * EPS * ref['sumsq']:.3e})")
    assert rec[0] == ref["n"] and rec[5] == ref["neg"] and rec[6] == ref["bad"] and rec[7] == ref["total"], (what, rec, ref)
    assert rec[3] == ref["min"] and rec[4] == ref["max"], (what, rec, ref)
    assert abs(rec[1] - ref["sum"]) <= ref["n"] * EPS * ref["abs"], (what, rec[1], ref["sum"])
    assert abs(rec[2] - ref["sumsq"]) <= ref["n"] * EPS * ref["sumsq"], (what, rec[2], ref["sumsq"])


def _host64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


# ---- the C ABI with `out` and `ws` filled with 0xFF bytes and guarded -------------------------------------------------------------------
def _run_abi(entries):
    """entries: [(tensor, n_pix, c_real, c_pad)] -> [n, 8] float64 host records."""
    import mil_amd
    lib = mil_amd.lib()
    n, rec = len(entries), lib.mil_stats_job_bytes()
    host = (ctypes.c_char * (rec * n))()
    guard = torch.full((8,), 1.5, dtype=torch.float64, device="cuda")
    for i, (t, n_pix, c_real, c_pad) in enumerate(entries):
        dt = {torch.float32: F32, torch.bfloat16: BF16}[t.dtype]
        assert lib.mil_stats_job_fill(ctypes.byref(host, i * rec), t.data_ptr() or guard.data_ptr(), n_pix, c_real, c_pad, dt) == 0
    need = ctypes.c_size_t(0)
    assert lib.mil_tensor_stats_workspace(ctypes.byref(need), host, n) == 0 and need.value > 0 and need.value % 8 == 0
    table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).cuda()
    ws = torch.full((need.value + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + 1) * 64,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = lib.mil_tensor_stats_all(table.data_ptr(), host, n, out.data_ptr(), ws.data_ptr(), need.value, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert bool((ws[need.value:] == 0xFF).all()) and bool((out[n * 64:] == 0xFF).all())          # nothing behind what the call owns
    recs = out[:n * 64].view(torch.float64).view(n, 8).cpu()
    assert not bool(torch.isnan(recs).any()), recs                                               # every word of out written (0xFF.. is a NaN)
    return recs


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def _specials(dtype):
    fi = torch.finfo(dtype)
    return [NAN, INF, -INF, -0.0, 1e-40, -3e-42, fi.max, fi.min, fi.tiny, -fi.tiny, 0.0]


def _padded(n_pix, c_pad, c_real, dtype, seed):
    """[n_pix, c_pad] device tensor: real channels random with the specials planted, pad channels NaN and 3e38."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_pix, c_pad, generator=g) * 3.0
    x[:, c_real:] = NAN
    x[::2, c_real:] = 3e38
    real = n_pix * c_real
    if real >= 64:
        pos = torch.randperm(real, generator=g)[:33]
        for k, p in enumerate(pos.tolist()):
            x[p // c_real, p % c_real] = _specials(dtype)[k % 11]
    return x.to(dtype).cuda().contiguous()


SHAPES = {"3x5x7x24r20": ((3, 5, 7, 24), 20), "2x3x3x40": ((2, 3, 3, 40), 40), "1x4x4x64": ((1, 4, 4, 64), 64),
          "5x1x1x80": ((5, 1, 1, 80), 80), "70001x24r20": ((70001, 24), 20), "0x24r20": ((0, 24), 20), "0x1": ((0, 1), 1)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_kernel_matches_numpy_on_padded_tensors(shape, dtype):
    dims, c_real = SHAPES[shape]
    c_pad = dims[-1]
    n_pix = int(np.prod(dims[:-1]))
    x = _padded(n_pix, c_pad, c_real, dtype, seed=len(shape) * 7 + c_pad).view(dims)
    before = x.clone()
    rec = _run_abi([(x, n_pix, c_real, c_pad)])[0]
    _check(rec, _ref(_host64(x).reshape(n_pix, c_pad)[:, :c_real]), f"{shape} {dtype}")
    assert torch.equal(x.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), before.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    if n_pix == 0:
        assert rec.tolist() == [0, 0, 0, INF, -INF, 0, 0, 0]
    # the public entry point gives the same bits
    import mil_amd
    pub = mil_amd.tensor_stats([(x, c_real)])
    assert pub.dtype == torch.float64 and pub.is_cuda and tuple(pub.shape) == (1, 8)
    assert torch.equal(pub[0].cpu().view(torch.int64), rec.view(torch.int64))


def test_all_nonfinite_and_any_record_length():
    """No finite element at all: min = +inf, max = -inf, sums 0.  And a record length that is no multiple of the vector width
    (the modulo path) in both dtypes, two-byte aligned for bf16."""
    x = torch.tensor([NAN, INF, -INF, NAN, NAN], device="cuda")
    assert _run_abi([(x, 5, 1, 1)])[0].tolist() == [0, 0, 0, INF, -INF, 0, 5, 5]
    for dtype in (torch.float32, torch.bfloat16):
        base = _padded(1003 + 1, 7, 7, dtype, seed=3).view(-1)
        for off in (0, 1, 3):
            t = base[off:off + 1003 * 7].view(1003, 7)
            h = _host64(t)
            for c_real in (1, 5, 7):
                _check(_run_abi([(t, 1003, c_real, 7)])[0], _ref(h[:, :c_real]), f"c_pad 7 real {c_real} off {off} {dtype}")


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 20, 57601])
def test_flat_runs_at_every_alignment(n, off):
    """Flat fp32 runs (a parameter inside the flat bucket) started 0..3 floats behind a 16-byte boundary, sentinels around."""
    g = torch.Generator().manual_seed(n + off)
    buf = torch.full((n + 16,), 7.25e30)
    start = 4 + off
    vals = torch.randn(n, generator=g)
    if n == 3:
        vals = torch.tensor([NAN, -0.0, 1.5])
    elif n >= 20:
        sp = _specials(torch.float32)
        vals[torch.randperm(n, generator=g)[:11]] = torch.tensor(sp)
    buf[start:start + n] = vals
    dev = buf.cuda()
    assert dev.data_ptr() % 16 == 0
    run = dev[start:start + n]
    assert run.data_ptr() % 16 == 4 * off
    rec = _run_abi([(run, n, 1, 1)])[0]
    _check(rec, _ref(buf[start:start + n].numpy()), f"flat {n} +{off}")
    assert torch.equal(dev.cpu().view(torch.int32), buf.view(torch.int32))                    # sentinels (and data) untouched
    if off:     # the same values on a 16-byte boundary: the same bits (the order does not depend on the alignment)
        al = dev[start:start + n].clone()
        assert al.data_ptr() % 16 == 0
        assert torch.equal(_run_abi([(al, n, 1, 1)])[0].view(torch.int64), rec.view(torch.int64))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_independent_of_the_other_jobs_and_repeatable(dtype):
    big = _padded(70001, 24, 20, dtype, seed=11)
    job = (big, 70001, 20, 24)
    small = [(_padded(105, 24, 20, torch.bfloat16, seed=1), 105, 20, 24), (_padded(5, 80, 80, torch.float32, seed=2), 5, 80, 80),
             (torch.randn(57604, generator=torch.Generator().manual_seed(5)).cuda()[1:57602], 57601, 1, 1),
             (_padded(0, 24, 20, torch.float32, seed=4), 0, 20, 24), (_padded(9000, 40, 40, dtype, seed=6), 9000, 40, 40)]
    table = [small[i % len(small)] for i in range(300)]
    for i in (0, 37, 299):
        table[i] = job
    alone = _run_abi([job])[0]
    first = _run_abi(table)
    again = _run_abi(table)
    alone2 = _run_abi([job])[0]
    records = [alone, first[0], first[37], first[299], again[0], again[37], again[299], alone2]
    for r in records:
        assert torch.equal(r.view(torch.int64), alone.view(torch.int64))
    _check(alone, _ref(_host64(big)[:, :20]), "70001 alone")
    assert torch.equal(first.view(torch.int64), again.view(torch.int64))
    singles = [_run_abi([s])[0] for s in small]
    for i in range(300):                                # and every other job of the table equals its own single-job call
        if i not in (0, 37, 299):
            assert torch.equal(first[i].view(torch.int64), singles[i % len(small)].view(torch.int64)), i


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _model(golden_dir, dtype):
    import mil_amd
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    net = mil_amd.Attention(3, compute_dtype=dtype)
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()}, strict=True)
    return net


def _mode(name):
    import mil_amd
    return {"fp32": torch.float32, "bf16": torch.bfloat16, "bf16x3": mil_amd.BF16X3}[name]


@pytest.mark.parametrize("name", ["eval_n8_64", "eval_n5_50x70"])
def test_summary_matches_the_hooked_tensors_bf16(golden_dir, name):
    import mil_amd
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    net = _model(golden_dir, torch.bfloat16).eval()
    cnn = net.cnn.module
    x, y = torch.tensor(g["x"]).cuda(), torch.tensor(g["y"]).cuda()
    seen, handles = {}, []
    for key, mod in (("cnn.module.layer1.0", cnn.layer1[0]), ("cnn.module.layer2.0", cnn.layer2[0]),
                     ("cnn.module.layer3.2", cnn.layer3[2]), ("cnn.module.layer4.2", cnn.layer4)):
        handles.append(mod.register_forward_hook(lambda m, i, o, key=key: seen.__setitem__(key, o.detach().cpu().numpy())))
    net(x, y)
    for h in handles:
        h.remove()
    assert len(seen) == 4 and all(v.dtype == np.float32 and v.ndim == 4 for v in seen.values())
    with mil_amd.ActivationSummary(net, taps="blocks") as s:
        net(x, y)                                       # un-hooked: block hooks do not change the kernel choice (test_gpu_hooks.py)
        stats = s.stats.cpu()
        got = s.read()
    for key, arr in seen.items():
        rec = stats[s.names.index(key)]
        ref = _ref(arr)
        _check(rec, ref, f"{name} {key}")
        assert ref["total"] == arr.size and got[key]["count"] == arr.size and got[key]["nonfinite"] == 0
        assert got[key]["min"] == float(arr.min()) and got[key]["max"] == float(arr.max())
        assert abs(got[key]["mean"] - arr.astype(np.float64).mean()) <= 1e-12 * max(1.0, abs(got[key]["max"]))
        assert got[key]["negative_share"] == float((arr < 0).mean())


@pytest.mark.parametrize("name", ["eval_n8_64", "eval_n5_50x70"])
def test_summary_matches_the_golden_activations_fp32(golden_dir, name):
    import mil_amd
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    net = _model(golden_dir, torch.float32).eval()
    with mil_amd.ActivationSummary(net, taps="stages") as s:
        net(torch.tensor(g["x"]).cuda(), torch.tensor(g["y"]).cuda())
        got = s.read()
        assert s.first_nonfinite() is None
    keys = ["act.pool", "act.layer1", "act.layer2", "act.layer3", "act.layer4", "out.Fterm"]
    assert len(s.names) == len(keys)
    for tap, k in zip(s.names, keys):
        ref = g[k].astype(np.float64)
        tol = 2e-5 * float(np.abs(ref).max())           # the bound test_gpu_hooks.py holds these activations to
        print(f"{name} {tap}: mean {got[tap]['mean']:.8g} vs {ref.mean():.8g}, max {got[tap]['max']:.8g} vs {ref.max():.8g}, tol {tol:.3g}")
        assert got[tap]["count"] == ref.size and got[tap]["nonfinite"] == 0, tap
        assert abs(got[tap]["mean"] - ref.mean()) <= tol, tap
        assert abs(got[tap]["max"] - ref.max()) <= tol, tap


def _run(net, g, train):
    if train:
        net.train()
        net.rng_override = {"indices": torch.tensor(g["rec.indices"]), "keep_mask": torch.tensor(g["rec.keep_mask"])}
    else:
        net.eval()
    net.zero_grad(set_to_none=True)
    out = net(torch.tensor(g["x"]).cuda(), torch.tensor(g["y"]).cuda())
    out["loss"].backward()
    return ({k: v.detach().clone() for k, v in out.items()}, {k: p.grad.detach().clone() for k, p in net.named_parameters()})


@pytest.mark.parametrize("case", ["eval_n8_64", "train_n40_64"])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16x3"])
def test_observation_changes_nothing(golden_dir, mode, case):
    import mil_amd
    g = np.load(os.path.join(golden_dir, case + ".npz"))
    net = _model(golden_dir, _mode(mode))
    train = case.startswith("train")
    out0, grad0 = _run(net, g, train)
    s = mil_amd.ActivationSummary(net, taps="blocks")
    out1, grad1 = _run(net, g, train)
    one = s.stats.clone()
    assert float(one[:, 7].min()) > 0 and float(one[:, 6].sum()) == 0
    s.close()
    assert net.cnn.module.activation_summary is None
    out2, grad2 = _run(net, g, train)
    for k in out0:
        assert torch.equal(out0[k], out1[k]) and torch.equal(out0[k], out2[k]), k
    for k in grad0:
        assert torch.equal(grad0[k], grad1[k]) and torch.equal(grad0[k], grad2[k]), k
    # accumulate=True over two passes = the merge of the two single-pass records
    from mil_amd.summary import merge_stats
    other = np.load(os.path.join(golden_dir, "eval_n5_50x70.npz"))
    with mil_amd.ActivationSummary(net, taps="blocks") as single:
        _run(net, g, train)
        a = single.stats.clone()
        _run(net, other, False)
        b = single.stats.clone()
    assert torch.equal(a.view(torch.int64), one.view(torch.int64))                     # the same pass: the same bits
    with mil_amd.ActivationSummary(net, taps="blocks", accumulate=True) as acc:
        _run(net, g, train)
        _run(net, other, False)
        assert acc.passes == 2
        both = acc.stats.clone()
        acc.reset()
        _run(net, other, False)
        assert torch.equal(acc.stats.view(torch.int64), b.view(torch.int64))
    want = merge_stats(a, b)
    assert torch.equal(both.view(torch.int64), want.view(torch.int64))
    assert torch.equal(both[:, 7], a[:, 7] + b[:, 7]) and torch.equal(both[:, 3], torch.minimum(a[:, 3], b[:, 3]))


def test_parameter_and_gradient_statistics(golden_dir):
    import mil_amd
    g = np.load(os.path.join(golden_dir, "eval_n8_64.npz"))
    net = _model(golden_dir, mil_amd.BF16X3).eval()
    net(torch.tensor(g["x"]).cuda(), torch.tensor(g["y"]).cuda())["loss"].backward()
    keys = [k for k, _p in net.named_parameters()]
    assert len(keys) == 65
    host = {}
    for grads in (False, True):
        names, stats = mil_amd.parameter_stats(net, grads=grads)
        assert names == keys and tuple(stats.shape) == (65, 8) and stats.is_cuda and stats.dtype == torch.float64
        host[grads] = stats.cpu()
        for (k, p), rec in zip(net.named_parameters(), host[grads]):
            t = p.grad if grads else p.detach()
            _check(rec, _ref(t.cpu().numpy()), f"{k} grads={grads}")
    mx = mil_amd.layer_weight_summary_max(net.named_parameters())
    mean = mil_amd.layer_weight_summary_mean(net.named_parameters())
    assert list(mx) == keys and list(mean) == keys
    for k, p in net.named_parameters():
        assert isinstance(mx[k], float) and mx[k] == float(p.detach().max()), k          # the fp32 maxima exactly
        ref = p.detach().cpu().numpy().astype(np.float64)
        assert abs(mean[k] - math.fsum(ref.reshape(-1)) / ref.size) <= ref.size * EPS * float(np.abs(ref).sum()) / ref.size, k
    # through a FlatParams: the same values at other addresses (parameter slices start at any 4-byte offset): the same bits
    wgrad = {k: p.grad.clone() for k, p in net.named_parameters()}
    flat = mil_amd.FlatParams(net)
    for k, p in net.named_parameters():
        p.grad.copy_(wgrad[k])
    assert any(p.data_ptr() % 16 for p in net.parameters())
    for grads in (False, True):
        fnames, fstats = mil_amd.parameter_stats(flat, grads=grads)
        assert fnames == keys
        assert torch.equal(fstats.cpu().view(torch.int64), host[grads].view(torch.int64))
        mnames, mstats = mil_amd.parameter_stats(net, grads=grads)                        # the module's tensors ARE the bucket's now
        assert mnames == keys and torch.equal(mstats.cpu().view(torch.int64), host[grads].view(torch.int64))


def test_locating_a_nonfinite_value(golden_dir):
    """Ordinary NaN arithmetic: one NaN weight in layer3[1].conv2; the first tap that shows it is that block's output."""
    import mil_amd
    g = np.load(os.path.join(golden_dir, "eval_n8_64.npz"))
    net = _model(golden_dir, mil_amd.BF16X3).eval()
    with torch.no_grad():
        net.cnn.module.layer3[1].conv2.weight.view(-1)[17] = NAN
    mil_amd.invalidate_packed_weights()
    with mil_amd.ActivationSummary(net, taps="blocks") as s:
        with torch.no_grad():
            net(torch.tensor(g["x"]).cuda(), torch.tensor(g["y"]).cuda())
        assert s.first_nonfinite() == "cnn.module.layer3.1"
        bad = s.stats[:, 6].cpu().tolist()
        got = s.read()
    at = s.names.index("cnn.module.layer3.1")
    assert all(b == 0 for b in bad[:at]) and bad[at] > 0
    assert got["cnn.module.fc"]["nonfinite"] > 0 and bad[s.names.index("cnn.module.fc")] > 0
    names, wstats = mil_amd.parameter_stats(net)
    wbad = dict(zip(names, wstats[:, 6].cpu().tolist()))
    assert wbad["cnn.module.layer3.1.conv2.weight"] == 1 and sum(wbad.values()) == 1
    assert math.isnan(mil_amd.layer_weight_summary_max(net.named_parameters())["cnn.module.layer3.1.conv2.weight"])
