"""Pins oracle/mil_oracle.py to the golden vectors captured from the reference
(tests/golden/make_golden.py): outputs, stage activations and parameter gradients."""
import os

import numpy as np
import pytest
import torch

from oracle import mil_oracle as orc

CASES = ["eval_n8_64", "eval_n8_64_cw", "eval_n5_50x70", "train_n40_64", "eval_n2_256"]
OUT_KEYS = ["Aterm", "wROIs", "Bterm", "Mterm", "Fterm", "Aterm_mu", "Aterm_var", "loss", "l2",
            "KLD", "y_pred", "y_pred_hat", "error"]


def _run(golden_dir, name, x=None):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    sd = orc.load_state(w, requires_grad=True)
    x = torch.tensor(g["x"]) if x is None else x
    y = torch.tensor(g["y"])
    kw = {}
    if "rec.indices" in g:
        kw = dict(training=True, indices=torch.tensor(g["rec.indices"]),
                  keep_mask=torch.tensor(g["rec.keep_mask"]))
    if "class_weights" in g:
        kw["class_weights"] = torch.tensor(g["class_weights"])
    acts = {}
    out = orc.attention_forward(sd, x, y, acts=acts, **kw)
    out["loss"].backward()
    return sd, g, out, acts


def _close(a, b, rtol=2e-4, atol=2e-6):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    scale = max(1.0, float(np.abs(b).max()) if b.size else 1.0)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol * scale)


def test_state_dict_spec_matches_reference(golden_dir):
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    spec = orc.state_dict_spec()
    assert [k for k, _ in spec] == list(w.keys())          # same 65 keys, same order
    assert all(tuple(w[k].shape) == s for k, s in spec)
    assert sum(int(np.prod(s)) for _, s in spec) == 640967


@pytest.mark.parametrize("name", CASES)
def test_outputs_match_reference(golden_dir, name):
    sd, g, out, acts = _run(golden_dir, name)
    assert list(out.keys()) == OUT_KEYS
    for k in OUT_KEYS:
        ref = g["out." + k]
        got = out[k].detach().numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype, k
        if k in ("y_pred_hat", "error"):
            assert np.array_equal(got, ref), k
        else:
            _close(got, ref)
    for k, v in acts.items():
        if "act." + k in g:
            _close(v.detach().numpy(), g["act." + k])
    # only loss and l2 carry grad (gbm/model.py:249-262)
    assert [k for k in OUT_KEYS if out[k].requires_grad] == ["loss", "l2"]


@pytest.mark.parametrize("name", CASES)
def test_gradients_match_reference(golden_dir, name):
    sd, g, out, _ = _run(golden_dir, name)
    names = list(g["gradnorm.names"])
    assert names == list(sd.keys())
    for k, n_ref, s_ref in zip(names, g["gradnorm.l2"], g["gradnorm.sum"]):
        grad = sd[k].grad if sd[k].grad is not None else torch.zeros_like(sd[k])
        # N=2 bags make the batch-statistics BN backward ill-conditioned (x-mean = +-half-gap):
        # fp32 summation order alone moves those gradients by ~2e-4 relative.
        tol = 2e-3 if name == "eval_n2_256" else 2e-4
        assert abs(float(grad.double().norm()) - n_ref) <= tol * max(n_ref, 1e-3), k
        if "grad." + k in g:
            _close(grad.numpy(), g["grad." + k], rtol=1e-4, atol=1e-5)


def test_config1_regenerated_input(golden_dir):
    """BASELINE.json configs[0]: 1 bag x 64 tiles @256x256; the input is rebuilt from its seed."""
    gen = torch.Generator().manual_seed(20260104)
    x = torch.randn(64, 3, 256, 256, generator=gen).clamp_(-1.0, 1.0)
    sd, g, out, _ = _run(golden_dir, "eval_n64_256_cfg1", x=x)
    for k in ("Aterm", "Fterm", "loss", "y_pred", "Mterm"):
        _close(out[k].detach().numpy(), g["out." + k], rtol=1e-4)
    for k, n_ref in zip(g["gradnorm.names"], g["gradnorm.l2"]):
        assert abs(float(sd[k].grad.double().norm()) - n_ref) <= 5e-4 * max(n_ref, 1e-3), k


def test_single_instance_bag_raises(golden_dir):
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    sd = orc.load_state(w)
    with pytest.raises(ValueError):
        orc.attention_forward(sd, torch.zeros(1, 3, 32, 32), torch.tensor([0]))


@pytest.mark.parametrize("name", ["alt_l1111_n4_64", "alt_l2222_n2_96x80"])
def test_alt_backbone_oracle_matches_reference_golden(golden_dir, name):
    """Second encoder configuration (alt_resnet.py): restatement vs outputs of the reference itself."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    layers = tuple(int(v) for v in z["layers"])
    sd = orc.alt_seeded_state(layers, int(z["num_classes"]), int(z["wseed"]), requires_grad=True)
    feats = orc.alt_backbone(sd, torch.from_numpy(z["x"]), layers)
    ref = torch.from_numpy(z["feats"])
    assert float((feats.detach() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    feats.backward(torch.from_numpy(z["dfeats"]))
    for k, v in zip([str(k) for k in z["gradnorm.names"]], z["gradnorm.l2"]):
        assert abs(float(sd[k].grad.double().norm()) - v) <= 1e-5 * v, k


def own_patterns(acts, x_shape):
    """The activation pattern of an oracle run in the form `backbone(patterns=...)` takes (taps from max_pool2d's indices)."""
    import torch.nn.functional as F
    stem = acts["stem"]
    _n, _c, h, w = stem.shape
    _p, idx = F.max_pool2d(stem, 3, 2, 1, return_indices=True)
    hp, wp = idx.shape[2:]
    oy = torch.arange(hp).view(1, 1, hp, 1)
    ox = torch.arange(wp).view(1, 1, 1, wp)
    tap = (idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1))
    pat = {"stem_tap": tap, "stem_pos": acts["pool"] > 0}
    for k, v in acts.items():
        if k.count(".") >= 1:
            pat[k] = v > 0
    return pat


def test_forced_activation_pattern_reproduces_the_plain_run(golden_dir):
    """`backbone(patterns=...)` with the pattern of the plain run itself must give the plain run's features and gradients
    (fp64: to rounding) — it is the reference of tests/test_gpu_configs.py::test_encoder_gradients_on_its_own_activation_pattern."""
    import numpy as np
    import os
    w = np.load(os.path.join(golden_dir, "weights.npz"))
    sd = {k: torch.tensor(w[k], dtype=torch.float64, requires_grad=True) for k, _s in orc.state_dict_spec()}
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64).clamp_(-1, 1)
    acts = {}

    def run(patterns):
        for v in sd.values():
            v.grad = None
        a = {}
        o1 = {}
        # the blocks' inner activations are not in `acts`: capture them through the same function with a recording wrapper
        f = orc.backbone(sd, x, a, patterns=patterns)
        f.square().sum().backward()
        return f.detach().clone(), {k: v.grad.clone() for k, v in sd.items() if v.grad is not None}, a

    f0, g0, acts = run(None)
    # inner (o1) patterns: recompute each block's first LeakyReLU input sign from the block inputs the run recorded
    import torch.nn.functional as F
    pat = own_patterns(acts, x.shape)
    t = acts["pool"]
    with torch.no_grad():
        for li, _pl, stride in orc.STAGES:
            for b in range(orc.BLOCKS_PER_STAGE):
                q = f"cnn.module.layer{li}.{b}."
                pre = F.conv2d(t, sd[q + "conv1.weight"], sd[q + "conv1.bias"], stride=stride if b == 0 else 1, padding=1)
                pat[f"layer{li}.{b}.o1"] = pre > 0
                t = acts[f"layer{li}.{b}"]
    f1, g1, _ = run(pat)
    assert float((f1 - f0).abs().max()) <= 1e-12 * float(f0.abs().max())
    for k in g0:
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-10 * max(float(g0[k].abs().max()), 1e-30), k


def alt_own_patterns(acts):
    """The activation pattern of an `alt_backbone(acts=...)` run in the form its `patterns=` takes."""
    import torch.nn.functional as F
    stem = acts["stem"]
    w = stem.shape[3]
    _p, idx = F.max_pool2d(stem, 3, 2, 1, return_indices=True)
    hp, wp = idx.shape[2:]
    oy = torch.arange(hp).view(1, 1, hp, 1)
    ox = torch.arange(wp).view(1, 1, 1, wp)
    pat = {"stem_tap": (idx // w - (2 * oy - 1)) * 3 + (idx % w - (2 * ox - 1)), "stem_pos": acts["pool"] > 0}
    pat.update({k: v > 0 for k, v in acts.items() if k.startswith("layer")})
    return pat


@pytest.mark.parametrize("name", ["alt_l1111_n4_64", "alt_l2222_n2_96x80"])
def test_alt_forced_activation_pattern_reproduces_the_plain_run(golden_dir, name):
    """`alt_backbone(patterns=...)` with the pattern of its own fp64 run gives that run's features and every parameter
    gradient to 1e-12 — it is the reference of tests/test_gpu_alt_vjp.py."""
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    layers = tuple(int(v) for v in z["layers"])
    sd = {k: v.double().requires_grad_(True) for k, v in orc.alt_seeded_state(layers, int(z["num_classes"]), int(z["wseed"])).items()}
    x, dfe = torch.from_numpy(z["x"]).double(), torch.from_numpy(z["dfeats"]).double()

    def run(patterns, acts=None):
        for v in sd.values():
            v.grad = None
        f = orc.alt_backbone(sd, x, layers, patterns=patterns, acts=acts)
        f.backward(dfe)
        return f.detach().clone(), {k: v.grad.clone() for k, v in sd.items()}

    acts = {}
    f0, g0 = run(None, acts)
    pat = alt_own_patterns(acts)
    assert int(pat["stem_tap"].min()) >= 0 and int(pat["stem_tap"].max()) <= 8
    assert len(pat) == 2 + 2 * sum(layers)
    f1, g1 = run(pat)
    assert float((f1 - f0).abs().max()) <= 1e-12 * float(f0.abs().max())
    assert set(g0) == set(k for k, _s in orc.alt_state_dict_spec(layers, int(z["num_classes"])))
    for k in g0:
        assert float(g0[k].abs().max()) > 0, k
        assert float((g1[k] - g0[k]).abs().max()) <= 1e-12 * float(g0[k].abs().max()), k
