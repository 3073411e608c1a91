"""CPU (-m "not gpu"): the host layer of the attention heat maps (mil_amd.heatmap) — the colour tables against the recorded
golden (and matplotlib where it is installed), the index functions against restatements of the reference's float32
statements, every refusal that must fire before a launch, and the C entry's argument check."""
import os

import numpy as np
import pytest
import torch

import mil_amd
from mil_amd import heatmap as hm


def test_colour_tables_equal_the_golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "heatmap_luts.npz"))
    for got, want in ((hm.JET105, z["jet105"]), (hm.VIRIDIS256, z["viridis256"])):
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert hm.JET105.shape == (105, 3) and hm.VIRIDIS256.shape == (256, 3)


def test_colour_tables_equal_matplotlib():
    cm = pytest.importorskip("matplotlib.cm")
    assert np.array_equal(hm.JET105, cm.jet(np.linspace(0, 1, 105), bytes=True)[:, :3])
    assert np.array_equal(hm.VIRIDIS256, cm.viridis(np.arange(256), bytes=True)[:, :3])
    # the float table create_map indexes (gbm/classify_combined.py:172), as bytes
    assert np.array_equal(hm.JET105, (cm.jet(np.linspace(0, 1, 105))[:, :3] * 255).astype(np.uint8))


def _attention_indices_np(a):
    """gbm/classify_combined.py:178-202 on float32 numpy arrays: (1/3) * (A[0] + A[1] + A[2]), 100 * x, > 0.0, int(.)."""
    a = np.asarray(a, dtype=np.float32)
    mean = np.float32(1 / 3) * (a[0] + a[1] + a[2])
    att = np.stack([np.float32(100) * mean, np.float32(100) * a[0], np.float32(100) * a[1], np.float32(100) * a[2]])
    assert att.dtype == np.float32
    return np.where(att > 0, np.trunc(att).astype(np.int64), -1).astype(np.int16)


def test_attention_indices_around_integer_boundaries():
    ks = np.arange(1, 105, dtype=np.float64) / 100
    base = ks.astype(np.float32)
    below, above = np.nextafter(base, np.float32(0)), np.nextafter(base, np.float32(2))
    vals = np.concatenate([base, below, above, np.nextafter(below, np.float32(0)), np.nextafter(above, np.float32(2))])
    rng = np.random.default_rng(11)
    a = np.stack([vals, rng.permutation(vals), rng.permutation(vals)]).astype(np.float32)
    got = hm.attention_indices(torch.from_numpy(a))
    assert got.dtype == torch.int16 and tuple(got.shape) == (4, a.shape[1]) and not got.is_cuda
    want = _attention_indices_np(a)
    assert np.array_equal(got.numpy(), want)
    assert want.min() >= 0 and want.max() == 104 and len(np.unique(want[1])) >= 104
    # int(.) of the float32 product, not of the decimal: some k/100 land below k
    assert (want[1, :104] != np.arange(1, 105)).any()


def test_attention_indices_edges():
    tiny = float(np.nextafter(np.float32(0), np.float32(1)))
    a = torch.tensor([[0.0, tiny, 1.0, -0.5], [0.0, tiny, 1.0, 0.25], [0.0, tiny, 1.0, 0.25]])
    got = hm.attention_indices(a)
    assert got[1].tolist() == [-1, 0, 100, -1] and got[2].tolist() == [-1, 0, 100, 25]
    assert got[0].tolist()[:2] == [-1, 0] and got[0, 2] in (99, 100) and got[0, 3] == -1      # the mean of (-0.5, 0.25, 0.25) is not > 0
    assert np.array_equal(got.numpy(), _attention_indices_np(a.numpy()))
    with pytest.raises(ValueError):
        hm.attention_indices(torch.tensor([[0.1], [float("nan")], [0.2]]))
    with pytest.raises(ValueError):
        hm.attention_indices(torch.tensor([[0.1], [1.0501], [0.2]]))
    with pytest.raises(ValueError):
        hm.attention_indices(torch.tensor([[0.1], [float("inf")], [0.2]]))
    assert hm.attention_indices(torch.tensor([[0.1], [1.0499], [0.2]]))[2, 0] == 104
    with pytest.raises(ValueError):
        hm.attention_indices(torch.zeros(4, 3))
    assert tuple(hm.attention_indices(torch.zeros(3, 0)).shape) == (4, 0)


def test_feature_indices_equal_matplotlib():
    cm = pytest.importorskip("matplotlib.cm")
    from matplotlib.colors import Normalize
    f = torch.randn(9, 80, generator=torch.Generator().manual_seed(2))
    f[3] = 0.75                                                    # a constant tile
    f[4, :40] = f[4, 0]                                            # many cells at the minimum
    got = hm.feature_indices(f)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (9, 80)
    assert got[3].tolist() == [0] * 80 and int(got.max()) == 255 and int(got[0].min()) == 0
    for i in range(9):
        x = f[i].view(8, 10).numpy()
        want = cm.viridis(Normalize()(x), bytes=True)[:, :, :3]
        assert np.array_equal(hm.VIRIDIS256[got[i].numpy()].reshape(8, 10, 3), want), i


def test_feature_indices_without_matplotlib():
    """Colormap.__call__ restated: float32 times 256, truncated, 256 -> 255."""
    f = torch.tensor([[float(i) for i in range(80)]])
    x = (np.arange(80, dtype=np.float32).astype(np.float64) / 79.0).astype(np.float32)
    want = np.minimum((x * np.float32(256)).astype(np.int64), 255)
    assert np.array_equal(hm.feature_indices(f)[0].numpy(), want)
    with pytest.raises(ValueError):
        hm.feature_indices(torch.zeros(3, 79))
    with pytest.raises(ValueError):
        hm.feature_indices(torch.full((1, 80), float("nan")))


def test_every_refusal_fires_on_cpu_tensors_before_the_device_check():
    slide = torch.zeros((100, 120, 3), dtype=torch.uint8)
    a1, f = torch.rand(3, 2), torch.randn(2, 80)
    ok = [(0, 0), (48, 64)]
    r = mil_amd.AttentionMapRenderer(48, 16)
    with pytest.raises(ValueError, match="divide"):
        mil_amd.AttentionMapRenderer(48, 5).render(slide, ok, a1, f)
    for bad in ([(53, 0), (0, 0)], [(0, 73), (0, 0)], [(-1, 0), (0, 0)]):           # a window leaves the slide
        with pytest.raises(ValueError, match="inside"):
            r.render(slide, bad, a1, f)
    for bad in ([(0, 0), (47, 47)], [(0, 0), (0, 0)], [(16, 16), (0, 63)], [(0, 32), (40, 0)]):   # shared output pixels
        with pytest.raises(ValueError, match="own the same"):
            r.render(slide, bad, a1, f)
    with pytest.raises(ValueError):
        r.render(slide, ok, torch.rand(3, 3), f)                                   # shapes disagree
    with pytest.raises(ValueError):
        r.render(slide, ok, a1, torch.randn(3, 80))
    with pytest.raises(ValueError):
        r.render(slide, ok, a1, torch.randn(2, 40))
    with pytest.raises(ValueError):
        r.render(slide, [(0, 0)], a1, f)
    with pytest.raises(ValueError):
        r.render(slide.float(), ok, a1, f)
    with pytest.raises(ValueError):
        r.render(slide, [(0.5, 0.0), (48.0, 64.0)], a1, f)
    idx = hm.attention_indices(a1)
    with pytest.raises(ValueError, match="canvas"):
        r.render_into(torch.zeros((5, 6, 7, 4), dtype=torch.uint8), slide, ok, idx)
    with pytest.raises(ValueError):
        r.render_into(torch.zeros((5, 6, 7, 3), dtype=torch.uint8), slide, ok, idx.to(torch.int32))
    with pytest.raises(ValueError):
        mil_amd.AttentionMapRenderer(48, 16, alpha_map=1.5)
    with pytest.raises(ValueError):
        mil_amd.AttentionMapRenderer(48, 0)
    # valid arguments on a CPU slide: the package's usual refusal, after all of the above
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render(slide, ok, a1, f)
    with pytest.raises(RuntimeError, match="AMD GPU only"):
        r.render_into(torch.zeros((5, 6, 7, 3), dtype=torch.uint8), slide, ok, idx)
    assert (r.q_tissue, r.q_map) == (77, 230)
    # windows that touch without sharing a pixel are accepted (then refused for the device only)
    with pytest.raises(RuntimeError):
        r.render(slide, [(0, 0), (48, 0), (0, 48), (48, 48)], torch.rand(3, 4))


def test_collision_check_against_the_quadratic_definition():
    rng = np.random.default_rng(4)
    seen = set()
    for trial in range(300):
        n = int(rng.integers(1, 5))
        t = int(rng.integers(2, 7))
        oy, ox = rng.integers(0, 12, t), rng.integers(0, 12, t)
        want = any(abs(oy[i] - oy[j]) < n and abs(ox[i] - ox[j]) < n for i in range(t) for j in range(i))
        assert hm._owned_blocks_collide(oy.astype(np.int64), ox.astype(np.int64), n) == want, (n, oy, ox)
        seen.add(want)
    assert seen == {True, False}


def test_slide_bag_needs_build_first():
    bag = mil_amd.SlideBag(torch.zeros((100, 120, 3), dtype=torch.uint8), 48, 7, resolution=32)
    with pytest.raises(RuntimeError, match="build"):
        bag.attention_maps({}, 16)


def test_entry_point_refuses_bad_arguments_without_a_gpu():
    lib = mil_amd.lib()
    assert lib.mil_heatmap_render(None, 0, None, 0, 0, 16, 16, None, None, None, None, None, 16, 77, 230, None, 1, 1, None) == 1
    buf = np.zeros(4096, dtype=np.uint8)
    one = buf.ctypes.data                                                            # any non-null address: nothing is read

    def call(S=16, D=16, T=0, pitch=48, q0=77, q1=230, inset=16, feat=None, vir=one, ht=4, wt=4, nbytes=4096):
        return lib.mil_heatmap_render(one, nbytes, one, pitch, T, S, D, one, one, feat, one, vir, inset, q0, q1, one, ht, wt, None)
    assert call() == 0                                                               # T == 0: MIL_OK, no launch
    assert call(S=0) == 1 and call(D=0) == 1 and call(S=16, D=5) == 1 and call(T=-1) == 1 and call(pitch=47) == 1
    assert call(q0=257) == 1 and call(q1=-1) == 1 and call(inset=-1) == 1 and call(ht=0) == 1 and call(nbytes=-1) == 1
    assert call(feat=one, vir=None) == 1
    assert call(S=8192, D=8192, pitch=3 * 8192) == 2                                 # 32-bit sums stop at D = 4096
    assert call(S=4001, D=1, pitch=3 * 4001) == 2                                    # one output row's sums: 48 KB of LDS
    assert call(S=16, D=16, pitch=1 << 30) == 2                                      # 16 rows leave 31-bit offsets
    assert call(S=4096, D=4096, pitch=3 * 4096) == 0 and call(S=4000, D=1, pitch=12000) == 0
