"""-m gpu: bench.py's plain run (the headline line, nothing measured beside it) and `--dump-outputs` (the outputs of the last
timed step as float32 .npy files; the inputs are seeded and the kernels reduce in a fixed order, so two runs with the same
arguments write identical files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAGS, TILES = 2, 16


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--size", "64",
           "--bags", str(BAGS), "--tiles", str(TILES), "--dump-outputs", str(out_dir)]
    res = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}


def test_plain_run_line_and_dumped_outputs(tmp_path):
    line, got = _bench(tmp_path / "a")
    assert line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "bf16" and line["unit"] == "tiles/s"
    assert line["higher_is_better"] is True and line["metric"].startswith("tiles/sec fwd+bwd")
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(BAGS * TILES * 1e3 / line["ms_per_step"], rel=1e-9)
    # nothing beside the headline figure is measured without --full
    assert line["roofline"] is None and line["value_within_tolerance"] is None
    assert not {"cpu_baseline", "s2d_feed_path", "bf16x3_path", "fp32_path", "alt_resnet_path", "allreduce_ms"} & set(line)

    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["Aterm"].shape == (BAGS, 3, TILES) and got["Fterm"].shape == (BAGS, TILES, 80)
    assert got["y_pred"].shape == (BAGS, 1, 3) and got["loss"].shape == (BAGS,)
    assert got["grad_flat"].ndim == 1 and got["grad_flat"].shape == got["params_flat"].shape
    assert np.abs(got["grad_flat"]).max() > 0

    _line, again = _bench(tmp_path / "b")
    assert sorted(again) == sorted(got)
    for k in got:
        assert np.array_equal(again[k], got[k]), k
