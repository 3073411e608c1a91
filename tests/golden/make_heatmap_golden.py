"""Writes tests/golden/heatmap_luts.npz: the two colour tables of the attention heat maps as matplotlib returns them
(recorded with matplotlib 3.10.8).

  jet105      cm.jet(np.linspace(0, 1, 105), bytes=True)[:, :3]   — `cmap_lin` of the reference's create_map
                                                                     (gbm/classify_combined.py:172), as bytes
  viridis256  cm.viridis(np.arange(256), bytes=True)[:, :3]       — the table imshow's default colour map indexes

Only matplotlib and numpy are imported.  Run from the repository root: python tests/golden/make_heatmap_golden.py"""
import os

import matplotlib
import numpy as np
from matplotlib import cm


def tables():
    jet = np.ascontiguousarray(cm.jet(np.linspace(0, 1, 105), bytes=True)[:, :3])
    viridis = np.ascontiguousarray(cm.viridis(np.arange(256), bytes=True)[:, :3])
    assert jet.dtype == np.uint8 and jet.shape == (105, 3) and viridis.dtype == np.uint8 and viridis.shape == (256, 3)
    return jet, viridis


if __name__ == "__main__":
    jet, viridis = tables()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "heatmap_luts.npz")
    np.savez(out, jet105=jet, viridis256=viridis, matplotlib_version=np.array(matplotlib.__version__))
    print(out, jet.shape, viridis.shape, matplotlib.__version__)
