"""Host-only part of the split-precision (MIL_DT_F32S) wide-layer ABI: the workspace query needs no GPU."""
import ctypes

import pytest

import mil_amd

# (n, H, W, cin, Ho, Wo, cout, ks, stride, pad)
QUERIES = [(256, 32, 32, 128, 32, 32, 128, 3, 1, 1), (3, 11, 11, 64, 6, 6, 128, 3, 2, 1), (2, 10, 7, 96, 5, 4, 64, 1, 2, 0)]


@pytest.mark.parametrize("q", QUERIES)
def test_wide_wgrad_workspace_split_equals_exact_fp32(q):
    lib = mil_amd.lib()
    exact, split = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.mil_wide_wgrad_workspace(ctypes.byref(exact), *q, mil_amd._lib.MIL_DT_F32) == 0
    assert lib.mil_wide_wgrad_workspace(ctypes.byref(split), *q, mil_amd._lib.MIL_DT_F32S) == 0
    assert split.value == exact.value > 0


def test_wide_wgrad_workspace_refuses_unknown_dtype_and_widths():
    lib = mil_amd.lib()
    n = ctypes.c_size_t(0)
    assert lib.mil_wide_wgrad_workspace(ctypes.byref(n), 4, 16, 16, 128, 16, 16, 128, 3, 1, 1, mil_amd._lib.MIL_DT_F32S_DGRAD) == 1
    assert lib.mil_wide_wgrad_workspace(ctypes.byref(n), 4, 16, 16, 48, 16, 16, 128, 3, 1, 1, mil_amd._lib.MIL_DT_F32S) == 2
