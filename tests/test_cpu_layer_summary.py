"""CPU (-m "not gpu"): the host side of the device summaries (mil_tensor_stats_all, mil_amd.summary): the symbols load, the
host-side queries answer, every argument error is a status code decided before any GPU call, and the tap / parameter names
are what the reference's keys are."""
import ctypes

import pytest
import torch

OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 2
F32, BF16 = 0, 1


def _lib():
    import mil_amd
    return mil_amd.lib()


def _job(lib, x=0x1000, n_pix=10, c_real=20, c_pad=24, dtype=F32):
    rec = lib.mil_stats_job_bytes()
    host = (ctypes.c_char * rec)()
    return host, lib.mil_stats_job_fill(host, x, n_pix, c_real, c_pad, dtype)


def test_symbols_load_and_host_queries_answer():
    lib = _lib()
    for name in ("mil_stats_job_bytes", "mil_stats_job_fill", "mil_tensor_stats_workspace", "mil_tensor_stats_all"):
        assert hasattr(lib, name), name
    assert lib.mil_abi_version() == 2
    assert lib.mil_stats_job_bytes() > 0
    host, rc = _job(lib)
    assert rc == OK
    n = ctypes.c_size_t(0)
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), host, 1) == OK and n.value > 0
    one = n.value
    # a tensor of several chunks needs more; an empty one still a positive size
    big, rc = _job(lib, n_pix=70001)
    assert rc == OK and lib.mil_tensor_stats_workspace(ctypes.byref(n), big, 1) == OK and n.value > one
    empty, rc = _job(lib, n_pix=0)
    assert rc == OK and lib.mil_tensor_stats_workspace(ctypes.byref(n), empty, 1) == OK and n.value > 0
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), None, 0) == OK and n.value == 0


def test_argument_errors_are_status_codes_without_a_gpu():
    lib = _lib()
    rec = lib.mil_stats_job_bytes()
    host = (ctypes.c_char * rec)()
    assert lib.mil_stats_job_fill(None, 0x1000, 10, 20, 24, F32) == ERR_ARG
    assert lib.mil_stats_job_fill(host, None, 10, 20, 24, F32) == ERR_ARG
    assert lib.mil_stats_job_fill(host, 0x1000, 10, 0, 24, F32) == ERR_ARG           # c_real < 1
    assert lib.mil_stats_job_fill(host, 0x1000, 10, 25, 24, F32) == ERR_ARG          # c_real > c_pad
    assert lib.mil_stats_job_fill(host, 0x1000, -1, 20, 24, F32) == ERR_ARG          # n_pix < 0
    assert lib.mil_stats_job_fill(host, 0x1002, 10, 1, 1, F32) == ERR_ARG            # not aligned to the element
    assert lib.mil_stats_job_fill(host, 0x1002, 10, 1, 1, BF16) == OK
    for dt in (2, 3, 4, 7, -1):                                                      # the gradient / split codes are not tensors' dtypes
        assert lib.mil_stats_job_fill(host, 0x1000, 10, 20, 24, dt) == ERR_UNSUPPORTED, dt
    good, rc = _job(lib)
    assert rc == OK
    n = ctypes.c_size_t(0)
    assert lib.mil_tensor_stats_workspace(None, good, 1) == ERR_ARG
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), None, 1) == ERR_ARG
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), good, -1) == ERR_ARG
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), good, 1) == OK
    ws_bytes = n.value
    dev, out, ws = 0x2000, 0x3000, 0x4000               # never dereferenced: every call below returns before a launch
    assert lib.mil_tensor_stats_all(dev, good, -1, out, ws, ws_bytes, None) == ERR_ARG
    assert lib.mil_tensor_stats_all(None, None, 0, None, None, 0, None) == OK            # njobs == 0: nothing to do
    assert lib.mil_tensor_stats_all(None, good, 1, out, ws, ws_bytes, None) == ERR_ARG
    assert lib.mil_tensor_stats_all(dev, None, 1, out, ws, ws_bytes, None) == ERR_ARG
    assert lib.mil_tensor_stats_all(dev, good, 1, None, ws, ws_bytes, None) == ERR_ARG
    assert lib.mil_tensor_stats_all(dev, good, 1, out, None, ws_bytes, None) == ERR_ARG
    assert lib.mil_tensor_stats_all(dev, good, 1, out, ws, ws_bytes - 1, None) == ERR_ARG    # short workspace
    # a table whose records the fill function did not write: the same codes, from the table
    raw = bytearray(good.raw)
    bad = (ctypes.c_char * rec).from_buffer_copy(bytes(rec))                         # all zero: null pointer
    assert lib.mil_tensor_stats_workspace(ctypes.byref(n), bad, 1) == ERR_ARG
    assert lib.mil_tensor_stats_all(dev, bad, 1, out, ws, ws_bytes, None) == ERR_ARG
    assert bytes(raw) == good.raw                                                    # the calls leave the host table alone


@pytest.mark.parametrize("taps,count", [("stages", 6), ("blocks", 27)])
def test_activation_summary_names_in_forward_order(taps, count):
    import mil_amd
    net = mil_amd.Attention(3, device="cpu")
    assert net.cnn.module.activation_summary is None
    s = mil_amd.ActivationSummary(net, taps=taps)
    assert net.cnn.module.activation_summary is s
    assert len(s.names) == count and len(set(s.names)) == count
    if taps == "stages":
        assert s.names == ["cnn.module.maxpool"] + [f"cnn.module.layer{i}" for i in (1, 2, 3, 4)] + ["cnn.module.fc"]
    else:
        want = ["cnn.module.maxpool"]
        for i in (1, 2, 3, 4):
            for b in range(3):
                want += [f"cnn.module.layer{i}.{b}:mid", f"cnn.module.layer{i}.{b}"]
        assert s.names == want + ["cnn.module.avgpool", "cnn.module.fc"]
    with pytest.raises(RuntimeError, match="already"):
        mil_amd.ActivationSummary(net)
    with pytest.raises(RuntimeError, match="no encoder pass"):
        s.read()
    s.close()
    assert net.cnn.module.activation_summary is None
    # a bare encoder: the same names without the wrapper's prefix
    with mil_amd.ActivationSummary(net.cnn.module, taps=taps) as bare:
        assert bare.names == [n[len("cnn.module."):] for n in s.names]
    assert net.cnn.module.activation_summary is None
    with pytest.raises(ValueError):
        mil_amd.ActivationSummary(net, taps="convs")
    with pytest.raises(TypeError):
        mil_amd.ActivationSummary(torch.nn.Linear(2, 2))


def test_parameter_names_are_the_reference_keys_and_there_is_no_cpu_path():
    import mil_amd
    from mil_amd import summary
    net = mil_amd.Attention(3, device="cpu")
    keys = [k for k, _p in net.named_parameters()]
    names, tensors = summary.parameter_jobs(net)
    assert names == keys and len(names) == 65
    assert all(t.data_ptr() == p.data_ptr() for t, (_k, p) in zip(tensors, net.named_parameters()))      # views, no copies
    with pytest.raises(ValueError, match="no gradient"):
        summary.parameter_jobs(net, grads=True)
    flat = mil_amd.FlatParams(net)
    fnames, ftensors = summary.parameter_jobs(flat)
    assert fnames == keys
    assert [t.data_ptr() for t in ftensors] == [p.data_ptr() for p in net.parameters()]                  # slices of the flat bucket
    gnames, gtensors = summary.parameter_jobs(flat, grads=True)
    assert gnames == keys and [t.data_ptr() for t in gtensors] == [p.grad.data_ptr() for p in net.parameters()]
    with pytest.raises(RuntimeError):                  # statistics are computed on the GPU only
        mil_amd.parameter_stats(net)
    with pytest.raises(RuntimeError):
        mil_amd.layer_weight_summary_mean(net.named_parameters())
    with pytest.raises(RuntimeError):
        mil_amd.tensor_stats([torch.zeros(4)])
    assert summary.describe([4, 2.0, 3.0, -1.0, 2.0, 1, 0, 4]) == {
        "mean": 0.5, "std": (3.0 / 4 - 0.25) ** 0.5, "min": -1.0, "max": 2.0, "negative_share": 0.25, "nonfinite": 0, "count": 4}
    a = torch.tensor([[2, 1.0, 1.0, -1.0, 1.0, 1, 0, 2]], dtype=torch.float64)
    b = torch.tensor([[1, 5.0, 25.0, 5.0, 5.0, 0, 1, 2]], dtype=torch.float64)
    assert summary.merge_stats(a, b).tolist() == [[3, 6.0, 26.0, -1.0, 5.0, 1, 1, 4]]
