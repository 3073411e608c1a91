"""Per-layer activation and weight summaries computed on the device.

The reference's training loop watches its own layers: `prime_activation_summary` on the classifier before every epoch
(gbm/classify_combined.py:418) and a per-parameter weight mean / max written into `epoch_stats` after it (:484-485).
Here every tensor such a summary needs is already in HBM in the layout the kernels wrote — the encoder's forward
(`_encoder_forward_body`, a loop over the stages with one function per block kind) keeps the max-pool output, `(x, o1, out)` of every block, the pooled features and `feats` on every path and in every compute mode;
parameters and gradients of a `FlatParams` sit in two flat fp32 buckets — so the summaries read them where they lie
(`mil_tensor_stats_all`, csrc/tensor_stats.hip): channel-padded NHWC, bf16 or fp32, pad channels skipped, a whole table of
tensors in two launches, eight fp64 numbers per tensor, no copy, no host synchronisation, and no influence on which
kernels run (a forward hook on the stem switches the forward to the un-fused stem; an attached summary switches nothing).

Record of a tensor (`STAT_FIELDS`): [0] finite elements, [1] their sum, [2] their sum of squares, [3] min, [4] max over
them, [5] finite elements < 0 (the leaking side of the LeakyReLUs), [6] NaN / +-inf elements, [7] real elements.
"""
import ctypes

import torch

from . import _lib as L

STAT_FIELDS = ("finite", "sum", "sumsq", "min", "max", "negative", "nonfinite", "count")
_DT = {torch.float32: L.MIL_DT_F32, torch.bfloat16: L.MIL_DT_BF16}


def _entry(item):
    """(tensor, n_pix, c_real, c_pad) of one `tensor_stats` item."""
    if isinstance(item, (tuple, list)):
        t, c_real = item
        if t.dim() < 1 or t.shape[-1] < 1:
            raise ValueError("a (tensor, c_real) item needs a last dimension (the padded channel count) of at least 1")
        c_pad = int(t.shape[-1])
        n_pix = t.numel() // c_pad
    else:
        t, c_real, c_pad = item, 1, 1
        n_pix = t.numel()
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("tensor statistics are computed on an AMD GPU only (the tensor is not on a CUDA/HIP device)")
    if t.dtype not in _DT:
        raise ValueError(f"tensor statistics read float32 or bfloat16 tensors, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor statistics read tensors where they lie: the tensor must be contiguous")
    if not 1 <= int(c_real) <= c_pad:
        raise ValueError(f"c_real must be in 1..{c_pad}, got {c_real}")
    return t, n_pix, int(c_real), c_pad


class _StatsTable:
    """A job table (host records + device copy) and its workspace, rebuilt only when a pointer or a shape changes."""

    def __init__(self):
        self.tag = None
        self.host = self.table = self.ws = None
        self.ws_bytes = 0

    def run(self, entries, out):
        """entries: [(tensor, n_pix, c_real, c_pad)]; writes out [n,8] float64 (device) on the current stream."""
        lib = L.lib()
        n = len(entries)
        if n == 0:
            return out
        dev = out.device
        # an empty tensor has no storage to point at: any non-null pointer does (n_pix = 0: nothing is read)
        tag = tuple((t.data_ptr() or out.data_ptr(), n_pix, c_real, c_pad, _DT[t.dtype]) for t, n_pix, c_real, c_pad in entries)
        if tag != self.tag:
            rec = lib.mil_stats_job_bytes()
            host = (ctypes.c_char * (rec * n))()
            for i, job in enumerate(tag):
                L.check(lib.mil_stats_job_fill(ctypes.byref(host, i * rec), *job), "mil_stats_job_fill")
            need = ctypes.c_size_t(0)
            L.check(lib.mil_tensor_stats_workspace(ctypes.byref(need), host, n), "mil_tensor_stats_workspace")
            if self.ws is None or self.ws_bytes < need.value or self.ws.device != dev:
                self.ws = torch.empty((need.value + 7) // 8, dtype=torch.int64, device=dev)
                self.ws_bytes = self.ws.numel() * 8
            self.table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
            self.host, self.tag = host, tag
        L.check(lib.mil_tensor_stats_all(self.table.data_ptr(), self.host, n, out.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                                         L.stream_ptr()), "mil_tensor_stats_all")
        return out


def tensor_stats(items):
    """Statistics of a list of tensors in ONE call (two launches): `items` holds contiguous CUDA tensors (every element counts)
    or `(tensor, c_real)` pairs (records of `tensor.shape[-1]` elements of which the first `c_real` count: a channel-padded
    NHWC activation).  Returns the float64 [n, 8] records (`STAT_FIELDS`) on the device; nothing is copied and nothing
    synchronises with the host."""
    entries = [_entry(it) for it in items]
    if not entries:
        return torch.empty((0, 8), dtype=torch.float64)
    out = torch.empty((len(entries), 8), dtype=torch.float64, device=entries[0][0].device)
    return _StatsTable().run(entries, out)


def merge_stats(a, b):
    """Records of two passes over the same taps -> the record of both: counts and sums added, min / max taken."""
    out = a + b
    out[:, 3] = torch.minimum(a[:, 3], b[:, 3])
    out[:, 4] = torch.maximum(a[:, 4], b[:, 4])
    return out


def describe(rec):
    """One host record of 8 numbers -> the dictionary `ActivationSummary.read` returns per tap.  mean / std (population) / min /
    max / negative_share are over the FINITE elements (nan when there is none)."""
    finite, s, q, mn, mx, neg, bad, count = (float(v) for v in rec)
    nan = float("nan")
    mean = s / finite if finite else nan
    var = max(q / finite - mean * mean, 0.0) if finite else nan
    return {"mean": mean, "std": var ** 0.5 if finite else nan, "min": mn if finite else nan, "max": mx if finite else nan,
            "negative_share": neg / finite if finite else nan, "nonfinite": int(bad), "count": int(count)}


# ---- activations ----------------------------------------------------------------------------------------------------------------
def _encoder_of(model):
    from .encoder import ResNet
    from .model import Attention
    if isinstance(model, Attention):
        return model.cnn.module, "cnn.module."
    if isinstance(model, ResNet):
        return model, ""
    raise TypeError("ActivationSummary watches an Attention or the narrow ResNet encoder")


class ActivationSummary:
    """Statistics of the encoder's activations, taken on the device behind every encoder pass while attached.

    taps="stages": `cnn.module.maxpool`, `cnn.module.layer1` .. `layer4`, `cnn.module.fc` (6 tensors).
    taps="blocks": every block's inner activation after conv1 + LeakyReLU `...layerL.B:mid` and its output `...layerL.B`
    (the last block's output IS the stage's: `layerL` above), plus `cnn.module.avgpool`: 27 tensors for [3,3,3,3].
    (A bare `ResNet` carries the same names without the `cnn.module.` prefix.)

    The encoder hands the tensors over at the end of its forward; one `mil_tensor_stats_all` (two launches) reads them where
    they lie and no reference to an activation is kept.  `forward_bags` is one encoder pass: its numbers cover all tiles of the
    call.  `stats` is the device [n, 8] float64 of the last pass, or with `accumulate=True` the merge over the passes since
    `reset()` (counts and sums added, min / max taken).  Nothing synchronises until `read()` / `first_nonfinite()`."""

    def __init__(self, model, taps="stages", accumulate=False):
        if taps not in ("stages", "blocks"):
            raise ValueError('taps must be "stages" or "blocks"')
        enc, prefix = _encoder_of(model)
        if getattr(enc, "activation_summary", None) is not None:
            raise RuntimeError("this encoder already has an ActivationSummary attached: close() it first")
        self.taps, self.accumulate = taps, accumulate
        self._enc = enc
        names = [prefix + "maxpool"]
        self._widths = [enc.conv1.out_channels]
        for li in range(4):
            stage = getattr(enc, f"layer{li + 1}")
            for bi, blk in enumerate(stage):
                w = blk.conv1.out_channels
                if taps == "blocks":
                    names += [f"{prefix}layer{li + 1}.{bi}:mid", f"{prefix}layer{li + 1}.{bi}"]
                    self._widths += [w, w]
                elif bi == len(stage) - 1:
                    names.append(f"{prefix}layer{li + 1}")
                    self._widths.append(w)
        if taps == "blocks":
            names.append(prefix + "avgpool")
            self._widths.append(enc.fc.in_features)
        names.append(prefix + "fc")
        self._widths.append(enc.fc.out_features)
        self.names = names
        self._table = _StatsTable()
        self._last = None
        self.stats = None
        self.passes = 0
        enc.activation_summary = self

    # called by encoder._encoder_forward_body
    def observe(self, pool, blocks, pooled, feats):
        depths = [len(getattr(self._enc, f"layer{li + 1}")) for li in range(4)]
        tensors = [pool]
        if self.taps == "blocks":
            for _x, o1, out in blocks:
                tensors += [o1, out]
            tensors.append(pooled)
        else:
            last = -1
            for d in depths:
                last += d
                tensors.append(blocks[last][2])
        tensors.append(feats)
        if len(tensors) != len(self.names):
            raise RuntimeError(f"the encoder handed over {len(tensors)} tensors for {len(self.names)} taps")
        entries = [_entry((t, w)) for t, w in zip(tensors, self._widths)]
        if self._last is None or self._last.device != feats.device:
            self._last = torch.empty((len(entries), 8), dtype=torch.float64, device=feats.device)
        self._table.run(entries, self._last)
        if self.accumulate and self.stats is not None and self.passes:
            self.stats = merge_stats(self.stats, self._last)
        elif self.accumulate:
            self.stats = self._last.clone()
        else:
            self.stats = self._last
        self.passes += 1

    def _host(self):
        if self.stats is None:
            raise RuntimeError("no encoder pass has run since the summary was attached / reset")
        return self.stats.cpu()

    def read(self):
        """One device-to-host copy -> {name: {mean, std, min, max, negative_share, nonfinite, count}}."""
        return {name: describe(rec) for name, rec in zip(self.names, self._host().tolist())}

    def first_nonfinite(self):
        """The first tap in forward order that holds a NaN / +-inf element, or None."""
        for name, bad in zip(self.names, self._host()[:, 6].tolist()):
            if bad > 0:
                return name
        return None

    def reset(self):
        self.stats = None
        self.passes = 0

    def close(self):
        """Detach from the encoder and drop the buffers."""
        if getattr(self._enc, "activation_summary", None) is self:
            self._enc.activation_summary = None
        self._table = _StatsTable()
        self._last = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


# ---- parameters and gradients ---------------------------------------------------------------------------------------------------
def parameter_jobs(module_or_flat, grads=False):
    """(names, tensors) that `parameter_stats` reads: a module's `named_parameters()` (or their `.grad`), or the slices of a
    `FlatParams`' `flat` / `flat_grad` bucket — views, no copies."""
    from .dist import FlatParams
    if isinstance(module_or_flat, FlatParams):
        fp = module_or_flat
        bucket = fp.flat_grad if grads else fp.flat
        tensors, off = [], 0
        for p in fp.params:
            tensors.append(bucket[off:off + p.numel()])
            off += p.numel()
        return list(fp.names), tensors
    named = list(module_or_flat.named_parameters()) if hasattr(module_or_flat, "named_parameters") else list(module_or_flat)
    names = [n for n, _p in named]
    if not grads:
        return names, [p.detach() for _n, p in named]
    missing = [n for n, p in named if p.grad is None]
    if missing:
        raise ValueError(f"no gradient yet for {missing[0]} (and {len(missing) - 1} more): run a backward pass first")
    return names, [p.grad for _n, p in named]


def parameter_stats(module_or_flat, grads=False):
    """(names, stats): one record (`STAT_FIELDS`) per parameter — or per gradient — of a module or a `FlatParams`, in
    `named_parameters()` order (the 65 reference keys for `Attention`), in ONE call (two launches) on the tensors where they
    lie; `stats` is float64 [n, 8] on the device."""
    names, tensors = parameter_jobs(module_or_flat, grads)
    return names, tensor_stats(tensors)
