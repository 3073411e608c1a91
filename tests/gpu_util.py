"""Helpers shared by the -m gpu parity tests (layout conversion between the reference's NCHW fp32
tensors and the kernels' channel-padded NHWC tensors)."""
import torch

X3 = "bf16x3"        # compute mode of the split-precision path: fp32 tensors, three bf16 MFMAs per k-step (mil_amd._lib.BF16X3)


def storage(dtype):
    return torch.float32 if dtype == X3 else dtype


def cpad(c):
    return (c + 7) // 8 * 8


def to_nhwc(x_nchw, dtype, device="cuda"):
    n, c, h, w = x_nchw.shape
    out = torch.zeros((n, h, w, cpad(c)), dtype=torch.float32)
    out[..., :c] = x_nchw.permute(0, 2, 3, 1)
    return out.to(device=device, dtype=storage(dtype)).contiguous()


def from_nhwc(y, c):
    return y[..., :c].float().cpu().permute(0, 3, 1, 2).contiguous()


def round_to(x, dtype):
    """What the kernel sees after the operand is stored in `dtype`."""
    return x.to(storage(dtype)).float()


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


# ---- allocation poison -------------------------------------------------------------------------------------------------------
# The wrappers hand kernels 70-odd `torch.empty` / `empty_like` buffers as outputs, winner records and slab workspaces.  What a
# kernel leaves unwritten there is the caching allocator's residue — inside one test very often the previous, CORRECT result
# of the same shape.  Under `poison_allocations()` a never-written float is a NaN and a never-written byte is 255 instead.
#   * floating dtypes: every byte 0xFF (a NaN in fp32, bf16, fp16 and fp64);
#   * uint8: 255.  The one-byte max-pool winner records are only ever COMPARED with tap numbers 0..8 by their consumers
#     (pointwise.hip maxpool_bwd_kernel, the fused stem backward kernels in conv_wgrad.hip and stem_bwd_walk.cuh: `(w & 15) ==
#     tap`), never used to form an address: an unwritten record drops a gradient — a mismatch — instead of faulting;
#   * int32 / int64 and every other dtype: untouched (they hold offsets and indices).
# The fill runs on the current stream, like the kernel launch that follows it (also inside `with torch.cuda.stream(side)`).
_POISON_TAG = "_mil_poison_wrapper"


def _poison_fill(t):
    if not isinstance(t, torch.Tensor) or t.numel() == 0 or t.layout != torch.strided:
        return t
    if not (t.is_floating_point() or t.dtype == torch.uint8):
        return t
    with torch.no_grad():
        if t.is_contiguous():
            torch.Tensor.fill_(t.view(-1).view(torch.uint8), 255)
        else:                                   # e.g. empty_like of a permuted tensor: same values, through the strides
            torch.Tensor.fill_(t, 255 if t.dtype == torch.uint8 else float("nan"))
    return t


class poison_allocations:
    """Switches the poison on when constructed: `poison_allocations()` alone is a one-way switch for a whole process,
    `with poison_allocations():` restores the three originals on exit (also after an exception).  `device_predicate(tensor)`
    says which fresh tensors are filled — CUDA tensors by default; the CPU tests pass their own.  `reduce_batch=True` also
    re-fills a `ReduceBatch.workspace` buffer every time it is handed out (the persistent slab buffers keep LAST step's
    slabs otherwise).  That fill is ordered before the producer because both go to the current stream: the deferred
    reductions are not used together with side streams (encoder.py: `batch` is None when `overlap_wgrad` is set; the
    side-stream path allocates with torch.empty inside its `with torch.cuda.stream(side)`, which the wrapper above covers)."""

    def __init__(self, device_predicate=None, reduce_batch=True):
        pred = device_predicate or (lambda t: t.is_cuda)
        self._saved = [(torch, "empty", torch.empty), (torch, "empty_like", torch.empty_like),
                       (torch.Tensor, "new_empty", torch.Tensor.new_empty)]
        if reduce_batch:
            from mil_amd import ops
            self._saved.append((ops.ReduceBatch, "workspace", ops.ReduceBatch.workspace))

        def wrap(orig):
            def poisoned(*args, **kwargs):
                t = orig(*args, **kwargs)
                return _poison_fill(t) if isinstance(t, torch.Tensor) and pred(t) else t
            setattr(poisoned, _POISON_TAG, True)
            poisoned.__name__ = getattr(orig, "__name__", "poisoned")
            return poisoned

        for owner, name, orig in self._saved:
            setattr(owner, name, wrap(orig))

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        for owner, name, orig in reversed(self._saved):
            setattr(owner, name, orig)
        self._saved = []
        return False


def allocations_poisoned():
    return bool(getattr(torch.empty, _POISON_TAG, False))
