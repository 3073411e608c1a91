"""Thin tensor-level wrappers over the C ABI (include/mil_hip.h).  Each wrapper checks shapes on the
host (a wrong extent in a hand-written kernel is a GPU fault, not an exception), allocates outputs with
torch (plumbing) and enqueues the HIP kernel on torch's current stream."""
import collections
import ctypes

import torch

from . import _lib as L

LEAK = 0.1   # LeakyReLU slope of the reference (nnBlocks.py:170, gbm/model.py:25)


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
    `want(label)` selects which launches are bracketed; everything else runs untouched."""

    def __init__(self, want):
        self.want = want
        self.spans = []

    def bracket(self, label):
        if not self.want(label):
            return None
        start = torch.cuda.Event(enable_timing=True)
        end = torch.cuda.Event(enable_timing=True)
        start.record()
        self.spans.append((label, start, end))
        return end

    def durations_ms(self):
        torch.cuda.synchronize()
        return [(label, s.elapsed_time(e)) for label, s, e in self.spans]


TIMER = None   # set to a KernelTimer by bench.py


class ReduceBatch:
    """Deferred slab reductions (mil_reduce_defer_begin / _end / mil_wgrad_reduce_all): inside `with batch:` every
    weight-gradient producer records its reduction instead of launching it; leaving the block runs them all in ONE
    launch.  The producers' workspaces must stay untouched until then: `workspace(key, nbytes)` hands out one persistent
    buffer per call site."""
    MAX_JOBS = 64

    def __init__(self, device):
        self.device = device
        self.rec = L.lib().mil_reduce_job_bytes()
        self.host = (ctypes.c_char * (self.rec * self.MAX_JOBS))()
        self.dev = torch.empty(self.rec * self.MAX_JOBS, dtype=torch.uint8, device=device)
        self.uploaded = None                 # bytes of the table the device copy holds
        self.ws = {}                         # persistent slab buffers, one per call site (about 0.7 GB at 2048 tiles of 256x256)
        self.handed = None                   # keys handed out inside the current `with` block

    def workspace(self, key, nbytes):
        if self.handed is not None:
            if key in self.handed:
                raise RuntimeError(f"slab workspace {key!r} handed out twice inside one deferred-reduction block: the second "
                                   "producer would overwrite slabs the batched reduction has not read yet")
            self.handed.add(key)
        t = self.ws[key] = workspace_for(self.ws.get(key), nbytes, self.device)
        return t

    def __enter__(self):
        L.check(L.lib().mil_reduce_defer_begin(ctypes.addressof(self.host), self.MAX_JOBS), "mil_reduce_defer_begin")
        self.handed = set()
        return self

    def __exit__(self, exc_type, exc, tb):
        n = ctypes.c_int(0)
        self.handed = None
        L.check(L.lib().mil_reduce_defer_end(ctypes.byref(n)), "mil_reduce_defer_end")
        if exc_type is not None or n.value == 0:
            return False
        raw = bytes(self.host[: self.rec * n.value])
        if raw != self.uploaded:             # pointers and shapes repeat step after step: the table is uploaded once
            self.dev[: len(raw)].copy_(torch.frombuffer(bytearray(raw), dtype=torch.uint8))
            self.uploaded = raw
        L.check(L.lib().mil_wgrad_reduce_all(self.dev.data_ptr(), ctypes.addressof(self.host), n.value, L.stream_ptr()),
                "mil_wgrad_reduce_all")
        return False


def cpad(c):
    return (c + 7) // 8 * 8


def _need(t, shape, dtype, name):
    if t is None:
        return
    if not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous CUDA tensor")
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise ValueError(f"{name}: expected {tuple(shape)} {dtype}, got {tuple(t.shape)} {t.dtype}")


def workspace_for(workspace, need, device):
    """`workspace` when it holds `need` bytes, else a fresh fp32 buffer that does."""
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=device)
    return workspace


def _grad_out(out, specs, device):
    """(gradient tensors, accumulate flag) for `specs` = (shape, name) per tensor: fresh fp32 tensors the kernel overwrites
    (out None), or the caller's own tensors, checked, which it accumulates into (p.grad views).  A spec of None stands for
    a tensor the caller does not want: None when allocating."""
    if out is None:
        return [None if sp is None else torch.empty(sp[0], dtype=torch.float32, device=device) for sp in specs], 0
    for t, (shape, name) in zip(out, specs):
        _need(t, shape, torch.float32, name)
    return out, 1


def _launch(symbol, label, *args, missing_ok=False):
    """Enqueue `symbol(*args)`, bracketed with events when TIMER wants `label` (None: a launch that is never timed).  False
    when the library has no kernel for these arguments (rc 2) and the caller has another path (`missing_ok`) — no end event
    is recorded then; every other failure raises."""
    end = TIMER.bracket(label) if TIMER and label is not None else None
    rc = getattr(L.lib(), symbol)(*args)
    if rc == 2 and missing_ok:
        return False
    L.check(rc, symbol)
    if end is not None:
        end.record()
    return True


def pack_weights(w, bias, mode, dtype):
    """fp32 [Cout,Cin,k,k] -> (packed MFMA-fragment weights, zero-padded fp32 bias)."""
    w = w.detach()
    if w.dtype != torch.float32 or not w.is_cuda or w.dim() != 4:
        raise ValueError("weights must be CUDA fp32 [Cout,Cin,k,k]")
    w = w.contiguous()
    cout, cin, ks, _ = w.shape
    elems = ctypes.c_size_t(0)
    L.check(L.lib().mil_packed_weight_elems(ctypes.byref(elems), cout, cin, ks, mode), "mil_packed_weight_elems")
    if dtype == L.BF16X3:                 # the split path's filters: fp32-sized fragments [hi | lo], packed under MIL_DT_F32S
        with L.f32_mma(L.MIL_DT_F32S):
            return pack_weights(w, bias, mode, torch.float32)
    packed = torch.empty(elems.value, dtype=dtype, device=w.device)
    n_out = cin if mode == L.PACK_DGRAD else cout
    nt = (cpad(n_out) + 15) // 16
    bias_pad = torch.empty(nt * 16, dtype=torch.float32, device=w.device)
    b = None if bias is None else bias.detach().contiguous()
    L.check(L.lib().mil_pack_conv_weights(w.data_ptr(), L.ptr(b), packed.data_ptr(), bias_pad.data_ptr(), cout, cin, ks,
                                          mode, L.dt_code(dtype, mma=True), L.stream_ptr()), "mil_pack_conv_weights")
    return packed, bias_pad


def conv(x, wpack, bias_pad, cout_p, *, ks, stride, pad, out_hw=None, res=None, act=None, lrelu=False,
         zero_insert=False, slope=LEAK):
    """y = mask(lrelu?(conv(x)+bias+res)) — see mil_conv_igemm in include/mil_hip.h."""
    n, h, w, cin_p = x.shape
    if zero_insert:
        if out_hw is None:
            raise ValueError("zero_insert needs the full-resolution output size")
        ho, wo = out_hw
    else:
        ho = (h + 2 * pad - ks) // stride + 1 if ks != 4 else h
        wo = (w + 2 * pad - ks) // stride + 1 if ks != 4 else w
    y = torch.empty((n, ho, wo, cout_p), dtype=x.dtype, device=x.device)
    _need(x, x.shape, x.dtype, "x")
    _need(res, y.shape, x.dtype, "res")
    _need(act, y.shape, x.dtype, "act")
    _launch("mil_conv_igemm", ("conv", cin_p, cout_p, ks, stride, bool(zero_insert), n, ho, wo),
            x.data_ptr(), wpack.data_ptr(), L.ptr(bias_pad), L.ptr(res), L.ptr(act), y.data_ptr(),
            n, h, w, cin_p, ho, wo, cout_p, ks, 1 if zero_insert else stride, pad,
            1 if zero_insert else 0, 1 if lrelu else 0, slope, L.dt_code(x.dtype, mma=True), L.stream_ptr())
    return y


RULES = (0, 1)                                    # mil_conv_dgrad_rule's rule: 0 the plain LeakyReLU derivative, 1 guided backpropagation


def _check_rule(rule):
    if isinstance(rule, bool) or rule not in RULES:
        raise ValueError(f"rule must be 0 (plain) or 1 (guided), got {rule!r}")
    return int(rule)


def conv_dgrad_rule(x, wpack, cout_p, *, ks, pad, rule, res=None, act=None, zero_insert=False, out_hw=None, slope=LEAK):
    """A stride-1 (or, with zero_insert, transposed stride-2) data gradient on the generic implicit-GEMM kernel — see
    mil_conv_dgrad_rule: x = dz, wpack = MIL_PACK_DGRAD fragments.  rule=0: (conv(x) + res) * lrelu'(act), what `conv` computes;
    rule=1, guided backpropagation: v = conv(x) + res, y = v where act > 0 and v > 0, else +0 — `act` is required.  Never the
    persistent, resident or streaming kernels `conv` may choose."""
    rule = _check_rule(rule)
    if rule == 1 and act is None:
        raise ValueError("rule=1 gates by the saved activation: act is required")
    if x.dim() != 4:
        raise ValueError(f"x must be [n,h,w,cin_p], got {tuple(x.shape)}")
    n, h, w, cin_p = x.shape
    if zero_insert:
        if out_hw is None:
            raise ValueError("zero_insert needs the full-resolution output size")
        ho, wo = (int(v) for v in out_hw)
        if ((ho + 2 * pad - ks) // 2 + 1, (wo + 2 * pad - ks) // 2 + 1) != (h, w):
            raise ValueError(f"a {ks}x{ks} stride-2 conv (pad {pad}) of {ho}x{wo} maps is not {h}x{w}")
    else:
        if out_hw is not None:
            raise ValueError("out_hw goes with zero_insert")
        ho, wo = h + 2 * pad - ks + 1, w + 2 * pad - ks + 1
        if ho < 1 or wo < 1:
            raise ValueError(f"no output for {h}x{w} maps, ks {ks}, pad {pad}")
    if cin_p % 8 or cout_p % 8:
        raise ValueError(f"padded channel counts are multiples of 8, got {cin_p} -> {cout_p}")
    frag_elems = (ks * ks * (cin_p // 8) + 3) // 4 * ((cout_p + 15) // 16) * 64 * 8      # [kstep][column tile][64 lanes][8]
    if not wpack.is_cuda or wpack.dtype != x.dtype or wpack.numel() < frag_elems:
        raise ValueError(f"wpack: expected {frag_elems} {x.dtype} elements of MIL_PACK_DGRAD fragments on the device, got "
                         f"{wpack.numel()} {wpack.dtype}")
    y = torch.empty((n, ho, wo, cout_p), dtype=x.dtype, device=x.device)
    _need(x, x.shape, x.dtype, "x")
    _need(res, y.shape, x.dtype, "res")
    _need(act, y.shape, x.dtype, "act")
    _launch("mil_conv_dgrad_rule", ("conv_dgrad_rule", cin_p, cout_p, ks, rule, bool(zero_insert), n, ho, wo),
            x.data_ptr(), wpack.data_ptr(), None, L.ptr(res), L.ptr(act), y.data_ptr(),
            n, h, w, cin_p, ho, wo, cout_p, ks, 1, pad, 1 if zero_insert else 0, 0, slope, rule,
            L.dt_code(x.dtype, mma=True), L.stream_ptr())
    return y


def wgrad_workspace_bytes(n, h, w, cin, ho, wo, cout, ks, stride, pad, stem, dtype):
    need = ctypes.c_size_t(0)
    L.check(L.lib().mil_conv_wgrad_workspace(ctypes.byref(need), n, h, w, cin, ho, wo, cout, ks, stride, pad,
                                             1 if stem else 0, L.dt_code(dtype, mma=True)), "mil_conv_wgrad_workspace")
    return need.value


def conv_wgrad(x, dz, cin, cout, *, ks, stride, pad, stem=False, want_bias=True, workspace=None, out=None):
    """(dW [cout,cin,k,k] fp32, db [cout] fp32 or None) — see mil_conv_wgrad."""
    n, h, w, cin_p = x.shape
    _, ho, wo, cout_p = dz.shape
    _need(dz, (n, ho, wo, cpad(cout)), x.dtype, "dz")
    _need(x, (n, h, w, 16 if stem else cpad(cin)), x.dtype, "x")
    workspace = workspace_for(workspace, wgrad_workspace_bytes(n, h, w, cin, ho, wo, cout, ks, stride, pad, stem, x.dtype), x.device)
    kk = 7 if stem else ks
    (dw, db), accumulate = _grad_out(out, (((cout, cin, kk, kk), "dw"), ((cout,), "db") if want_bias or out is not None else None),
                                     x.device)
    _launch("mil_conv_wgrad", ("wgrad", cin_p, cout_p, ks, stride, n, ho, wo),
            x.data_ptr(), dz.data_ptr(), dw.data_ptr(), L.ptr(db), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), n, h, w, cin, ho, wo, cout, ks, stride,
            pad, 1 if stem else 0, accumulate, L.dt_code(x.dtype, mma=True), L.stream_ptr())
    return dw, db


def bwd_fused_workspace_bytes(n, h, w, cout, cin, ks, pad, dtype, dense=False):
    """Slab bytes the fused backward needs, or None when this shape (and gradient layout) has no fused kernel."""
    need = ctypes.c_size_t(0)
    rc = L.lib().mil_conv_bwd_fused_workspace(ctypes.byref(need), n, h, w, cout, cin, ks, pad, L.dt_code(dtype, dense, mma=True))
    if rc == 2:
        return None
    L.check(rc, "mil_conv_bwd_fused_workspace")
    return need.value


def conv_bwd_fused(dz, wpack_dgrad, x, cin, cout, *, addend=None, mask=True, ks=3, pad=1, workspace=None, slope=LEAK,
                   out=None):
    """(dx, dW, db) of a 3x3 stride-1 conv in one pass, or None if unsupported — see mil_conv_bwd_fused.  A dz with exactly
    `cout` (unpadded) channels selects the dense gradient layout (MIL_DT_BF16_DGRAD): addend and dx are then [n,h,w,cin]
    too, x keeps its padded channels."""
    n, h, w, cz = dz.shape
    dense = cz == cout and cpad(cout) != cout
    need = bwd_fused_workspace_bytes(n, h, w, cout, cin, ks, pad, dz.dtype, dense)
    if need is None:
        return None
    _need(dz, (n, h, w, cout if dense else cpad(cout)), dz.dtype, "dz")
    _need(x, (n, h, w, cpad(cin)), dz.dtype, "x")
    _need(addend, (n, h, w, cin if dense else cpad(cin)), dz.dtype, "addend")
    workspace = workspace_for(workspace, need, dz.device)
    dx = torch.empty((n, h, w, cin), dtype=dz.dtype, device=dz.device) if dense else torch.empty_like(x)
    (dw, db), accumulate = _grad_out(out, (((cout, cin, ks, ks), "dw"), ((cout,), "db")), dz.device)
    _launch("mil_conv_bwd_fused", ("bwd_fused", cpad(cout), cpad(cin), ks, 1, False, n, h, w, addend is not None),
            dz.data_ptr(), wpack_dgrad.data_ptr(), x.data_ptr(), L.ptr(addend), dx.data_ptr(),
            dw.data_ptr(), db.data_ptr(), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), n, h, w, cout, cin, ks, pad,
            1 if mask else 0, accumulate, slope, L.dt_code(dz.dtype, dense, mma=True), L.stream_ptr())
    return dx, dw, db


def maxpool_fwd(x):
    n, h, w, cp = x.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = torch.empty((n, ho, wo, cp), dtype=x.dtype, device=x.device)
    widx = torch.empty((n, ho, wo, cp), dtype=torch.uint8, device=x.device)
    L.check(L.lib().mil_maxpool_fwd(x.data_ptr(), y.data_ptr(), widx.data_ptr(), n, h, w, cp, L.dt_code(x.dtype),
                                    L.stream_ptr()), "mil_maxpool_fwd")
    return y, widx


def maxpool_bwd(gy, widx, in_hw, lrelu_mask=True, slope=LEAK, rule=0):
    """Gradient of the pooled tensor scattered back to the [n,H,W,cp] pool input; with lrelu_mask the LeakyReLU
    backward of that input is applied too (from the sign bit recorded in widx).  rule=1 (mil_maxpool_bwd_guided): the guided
    gate in place of that factor — the summed gradient of a pixel where the pixel's value and the sum are positive, else +0."""
    rule = _check_rule(rule)
    if rule == 1 and not lrelu_mask:
        raise ValueError("rule=1 replaces the LeakyReLU factor: it does not go with lrelu_mask=False")
    n, ho, wo, cp = widx.shape
    h, w = in_hw
    if ((h - 1) // 2 + 1, (w - 1) // 2 + 1) != (ho, wo):
        raise ValueError(f"pool input {h}x{w} does not produce {ho}x{wo}")
    _need(gy, widx.shape, gy.dtype, "gy")
    gx = torch.empty((n, h, w, cp), dtype=gy.dtype, device=gy.device)
    if rule == 1:
        _need(widx, widx.shape, torch.uint8, "widx")
        L.check(L.lib().mil_maxpool_bwd_guided(gy.data_ptr(), widx.data_ptr(), gx.data_ptr(), n, h, w, cp, L.dt_code(gy.dtype),
                                               L.stream_ptr()), "mil_maxpool_bwd_guided")
        return gx
    L.check(L.lib().mil_maxpool_bwd(gy.data_ptr(), widx.data_ptr(), gx.data_ptr(), n, h, w, cp, 1 if lrelu_mask else 0,
                                    slope, L.dt_code(gy.dtype), L.stream_ptr()), "mil_maxpool_bwd")
    return gx


# channel counts for which the one-pass block forward beats the two persistent launches (measured: 40 channels leave
# room for only one workgroup per CU and lose)
BLOCK_FWD_CHANNELS = (24,)


def conv_block_fwd(x, wpack1, bias1, wpack2, bias2, *, slope=LEAK):
    """(o1, y) of an identity-shortcut residual block in one pass (see mil_conv_block_fwd), or None when the shape/dtype
    has no such kernel."""
    n, h, w, cp = x.shape
    code = L.dt_code(x.dtype, mma=True)
    if code == L.MIL_DT_F32S:                 # fp32 tensors, split products: the 20-channel stage (16 x 8 tiles)
        if cp != 24 or h < 8 or w < 16:
            return None
    elif x.dtype != torch.bfloat16 or cp not in BLOCK_FWD_CHANNELS or h < 16 or w < 16:
        return None
    _need(x, x.shape, x.dtype, "x")
    o1 = torch.empty_like(x)
    y = torch.empty_like(x)
    if not _launch("mil_conv_block_fwd", ("block_fwd", cp, n, h, w),
                   x.data_ptr(), wpack1.data_ptr(), L.ptr(bias1), wpack2.data_ptr(), L.ptr(bias2),
                   o1.data_ptr(), y.data_ptr(), n, h, w, cp, slope, code, L.stream_ptr(), missing_ok=True):
        return None
    return o1, y


RESIDENT_SHAPES = ((80, 8, 8), (64, 16, 16), (80, 10, 10), (64, 19, 19))     # (padded channels, H, W) with a pixel-resident kernel (the last two: the 300x300 driver size)


class _ChainConv(ctypes.Structure):
    _fields_ = [("wpack", ctypes.c_void_p), ("bias", ctypes.c_void_p), ("res", ctypes.c_void_p), ("act", ctypes.c_void_p),
                ("out", ctypes.c_void_p), ("lrelu", ctypes.c_int), ("pad_", ctypes.c_int)]


def conv_chain(x, convs, *, slope=LEAK):
    """Outputs of a chain of 3x3 stride-1 convs on LDS-resident whole images, one launch (see mil_conv_chain), or None
    when the shape/dtype has no such kernel.  `convs`: dicts with w, and optionally bias, res, act, lrelu; res / act are
    tensors, or an int k = the output of conv k of this chain (k earlier than the conv that names it)."""
    n, h, w, cp = x.shape
    code = L.dt_code(x.dtype, mma=True)
    if code not in (L.MIL_DT_BF16, L.MIL_DT_F32S) or (cp, h, w) not in RESIDENT_SHAPES or not 1 <= len(convs) <= 6:
        return None
    _need(x, x.shape, x.dtype, "x")
    outs = [torch.empty_like(x) for _ in convs]
    arr = (_ChainConv * len(convs))()
    for k, c in enumerate(convs):
        ops_ = {}
        for name in ("res", "act"):
            t = c.get(name)
            if isinstance(t, int):
                if not 0 <= t < k:
                    raise ValueError(f"conv {k}: {name} refers to conv {t}, which is not earlier in the chain")
                t = outs[t]
            _need(t, x.shape, x.dtype, name)
            ops_[name] = t
        arr[k].wpack = c["w"].data_ptr()
        arr[k].bias = L.ptr(c.get("bias"))
        arr[k].res, arr[k].act = L.ptr(ops_["res"]), L.ptr(ops_["act"])
        arr[k].out = outs[k].data_ptr()
        arr[k].lrelu = 1 if c.get("lrelu") else 0
    if not _launch("mil_conv_chain", ("chain", cp, n, h, w, len(convs)),
                   x.data_ptr(), ctypes.addressof(arr), len(convs), n, h, w, cp, slope, code, L.stream_ptr(), missing_ok=True):
        return None
    return outs


def conv_pair(x, wA, biasA, wB, biasB, *, resA=None, actA=None, lreluA=False, resB=None, actB=None, lreluB=False, slope=LEAK):
    """(outA, outB) = two 3x3 stride-1 convs back to back on LDS-resident whole images in one launch (conv_chain with two
    convs: 80 channels on 8x8 maps, 64 channels on 16x16 maps), or None when the shape/dtype has no such kernel."""
    outs = conv_chain(x, [dict(w=wA, bias=biasA, res=resA, act=actA, lrelu=lreluA),
                          dict(w=wB, bias=biasB, res=resB, act=actB, lrelu=lreluB)], slope=slope)
    return None if outs is None else (outs[0], outs[1])


def conv_s2_entry(x, wpack3, bias_pad, wpack1, cout_p, *, slope=LEAK):
    """(lrelu(conv3x3_s2(x)+b), conv1x1_s2(x)) in one pass over x (see mil_conv_s2_entry), or None when the shape/dtype
    has no such kernel."""
    n, h, w, cin_p = x.shape
    code = L.dt_code(x.dtype, mma=True)
    if code not in (L.MIL_DT_BF16, L.MIL_DT_F32S):
        return None
    _need(x, x.shape, x.dtype, "x")
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y1 = torch.empty((n, ho, wo, cout_p), dtype=x.dtype, device=x.device)
    y2 = torch.empty_like(y1)
    if not _launch("mil_conv_s2_entry", ("s2_entry", cin_p, cout_p, n, h, w),
                   x.data_ptr(), wpack3.data_ptr(), L.ptr(bias_pad), wpack1.data_ptr(), y1.data_ptr(),
                   y2.data_ptr(), n, h, w, cin_p, cout_p, slope, code, L.stream_ptr(), missing_ok=True):
        return None
    return y1, y2


def conv_wgrad_pair(x, dz1, dz2, cin, cout, *, workspace=None, out=None):
    """(dW3, db3, dW1) of a stage-entry block's 3x3/s2 conv and 1x1/s2 projection from one pass over x (see
    mil_conv_wgrad_pair), or None when the shape/dtype has no such kernel.  out = (dw3, db3, dw1) accumulates in place."""
    n, h, w, _ = x.shape
    _, ho, wo, _ = dz1.shape
    code = L.dt_code(x.dtype, mma=True)
    if code not in (L.MIL_DT_BF16, L.MIL_DT_F32S):
        return None
    _need(x, (n, h, w, cpad(cin)), x.dtype, "x")
    _need(dz1, (n, ho, wo, cpad(cout)), x.dtype, "dz1")
    _need(dz2, (n, ho, wo, cpad(cout)), x.dtype, "dz2")
    need = ctypes.c_size_t(0)
    rc = L.lib().mil_conv_wgrad_pair_workspace(ctypes.byref(need), n, h, w, cin, ho, wo, cout, code)
    if rc == 2:
        return None
    L.check(rc, "mil_conv_wgrad_pair_workspace")
    workspace = workspace_for(workspace, need.value, x.device)
    (dw3, db3, dw1), accumulate = _grad_out(out, (((cout, cin, 3, 3), "dw3"), ((cout,), "db3"), ((cout, cin, 1, 1), "dw1")), x.device)
    if not _launch("mil_conv_wgrad_pair", None,
                   x.data_ptr(), dz1.data_ptr(), dz2.data_ptr(), dw3.data_ptr(), db3.data_ptr(), dw1.data_ptr(),
                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), n, h, w, cin, ho, wo,
                   cout, accumulate, code, L.stream_ptr(), missing_ok=True):
        return None
    return dw3, db3, dw1, workspace


def conv_dgrad_s2(dz1, dz2, wpack, cx_p, out_hw, *, act=None, slope=LEAK, dense_cx=None):
    """lrelu'(act) * (conv3x3_s2^T(dz1) + conv1x1_s2^T(dz2)) in one pass (see mil_conv_dgrad_s2), or None when the
    shape/dtype has no such kernel.  dense_cx = the unpadded channel count: the result is [n,H,W,dense_cx] (dense gradient
    layout, MIL_DT_BF16_DGRAD); act keeps its padded channels."""
    n, h, w, cz_p = dz1.shape
    hh, ww = out_hw
    dense = dense_cx is not None
    if dz1.dtype != torch.bfloat16 and L.dt_code(dz1.dtype, mma=True) != L.MIL_DT_F32S:
        return None               # bf16, or fp32 tensors with split-precision products (the 40 -> 24 channel entry)
    _need(dz1, dz1.shape, dz1.dtype, "dz1")
    _need(dz2, dz1.shape, dz1.dtype, "dz2")
    y = torch.empty((n, hh, ww, dense_cx if dense else cx_p), dtype=dz1.dtype, device=dz1.device)
    _need(act, (n, hh, ww, cx_p), dz1.dtype, "act")
    if not _launch("mil_conv_dgrad_s2", ("dgrad_s2", cz_p, cx_p, n, hh, ww),
                   dz1.data_ptr(), L.ptr(dz2), wpack.data_ptr(), L.ptr(act), y.data_ptr(), n, h, w, cz_p,
                   hh, ww, cx_p, slope, L.dt_code(dz1.dtype, dense, mma=True), L.stream_ptr(), missing_ok=True):
        return None
    return y


def conv_entry_bwd(dz1, dz2, wpack, xin, cin, cout, *, masked=True, slope=LEAK, dense_cx=None, workspace=None, out=None):
    """(dx, dW3, db3, dW1) of a stage-entry block's two stride-2 convs in one launch (see mil_conv_entry_bwd): dx as
    conv_dgrad_s2 computes it (act = xin when masked) and the weight gradients as conv_wgrad_pair computes them, all bit for
    bit — or None when the shape/dtype has no such kernel.  out = (dw3, db3, dw1) accumulates in place; dense_cx as in
    conv_dgrad_s2."""
    n, h, w, _ = dz1.shape
    _, hh, ww, _ = xin.shape
    if dz1.dtype != torch.bfloat16:
        return None
    dense = dense_cx is not None
    code = L.dt_code(dz1.dtype, dense, mma=True)
    _need(dz1, (n, h, w, cpad(cout)), dz1.dtype, "dz1")
    _need(dz2, (n, h, w, cpad(cout)), dz1.dtype, "dz2")
    _need(xin, (n, hh, ww, cpad(cin)), dz1.dtype, "xin")
    need = ctypes.c_size_t(0)
    rc = L.lib().mil_conv_entry_bwd_workspace(ctypes.byref(need), n, h, w, cout, hh, ww, cin, code)
    if rc == 2:
        return None
    L.check(rc, "mil_conv_entry_bwd_workspace")
    workspace = workspace_for(workspace, need.value, dz1.device)
    dx = torch.empty((n, hh, ww, dense_cx if dense else cpad(cin)), dtype=dz1.dtype, device=dz1.device)
    (dw3, db3, dw1), accumulate = _grad_out(out, (((cout, cin, 3, 3), "dw3"), ((cout,), "db3"), ((cout, cin, 1, 1), "dw1")), dz1.device)
    if not _launch("mil_conv_entry_bwd", ("entry_bwd", cpad(cout), cpad(cin), n, hh, ww),
                   dz1.data_ptr(), dz2.data_ptr(), wpack.data_ptr(), xin.data_ptr(), dx.data_ptr(), dw3.data_ptr(),
                   db3.data_ptr(), dw1.data_ptr(), workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                   n, h, w, cout, hh, ww, cin, 1 if masked else 0, slope, accumulate, code, L.stream_ptr(), missing_ok=True):
        return None
    return dx, dw3, db3, dw1, workspace


# ---- the stem: one description per feed ---------------------------------------------------------------------
# The tiles reach the stem as fp32 [n,3,H,W] ("f32"), as the uint8 images they are ("u8", preprocess.U8Tiles) or as the bf16
# space-to-depth tensor [n,H/2,W/2,16] ("s2d", preprocess.S2dTiles).  The kernels are one template family
# (csrc/stem_fused.hip); a feed is what differs on the host: which tensor is acceptable (`ok`; `strict`: it must be
# contiguous already, else a contiguous copy is made; `expected`: the ValueError's text), the pointer alignment the fused
# kernels' vector loads need, the layout its extents are read from (`planar`: [n,3,H,W]), the C symbols and the timer labels.
StemFeed = collections.namedtuple("StemFeed", "planar ok strict expected align fwd bwd bwd_ws s2d fwd_label bwd_label")


def _planar_tiles(dtype):
    return lambda x: x.dim() == 4 and x.shape[1] == 3 and x.dtype == dtype and x.is_cuda


STEM_FEEDS = {
    "f32": StemFeed(planar=True, ok=_planar_tiles(torch.float32), strict=False, align=16,
                    expected="expected a CUDA fp32 [N,3,H,W] tile stack, got {shape} {dtype} on {device}",
                    fwd="mil_stem_fwd_fused", bwd="mil_stem_bwd_fused_nchw", bwd_ws="mil_stem_bwd_fused_nchw_workspace",
                    s2d="mil_stem_s2d", fwd_label="stem_fwd", bwd_label="stem_bwd"),
    "u8": StemFeed(planar=True, ok=_planar_tiles(torch.uint8), strict=True, align=4,
                   expected="expected a contiguous CUDA uint8 [N,3,H,W] tile stack, got {shape} {dtype} on {device}",
                   fwd="mil_stem_fwd_fused_u8", bwd="mil_stem_bwd_fused_u8", bwd_ws="mil_stem_bwd_fused_u8_workspace",
                   s2d="mil_stem_s2d_u8", fwd_label="stem_fwd_u8", bwd_label="stem_bwd_u8"),
    "s2d": StemFeed(planar=False, ok=lambda x: x.dim() == 4 and x.shape[3] == 16 and x.dtype == torch.bfloat16 and x.is_cuda,
                    strict=True, align=16, expected="expected a contiguous CUDA bf16 [N,H/2,W/2,16] tensor, got {shape} {dtype}",
                    fwd="mil_stem_fwd_fused_xs", bwd="mil_stem_bwd_fused", bwd_ws="mil_stem_bwd_fused_workspace",
                    s2d=None, fwd_label="stem_fwd_xs", bwd_label="stem_bwd_xs"),
}


def stem_feed_kind(x, mode):
    """Which of the three feeds the tensor `x` is, "f32", "u8" or "s2d" (by its dtype); raises for a feed that the compute
    mode (or its storage dtype) `mode` does not take."""
    if x.dtype == torch.bfloat16:       # the bf16 space-to-depth tensor [T,H/2,W/2,16] (preprocess.S2dTiles)
        if x.dim() != 4 or x.shape[3] != 16:
            raise ValueError(f"a bf16 input must be the space-to-depth tensor [T,H/2,W/2,16], got {tuple(x.shape)}")
        if mode != torch.bfloat16:
            raise ValueError("space-to-depth bf16 tiles feed the bf16 compute mode only (the fp32 modes take fp32 [T,3,H,W] tiles)")
        return "s2d"
    if x.dtype == torch.uint8:          # the uint8 images themselves (preprocess.U8Tiles): every compute mode
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"a uint8 input must be the planar tile stack [T,3,H,W], got {tuple(x.shape)}")
        return "u8"
    return "f32"


def _feed_tensor(f, x):
    """The tensor the kernels of feed `f` read: `x`, checked and contiguous."""
    if not f.ok(x) or (f.strict and not x.is_contiguous()):
        raise ValueError(f.expected.format(shape=tuple(x.shape), dtype=x.dtype, device=x.device))
    return x.contiguous()


def _stem_extents(f, x):
    """(n, (H, W) of the tiles, (h2, w2) of their space-to-depth form, the extents the feed's kernels are given)."""
    if f.planar:
        n, _, h, w = x.shape
        return n, (h, w), (h // 2, w // 2), (h, w)
    n, h2, w2, _ = x.shape
    return n, (2 * h2, 2 * w2), (h2, w2), (h2, w2)


def _stem_s2d(kind, x, dtype):
    f = STEM_FEEDS[kind]
    x = _feed_tensor(f, x)
    n, _, h, w = x.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, 16), dtype=dtype, device=x.device)
    _launch(f.s2d, None, x.data_ptr(), out.data_ptr(), n, h, w, L.dt_code(dtype), L.stream_ptr())
    return out


def _stem_fwd(kind, x, wpack, bias_pad, cout_p, slope, dtype, keep_s2d):
    """(xs, pool, widx) of the whole stem in one pass over the tiles of feed `kind` (xs: the space-to-depth copy the f32 feed
    writes under keep_s2d, else None), or None when the shape / mode has no fused kernel.  bf16 with 24 or 64 channels; split
    precision: the 20-channel stem only, fp32 pooled map, never an s2d copy."""
    f = STEM_FEEDS[kind]
    x = _feed_tensor(f, x)
    code = L.dt_code(dtype, mma=True)
    if code == L.MIL_DT_F32S:
        if keep_s2d or cout_p != 24:
            return None
    elif dtype != torch.bfloat16:
        return None
    n, (h, w), (h2, w2), ext = _stem_extents(f, x)
    if (f.planar and (h % 2 or w % 4)) or cout_p not in (24, 64) or x.data_ptr() % f.align:
        return None
    hp, wp = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    xs = torch.empty((n, h2, w2, 16), dtype=dtype, device=x.device) if keep_s2d else None
    pool = torch.empty((n, hp, wp, cout_p), dtype=dtype, device=x.device)
    widx = torch.empty((n, hp, wp, cout_p), dtype=torch.uint8, device=x.device)
    dst = (L.ptr(xs), pool.data_ptr(), widx.data_ptr()) if kind == "f32" else (pool.data_ptr(), widx.data_ptr())
    if not _launch(f.fwd, (f.fwd_label, cout_p, n, h, w), x.data_ptr(), wpack.data_ptr(), L.ptr(bias_pad), *dst, n, *ext,
                   cout_p, slope, code, L.stream_ptr(), missing_ok=True):
        return None
    return xs, pool, widx


def _stem_bwd(kind, x, g_pool, widx, workspace, out, slope, ws_alloc):
    """(dW [20,3,7,7], db [20]) of the stem from the pooled-output gradient in one pass over the saved input of feed `kind`, or
    None when the input is not that feed's or the shape / dtype / alignment has no fused kernel.  A 20-channel g_pool is the
    dense gradient layout (MIL_DT_BF16_DGRAD / MIL_DT_F32S_DGRAD)."""
    f = STEM_FEEDS[kind]
    if not f.ok(x) or not x.is_contiguous() or x.data_ptr() % f.align:
        return None
    n, (h, w), (h2, w2), ext = _stem_extents(f, x)
    dense = g_pool.shape[-1] == 20
    gdt = g_pool.dtype if f.planar else x.dtype
    code = L.dt_code(gdt, dense, mma=True)
    need = ctypes.c_size_t(0)
    rc = getattr(L.lib(), f.bwd_ws)(ctypes.byref(need), n, *ext, code)
    if rc == 2:
        return None
    L.check(rc, f.bwd_ws)
    hp, wp = (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1
    _need(g_pool, (n, hp, wp, 20 if dense else 24), gdt, "g_pool")
    _need(widx, (n, hp, wp, 24), torch.uint8, "widx")
    if ws_alloc is not None:                 # deferred reductions: the slab buffer must outlive this call
        workspace = ws_alloc(need.value)
    workspace = workspace_for(workspace, need.value, x.device)
    (dw, db), accumulate = _grad_out(out, (((20, 3, 7, 7), "dw"), ((20,), "db")), x.device)
    if not _launch(f.bwd, (f.bwd_label, n, h, w), x.data_ptr(), g_pool.data_ptr(), widx.data_ptr(), dw.data_ptr(), db.data_ptr(),
                   workspace.data_ptr(), workspace.numel() * workspace.element_size(), n, *ext, slope, accumulate, code,
                   L.stream_ptr(), missing_ok=True):
        return None
    return dw, db


# The public names: what bench.py, tools/ and the tests call (and spy on).  The encoders reach the kernels through these
# module attributes too (`stem_forward`, `stem_backward`, `stem_to_s2d` below look them up at call time).
def stem_s2d(x, dtype):
    """[n,3,H,W] fp32 NCHW -> [n,ceil(H/2),ceil(W/2),16] NHWC space-to-depth of `dtype`."""
    return _stem_s2d("f32", x, dtype)


def stem_s2d_u8(x, dtype):
    """stem_s2d from uint8 tiles [n,3,H,W] (the uint8 feed, see mil_stem_s2d_u8): bit for bit stem_s2d of the decoded tensor."""
    return _stem_s2d("u8", x, dtype)


def stem_fwd_fused(x, wpack, bias_pad, cout_p, *, slope=LEAK, dtype=torch.bfloat16, keep_s2d=True):
    """(xs, pool, widx) of the whole stem in one pass over the fp32 NCHW tiles (see mil_stem_fwd_fused), or None when
    the shape/dtype has no fused kernel (the caller then runs stem_s2d / conv / maxpool_fwd).  keep_s2d=False: no
    space-to-depth copy is written (xs is None); the backward then reads x itself (stem_bwd_fused_nchw)."""
    return _stem_fwd("f32", x, wpack, bias_pad, cout_p, slope, dtype, keep_s2d)


def stem_fwd_fused_u8(x, wpack, bias_pad, cout_p, *, slope=LEAK, dtype=torch.bfloat16):
    """(pool, widx) of the whole stem in one pass over uint8 tiles x [n,3,H,W] (see mil_stem_fwd_fused_u8): bit for bit
    stem_fwd_fused(decoded tiles, keep_s2d=False).  cout_p 24 (the narrow encoder: bf16 or split precision) or 64
    (alt_resnet: bf16 only)."""
    fused = _stem_fwd("u8", x, wpack, bias_pad, cout_p, slope, dtype, False)
    return None if fused is None else fused[1:]


def stem_fwd_fused_xs(xs, wpack, bias_pad, cout_p, *, slope=LEAK):
    """(pool, widx) of the whole stem in one pass over the bf16 space-to-depth tiles xs [n,H2,W2,16] (see
    mil_stem_fwd_fused_xs), or None when the shape has no fused kernel."""
    fused = _stem_fwd("s2d", xs, wpack, bias_pad, cout_p, slope, torch.bfloat16, False)
    return None if fused is None else fused[1:]


def stem_bwd_fused(xs, g_pool, widx, *, workspace=None, out=None, slope=LEAK, ws_alloc=None):
    """The fused stem backward reading the bf16 space-to-depth copy xs [n,H2,W2,16] (see mil_stem_bwd_fused)."""
    return _stem_bwd("s2d", xs, g_pool, widx, workspace, out, slope, ws_alloc)


def stem_bwd_fused_nchw(x, g_pool, widx, *, workspace=None, out=None, slope=LEAK, ws_alloc=None):
    """The fused stem backward without a kept space-to-depth copy: reads the fp32 tiles x [n,3,H,W] (see mil_stem_bwd_fused_nchw)."""
    return _stem_bwd("f32", x, g_pool, widx, workspace, out, slope, ws_alloc)


def stem_bwd_fused_u8(x, g_pool, widx, *, workspace=None, out=None, slope=LEAK, ws_alloc=None):
    """stem_bwd_fused_nchw reading uint8 tiles x [n,3,H,W] (see mil_stem_bwd_fused_u8)."""
    return _stem_bwd("u8", x, g_pool, widx, workspace, out, slope, ws_alloc)


def stem_bwd_dense_ok(src, dtype):
    """True when the fused stem backward for this saved input (the fp32 or uint8 tiles [n,3,H,W], or the s2d copy
    [n,H2,W2,16]) exists with the dense pooled-gradient layout.  (An fp32 s2d copy — hooked or un-fused stem of the fp32
    modes — is no feed: no fused backward reads it.)"""
    for f in STEM_FEEDS.values():
        if f.ok(src):
            break
    else:
        return False
    if not src.is_contiguous() or src.data_ptr() % f.align or (not f.planar and dtype != torch.bfloat16):
        return False
    n, _, _, ext = _stem_extents(f, src)
    need = ctypes.c_size_t(0)
    return getattr(L.lib(), f.bwd_ws)(ctypes.byref(need), n, *ext, L.dt_code(dtype, True, mma=True)) == 0


def _public(symbol):
    """The public wrapper of a stem symbol: this module's attribute of the same name without `mil_`, as it is NOW."""
    return globals()[symbol[4:]]


def stem_to_s2d(kind, x, dtype):
    """The space-to-depth tensor of the tiles `x` of feed `kind` (an "s2d" feed is that tensor)."""
    return x if kind == "s2d" else _public(STEM_FEEDS[kind].s2d)(x, dtype)


def stem_backward(kind, src, g_pool, widx, **kw):
    """The fused stem backward of feed `kind` (stem_bwd_fused_nchw / _u8 / stem_bwd_fused) on its saved input, or None."""
    return _public(STEM_FEEDS[kind].bwd)(src, g_pool, widx, **kw)


def stem_forward(kind, x, wpack, bias_pad, cout_p, *, dtype, slope=LEAK, keep_s2d=False, allow_fused=True):
    """The stem on the tiles `x` of feed `kind`: the fused kernel when allowed and there is one, else stem_s2d* -> conv(ks=4)
    -> maxpool_fwd.  Returns (xs, pool, widx, stem_hw, stem): xs is the space-to-depth tensor where one exists (the caller's
    own for the "s2d" feed, the converter's when the chain ran, the fused kernel's under keep_s2d — "f32" only — else None);
    stem is the un-pooled map when the chain ran (forward hooks are shown it), else None."""
    fused = None
    if allow_fused and kind == "f32":       # the three public signatures differ: the one place that tells them apart
        fused = stem_fwd_fused(x, wpack, bias_pad, cout_p, slope=slope, dtype=dtype, keep_s2d=keep_s2d)
    elif allow_fused and kind == "u8":
        fused = stem_fwd_fused_u8(x, wpack, bias_pad, cout_p, slope=slope, dtype=dtype)
    elif allow_fused:
        fused = stem_fwd_fused_xs(x, wpack, bias_pad, cout_p, slope=slope)
    if fused is not None:
        xs, pool, widx = fused if kind == "f32" else ((x if kind == "s2d" else None),) + fused
        return xs, pool, widx, _stem_extents(STEM_FEEDS[kind], x)[2], None
    xs = stem_to_s2d(kind, x, dtype)
    stem = conv(xs, wpack, bias_pad, cout_p, ks=4, stride=1, pad=2, lrelu=True, slope=slope)
    pool, widx = maxpool_fwd(stem)
    return xs, pool, widx, tuple(stem.shape[1:3]), stem


def stem_dgrad(dstem, wpack, hw, *, reduce=None, dx=None, sal=None, gate=None):
    """Data gradient of the stem convolution (see mil_stem_dgrad): dstem [n,ceil(H/2),ceil(W/2),24] — the un-pooled stem
    gradient `maxpool_bwd` returns, bf16 or fp32 — and the MIL_PACK_STEM_DGRAD fragments of conv1.weight -> (dx, sal) for
    tiles of hw = (H, W).  reduce=None: dx [n,3,H,W] fp32 and sal None.  reduce="max_abs": sal [n,H,W] fp32 = max_c |dx| from
    the same accumulators, and dx None unless a `dx` tensor is handed in to be written too.  `dx` / `sal`: the caller's own
    output tensors (checked) in place of fresh ones.  gate: uint8 [n,H,W], with reduce=None only (see mil_stem_dgrad_gated) —
    dx is then the gradient times gate / 255 per pixel, multiplied in the kernel's store epilogue: no ungated tensor is made."""
    if reduce not in (None, "max_abs"):
        raise ValueError(f"reduce must be None or 'max_abs', got {reduce!r}")
    if gate is not None and (reduce is not None or sal is not None):
        raise ValueError("gate multiplies the three-channel gradient: it goes with reduce=None and without sal")
    if dstem.dim() != 4:
        raise ValueError(f"dstem must be [n,H2,W2,24], got {tuple(dstem.shape)}")
    n = dstem.shape[0]
    h, w = hw
    code = L.dt_code(dstem.dtype, mma=True)
    _need(dstem, (n, (h + 1) // 2, (w + 1) // 2, 24), dstem.dtype, "dstem")
    elems = ctypes.c_size_t(0)
    L.check(L.lib().mil_packed_weight_elems(ctypes.byref(elems), 20, 3, 7, L.PACK_STEM_DGRAD), "mil_packed_weight_elems")
    _need(wpack, (elems.value,), dstem.dtype, "wpack")
    if reduce is None:
        if sal is not None:
            raise ValueError("sal is written under reduce='max_abs' only")
        if dx is None:
            dx = torch.empty((n, 3, h, w), dtype=torch.float32, device=dstem.device)
    elif sal is None:
        sal = torch.empty((n, h, w), dtype=torch.float32, device=dstem.device)
    _need(dx, (n, 3, h, w), torch.float32, "dx")
    _need(sal, (n, h, w), torch.float32, "sal")
    if gate is not None:
        if not isinstance(gate, torch.Tensor):
            raise ValueError("gate must be a uint8 [n,H,W] tensor on the device")
        _need(gate, (n, h, w), torch.uint8, "gate")
        _launch("mil_stem_dgrad_gated", ("stem_dgrad_gated", n, h, w), dstem.data_ptr(), wpack.data_ptr(), gate.data_ptr(),
                dx.data_ptr(), n, h, w, code, L.stream_ptr())
        return dx, None
    _launch("mil_stem_dgrad", ("stem_dgrad", n, h, w, reduce is not None), dstem.data_ptr(), wpack.data_ptr(), L.ptr(dx),
            L.ptr(sal), n, h, w, 0 if reduce is None else 1, code, L.stream_ptr())
    return dx, sal


def stem_dgrad_acc(dstem, wpack, hw, acc, scale):
    """acc [n,3,H,W] fp32 += scale * dx in place (see mil_stem_dgrad_acc), dx what `stem_dgrad(dstem, wpack, hw)` returns: a
    product and a sum per element, no temporary gradient tensor.  Returns acc."""
    if dstem.dim() != 4:
        raise ValueError(f"dstem must be [n,H2,W2,24], got {tuple(dstem.shape)}")
    n = dstem.shape[0]
    h, w = hw
    code = L.dt_code(dstem.dtype, mma=True)
    _need(dstem, (n, (h + 1) // 2, (w + 1) // 2, 24), dstem.dtype, "dstem")
    elems = ctypes.c_size_t(0)
    L.check(L.lib().mil_packed_weight_elems(ctypes.byref(elems), 20, 3, 7, L.PACK_STEM_DGRAD), "mil_packed_weight_elems")
    _need(wpack, (elems.value,), dstem.dtype, "wpack")
    if acc is None:
        raise ValueError("acc: the running sum [n,3,H,W] fp32 is the caller's")
    _need(acc, (n, 3, h, w), torch.float32, "acc")
    _launch("mil_stem_dgrad_acc", ("stem_dgrad_acc", n, h, w), dstem.data_ptr(), wpack.data_ptr(), acc.data_ptr(), float(scale), n, h,
            w, code, L.stream_ptr())
    return acc


def _tile_stack(tiles, name="tiles"):
    """(the contiguous CUDA tensor behind fp32 tiles or `U8Tiles`, is_u8) for the path-attribution kernels."""
    from .preprocess import U8Tiles
    x = tiles.u8 if isinstance(tiles, U8Tiles) else tiles
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{name} must be fp32 [T,3,H,W] or U8Tiles, got {tuple(getattr(x, 'shape', ()))}")
    if x.dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"{name} must be fp32 [T,3,H,W] or U8Tiles, got {x.dtype}")
    if x.dtype == torch.uint8 and not isinstance(tiles, U8Tiles):
        raise ValueError(f"{name}: uint8 images come wrapped in U8Tiles")
    _need(x, x.shape, x.dtype, name)
    return x, x.dtype == torch.uint8


def _base3(base):
    """Three per-channel floats from a scalar or a sequence of three."""
    vals = [float(base)] * 3 if isinstance(base, (int, float)) else [float(v) for v in base]
    if len(vals) != 3:
        raise ValueError(f"base: a scalar or three per-channel values, got {len(vals)}")
    return vals


def path_point(tiles, alpha, base, *, noise_level=0.0, value_range=None, seed=0, sample=0, out=None):
    """base[c] + alpha * (tiles - base[c]) + sigma * noise as fp32 [T,3,H,W] (see mil_path_point): tiles an fp32 stack or
    `U8Tiles`; base a scalar or three per-channel values; sigma = noise_level * (value_range[1] - value_range[0]) with
    value_range a device fp32 tensor (lo, hi), or noise_level itself without one; the noise of element i is a function of
    (seed, sample, i) only (Philox4x32-10 + Box-Muller) and torch's generator is not involved.  `out`: the caller's tensor."""
    b = _base3(base)
    noise_level = float(noise_level)
    if not noise_level >= 0.0:
        raise ValueError(f"noise_level must be >= 0, got {noise_level}")
    seed, sample = int(seed), int(sample)
    if not 0 <= seed < 1 << 64 or not 0 <= sample < 1 << 32:
        raise ValueError(f"seed must fit 64 bits and sample 32, got {seed} and {sample}")
    x, is_u8 = _tile_stack(tiles)
    n, _, h, w = x.shape
    _need(value_range, (2,), torch.float32, "value_range")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=x.device)
    _need(out, (n, 3, h, w), torch.float32, "out")
    _launch("mil_path_point", ("path_point", n, h, w, is_u8, noise_level != 0.0), x.data_ptr(), int(is_u8), out.data_ptr(), *b,
            float(alpha), noise_level, L.ptr(value_range), seed, sample, n, h, w, L.stream_ptr())
    return out


ATTR_MAP_MODES = ("sum", "max", "grad_max")       # mil_attr_finish's map_mode 0, 1, 2


def attr_finish(acc, tiles, base, *, want_attr=True, want_map=False, map_mode="sum", want_sums=False):
    """From an accumulated gradient acc [T,3,H,W] fp32 to (attr, map, tile_sum) (see mil_attr_finish; None for what is not
    wanted): attr = (tiles - base[c]) * acc; map [T,H,W] = |sum_c attr| ("sum"), max_c |attr| ("max") or max_c |acc|
    ("grad_max": reads no tiles, which may then be None); tile_sum [T] = the sum of attr per tile in a fixed order."""
    if map_mode not in ATTR_MAP_MODES:
        raise ValueError(f"map_mode must be one of {ATTR_MAP_MODES}, got {map_mode!r}")
    if not (want_attr or want_map or want_sums):
        raise ValueError("nothing is wanted")
    if not isinstance(acc, torch.Tensor) or acc.dim() != 4 or acc.shape[1] != 3:
        raise ValueError(f"acc must be fp32 [T,3,H,W], got {tuple(getattr(acc, 'shape', ()))}")
    _need(acc, acc.shape, torch.float32, "acc")
    n, _, h, w = acc.shape
    x, is_u8 = None, False
    if tiles is not None:
        x, is_u8 = _tile_stack(tiles)
        if x.shape != acc.shape:
            raise ValueError(f"tiles {tuple(x.shape)} and acc {tuple(acc.shape)} differ")
    elif want_attr or want_sums or map_mode != "grad_max":
        raise ValueError("only the 'grad_max' map is made without tiles")
    b = _base3(base)
    dev = acc.device
    attr = torch.empty_like(acc) if want_attr else None
    amap = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_map else None
    sums = torch.empty((n,), dtype=torch.float32, device=dev) if want_sums else None
    ws = torch.empty((n, L.ATTR_SLICES), dtype=torch.float32, device=dev) if want_sums else None
    _launch("mil_attr_finish", ("attr_finish", n, h, w, is_u8, want_attr, want_map, want_sums), acc.data_ptr(), L.ptr(x), int(is_u8),
            *b, L.ptr(attr), L.ptr(amap), ATTR_MAP_MODES.index(map_mode), L.ptr(sums), L.ptr(ws), n, h, w, L.stream_ptr())
    return attr, amap, sums


def _stage_map(t, c, name):
    """(n, h, w, cp, dtype code) of a stage output [T,h,w,cpad(c)], checked."""
    if not isinstance(t, torch.Tensor) or t.dim() != 4:
        raise ValueError(f"{name} must be [T,h,w,cp], got {tuple(getattr(t, 'shape', ()))}")
    n, h, w, cp = t.shape
    if cp != cpad(c) or c < 1:
        raise ValueError(f"{c} real channels go with {cpad(c)} stored ones, got {cp}")
    if h < 1 or w < 1:
        raise ValueError(f"maps of {h}x{w}")
    code = L.dt_code(t.dtype)
    _need(t, t.shape, t.dtype, name)
    return n, h, w, cp, code


def stage_seed(act, channels, c, *, objective=None, dz=None, slope=LEAK):
    """Objective and seed gradient of activation maximisation at a stage output (see mil_stage_seed): act [T,h,w,cpad(c)] — the
    stage's output as the forward keeps it, bf16 or fp32 — and channels, int32 [T] on the device, one channel in [0, c) per tile
    -> (objective fp32 [T] = the mean of each tile's channel, dz like act = the gradient of MINUS that mean with respect to the
    pre-activation map: -(1/(h w)) lrelu'(act) at the tile's channel, zero elsewhere).  `objective` / `dz`: the caller's own
    output tensors (checked) — a row of a trace, for one."""
    c = int(c)
    n, h, w, cp, code = _stage_map(act, c, "act")
    if not isinstance(channels, torch.Tensor):
        raise ValueError("channels must be an int32 [T] tensor on the device")
    _need(channels, (n,), torch.int32, "channels")
    if objective is None:
        objective = torch.empty((n,), dtype=torch.float32, device=act.device)
    _need(objective, (n,), torch.float32, "objective")
    if dz is None:
        dz = torch.empty_like(act)
    _need(dz, act.shape, act.dtype, "dz")
    ws = torch.empty((n, L.SEED_SLICES), dtype=torch.float32, device=act.device)
    _launch("mil_stage_seed", ("stage_seed", n, h, w, cp), act.data_ptr(), channels.data_ptr(), objective.data_ptr(), dz.data_ptr(),
            ws.data_ptr(), n, h, w, cp, c, slope, code, L.stream_ptr())
    return objective, dz


PIXEL_RULES = ("sgd", "adam")                     # mil_pixel_step's rule 0, 1
PIXEL_PROJECTIONS = ("none", "clamp", "u8")       # mil_pixel_step's project 0, 1, 2


def pixel_step_scalars(rule, lr, weight_decay, betas, eps, step):
    """The nine fp32 scalars of mil_pixel_step — (lr, wd, beta1, 1 - beta1, beta2, 1 - beta2, bc1, sqrt(bc2), eps) — checked;
    the differences, powers and the root are taken in double here and rounded once by the call."""
    if rule not in PIXEL_RULES:
        raise ValueError(f"rule must be one of {PIXEL_RULES}, got {rule!r}")
    lr, wd, eps = float(lr), float(weight_decay), float(eps)
    b1, b2 = (float(b) for b in betas)
    if lr != lr or not wd >= 0.0:
        raise ValueError(f"lr must be a number and weight_decay >= 0, got {lr} and {wd}")
    if int(step) != step or step < 1:
        raise ValueError(f"step counts from 1, got {step!r}")
    if rule == "adam" and not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0):
        raise ValueError(f"betas must lie in [0, 1) and eps be >= 0, got {betas!r} and {eps}")
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    return lr, wd, b1, 1.0 - b1, b2, 1.0 - b2, bc1, bc2 ** 0.5, eps


def _pixel_step_tail(symbol, label, x, g, state, u8_out, project, *scalars):
    """What `pixel_step` and `pixel_momentum_step` share behind their own checks of the rule: g, the rule's state tensors
    ((name, tensor) pairs, None where it keeps none) and u8_out checked against x, the decode table of project="u8", and the
    launch, timed as label + (project, whether it encodes).  Returns x."""
    for name, t in (("x", x), ("g", g)) + state:
        _need(t, x.shape, torch.float32, name)
    _need(u8_out, x.shape, torch.uint8, "u8_out")
    table = None
    if project == "u8":
        from .preprocess import U8Tiles
        table = U8Tiles.decode_table(x.device)
    _launch(symbol, label + (project, u8_out is not None), x.data_ptr(), g.data_ptr(), *(L.ptr(t) for _name, t in state), L.ptr(u8_out),
            L.ptr(table), x.numel(), *scalars, L.stream_ptr())
    return x


def pixel_step(x, g, state=None, *, rule="adam", lr=0.1, weight_decay=0.0, betas=(0.9, 0.999), eps=1e-8, step=1, project="none",
               u8_out=None):
    """One optimiser step on the images x [T,3,H,W] fp32 for the gradient g, in place and in one pass (see mil_pixel_step).
    rule="sgd": `torch.optim.SGD` without momentum; rule="adam": `torch.optim.Adam` with its coupled L2 decay, `state` = (m, v),
    two fp32 tensors like x that are updated in place, `step` counting from 1.  project: "none", "clamp" (to [-1, 1]) or "u8"
    (the round trip x <- decode(encode(x)) through the table `U8Tiles.float()` looks up).  u8_out: a uint8 tensor like x that
    receives encode(x) = rint(clip(x / 2 + 0.5, 0, 1) * 255) of the value stored.  Returns x."""
    if project not in PIXEL_PROJECTIONS:
        raise ValueError(f"project must be one of {PIXEL_PROJECTIONS}, got {project!r}")
    scalars = pixel_step_scalars(rule, lr, weight_decay, betas, eps, step)
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"x must be fp32 [T,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
    m = v = None
    if rule == "adam":
        if state is None or len(state) != 2 or state[0] is None or state[1] is None:
            raise ValueError("rule='adam' keeps two moments: state = (m, v), fp32 tensors like x")
        m, v = state
    elif state is not None:
        raise ValueError("rule='sgd' keeps no state")
    return _pixel_step_tail("mil_pixel_step", ("pixel_step", x.numel(), rule), x, g, (("m", m), ("v", v)), u8_out, project,
                            PIXEL_RULES.index(rule), PIXEL_PROJECTIONS.index(project), *scalars)


def stage_energy(target, c, *, energy=None):
    """E_t = the sum of target^2 over the c real channels of a stage output [T,h,w,cpad(c)] (bf16 or fp32) -> fp32 [T]: what
    `stage_match` divides by (see mil_stage_energy); computed once per inversion."""
    c = int(c)
    n, h, w, cp, code = _stage_map(target, c, "target")
    if energy is None:
        energy = torch.empty((n,), dtype=torch.float32, device=target.device)
    _need(energy, (n,), torch.float32, "energy")
    ws = torch.empty((n, L.SEED_SLICES), dtype=torch.float32, device=target.device)
    _launch("mil_stage_energy", ("stage_energy", n, h, w, cp), target.data_ptr(), energy.data_ptr(), ws.data_ptr(), n, h, w, cp, c, code,
            L.stream_ptr())
    return energy


def stage_match(act, target, c, *, weight=0.1, energy=None, loss=None, dz=None, slope=LEAK):
    """Loss and seed gradient of feature inversion at a stage output (see mil_stage_match): act and target [T,h,w,cpad(c)], two
    outputs of one stage as the forward keeps them -> (loss fp32 [T] = weight * sum (act - target)^2 / E_t over the real
    channels, dz like act = the gradient of loss_t with respect to the pre-activation map, ((2 weight / E_t) (act - target))
    lrelu'(act), zero in the padding channels).  energy: `stage_energy(target, c)` (None: computed here).  `loss` / `dz`: the
    caller's own output tensors (checked) — a row of a trace, for one.  E_t == 0 gives what IEEE division gives."""
    c = int(c)
    if not isinstance(target, torch.Tensor):
        raise ValueError("target must be a tensor like act")
    weight = float(weight)
    if weight != weight:
        raise ValueError("weight must be a number")
    n, h, w, cp, code = _stage_map(act, c, "act")
    _need(target, act.shape, act.dtype, "target")
    if energy is None:
        energy = stage_energy(target, c)
    _need(energy, (n,), torch.float32, "energy")
    if loss is None:
        loss = torch.empty((n,), dtype=torch.float32, device=act.device)
    _need(loss, (n,), torch.float32, "loss")
    if dz is None:
        dz = torch.empty_like(act)
    _need(dz, act.shape, act.dtype, "dz")
    ws = torch.empty((n, L.SEED_SLICES), dtype=torch.float32, device=act.device)
    _launch("mil_stage_match", ("stage_match", n, h, w, cp), act.data_ptr(), target.data_ptr(), energy.data_ptr(), loss.data_ptr(),
            dz.data_ptr(), ws.data_ptr(), n, h, w, cp, c, weight, slope, code, L.stream_ptr())
    return loss, dz


REG_ALPHAS = (2, 4, 6, 8)                         # mil_pixel_reg's alpha: the even powers it forms by repeated products


def _pixel_stack(x, name):
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{name} must be fp32 [T,3,H,W], got {tuple(getattr(x, 'shape', ()))}")
    if x.shape[2] < 1 or x.shape[3] < 1:
        raise ValueError(f"{name}: tiles of {x.shape[2]}x{x.shape[3]}")
    return x.shape[0], x.shape[2], x.shape[3]


def _shift(shift, h, w):
    """An integer (dy, dx) reduced mod (h, w)."""
    try:
        dy, dx = shift
        if any(isinstance(v, bool) or int(v) != v for v in (dy, dx)):
            raise TypeError
    except (TypeError, ValueError):
        raise ValueError(f"shift must be two integers (dy, dx), got {shift!r}") from None
    return int(dy) % h, int(dx) % w


def _overlap(a, b):
    """True when the two contiguous tensors share memory."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def reg_weights(alpha, alpha_weight, tv_weight):
    """(alpha, alpha_weight, tv_weight) of `pixel_reg`, checked: an even power in 2..8 and two weights >= 0."""
    if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or alpha not in REG_ALPHAS:
        raise ValueError(f"alpha must be one of {REG_ALPHAS}, got {alpha!r}")
    aw, tw = float(alpha_weight), float(tv_weight)
    if not (aw >= 0.0 and tw >= 0.0) or aw == float("inf") or tw == float("inf"):
        raise ValueError(f"alpha_weight and tv_weight must be finite and >= 0, got {alpha_weight!r} and {tv_weight!r}")
    return int(alpha), aw, tw


def pixel_reg(x, g, out=None, *, alpha=6, alpha_weight=0.0, tv_weight=0.0, shift=(0, 0), terms=None):
    """The pixel gradient g moved back through a jitter, plus the gradients of the two regularisers of x (see mil_pixel_reg):
    out[t,c,i,j] = g[t,c,(i+dy) mod H,(j+dx) mod W] + alpha_weight alpha x^(alpha-1) + tv_weight dTV/dx[i,j] for x, g fp32
    [T,3,H,W]; x is only read.  alpha: 2, 4, 6 or 8; TV: the toolkit's `total_variation_norm` with beta = 2.  shift: any two
    integers (dy, dx), reduced mod (H, W).  out: None (a fresh tensor) or the caller's; it may be g itself when the reduced
    shift is (0, 0) and may not overlap g or x otherwise.  terms: an fp32 [2,T] tensor that receives each tile's sum of x^alpha
    and its total variation.  Returns out."""
    alpha, aw, tw = reg_weights(alpha, alpha_weight, tv_weight)
    n, h, w = _pixel_stack(x, "x")
    dy, dx = _shift(shift, h, w)
    if not isinstance(g, torch.Tensor):
        raise ValueError("g must be a tensor like x")
    _need(x, x.shape, torch.float32, "x")
    _need(g, x.shape, torch.float32, "g")
    if out is None:
        out = torch.empty_like(x)
    _need(out, x.shape, torch.float32, "out")
    if out.data_ptr() == g.data_ptr() and n:
        if dy or dx:
            raise ValueError(f"out may be g itself only without a shift, got shift {(dy, dx)}")
    elif _overlap(out, g):
        raise ValueError("out overlaps g")
    if _overlap(out, x):
        raise ValueError("out overlaps x, which is only read")
    _need(terms, (2, n), torch.float32, "terms")
    ws = torch.empty((2, n, L.REG_SLICES), dtype=torch.float32, device=x.device) if terms is not None else None
    _launch("mil_pixel_reg", ("pixel_reg", n, h, w, terms is not None), x.data_ptr(), g.data_ptr(), out.data_ptr(), L.ptr(terms), L.ptr(ws),
            n, h, w, alpha, aw, tw, dy, dx, L.stream_ptr())
    return out


def pixel_shift(x, out, shift):
    """The jittered copy out[t,c,i,j] = x[t,c,(i-dy) mod H,(j-dx) mod W] of an fp32 stack [T,3,H,W] (see mil_pixel_shift): a bit
    copy, the inverse of `pixel_reg`'s index map.  out: None or the caller's tensor, not overlapping x.  Returns out."""
    n, h, w = _pixel_stack(x, "x")
    dy, dx = _shift(shift, h, w)
    _need(x, x.shape, torch.float32, "x")
    if out is None:
        out = torch.empty_like(x)
    _need(out, x.shape, torch.float32, "out")
    if _overlap(out, x):
        raise ValueError("out overlaps x")
    _launch("mil_pixel_shift", ("pixel_shift", n, h, w), x.data_ptr(), out.data_ptr(), n, h, w, dy, dx, L.stream_ptr())
    return out


BLUR_EDGES = ("reflect", "replicate", "wrap")     # mil_pixel_blur's edge 0, 1, 2
_blur_taps = {}                                   # (sigma, device) -> the fp32 taps on the device


def gauss_taps(sigma):
    """(radius, fp64 numpy [radius + 1]): the centre and one half of `scipy.ndimage`'s Gaussian kernel at truncate=4.0 —
    radius = int(4 sigma + 0.5), exp(-0.5 / sigma^2 * k^2) over k = -radius .. radius in fp64, divided by their sum.  sigma must
    give 1 <= radius <= 16 (about 0.125 <= sigma < 4.125): no tap is then zero or denormal as fp32."""
    import numpy as np
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float)):
        raise ValueError(f"sigma must be a number, got {sigma!r}")
    sigma = float(sigma)
    radius = int(4.0 * sigma + 0.5) if sigma == sigma and 0.0 < sigma < float("inf") else 0
    if not 1 <= radius <= L.BLUR_MAX_RADIUS:
        raise ValueError(f"sigma must give a radius int(4 sigma + 0.5) in 1..{L.BLUR_MAX_RADIUS} (about 0.125 <= sigma < 4.125), got {sigma!r}")
    k = np.arange(-radius, radius + 1)
    p = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    p = p / p.sum()
    return radius, p[radius:].copy()


def gauss_taps_device(sigma, device):
    """(radius, the taps of `gauss_taps(sigma)` rounded to fp32 on `device`): uploaded once and cached per (sigma, device)."""
    key = (float(sigma), torch.device(device))
    hit = _blur_taps.get(key)
    if hit is None:
        radius, taps = gauss_taps(sigma)
        hit = _blur_taps[key] = (radius, torch.from_numpy(taps).to(torch.float32).to(key[1]))
    return hit


def blur_edge(edge):
    if edge not in BLUR_EDGES:
        raise ValueError(f"edge must be one of {BLUR_EDGES}, got {edge!r}")
    return edge


def pixel_blur(x, out=None, *, sigma=None, taps=None, edge="reflect"):
    """A separable symmetric filter along W, then along H, of every plane of x (see mil_pixel_blur): fp32, contiguous, at least
    2 dimensions, the leading ones being the planes — a stack [T,3,H,W], a map [T,H,W], one plane [H,W].  Exactly one of
    `sigma` (the Gaussian of `gauss_taps`) and `taps` (w[0..radius], radius + 1 finite numbers, rounded to fp32: the centre tap
    and one half of any symmetric filter) is given.  edge: "reflect" (the edge sample not repeated; radius <= min(H, W) - 1),
    "replicate" or "wrap".  out: None (a fresh tensor) or the caller's, which may not overlap x: the filter is never in place.
    Returns out."""
    blur_edge(edge)
    if (sigma is None) == (taps is None):
        raise ValueError("exactly one of sigma and taps must be given")
    if not isinstance(x, torch.Tensor) or x.dim() < 2:
        raise ValueError(f"x must be an fp32 tensor [..., H, W], got {tuple(getattr(x, 'shape', ()))}")
    h, w = x.shape[-2], x.shape[-1]
    if h < 1 or w < 1:
        raise ValueError(f"x: planes of {h}x{w}")
    # what can be decided without a device comes first
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"x must be a contiguous fp32 tensor, got {x.dtype}, strides {tuple(x.stride())}")
    if sigma is not None:
        radius, vals = gauss_taps(sigma)
    else:
        try:
            vals = [float(v) for v in taps]
        except (TypeError, ValueError):
            raise ValueError(f"taps must be a sequence of numbers w[0..radius], got {taps!r}") from None
        radius = len(vals) - 1
        if not 1 <= radius <= L.BLUR_MAX_RADIUS or any(v != v or v in (float("inf"), float("-inf")) for v in vals):
            raise ValueError(f"taps must be radius + 1 finite numbers with 1 <= radius <= {L.BLUR_MAX_RADIUS}, got {taps!r}")
    if edge == "reflect" and radius > min(h, w) - 1:
        raise ValueError(f"edge 'reflect' needs radius <= min(H, W) - 1, got radius {radius} for planes of {h}x{w}")
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(x.shape) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous fp32 tensor like x {tuple(x.shape)}, got {tuple(getattr(out, 'shape', ()))} "
                             f"{getattr(out, 'dtype', None)}")
        if _overlap(out, x):
            raise ValueError("out overlaps x: the filter is never in place")
    _need(x, x.shape, torch.float32, "x")
    _need(out, x.shape, torch.float32, "out")
    if out is None:
        out = torch.empty_like(x)
    planes = x.numel() // (h * w)
    if planes == 0:
        return out
    tdev = gauss_taps_device(sigma, x.device)[1] if sigma is not None else torch.tensor(vals, dtype=torch.float64).to(torch.float32).to(x.device)
    _launch("mil_pixel_blur", ("pixel_blur", planes, h, w, radius, edge), x.data_ptr(), out.data_ptr(), tdev.data_ptr(), planes, h, w, radius,
            BLUR_EDGES.index(edge), L.stream_ptr())
    return out


BLUR_U8_MAX_SIGMA = 8.0                            # the largest sigma whose box radius is <= MIL_BLUR_U8_MAX_BOX


def _box_params(sigma):
    """(r, ww, fw) of one axis of `mil_gaussian_blur_u8` for a sigma in [0, 8]: Pillow's fp32 arithmetic (include/mil_hip.h), every
    operation rounded to fp32, sqrt and floor taken in double."""
    import math
    import numpy as np
    f32 = np.float32
    radius = f32(sigma)
    sigma2 = f32(f32(radius * radius) / f32(3))
    big = f32(math.sqrt(12.0 * float(sigma2) + 1.0))
    l = f32(math.floor((float(big) - 1.0) / 2.0))
    a = f32(f32(f32(f32(2) * l) + f32(1)) * f32(f32(l * f32(l + f32(1))) - f32(f32(3) * sigma2)))
    a = f32(a / f32(f32(6) * f32(sigma2 - f32(f32(l + f32(1)) * f32(l + f32(1))))))
    fr = f32(l + a)
    r = int(fr)
    ww = int(f32(f32(16777216) / f32(f32(fr * f32(2)) + f32(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def _sigma_column(sigma, name):
    """float64 [n] on the host from a number or a 1-D sequence / tensor of sigmas, each finite and in [0, 8]."""
    if isinstance(sigma, bool) or isinstance(sigma, str):
        raise ValueError(f"{name} must be a number or a 1-D sequence of numbers, got {sigma!r}")
    try:
        s = torch.as_tensor(sigma).detach().cpu()
        if s.dtype == torch.bool or s.is_complex():
            raise TypeError
        s = s.to(torch.float64)
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be a number or a 1-D sequence of numbers, got {sigma!r}") from None
    if s.dim() > 1:
        raise ValueError(f"{name} must be a number or a 1-D sequence of numbers, got shape {tuple(s.shape)}")
    s = s.reshape(-1)
    if s.numel() and (not bool(torch.isfinite(s).all()) or float(s.min()) < 0.0 or float(s.max()) > BLUR_U8_MAX_SIGMA):
        raise ValueError(f"{name} must be finite and lie in [0, {BLUR_U8_MAX_SIGMA:g}] (box radius <= {L.BLUR_U8_MAX_BOX})")
    return s


def box_blur_params(sigma_x, sigma_y=None):
    """int32 [n,6] on the host, the rows (r_x, ww_x, fw_x, r_y, ww_y, fw_y) `mil_gaussian_blur_u8` takes, from the sigmas of
    `PIL.ImageFilter.GaussianBlur`: a number or n of them per axis (sigma_y None: sigma_x on both axes; a single number beside n
    is repeated).  sigma 0 on an axis gives (0, 2^24, 0), the identity.  A sigma that is negative, not finite or above 8 raises
    ValueError."""
    sx = _sigma_column(sigma_x, "sigma_x")
    sy = sx if sigma_y is None else _sigma_column(sigma_y, "sigma_y")
    if sx.numel() != sy.numel():
        if sx.numel() == 1:
            sx = sx.expand(sy.numel())
        elif sy.numel() == 1:
            sy = sy.expand(sx.numel())
        else:
            raise ValueError(f"sigma_x holds {sx.numel()} values, sigma_y {sy.numel()}")
    cache = {}
    rows = []
    for a, b in zip(sx.tolist(), sy.tolist()):
        for v in (a, b):
            if v not in cache:
                cache[v] = _box_params(v)
        rows.append(cache[a] + cache[b])
    return torch.tensor(rows, dtype=torch.int32).reshape(-1, 6)


def checked_box_params(params, n):
    """`params` as a contiguous int32 [n,6] HOST tensor, every row inside the kernel's contract: 0 <= r <= 7, ww >= 0, fw >= 0 and
    (2 r + 1) ww + 2 fw <= 2^24 per axis — the check `mil_gaussian_blur_u8` leaves to its caller."""
    if not isinstance(params, torch.Tensor) or params.is_floating_point() or params.dtype == torch.bool or params.is_complex():
        raise ValueError(f"params must be an integer tensor [{n},6], got {getattr(params, 'dtype', type(params).__name__)}")
    if tuple(params.shape) != (n, 6):
        raise ValueError(f"params must be an integer tensor [{n},6], got {tuple(params.shape)}")
    p = params.detach().cpu().to(torch.int64)
    for axis in (0, 3):
        r, ww, fw = p[:, axis], p[:, axis + 1], p[:, axis + 2]
        if n and (int(r.min()) < 0 or int(r.max()) > L.BLUR_U8_MAX_BOX):
            raise ValueError(f"params: a box radius outside 0..{L.BLUR_U8_MAX_BOX}")
        if n and (int(ww.min()) < 0 or int(fw.min()) < 0 or int(((2 * r + 1) * ww + 2 * fw).max()) > 1 << 24):
            raise ValueError("params: weights must be >= 0 with (2 r + 1) ww + 2 fw <= 2^24")
    return p.to(torch.int32).contiguous()


def gaussian_blur_u8(u8, params, planes_per_item, out=None):
    """Pillow's Gaussian blur of every plane of u8 (see mil_gaussian_blur_u8): uint8, contiguous, at least 2 dimensions, the
    leading ones being the planes — a stack [T,3,H,W] with planes_per_item 3, maps [T,H,W] with 1.  params: int32 [n,6] from
    `box_blur_params` (on the host or on the device; its host copy is range-checked here), n = planes / planes_per_item.  out:
    None (a fresh tensor) or the caller's, which may not overlap u8: the blur is never in place.  Returns out."""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() < 2:
        raise ValueError(f"u8 must be a uint8 tensor [..., H, W], got {getattr(u8, 'dtype', type(u8).__name__)} "
                         f"{tuple(getattr(u8, 'shape', ()))}")
    h, w = u8.shape[-2], u8.shape[-1]
    if h < 1 or w < 1:
        raise ValueError(f"u8: planes of {h}x{w}")
    if h * w > 2 ** 31 - 1 - 4096:
        raise ValueError(f"u8: planes of {h} x {w} pixels are beyond 32-bit indexing")
    if not u8.is_contiguous():
        raise ValueError(f"u8 must be contiguous, got strides {tuple(u8.stride())}")
    if isinstance(planes_per_item, bool) or not isinstance(planes_per_item, int) or planes_per_item < 1:
        raise ValueError(f"planes_per_item must be a positive integer, got {planes_per_item!r}")
    planes = u8.numel() // (h * w)
    if planes % planes_per_item:
        raise ValueError(f"{planes} planes are no multiple of planes_per_item = {planes_per_item}")
    p = checked_box_params(params, planes // planes_per_item)
    if out is not None:
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(u8.shape) or out.dtype != torch.uint8 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor like u8 {tuple(u8.shape)}, got {tuple(getattr(out, 'shape', ()))} "
                             f"{getattr(out, 'dtype', None)}")
        if _overlap(out, u8):
            raise ValueError("out overlaps u8: the blur is never in place")
    if not u8.is_cuda:
        raise RuntimeError("the uint8 Gaussian blur runs on an AMD GPU only (no CPU fallback)")
    _need(out, u8.shape, torch.uint8, "out")
    if out is None:
        out = torch.empty_like(u8)
    if planes == 0:
        return out
    if (-(-h // 64)) * (-(-w // 64)) * planes > 2 ** 31 - 1:
        raise ValueError(f"u8: {planes} planes of {h} x {w} pixels are more than 2^31 - 1 blocks of 64 x 64")
    pd = p.to(u8.device)
    _launch("mil_gaussian_blur_u8", ("gaussian_blur_u8", planes, planes_per_item, h, w), u8.data_ptr(), out.data_ptr(), pd.data_ptr(), planes,
            planes_per_item, h, w, L.stream_ptr())
    return out


def momentum_scalars(lr, momentum, weight_decay):
    """(lr, weight_decay, momentum) of `pixel_momentum_step`, checked."""
    lr, mo, wd = float(lr), float(momentum), float(weight_decay)
    if lr != lr or not wd >= 0.0 or not 0.0 <= mo < 1.0:
        raise ValueError(f"lr must be a number, weight_decay >= 0 and momentum in [0, 1), got {lr}, {wd} and {mo}")
    return lr, wd, mo


def pixel_momentum_step(x, g, buf, *, lr, momentum=0.9, weight_decay=0.0, project="none", u8_out=None):
    """One step of `torch.optim.SGD` with momentum (no dampening, no Nesterov) on the images x [T,3,H,W] fp32, in place and in
    one pass (see mil_pixel_momentum_step): buf <- momentum buf + (g + weight_decay x); x <- x - lr buf.  buf: an fp32 tensor
    like x, updated in place; zeros give torch's first step.  project, u8_out: `pixel_step`'s.  Returns x."""
    if project not in PIXEL_PROJECTIONS:
        raise ValueError(f"project must be one of {PIXEL_PROJECTIONS}, got {project!r}")
    lr, wd, mo = momentum_scalars(lr, momentum, weight_decay)
    _pixel_stack(x, "x")
    if not isinstance(g, torch.Tensor) or not isinstance(buf, torch.Tensor):
        raise ValueError("g and buf must be fp32 tensors like x")
    return _pixel_step_tail("mil_pixel_momentum_step", ("pixel_momentum_step", x.numel()), x, g, (("buf", buf),), u8_out, project,
                            PIXEL_PROJECTIONS.index(project), lr, wd, mo)


QUANTILE_GROUPS = ("tile", "bag")
RENDER_MODES =("grayscale", "colour", "pos_neg")     # mil_attr_render's mode 0, 1, 2
MapStats = collections.namedtuple("MapStats", "stats p group")
MapStats.__doc__ = """What `map_quantile` returns: stats [G,4] fp32 = (min, max, s[lo], s[hi]) and p [G] fp64 per group (G = T for
group "tile", 1 for "bag"), on the device."""


def _attr_tensor(x, name, ranks=(3, 4)):
    """(T, channels, H, W) of an fp32 attribution tensor: a gradient [T,3,H,W] or a map [T,H,W]."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be an fp32 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() not in ranks or (x.dim() == 4 and x.shape[1] != 3):
        want = " or ".join({3: "[T,H,W]", 4: "[T,3,H,W]"}[r] for r in sorted(ranks, reverse=True))
        raise ValueError(f"{name} must be fp32 {want}, got {tuple(x.shape)}")
    t, h, w = x.shape[0], x.shape[-2], x.shape[-1]
    if t < 1 or h < 1 or w < 1:
        raise ValueError(f"{name}: an empty bag (or empty tiles) has nothing to rank or render, got {tuple(x.shape)}")
    return t, (3 if x.dim() == 4 else 1), h, w


def _check_stats(st, x, t):
    if not isinstance(st, MapStats) or st.group not in QUANTILE_GROUPS:
        raise ValueError("stats: what ops.map_quantile returned")
    g = t if st.group == "tile" else 1
    if tuple(st.stats.shape) != (g, 4) or tuple(st.p.shape) != (g,):
        raise ValueError(f"stats of {st.stats.shape[0]} groups for {g} (group {st.group!r}, {t} tiles)")
    _need(x, x.shape, torch.float32, "x")
    _need(st.stats, (g, 4), torch.float32, "stats.stats")
    _need(st.p, (g,), torch.float64, "stats.p")
    if st.stats.device != x.device:
        raise ValueError("stats and the tensor they are applied to are on different devices")


def map_quantile(x, q=99.0, group="tile", *, raw=False):
    """Per-group order statistics of an attribution tensor (see mil_map_quantile) as `MapStats`: the minimum, the maximum, the
    two order statistics that bracket the q-th percentile and the percentile itself in fp64, bit for bit
    `np.percentile(values.astype(np.float64), q)`.  x: a gradient [T,3,H,W] (ranked: (|g0| + |g1|) + |g2|, or with raw=True
    every element of the gradient as it is) or a map [T,H,W]; group "tile" or "bag".  No host synchronisation."""
    q = float(q)
    if not (0.0 < q <= 100.0):
        raise ValueError(f"q must be in (0, 100], got {q}")
    if group not in QUANTILE_GROUPS:
        raise ValueError(f"group must be one of {QUANTILE_GROUPS}, got {group!r}")
    t, c, h, w = _attr_tensor(x, "x")
    _need(x, x.shape, torch.float32, "x")
    if raw and c == 3:
        c, h = 1, 3 * h
    bag = group == "bag"
    groups = 1 if bag else t
    need = ctypes.c_size_t(0)
    L.check(L.lib().mil_map_quantile_workspace(ctypes.byref(need), t, int(bag)), "mil_map_quantile_workspace")
    ws = torch.empty(need.value // 4, dtype=torch.int32, device=x.device)
    stats = torch.empty((groups, 4), dtype=torch.float32, device=x.device)
    p = torch.empty((groups,), dtype=torch.float64, device=x.device)
    _launch("mil_map_quantile", ("map_quantile", t, c, h, w, q, bag), x.data_ptr(), t, c, h, w, q, int(bag), ws.data_ptr(), need.value,
            stats.data_ptr(), p.data_ptr(), L.stream_ptr())
    return MapStats(stats, p, group)


def attr_render(x, stats, mode="grayscale"):
    """An attribution tensor and its `MapStats` to the toolkit's bytes (see mil_attr_render): "grayscale" — a gradient [T,3,H,W]
    or a map [T,H,W] to uint8 [T,H,W], clipped between the group's minimum and its percentile; "colour" — a gradient to uint8
    [T,H,W,3], min-max over the group; "pos_neg" — (positive, negative) saliency, two uint8 [T,H,W,3].  The statistics of
    "colour" and "pos_neg" are those of `map_quantile(x, 100, group, raw=True)`."""
    if mode not in RENDER_MODES:
        raise ValueError(f"mode must be one of {RENDER_MODES}, got {mode!r}")
    t, c, h, w = _attr_tensor(x, "x", ranks=(3, 4) if mode == "grayscale" else (4,))
    _check_stats(stats, x, t)
    dev = x.device
    shape = (t, h, w) if mode == "grayscale" else (t, h, w, 3)
    out0 = torch.empty(shape, dtype=torch.uint8, device=dev)
    out1 = torch.empty(shape, dtype=torch.uint8, device=dev) if mode == "pos_neg" else None
    _launch("mil_attr_render", ("attr_render", t, c, h, w, mode), x.data_ptr(), t, c, h, w, RENDER_MODES.index(mode),
            int(stats.group == "bag"), stats.stats.data_ptr(), stats.p.data_ptr(), out0.data_ptr(), L.ptr(out1), L.stream_ptr())
    return (out0, out1) if mode == "pos_neg" else out0


PROJECT_MODES = ("concentrations", "ratio")         # mil_od_project_u8's mode 0, 1
_od_tables = {}                                     # device -> the 511 fp32 values on it
_elastic_tables = {}                                # (size, cells, device) -> (idx, w) of `elastic_tables` on it


def od_tables_host():
    """The 511 fp32 values of the stain kernels' byte contract as numpy: L[v] = -ln((v + 1) / 256) for v = 0..255, then
    TH[k] = -ln((k + 0.5) / 256) for k = 1..255 — `math.log` in fp64, rounded once to fp32."""
    import math
    import numpy as np
    vals = [-math.log((v + 1) / 256.0) for v in range(256)] + [-math.log((k + 0.5) / 256.0) for k in range(1, 256)]
    return np.asarray(vals, dtype=np.float64).astype(np.float32)


def od_tables(device):
    """`od_tables_host()` on `device`: uploaded once and cached per device (as `U8Tiles.decode_table` is)."""
    dev = torch.device(device)
    tab = _od_tables.get(dev)
    if tab is None:
        tab = _od_tables[dev] = torch.from_numpy(od_tables_host()).to(dev)
    return tab


def _u8_stack(u8, name="tiles"):
    """(T, H, W) of a uint8 planar stack [T,3,H,W] on the GPU (what `U8Tiles.u8` is; a contiguous view at any byte offset)."""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[1] != 3:
        raise ValueError(f"{name} must be a uint8 tensor [T,3,H,W], got {getattr(u8, 'dtype', type(u8).__name__)} "
                         f"{tuple(getattr(u8, 'shape', ()))}")
    t, _, h, w = u8.shape
    if h < 1 or w < 1:
        raise ValueError(f"{name}: empty tiles {tuple(u8.shape)}")
    if h * w > 2 ** 31 - 1 - 4096:
        raise ValueError(f"{name}: tiles of {h} x {w} pixels are beyond 32-bit indexing")
    _need(u8, u8.shape, torch.uint8, name)
    return t, h, w


def _beta(beta):
    beta = float(beta)
    if beta != beta:
        raise ValueError("beta must be a number")
    return beta


def stain_affine(u8, affine):
    """The OD-space affine map of `mil_stain_affine_u8` on the uint8 stack u8 [T,3,H,W], in place: affine fp32 [T,12] (per tile)
    or [1,12] (one map for the stack), rows A[i,0..2], b[i]; on the host or on u8's device.  A non-finite entry is refused.
    Returns u8."""
    t, h, w = _u8_stack(u8)
    if not isinstance(affine, torch.Tensor) or affine.dtype != torch.float32 or affine.dim() != 2 or affine.shape[1] != 12 \
            or affine.shape[0] not in (1, t):
        raise ValueError(f"affine must be fp32 [{t},12] or [1,12], got {getattr(affine, 'dtype', type(affine).__name__)} "
                         f"{tuple(getattr(affine, 'shape', ()))}")
    if not bool(torch.isfinite(affine).all()):
        raise ValueError("affine holds a non-finite entry")
    if t == 0:
        return u8
    shared = int(affine.shape[0] == 1)
    affine = affine.to(u8.device).contiguous()
    _launch("mil_stain_affine_u8", ("stain_affine", t, h, w, shared), u8.data_ptr(), affine.data_ptr(), od_tables(u8.device).data_ptr(),
            t, h, w, shared, L.stream_ptr())
    return u8


def od_moments(u8, beta=0.15, group="tile"):
    """Tissue statistics in OD space (see mil_od_moments_u8): fp64 [G,10] on the device = the count of tissue pixels (all three
    of L[r], L[g], L[b] >= beta), sum od_c (r, g, b) and sum od_c od_d (rr, rg, rb, gg, gb, bb) per group — G = T for group
    "tile", 1 for "bag".  Fixed summation tree: two calls give the same bits.  No host synchronisation."""
    if group not in QUANTILE_GROUPS:
        raise ValueError(f"group must be one of {QUANTILE_GROUPS}, got {group!r}")
    beta = _beta(beta)
    t, h, w = _u8_stack(u8)
    bag = group == "bag"
    out = torch.empty((1 if bag else t, 10), dtype=torch.float64, device=u8.device)
    ws = torch.empty((max(t, 1) * L.OD_SLICES, 10), dtype=torch.float64, device=u8.device)
    _launch("mil_od_moments_u8", ("od_moments", t, h, w, bag), u8.data_ptr(), od_tables(u8.device).data_ptr(), t, h, w, beta, int(bag),
            ws.data_ptr(), ws.numel() * 8, out.data_ptr(), L.stream_ptr())
    return out


def _snmf_lam(lam):
    lam = float(lam)
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"lam must be finite and >= 0, got {lam}")
    return lam


def snmf_dictionary(W, name="W"):
    """`W` (a tensor, an array, nested lists) as a contiguous fp64 [3,2] host tensor; ValueError for another shape or a
    non-finite entry."""
    try:
        W = torch.as_tensor(W).detach().to("cpu", torch.float64).contiguous()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must hold 3 x 2 finite numbers") from None
    if tuple(W.shape) != (3, 2) or not bool(torch.isfinite(W).all()):
        raise ValueError(f"{name} must hold 3 x 2 finite numbers, got {tuple(W.shape)}")
    return W


def snmf_coder(W, lam):
    """The nine fp32 values the coder of the sparse factorisation takes (see mil_od_snmf_sums_u8), on the host: W row-major
    rounded to fp32, c = W_0 . W_1 and d = 1 / (1 - c c) formed in fp64 in the header's order and rounded once (d = 0 for
    collinear columns), lam."""
    w = [float(v) for v in snmf_dictionary(W).reshape(6)]
    c = (w[0] * w[1] + w[2] * w[3]) + w[4] * w[5]
    e = 1.0 - c * c
    d = 1.0 / e if e > 0.0 else 0.0
    return torch.tensor(w + [c, d, _snmf_lam(lam)], dtype=torch.float64).to(torch.float32)


def od_snmf_sums(u8, W, lam=0.1, beta=0.15):
    """One coding pass of the sparse non-negative factorisation (see mil_od_snmf_sums_u8): every tissue pixel's code (h0, h1)
    for the dictionary W [3,2] and the penalty lam, and fp64 [12] on the device = count, sum h0 h0, h0 h1, h1 h1, sum v_c h_j
    (r0, r1, g0, g1, b0, b1), sum h0, sum h1.  Fixed summation tree: two calls give the same bits.  No host synchronisation."""
    beta = _beta(beta)
    t, h, w = _u8_stack(u8)
    coder = snmf_coder(W, lam).to(u8.device)
    if t == 0:                                                           # no tile: twelve zeros, no launch
        return torch.zeros((L.SNMF_TERMS,), dtype=torch.float64, device=u8.device)
    out = torch.empty((L.SNMF_TERMS,), dtype=torch.float64, device=u8.device)
    ws = torch.empty((max(t, 1) * L.OD_SLICES, L.SNMF_TERMS), dtype=torch.float64, device=u8.device)
    _launch("mil_od_snmf_sums_u8", ("od_snmf_sums", t, h, w), u8.data_ptr(), od_tables(u8.device).data_ptr(), coder.data_ptr(), t, h, w,
            beta, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), L.stream_ptr())
    return out


def od_snmf_fit(u8, W0, lam=0.1, iters=64, beta=0.15):
    """`iters` iterations of the sparse non-negative factorisation from the dictionary W0 [3,2] (see mil_od_snmf_fit_u8): one
    `od_moments` launch for sum |v|^2, then ONE C call that enqueues every coding pass and every update; the fp64 dictionary
    stays on the device in between.  Returns (W fp64 [3,2], history fp64 [iters,2] = (objective of the W coded with, largest
    |change of an entry of W|) per iteration, count fp64 [1] of the tissue pixels), all on the device, with no host
    synchronisation."""
    beta, lam, iters = _beta(beta), _snmf_lam(lam), int(iters)
    if iters < 1:
        raise ValueError(f"iters must be at least 1, got {iters}")
    W0 = snmf_dictionary(W0, "W0")
    t, h, w = _u8_stack(u8)
    dev = u8.device
    W = W0.to(dev)
    if t == 0:                                                           # no tile: W as it came, a history of zeros, no launch
        return W, torch.zeros((iters, 2), dtype=torch.float64, device=dev), torch.zeros((1,), dtype=torch.float64, device=dev)
    moments = od_moments(u8, beta, "bag")
    history = torch.empty((iters, 2), dtype=torch.float64, device=dev)
    ws = torch.empty((t * L.OD_SLICES * L.SNMF_TERMS + L.SNMF_EXTRA,), dtype=torch.float64, device=dev)
    _launch("mil_od_snmf_fit_u8", ("od_snmf_fit", t, h, w, iters), u8.data_ptr(), od_tables(dev).data_ptr(), W.data_ptr(),
            moments.data_ptr(), t, h, w, lam, iters, beta, ws.data_ptr(), ws.numel() * 8, history.data_ptr(), L.stream_ptr())
    return W, history, moments[0, :1]


def od_project(u8, P, mode="concentrations", beta=0.15, lam=None):
    """Two projections of every pixel's OD as maps (see mil_od_project_u8): P [2,3] (rounded to fp32).  Returns (maps, valid):
    mode "concentrations" — maps fp32 [2,T,H,W] = (p_0, p_1) at tissue pixels; mode "ratio" — maps fp32 [T,H,W] = p_1 / p_0 at
    tissue pixels with p_0 > 0; +inf everywhere else.  valid int32 [T]: the pixels of each tile that got a value.  Mode
    "sparse" (mil_od_code_u8) takes the dictionary W [3,2] in place of P and the penalty `lam`: maps fp32 [2,T,H,W] = the
    non-negative lasso code (h0, h1) of every tissue pixel, the arithmetic of `od_snmf_sums`."""
    if mode == "sparse":
        beta = _beta(beta)
        if lam is None:
            raise ValueError("mode 'sparse' needs lam")
        coder = snmf_coder(P, lam)
        t, h, w = _u8_stack(u8)
        maps = torch.empty((2, t, h, w), dtype=torch.float32, device=u8.device)
        valid = torch.empty((t,), dtype=torch.int32, device=u8.device)
        if t:
            coder = coder.to(u8.device)
            _launch("mil_od_code_u8", ("od_project", t, h, w, mode), u8.data_ptr(), od_tables(u8.device).data_ptr(), coder.data_ptr(),
                    t, h, w, beta, maps.data_ptr(), valid.data_ptr(), L.stream_ptr())
        return maps, valid
    if lam is not None:
        raise ValueError("lam belongs to mode 'sparse'")
    if mode not in PROJECT_MODES:
        raise ValueError(f"mode must be one of {PROJECT_MODES + ('sparse',)}, got {mode!r}")
    beta = _beta(beta)
    t, h, w = _u8_stack(u8)
    P = torch.as_tensor(P).detach().to("cpu", torch.float64)
    if tuple(P.shape) != (2, 3) or not bool(torch.isfinite(P).all()):
        raise ValueError(f"P must hold 2 x 3 finite numbers, got {tuple(P.shape)}")
    dev = u8.device
    maps = torch.empty((2, t, h, w) if mode == "concentrations" else (t, h, w), dtype=torch.float32, device=dev)
    valid = torch.empty((t,), dtype=torch.int32, device=dev)
    if t == 0:
        return maps, valid
    pd = P.to(torch.float32).to(dev)
    _launch("mil_od_project_u8", ("od_project", t, h, w, mode), u8.data_ptr(), od_tables(dev).data_ptr(), pd.data_ptr(), t, h, w,
            PROJECT_MODES.index(mode), beta, maps.data_ptr(), valid.data_ptr(), L.stream_ptr())
    return maps, valid


def affine_matrices(matrices, n, name="matrices"):
    """`matrices` (a tensor, an array or nested lists) as a contiguous float64 [n,6] host tensor; ValueError for another shape,
    a non-numeric dtype or a non-finite entry.  Needs no device."""
    try:
        m = torch.as_tensor(matrices).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be float64 [{n},6]") from None
    if m.dtype == torch.bool or m.is_complex() or tuple(m.shape) != (n, 6):
        raise ValueError(f"{name} must be float64 [{n},6], got {tuple(m.shape)} {m.dtype}")
    m = m.to(torch.float64).contiguous()
    if not bool(torch.isfinite(m).all()):
        raise ValueError(f"{name} holds a non-finite entry")
    return m


def affine_fill(fill):
    """A fill colour, one byte or three, as mil_affine_u8 takes it: r | g << 8 | b << 16.  ValueError otherwise."""
    import numbers
    vals = (fill,) * 3 if isinstance(fill, numbers.Integral) and not isinstance(fill, bool) else fill
    if not isinstance(vals, (tuple, list)) or len(vals) != 3 or any(
            not isinstance(v, numbers.Integral) or isinstance(v, bool) or not 0 <= v <= 255 for v in vals):
        raise ValueError(f"fill must be a byte or three bytes, got {fill!r}")
    return int(vals[0]) | int(vals[1]) << 8 | int(vals[2]) << 16


def _affine_hw(out_hw, h, w):
    if out_hw is None:
        return h, w
    try:
        oh, ow = (int(v) for v in out_hw)
    except (TypeError, ValueError):
        raise ValueError(f"out_hw must be (height, width), got {out_hw!r}") from None
    if oh < 1 or ow < 1 or oh * ow > 2 ** 31 - 1 - 4096:
        raise ValueError(f"out_hw must be positive and within 32-bit indexing, got {out_hw!r}")
    return oh, ow


def affine_u8(src, matrices, fill=0, out_hw=None):
    """Pillow's bilinear `Image.transform(size, Image.AFFINE, m, Image.BILINEAR, fillcolor=fill)` of every tile of the planar
    uint8 stack src [n,3,h,w], bit for bit (see mil_affine_u8): matrices float64 [n,6], the map from output pixel centres to
    input coordinates, one per tile; fill a byte or three; out_hw the output size (default: the input's).  Returns a NEW uint8
    [n,3,oh,ow] on src's device.  Every refusal comes before the launch."""
    n, h, w = _u8_stack(src, "src")
    oh, ow = _affine_hw(out_hw, h, w)
    m = affine_matrices(matrices, n)
    fill = affine_fill(fill)
    out = torch.empty((n, 3, oh, ow), dtype=torch.uint8, device=src.device)
    if n:
        md = m.to(src.device)
        _launch("mil_affine_u8", ("affine_u8", n, h, w, oh, ow), src.data_ptr(), 3 * h * w, w, 1, h * w, w, h, out.data_ptr(), 1, oh * ow,
                ow, oh, md.data_ptr(), fill, n, L.stream_ptr())
    return out


def affine_windows_u8(source, coords, matrices, fill=0, size=None):
    """The window form of `affine_u8`, interleaved: source a uint8 slide [H,W,3] with coords (int [n,2] of (row, col), the
    origins of S x S windows, S = `size`) or an ROI stack [n,S,S,3] with coords=None (`size` is then not needed); matrices
    float64 [n,6] in WINDOW coordinates.  Returns a NEW uint8 [n,S,S,3].  For a slide every window reads the slide itself — the host adds the window's
    origin to the matrix (a2 + col, a5 + row: one double addition each), W, H and the clips are the slide's — so a rotated
    window shows the tissue that lies beside it, and only what lies outside the slide becomes `fill`:
    `Image.fromarray(slide).transform((S, S), Image.AFFINE, m', Image.BILINEAR, fillcolor=fill)`.  For a stack the source of a
    window is the window, and what lies outside it is `fill`.  Every refusal comes before the launch."""
    from .preprocess import source_windows
    if coords is None:
        if not isinstance(source, torch.Tensor) or source.dim() != 4:
            raise ValueError("without coords the source is an ROI stack [n,S,S,3]")
        s = int(source.shape[1]) if size is None else int(size)
        src, off, _ = source_windows(source, None, s)
        origins = None
    else:
        if size is None or int(size) < 1:
            raise ValueError("windows of a slide need their size (a positive number of pixels)")
        s = int(size)
        src, off, _ = source_windows(source, coords, s)
        width = int(src.shape[1])
        origins = torch.stack([off // 3 % width, off // 3 // width], dim=1).to(torch.float64)          # (col, row)
    n = int(off.numel())
    m = affine_matrices(matrices, n)
    fill = affine_fill(fill)
    if not src.is_cuda:
        raise RuntimeError("the affine transform runs on an AMD GPU only (no CPU fallback)")
    out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=src.device)
    if n == 0:
        return out
    if origins is None:
        tile, width, height = 3 * s * s, s, s
    else:
        m = m.clone()
        m[:, 2] += origins[:, 0]
        m[:, 5] += origins[:, 1]
        tile, height = 0, int(src.shape[0])
    md = m.to(src.device)
    _launch("mil_affine_u8", ("affine_windows_u8", n, s, tile == 0), src.data_ptr(), tile, 3 * width, 3, 1, width, height,
            out.data_ptr(), 3, 1, s, s, md.data_ptr(), fill, n, L.stream_ptr())
    return out


def elastic_tables(size, cells):
    """The table pair of the uniform cubic B-spline for an axis of `size` output pixels divided into `cells` cells (see
    mil_affine_elastic_u8): (idx int32 [size], w float64 [size,4]) on the host, in numpy doubles, one rounded operation at a time:

        u = ((x + 0.5) * cells) / size ;  i = min(floor(u), cells-1) ;  t = u - i ;  s = 1 - t ;  t2 = t*t ;  t3 = t2*t
        w0 = ((s*s)*s)/6      w1 = ((3*t3 - 6*t2) + 4)/6      w2 = (((-3*t3 + 3*t2) + 3*t) + 1)/6      w3 = t3/6

    Output position x reads lattice entries idx[x] .. idx[x] + 3.  ValueError unless size and cells are positive integers."""
    import numbers
    import numpy as np
    if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and v >= 1 for v in (size, cells)):
        raise ValueError(f"size and cells must be positive integers, got {size!r}, {cells!r}")
    x = np.arange(int(size), dtype=np.float64)
    u = ((x + 0.5) * np.float64(cells)) / np.float64(size)
    i = np.minimum(np.floor(u), np.float64(int(cells) - 1))
    t = u - i
    s = 1.0 - t
    t2 = t * t
    t3 = t2 * t
    w = np.stack([((s * s) * s) / 6.0, ((3.0 * t3 - 6.0 * t2) + 4.0) / 6.0, (((-3.0 * t3 + 3.0 * t2) + 3.0 * t) + 1.0) / 6.0, t3 / 6.0],
                 axis=1)
    return torch.from_numpy(i.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(w))


def _elastic_tables_on(size, cells, device):
    """`elastic_tables(size, cells)`, checked on the host (indices in [0, cells-1], finite weights: what keeps the kernel inside
    the lattice) and uploaded; a few recent ones are kept per device."""
    key = (int(size), int(cells), torch.device(device))
    tab = _elastic_tables.get(key)
    if tab is None:
        idx, w = elastic_tables(int(size), int(cells))
        if int(idx.min()) < 0 or int(idx.max()) > int(cells) - 1 or not bool(torch.isfinite(w).all()):
            raise ValueError(f"elastic tables for {size} pixels in {cells} cells are out of range")
        if len(_elastic_tables) >= 16:
            _elastic_tables.clear()
        tab = _elastic_tables[key] = (idx.to(key[2]), w.to(key[2]))
    return tab


def elastic_lattice(ctrl, n, name="ctrl"):
    """`ctrl` (a tensor, an array or nested lists) as a contiguous float64 [n,2,gy+3,gx+3] host tensor, gy, gx >= 1: one control
    lattice per tile, component 0 the x and component 1 the y displacement in source pixels; ValueError for another shape, a
    non-numeric dtype or a non-finite entry.  Needs no device."""
    try:
        c = torch.as_tensor(ctrl).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"{name} must be float64 [{n},2,gy+3,gx+3]") from None
    if c.dtype == torch.bool or c.is_complex() or c.dim() != 4 or c.shape[0] != n or c.shape[1] != 2 or c.shape[2] < 4 or c.shape[3] < 4:
        raise ValueError(f"{name} must be float64 [{n},2,gy+3,gx+3] with gy, gx >= 1, got {tuple(c.shape)} {c.dtype}")
    c = c.to(torch.float64).contiguous()
    if not bool(torch.isfinite(c).all()):
        raise ValueError(f"{name} holds a non-finite entry")
    return c


def _identity_matrices(n):
    return torch.tensor([[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], dtype=torch.float64).repeat(n, 1)


def _launch_elastic(label, src, strides, width, height, out, dst_strides, ow, oh, m, fill, c):
    """One mil_affine_elastic_u8 call for the host matrices m [n,6] and lattices c [n,2,ly,lx] (both checked)."""
    dev = src.device
    ly, lx = int(c.shape[2]), int(c.shape[3])
    iy, wy = _elastic_tables_on(oh, ly - 3, dev)
    ix, wx = _elastic_tables_on(ow, lx - 3, dev)
    md, cd = m.to(dev), c.to(dev)
    _launch("mil_affine_elastic_u8", label, src.data_ptr(), *strides, width, height, out.data_ptr(), *dst_strides, ow, oh,
            md.data_ptr(), fill, int(m.shape[0]), cd.data_ptr(), ly, lx, iy.data_ptr(), wy.data_ptr(), ix.data_ptr(), wx.data_ptr(),
            L.stream_ptr())


def elastic_u8(src, matrices, ctrl, fill=0, out_hw=None):
    """`affine_u8` with an elastic deformation fused into the same resampling (see mil_affine_elastic_u8): src planar uint8
    [n,3,h,w], matrices float64 [n,6] (None: the identity), ctrl float64 [n,2,gy+3,gx+3], one control lattice per tile in source
    pixels over gy x gx cells of the OUTPUT; fill, out_hw as in `affine_u8`.  Returns a NEW uint8 [n,3,oh,ow].  A lattice of zeros
    gives `affine_u8`'s bytes.  Every refusal comes before the launch."""
    n, h, w = _u8_stack(src, "src")
    oh, ow = _affine_hw(out_hw, h, w)
    m = _identity_matrices(n) if matrices is None else affine_matrices(matrices, n)
    c = elastic_lattice(ctrl, n)
    fill = affine_fill(fill)
    out = torch.empty((n, 3, oh, ow), dtype=torch.uint8, device=src.device)
    if n:
        _launch_elastic(("elastic_u8", n, h, w, oh, ow), src, (3 * h * w, w, 1, h * w), w, h, out, (1, oh * ow), ow, oh, m, fill, c)
    return out


def elastic_windows_u8(source, coords, matrices, ctrl, fill=0, size=None):
    """The window form of `elastic_u8`, interleaved, as `affine_windows_u8` is of `affine_u8`: source a uint8 slide [H,W,3] with
    coords (int [n,2] of (row, col)) and `size`, or an ROI stack [n,S,S,3] with coords=None; matrices float64 [n,6] in WINDOW
    coordinates (None: the identity); ctrl float64 [n,2,gy+3,gx+3] in source pixels.  Returns a NEW uint8 [n,S,S,3].  For a
    slide the window's origin is added to a2 and a5 on the host and every window reads the slide itself: a deformed window shows
    the tissue that lies beside it, and only what lies outside the slide becomes `fill`.  Every refusal comes before the launch."""
    from .preprocess import source_windows
    if coords is None:
        if not isinstance(source, torch.Tensor) or source.dim() != 4:
            raise ValueError("without coords the source is an ROI stack [n,S,S,3]")
        s = int(source.shape[1]) if size is None else int(size)
        src, off, _ = source_windows(source, None, s)
        origins = None
    else:
        if size is None or int(size) < 1:
            raise ValueError("windows of a slide need their size (a positive number of pixels)")
        s = int(size)
        src, off, _ = source_windows(source, coords, s)
        width = int(src.shape[1])
        origins = torch.stack([off // 3 % width, off // 3 // width], dim=1).to(torch.float64)          # (col, row)
    n = int(off.numel())
    m = _identity_matrices(n) if matrices is None else affine_matrices(matrices, n)
    c = elastic_lattice(ctrl, n)
    fill = affine_fill(fill)
    if not src.is_cuda:
        raise RuntimeError("the elastic deformation runs on an AMD GPU only (no CPU fallback)")
    out = torch.empty((n, s, s, 3), dtype=torch.uint8, device=src.device)
    if n == 0:
        return out
    if origins is None:
        tile, width, height = 3 * s * s, s, s
    else:
        m = m.clone()
        m[:, 2] += origins[:, 0]
        m[:, 5] += origins[:, 1]
        tile, height = 0, int(src.shape[0])
    _launch_elastic(("elastic_windows_u8", n, s, tile == 0), src, (tile, 3 * width, 3, 1), width, height, out, (3, 1), s, s, m, fill, c)
    return out


def cam_overlay(tiles, map_u8, lut, alpha_byte):
    """(heat, on_image), two uint8 [T,H,W,3] (see mil_cam_overlay): the colour table `lut` (uint8 [256,3]) looked up at the map
    bytes `map_u8` [T,H,W], and Pillow's alpha_composite of that with alpha `alpha_byte` (0..255) over the `U8Tiles`."""
    from .preprocess import U8Tiles
    if not isinstance(tiles, U8Tiles):
        raise ValueError(f"tiles must be U8Tiles, got {type(tiles).__name__}")
    x = tiles.u8
    t, _, h, w = x.shape
    if not isinstance(map_u8, torch.Tensor) or map_u8.dtype != torch.uint8 or tuple(map_u8.shape) != (t, h, w):
        raise ValueError(f"map_u8 must be uint8 {(t, h, w)}, got {getattr(map_u8, 'dtype', None)} {tuple(getattr(map_u8, 'shape', ()))}")
    if not isinstance(lut, torch.Tensor) or lut.dtype != torch.uint8 or tuple(lut.shape) != (256, 3):
        raise ValueError("lut must be a uint8 [256,3] tensor")
    if int(alpha_byte) != alpha_byte or not 0 <= alpha_byte <= 255:
        raise ValueError(f"alpha_byte must be an integer in [0, 255], got {alpha_byte}")
    if t < 1 or h < 1 or w < 1:
        raise ValueError(f"an empty bag has nothing to draw on, got {tuple(x.shape)}")
    _need(x, x.shape, torch.uint8, "tiles")
    _need(map_u8, (t, h, w), torch.uint8, "map_u8")
    _need(lut, (256, 3), torch.uint8, "lut")
    heat = torch.empty((t, h, w, 3), dtype=torch.uint8, device=x.device)
    on_image = torch.empty((t, h, w, 3), dtype=torch.uint8, device=x.device)
    _launch("mil_cam_overlay", ("cam_overlay", t, h, w), x.data_ptr(), map_u8.data_ptr(), lut.data_ptr(), int(alpha_byte), t, h, w,
            heat.data_ptr(), on_image.data_ptr(), L.stream_ptr())
    return heat, on_image


def attr_mosaic(maps, out_pos, n, lut, alpha_byte, alpha_by_value=False, heat=None, on_tissue=None):
    """Per-tile maps resampled into the n x n blocks of thumbnail pixels at `out_pos` (int32 [T,2] of (row, col), on the device)
    of the caller's canvases `heat` and / or `on_tissue` (uint8 [Ht,Wt,3]; see mil_attr_mosaic): maps uint8 [T,Hm,Wm] are
    coloured through `lut` (uint8 [256,3]), maps uint8 [T,Hm,Wm,3] are the colours themselves (`lut` may be None).  `heat`
    receives the colours, `on_tissue` their alpha_composite with `alpha_byte` (0..255; with `alpha_by_value` scaled by the map's
    value, one-channel maps only) over what it holds.  Blocks must not overlap; the part of a block outside the canvas is not
    stored, pixels no block owns keep their bytes.  Returns (heat, on_tissue)."""
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.uint8 or maps.dim() not in (3, 4) or (maps.dim() == 4 and maps.shape[3] != 3):
        raise ValueError(f"maps must be uint8 [T,Hm,Wm] or [T,Hm,Wm,3], got {getattr(maps, 'dtype', type(maps).__name__)} "
                         f"{tuple(getattr(maps, 'shape', ()))}")
    t, hm, wm = (int(v) for v in maps.shape[:3])
    channels = 1 if maps.dim() == 3 else 3
    if hm < 1 or wm < 1:
        raise ValueError(f"empty maps {tuple(maps.shape)}")
    if int(n) != n or n < 1:
        raise ValueError(f"n must be a positive integer, got {n}")
    if int(alpha_byte) != alpha_byte or not 0 <= alpha_byte <= 255:
        raise ValueError(f"alpha_byte must be an integer in [0, 255], got {alpha_byte}")
    if alpha_by_value and channels == 3:
        raise ValueError("alpha_by_value needs one-channel maps: a colour picture has no value to scale the alpha by")
    if channels == 1 and lut is None:
        raise ValueError("one-channel maps need a uint8 [256,3] colour table")
    canvas = heat if heat is not None else on_tissue
    if canvas is None:
        raise ValueError("neither heat nor on_tissue: nothing to draw on")
    if not isinstance(canvas, torch.Tensor) or canvas.dim() != 3 or canvas.shape[2] != 3 or canvas.shape[0] < 1 or canvas.shape[1] < 1:
        raise ValueError(f"a canvas is uint8 [Ht,Wt,3], got {tuple(getattr(canvas, 'shape', ()))}")
    if not isinstance(out_pos, torch.Tensor):
        raise ValueError(f"out_pos must be an int32 [{t},2] tensor on the device, got {type(out_pos).__name__}")
    _need(maps, maps.shape, torch.uint8, "maps")
    _need(out_pos, (t, 2), torch.int32, "out_pos")
    _need(lut, (256, 3), torch.uint8, "lut")
    _need(heat, canvas.shape, torch.uint8, "heat")
    _need(on_tissue, canvas.shape, torch.uint8, "on_tissue")
    if any(x is not None and x.device != maps.device for x in (out_pos, lut, heat, on_tissue)):
        raise ValueError("maps, out_pos, lut and the canvases must be on one device")
    _launch("mil_attr_mosaic", ("attr_mosaic", t, hm, wm, channels, int(n)), maps.data_ptr(), channels, t, hm, wm, int(n), out_pos.data_ptr(),
            L.ptr(lut), int(alpha_byte), int(bool(alpha_by_value)), L.ptr(heat), L.ptr(on_tissue), int(canvas.shape[0]),
            int(canvas.shape[1]), L.stream_ptr())
    return heat, on_tissue


_RESAMPLE_TABLES = {}


def resample_tables(in_size, out_size, filt, device):
    """(ksize, bounds [out,2], kk [out,ksize]) of `mil_resample_coeffs`: int32 tensors on `device` (any device: the tables
    are made on the host), cached per (sizes, filter, device)."""
    key = (int(in_size), int(out_size), int(filt), torch.device(device))
    got = _RESAMPLE_TABLES.get(key)
    if got is None:
        ks = ctypes.c_int(0)
        L.check(L.lib().mil_resample_plan(key[0], key[1], key[2], ctypes.byref(ks)), "mil_resample_plan")
        bounds = torch.empty((key[1], 2), dtype=torch.int32)
        kk = torch.empty((key[1], ks.value), dtype=torch.int32)
        L.check(L.lib().mil_resample_coeffs(key[0], key[1], key[2], bounds.data_ptr(), kk.data_ptr()), "mil_resample_coeffs")
        got = _RESAMPLE_TABLES[key] = (ks.value, bounds.to(key[3]), kk.to(key[3]))
    return got


def grad_cam(act, grad, c, tile_hw, *, offset=1.0, value_range=None, want_raw=True, want_map=True):
    """Grad-CAM maps of n tiles (see mil_grad_cam): act, grad [n,h,w,cs] — a stage's output and the gradient of the class
    evidence with respect to it, bf16 or fp32, c real channels — -> (raw [n,h,w] fp32, out [n,H,W] uint8) for tiles of
    tile_hw = (H, W); None for the one not wanted.  value_range: a device fp32 tensor (lo, hi) that replaces every tile's own
    minimum and maximum in the normalisation.  The Lanczos tables are cached per (h, H, w, W, device)."""
    if act.dim() != 4 or act.shape != grad.shape or act.dtype != grad.dtype:
        raise ValueError(f"act and grad must be two [n,h,w,cs] tensors of one dtype, got {tuple(act.shape)} {act.dtype} and "
                         f"{tuple(grad.shape)} {grad.dtype}")
    if not (want_raw or want_map):
        raise ValueError("neither raw nor the map is wanted")
    n, h, w, cs = act.shape
    hh, ww = (int(v) for v in tile_hw)
    code = L.dt_code(act.dtype)
    _need(act, act.shape, act.dtype, "act")
    _need(grad, act.shape, act.dtype, "grad")
    if not 1 <= c <= cs or cs % 8:
        raise ValueError(f"{c} real channels of {cs} stored (a multiple of 8)")
    if h < 1 or w < 1 or hh < 1 or ww < 1:
        raise ValueError(f"maps of {h}x{w} for tiles of {hh}x{ww}")
    _need(value_range, (2,), torch.float32, "value_range")
    dev = act.device
    raw = torch.empty((n, h, w), dtype=torch.float32, device=dev) if want_raw else None
    out = yb = yk = xb = xk = None
    yks = xks = 0
    if want_map:
        out = torch.empty((n, hh, ww), dtype=torch.uint8, device=dev)
        yks, yb, yk = resample_tables(h, hh, L.FILTER_LANCZOS, dev)
        xks, xb, xk = resample_tables(w, ww, L.FILTER_LANCZOS, dev)
    _launch("mil_grad_cam", ("grad_cam", n, h, w, cs, hh, ww, want_map), act.data_ptr(), grad.data_ptr(), n, h, w, c, cs, code,
            float(offset), L.ptr(value_range), L.ptr(yb), L.ptr(yk), yks, L.ptr(xb), L.ptr(xk), xks, L.ptr(raw), L.ptr(out), hh, ww,
            L.stream_ptr())
    return raw, out


def avgpool_fc_fwd(x, wfc, c, bias=None):
    n, h, w, cp = x.shape
    nf = wfc.shape[0]
    _need(wfc, (nf, c), torch.float32, "fc.weight")
    _need(bias, (nf,), torch.float32, "fc.bias")
    pooled = torch.empty((n, c), dtype=torch.float32, device=x.device)
    feats = torch.empty((n, nf), dtype=torch.float32, device=x.device)
    L.check(L.lib().mil_avgpool_fc_fwd(x.data_ptr(), wfc.data_ptr(), L.ptr(bias), pooled.data_ptr(), feats.data_ptr(), n,
                                       h * w, cp, c, nf, L.dt_code(x.dtype), L.stream_ptr()), "mil_avgpool_fc_fwd")
    return pooled, feats


def avgpool_fc_bwd_data(dfeats, wfc, pooled, act, masked=True, slope=LEAK, rule=0):
    """The data half of `avgpool_fc_bwd` alone: dz [n,h,w,cp] = (dfeats @ wfc) / (h w), times lrelu'(act) when `masked` — the
    gradient of the pre-activation map the backward chain carries; masked=False: the gradient of `act` itself, the stage's
    OUTPUT, which is what Grad-CAM reads.  No parameter gradient is computed.  rule=1 (mil_avgpool_fc_bwd_data_guided): the
    guided gate in place of lrelu' — the gradient where act and the gradient are positive, else +0."""
    rule = _check_rule(rule)
    if rule == 1 and not masked:
        raise ValueError("rule=1 replaces the LeakyReLU factor: it does not go with masked=False")
    n, h, w, cp = act.shape
    nf, c = wfc.shape
    _need(dfeats, (n, nf), torch.float32, "dfeats")
    _need(wfc, (nf, c), torch.float32, "fc.weight")
    _need(act, act.shape, act.dtype, "act")
    dz = torch.empty_like(act)
    _need(pooled, (n, c), torch.float32, "pooled")        # (read by the weight-gradient half only, which a null dwfc leaves out)
    if rule == 1:
        L.check(L.lib().mil_avgpool_fc_bwd_data_guided(dfeats.data_ptr(), wfc.data_ptr(), act.data_ptr(), dz.data_ptr(), n, h * w, cp,
                                                       c, nf, L.dt_code(act.dtype), L.stream_ptr()), "mil_avgpool_fc_bwd_data_guided")
        return dz
    L.check(L.lib().mil_avgpool_fc_bwd(dfeats.data_ptr(), wfc.data_ptr(), pooled.data_ptr(), act.data_ptr() if masked else None,
                                       dz.data_ptr(), None, None, n, h * w, cp, c, nf, 0, slope, L.dt_code(act.dtype),
                                       L.stream_ptr()), "mil_avgpool_fc_bwd")
    return dz


def avgpool_fc_bwd(dfeats, wfc, pooled, act, c, slope=LEAK, out=None, want_bias=False, out_bias=None):
    """`out` / `out_bias` given: the parameter gradients are ADDED to them (one accumulate flag for both, so with `want_bias` they
    come together or not at all); otherwise fresh tensors are returned."""
    if want_bias and (out is None) != (out_bias is None):
        raise ValueError("avgpool_fc_bwd: with want_bias, give both out and out_bias (accumulate into both) or neither")
    n, h, w, cp = act.shape
    nf = wfc.shape[0]
    _need(dfeats, (n, nf), torch.float32, "dfeats")
    dz = torch.empty_like(act)
    dwfc = torch.empty((nf, c), dtype=torch.float32, device=act.device) if out is None else out
    _need(dwfc, (nf, c), torch.float32, "dwfc")
    dbias = None
    if want_bias:
        dbias = torch.empty(nf, dtype=torch.float32, device=act.device) if out_bias is None else out_bias
    L.check(L.lib().mil_avgpool_fc_bwd(dfeats.data_ptr(), wfc.data_ptr(), pooled.data_ptr(), act.data_ptr(), dz.data_ptr(),
                                       None, None, n, h * w, cp, c, nf, 0, slope, L.dt_code(act.dtype), L.stream_ptr()),
            "mil_avgpool_fc_bwd")
    need = ctypes.c_size_t(0)
    L.check(L.lib().mil_fc_wgrad_workspace(ctypes.byref(need), n, c, nf), "mil_fc_wgrad_workspace")
    ws = torch.empty((need.value + 3) // 4, dtype=torch.float32, device=act.device)
    L.check(L.lib().mil_fc_wgrad(dfeats.data_ptr(), pooled.data_ptr(), dwfc.data_ptr(), L.ptr(dbias), ws.data_ptr(),
                                 ws.numel() * 4, n, c, nf, 0 if out is None else 1, L.stream_ptr()), "mil_fc_wgrad")
    if want_bias:
        return dz, dwfc, dbias
    return dz, dwfc


# ---- wide (multiples of 64 channels) layers: the alt_resnet configuration -----------------------------------
def wide_pack_weights(w, mode, dtype):
    """fp32 [Cout,Cin,k,k] -> the channel-blocked fragment order of mil_wide_conv; dtype torch.bfloat16, torch.float32 (exact, or
    split under `f32_mma`) or L.BF16X3."""
    if dtype == L.BF16X3:                 # the split path's filters: fp32-sized fragments [hi | lo], packed under MIL_DT_F32S
        with L.f32_mma(L.MIL_DT_F32S):
            return wide_pack_weights(w, mode, torch.float32)
    w = w.detach().contiguous()
    cout, cin, ks, _ = w.shape
    elems = ctypes.c_size_t(0)
    L.check(L.lib().mil_wide_packed_elems(ctypes.byref(elems), cout, cin, ks, mode), "mil_wide_packed_elems")
    packed = torch.empty(elems.value, dtype=dtype, device=w.device)
    L.check(L.lib().mil_wide_pack_weights(w.data_ptr(), packed.data_ptr(), cout, cin, ks, mode, L.dt_code(dtype, mma=True),
                                          L.stream_ptr()), "mil_wide_pack_weights")
    return packed


def wide_conv(x, wpack, cout, *, ks, stride, pad, out_hw=None, res=None, act=None, relu=False, zero_insert=False,
              slope=0.0, bias=None):
    n, h, w, cin = x.shape
    if zero_insert:
        ho, wo = out_hw
    else:
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    _need(res, y.shape, x.dtype, "res")
    _need(act, y.shape, x.dtype, "act")
    L.check(L.lib().mil_wide_conv(x.data_ptr(), wpack.data_ptr(), L.ptr(bias), L.ptr(res), L.ptr(act), y.data_ptr(), n, h, w,
                                  cin, ho, wo, cout, ks, 1 if zero_insert else stride, pad, 1 if zero_insert else 0,
                                  1 if relu else 0, slope, L.dt_code(x.dtype, mma=True), L.stream_ptr()), "mil_wide_conv")
    return y


def gconv_supported(cin_x, cout_x, ks, stride):
    """Whether the gather-GEMM kernel runs a conv that contracts `cin_x` channels into `cout_x` (bf16 only)."""
    return bool(L.lib().mil_gconv_supported(cin_x, cout_x, ks, stride))


def gconv_pack_weights(w, mode):
    w = w.detach().contiguous()
    cout, cin, ks, _ = w.shape
    elems = ctypes.c_size_t(0)
    L.check(L.lib().mil_gconv_packed_elems(ctypes.byref(elems), cout, cin, ks, mode), "mil_gconv_packed_elems")
    packed = torch.empty(elems.value, dtype=torch.bfloat16, device=w.device)
    L.check(L.lib().mil_gconv_pack_weights(w.data_ptr(), packed.data_ptr(), cout, cin, ks, mode, L.stream_ptr()),
            "mil_gconv_pack_weights")
    return packed


def gconv(x, wpack, cout, *, ks, stride, pad, transposed=False, out_hw=None, res=None, act=None, relu=False, slope=0.0):
    """y = mask(relu?(conv(x) + res?)) (transposed: the conv's data gradient, x = dz, out_hw = the conv's input extent)."""
    n, h, w, cin = x.shape
    if transposed:
        ho, wo = out_hw if out_hw is not None else (h * stride, w * stride)
    else:
        ho, wo = (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1
    y = torch.empty((n, ho, wo, cout), dtype=x.dtype, device=x.device)
    _need(res, y.shape, x.dtype, "res")
    _need(act, y.shape, x.dtype, "act")
    L.check(L.lib().mil_gconv(x.data_ptr(), wpack.data_ptr(), L.ptr(res), L.ptr(act), y.data_ptr(), n, h, w, cin, ho, wo, cout,
                              ks, stride, pad, 1 if transposed else 0, 1 if relu else 0, slope, L.stream_ptr()), "mil_gconv")
    return y


def wide_wgrad(x, dz, cin, cout, *, ks, stride, pad, workspace=None, out=None):
    n, h, w, _ = x.shape
    _, ho, wo, _ = dz.shape
    _need(x, (n, h, w, cin), x.dtype, "x")
    _need(dz, (n, ho, wo, cout), x.dtype, "dz")
    need = ctypes.c_size_t(0)
    L.check(L.lib().mil_wide_wgrad_workspace(ctypes.byref(need), n, h, w, cin, ho, wo, cout, ks, stride, pad,
                                             L.dt_code(x.dtype, mma=True)), "mil_wide_wgrad_workspace")
    workspace = workspace_for(workspace, need.value, x.device)
    (dw,), accumulate = _grad_out(None if out is None else (out,), (((cout, cin, ks, ks), "dw"),), x.device)
    _launch("mil_wide_wgrad", None, x.data_ptr(), dz.data_ptr(), dw.data_ptr(), workspace.data_ptr(),
            workspace.numel() * workspace.element_size(), n, h, w, cin, ho, wo, cout, ks, stride, pad,
            accumulate, L.dt_code(x.dtype, mma=True), L.stream_ptr())
    return dw, workspace
