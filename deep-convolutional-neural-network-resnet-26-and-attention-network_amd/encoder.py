"""ResNet-26 tile encoder on the HIP kernels: forward and hand-written backward.

Mirrors the reference's `ResNet` (gbm/model.py:14-61) built from `BasicResBlock`
(nnBlocks.py:157-189) with layers [3,3,3,3] and widths 20/40/60/80 — same module tree, same
state-dict keys — but `forward` never calls a torch conv: it sequences the C-ABI kernels of
include/mil_hip.h (NHWC, channel-padded, fp32 or bf16 operands) and a custom autograd Function
provides the backward (dgrad / wgrad / pooling backward) from saved NHWC activations.
"""
import contextlib
import ctypes
import functools

import torch
from torch import nn

from . import _lib as L
from . import hooks
from . import ops

STAGE_WIDTHS = (20, 40, 60, 80)        # gbm/model.py:27-30
WEIGHT_EPOCH = [0]                     # bumped by optimizers that update weights through raw kernels (FlatAdam)
STEM_WIDTH = 20                        # gbm/model.py:20


def invalidate_packed_weights():
    """Call after changing conv weights in a way autograd's version counters do not see — `conv.weight.data.normal_()` (as the
    reference itself does, nnBlocks.py:375), EMA / clipping code writing through `.data`, raw-pointer updates: the encoders
    keep MFMA-fragment-order copies of every filter, re-packed only when a parameter's `_version`, its storage or this
    epoch changes.  (`FlatAdam.step` bumps the epoch itself; `load_state_dict` and in-place ops on the Parameter bump
    `_version`.)"""
    WEIGHT_EPOCH[0] += 1


class BasicResBlock(nn.Module):
    """Parameter container with the reference block's layout (nnBlocks.py:157-173): conv1 (3x3,
    stride s, bias), conv2 (3x3, bias), optional `downsample` = Sequential(1x1 stride-s conv, no bias).
    The arithmetic of nnBlocks.py:175-189 is executed by the fused HIP kernels in `encoder_forward`."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, base_width=64):
        super().__init__()
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=1, bias=True)
        self.relu = nn.LeakyReLU(ops.LEAK)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=1, padding=1, bias=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        raise RuntimeError("BasicResBlock is executed by the fused HIP encoder (ResNet.forward); "
                           "it has no stand-alone torch path")


class ResNet(nn.Module):
    """Tile encoder [T,3,H,W] fp32 -> [T,num_classes] fp32 (gbm/model.py:14-61)."""

    def __init__(self, block=BasicResBlock, layers=(3, 3, 3, 3), num_classes=80, zero_init_residual=False,
                 groups=1, width_per_group=64, compute_dtype=L.BF16X3):
        super().__init__()
        if block is not BasicResBlock or groups != 1 or width_per_group != 64:
            raise ValueError("the HIP encoder implements BasicResBlock with groups=1, base_width=64")
        self.inplanes = STEM_WIDTH
        self.conv1 = nn.Conv2d(3, STEM_WIDTH, kernel_size=7, stride=2, padding=3)
        self.relu = nn.LeakyReLU(ops.LEAK, inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for i, (width, depth) in enumerate(zip(STAGE_WIDTHS, layers)):
            setattr(self, f"layer{i + 1}", self._make_layer(width, depth, stride=1 if i == 0 else 2))
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(STAGE_WIDTHS[-1], num_classes, bias=False)
        self.compute_dtype = compute_dtype
        # separate weight-gradient launches on a side stream: no longer a win once the hot layers run fused backward
        # kernels (same throughput at 2048 tiles, slower for small bags) — available, off by default
        self.overlap_wgrad = False
        self.direct_grad = False        # accumulate parameter gradients straight into existing .grad tensors
        self.n_side_streams = 1
        self.fuse_backward = True
        self.fuse_stem_forward = True
        self.keep_s2d = False           # True: the fused stem forward also writes the bf16 space-to-depth copy of the input (bf16 mode)
        self.fuse_stage_entry = True
        self.fuse_block_forward = True
        # gradient tensors of the 20-channel stage (produced and consumed only by the fused backward kernels) at 20 channels
        # per pixel instead of the padded 24: 17 % fewer bytes on three of the four tensor passes of its fused backward
        self.dense_grads = True
        # the 28 slab reductions of a backward pass recorded and run as ONE launch (ops.ReduceBatch) instead of one ~10 us
        # launch behind every weight-gradient kernel
        self.batch_reductions = True
        self._reduce_batch = None
        self._pack_table = None
        self._pack_version = None
        self._stem_dgrad_pack = None    # (tag, fragments) of the stem's data-gradient filter: packed on first use (encoder_backward, want_dx)
        self._side = None
        # a `summary.ActivationSummary` while one is attached: handed the tensors the forward keeps anyway, after the last launch
        self.activation_summary = None

    def _make_layer(self, planes, blocks, stride=1):
        shortcut = None
        if stride != 1 or self.inplanes != planes:
            shortcut = nn.Sequential(nn.Conv2d(self.inplanes, planes, kernel_size=1, stride=stride, bias=False))
        seq = [BasicResBlock(self.inplanes, planes, stride, shortcut)]
        self.inplanes = planes
        seq += [BasicResBlock(planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*seq)

    # ---- execution ---------------------------------------------------------------------------
    def blocks(self):
        for i in range(4):
            for blk in getattr(self, f"layer{i + 1}"):
                yield blk

    def stages(self):
        """The four stages as (index of the stage's first block in `blocks()`, [its blocks])."""
        out, first = [], 0
        for i in range(4):
            blks = list(getattr(self, f"layer{i + 1}"))
            out.append((first, blks))
            first += len(blks)
        return out

    def encoder_params(self):
        """Flat, ordered parameter list handed to the autograd Function."""
        ps = [self.conv1.weight, self.conv1.bias]
        for blk in self.blocks():
            ps += [blk.conv1.weight, blk.conv1.bias, blk.conv2.weight, blk.conv2.bias]
            if blk.downsample is not None:
                ps.append(blk.downsample[0].weight)
        ps.append(self.fc.weight)
        return ps

    def _side_streams(self):
        if self._side is None:
            self._side = [torch.cuda.Stream() for _ in range(self.n_side_streams)]
        return self._side

    # ---- packed (MFMA fragment order) copies of every filter, refreshed by ONE launch -------------------
    def _pack_specs(self):
        """(key, weight, bias, mode) for every packed filter the forward and backward passes use."""
        specs = [("stem", self.conv1.weight, self.conv1.bias, L.PACK_STEM)]
        for bi, blk in enumerate(self.blocks()):
            for name, conv in (("c1", blk.conv1), ("c2", blk.conv2)):
                specs.append((f"b{bi}.{name}", conv.weight, conv.bias, L.PACK_FWD))
                specs.append((f"b{bi}.{name}", conv.weight, None, L.PACK_DGRAD))
            if blk.downsample is not None:
                specs.append((f"b{bi}.ds", blk.downsample[0].weight, None, L.PACK_FWD))
                specs.append((f"b{bi}.ds", blk.downsample[0].weight, None, L.PACK_DGRAD))
                if blk.stride == 2:       # conv1's and the projection's transposed convs in one parity-class filter
                    specs.append((f"b{bi}.c1", blk.conv1.weight, blk.downsample[0].weight, L.PACK_DGRAD_S2))
        return specs

    def refresh_packed(self, dtype):
        """Make the packed filters current: rebuild the job table if storage moved, re-run the single pack launch
        if any weight changed (parameter version counters, or WEIGHT_EPOCH bumped by FlatAdam.step)."""
        lib = L.lib()
        specs = self._pack_specs()
        ptr_tag = (dtype, L.dt_code(dtype, mma=True)) + tuple(w.data_ptr() for _k, w, _b, _m in specs) + tuple(0 if b is None else b.data_ptr() for _k, _w, b, _m in specs)
        if self._pack_table is None or self._pack_table[0] != ptr_tag:
            dev = self.conv1.weight.device
            rec = lib.mil_pack_job_bytes()
            host = (ctypes.c_char * (rec * len(specs)))()
            store = {}
            for i, (key, w, b, mode) in enumerate(specs):
                if w.dtype != torch.float32 or not w.is_cuda or not w.is_contiguous():
                    raise ValueError("conv weights must be contiguous CUDA fp32 tensors")
                cout, cin, ks, _ = w.shape
                elems = ctypes.c_size_t(0)
                L.check(lib.mil_packed_weight_elems(ctypes.byref(elems), cout, cin, ks, mode), "mil_packed_weight_elems")
                packed = torch.empty(elems.value, dtype=dtype, device=dev)
                n_out = cin if mode == L.PACK_DGRAD else cout
                bias_pad = torch.empty((ops.cpad(n_out) + 15) // 16 * 16, dtype=torch.float32, device=dev)
                L.check(lib.mil_pack_job_fill(ctypes.byref(host, i * rec), w.data_ptr(), L.ptr(b), packed.data_ptr(),
                                              bias_pad.data_ptr(), cout, cin, ks, mode, L.dt_code(dtype, mma=True)), "mil_pack_job_fill")
                store[(key, mode)] = (packed, bias_pad)
            table = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(dev)
            self._pack_table = (ptr_tag, table, store, len(specs))
            self._pack_version = None
        ver = (WEIGHT_EPOCH[0],) + tuple(w._version for _k, w, _b, _m in specs) + tuple(0 if b is None else b._version for _k, _w, b, _m in specs)
        if self._pack_version != ver:
            _tag, table, _store, njobs = self._pack_table
            L.check(lib.mil_pack_all(table.data_ptr(), njobs, L.stream_ptr()), "mil_pack_all")
            self._pack_version = ver

    def _packed(self, key, mode):
        return self._pack_table[2][(key, mode)]

    def stem_dgrad_packed(self, dtype):
        """MIL_PACK_STEM_DGRAD fragments of conv1.weight for the storage dtype `dtype` (inside `L.f32_mma`, as the encoder
        passes run).  Not part of the per-step pack table: only a backward that asks for the tiles' gradient needs them, so
        they are packed on first use and again when the weight's storage, its `_version` or WEIGHT_EPOCH changes — the same
        three signals `refresh_packed` watches (`invalidate_packed_weights` bumps the last)."""
        w = self.conv1.weight
        tag = (dtype, L.dt_code(dtype, mma=True), w.data_ptr(), w._version, WEIGHT_EPOCH[0])
        if self._stem_dgrad_pack is None or self._stem_dgrad_pack[0] != tag:
            self._stem_dgrad_pack = (tag, ops.pack_weights(w, None, L.PACK_STEM_DGRAD, dtype)[0])
        return self._stem_dgrad_pack[1]

    # ---- forward hooks on children (the reference's children are live modules: SURVEY.md §8b) ----------------
    def block_position(self, bi):
        """(stage index, index inside the stage, stage depth) of block `bi` of `blocks()`."""
        for li in range(4):
            depth = len(getattr(self, f"layer{li + 1}"))
            if bi < depth:
                return li, bi, depth
            bi -= depth
        raise IndexError(bi)

    def child_hooks(self):
        """The children that carry a forward (pre-)hook, or None: the un-hooked forward builds no views."""
        hk = [m for m in self.modules() if m is not self and hooks.hooked(m)]
        return hk or None

    def _fire_block_hooks(self, bi, blk, stage_in, xin, o1, out):
        """Hooks of block `bi`, of its LeakyReLU (called twice per block upstream, nnBlocks.py:180,187) and — after a
        stage's last block — of the stage's Sequential, with NCHW fp32 views of the saved activations."""
        cin, cout = blk.conv1.in_channels, blk.conv1.out_channels
        if hooks.hooked(blk.relu):
            v1 = hooks.nchw(o1, cout)
            hooks.fire(blk.relu, v1, v1)
            v2 = hooks.nchw(out, cout)
            hooks.fire(blk.relu, v2, v2)
        if hooks.hooked(blk):
            hooks.fire(blk, hooks.nchw(xin, cin), hooks.nchw(out, cout))
        li, j, depth = self.block_position(bi)
        if j == depth - 1:
            stage = getattr(self, f"layer{li + 1}")
            if hooks.hooked(stage):
                hooks.fire(stage, hooks.nchw(stage_in, stage[0].conv1.in_channels), hooks.nchw(out, cout))

    def forward(self, x):
        """x: fp32 [T,3,H,W] tiles (the reference's tensor), or `preprocess.S2dTiles` — the same tiles as the bf16
        space-to-depth tensor the stem kernels read (bf16 compute mode only) — or `preprocess.U8Tiles`, the same tiles as
        the uint8 images they are (every compute mode; a CPU handle is moved to the module's device as uint8)."""
        from .preprocess import S2dTiles, U8Tiles
        if isinstance(x, S2dTiles):
            x = x.xs
        elif isinstance(x, U8Tiles):
            x = x.u8.to(self.conv1.weight.device)
        return _EncoderFn.apply(self, x, *self.encoder_params())


def encoder_forward(net, x, dtype, upto=None):
    """Runs the kernels; returns (feats [T,80] fp32, saved-state dict for the backward).  upto = 1..4: the forward cut short behind
    stage `upto` — the stages above it, the average pool and the fc layer do not run, feats is None, `saved["blocks"]` holds the
    blocks that ran (bit for bit those of the full forward) and an attached `ActivationSummary` is not called."""
    if upto is not None and upto not in (1, 2, 3, 4):
        raise ValueError(f"upto must be None or 1..4, got {upto!r}")
    net.refresh_packed(dtype)
    x = x.contiguous()                  # the tensor the kernels read — and, without a kept s2d copy, the one the backward re-reads
    kind = ops.stem_feed_kind(x, dtype)
    hk = net.child_hooks()              # None unless a forward hook sits on a child module (then views are built for it)
    wp, bp = net._packed("stem", L.PACK_STEM)
    stem_hooked = hk is not None and hooks.any_hooked((net.conv1, net.relu, net.maxpool))
    split = L.is_split(dtype)           # bf16x3: no s2d form feeds its fused kernels
    # What the stem keeps for the backward: the one place it is decided.  xs: the space-to-depth tensor; x: the tiles.
    #   feed | keep_s2d set                                      | no keep_s2d          | saved for the backward
    #   f32  | split: an fp32 clone of the tiles.  Otherwise the | x is saved and its   | as left
    #        | fused forward writes xs (also written when        | version recorded     |
    #        | not fuse_backward)                                |                      |
    #   u8   | a clone of the bytes, in every mode               | the fused forward    | xs is rebuilt by stem_s2d_u8 only when fused,
    #        |                                                   | never writes xs      | not fuse_backward and not split; else x
    #   s2d  | n/a                                               | n/a                  | xs is the caller's tensor, always version-checked
    # Where the three-call chain runs (no fused kernel, a hooked stem) the xs it made is saved and x is not.  A recorded
    # version makes an in-place change between forward and backward raise instead of silently giving a wrong conv1 gradient.
    if net.keep_s2d and (kind == "u8" or (kind == "f32" and split)):
        x = x.clone()
    xs, pool, widx, stem_hw, stem = ops.stem_forward(
        kind, x, wp, bp, ops.cpad(STEM_WIDTH), dtype=dtype, allow_fused=net.fuse_stem_forward and not stem_hooked,
        keep_s2d=kind == "f32" and (net.keep_s2d or not net.fuse_backward) and not split)
    if xs is None and kind == "u8" and not net.fuse_backward and not split:
        xs = ops.stem_s2d_u8(x, dtype)
    if stem_hooked:                     # the hooked children see what the reference's would (NCHW fp32, 20 channels)
        if hooks.hooked(net.conv1):     # pre-activation output: one extra launch, only ever paid under a hook
            from .preprocess import U8Tiles
            pre = ops.conv(xs, wp, bp, ops.cpad(STEM_WIDTH), ks=4, stride=1, pad=2, lrelu=False)
            shown = x if kind == "f32" else U8Tiles(x).float() if kind == "u8" else hooks.s2d_to_nchw(xs)
            hooks.fire(net.conv1, shown, hooks.nchw(pre, STEM_WIDTH))
        stem_v = hooks.nchw(stem, STEM_WIDTH)
        hooks.fire(net.relu, stem_v, stem_v)            # in place upstream (gbm/model.py:25): input is the output
        hooks.fire(net.maxpool, stem_v, hooks.nchw(pool, STEM_WIDTH))
    saved = {"kind": kind, "xs": xs, "x": x if xs is None else None, "x_src": x if (xs is None or kind == "s2d") else None,
             "x_version": x._version, "stem_hw": stem_hw, "widx": widx, "blocks": [],
             "tile_hw": (2 * x.shape[1], 2 * x.shape[2]) if kind == "s2d" else tuple(x.shape[2:])}
    return _encoder_forward_body(net, pool, saved, dtype, hk, upto)


class _Forward:
    """One forward pass behind the stem: keeps each block's (xin, o1, out) for the backward and shows them to the hooks."""

    def __init__(self, net, saved, hk):
        self.net, self.saved, self.hk = net, saved, hk
        self.stage_in = None                # input of the stage being run: what a hook on the stage's Sequential is shown

    def begin(self, blk):
        if self.hk is not None:             # the tensors inside a block never exist outside a kernel
            hooks.refuse(blk, ["conv1", "conv2"] + (["downsample", "downsample.0"] if blk.downsample is not None else []))

    def keep(self, bi, blk, xin, o1, out):
        self.saved["blocks"].append((xin, o1, out))
        if self.hk is not None:
            self.net._fire_block_hooks(bi, blk, self.stage_in, xin, o1, out)
        return out


def _identity_block_forward(fw, bi, blk, t):
    """A block with the identity shortcut: out = lrelu(conv2(lrelu(conv1(t))) + t)."""
    net = fw.net
    fw.begin(blk)
    w1, b1 = net._packed(f"b{bi}.c1", L.PACK_FWD)
    w2, b2 = net._packed(f"b{bi}.c2", L.PACK_FWD)
    both = None
    if net.fuse_block_forward:              # whole block in one pass (24/40 channels)
        both = ops.conv_block_fwd(t, w1, b1, w2, b2)
        if both is None:                    # 80 channels on 8x8 maps: both convs on the LDS-resident images
            both = ops.conv_pair(t, w1, b1, w2, b2, lreluA=True, resB=t, lreluB=True)
    if both is None:
        cp = ops.cpad(blk.conv1.out_channels)
        o1 = ops.conv(t, w1, b1, cp, ks=3, stride=1, pad=1, lrelu=True)
        both = o1, ops.conv(o1, w2, b2, cp, ks=3, stride=1, pad=1, res=t, lrelu=True)
    return fw.keep(bi, blk, t, *both)


def _entry_block_forward(fw, first, stage, t):
    """The first block of a stage that opens with a projection shortcut and, where the stage-wide chain runs, the identity
    blocks behind it.  Returns (output, how many of the stage's blocks have run)."""
    net, blk = fw.net, stage[0]
    fw.begin(blk)
    s, cp = blk.stride, ops.cpad(blk.conv1.out_channels)
    w1, b1 = net._packed(f"b{first}.c1", L.PACK_FWD)
    w2, b2 = net._packed(f"b{first}.c2", L.PACK_FWD)
    wd, _ = net._packed(f"b{first}.ds", L.PACK_FWD)
    pair = None
    if s == 2 and net.fuse_stage_entry:     # both stride-2 convs in one pass over the block input
        pair = ops.conv_s2_entry(t, w1, b1, wd, cp)
    if pair is None:
        pair = ops.conv(t, w1, b1, cp, ks=3, stride=s, pad=1, lrelu=True), ops.conv(t, wd, None, cp, ks=1, stride=s, pad=0)
    o1, short = pair
    # A stage whose maps fit the pixel-resident kernel (whole images in LDS: the 80-channel stage at 256x256 tiles): this
    # entry block's conv2 and BOTH convs of every identity block behind it as ONE chain launch
    rest = stage[1:]
    if rest and net.fuse_block_forward and len(rest) <= 2 and all(b.stride == 1 and b.downsample is None for b in rest):
        convs = [dict(w=w2, bias=b2, res=short, lrelu=True)]
        for j in range(len(rest)):
            wa, ba = net._packed(f"b{first + 1 + j}.c1", L.PACK_FWD)
            wb, bb = net._packed(f"b{first + 1 + j}.c2", L.PACK_FWD)
            convs += [dict(w=wa, bias=ba, lrelu=True), dict(w=wb, bias=bb, res=2 * j, lrelu=True)]
        outs = ops.conv_chain(o1, convs)
        if outs is not None:
            fw.keep(first, blk, t, o1, outs[0])
            for j, b in enumerate(rest):
                fw.begin(b)
                fw.keep(first + 1 + j, b, outs[2 * j], outs[2 * j + 1], outs[2 * j + 2])
            return outs[-1], len(stage)
    out = ops.conv(o1, w2, b2, cp, ks=3, stride=1, pad=1, res=short, lrelu=True)
    return fw.keep(first, blk, t, o1, out), 1


def _encoder_forward_body(net, pool, saved, dtype, hk, upto=None):
    """Everything behind the stem: the residual stages, the average pool and the fc layer — or, with `upto`, the first `upto`
    stages alone (stages are the cut points: the stage-wide forward chains never span two)."""
    fw = _Forward(net, saved, hk)
    t = pool
    for first, stage in net.stages()[:upto]:
        fw.stage_in = t
        ran = 0
        if stage[0].downsample is not None:
            t, ran = _entry_block_forward(fw, first, stage, t)
        for j in range(ran, len(stage)):
            t = _identity_block_forward(fw, first + j, stage[j], t)
    if upto is not None:
        return None, saved
    pooled, feats = ops.avgpool_fc_fwd(t, net.fc.weight.detach(), STAGE_WIDTHS[-1])
    saved["pooled"] = pooled
    if hk is not None:
        if hooks.hooked(net.avgpool):
            hooks.fire(net.avgpool, hooks.nchw(t, STAGE_WIDTHS[-1]), pooled.view(pooled.shape[0], -1, 1, 1))
        if hooks.hooked(net.fc):
            hooks.fire(net.fc, pooled, feats)
    watcher = getattr(net, "activation_summary", None)      # (getattr: a module object pickled before the attribute existed)
    if watcher is not None:             # statistics of what the kernels stored, read where it lies (summary.py)
        watcher.observe(pool, saved["blocks"], pooled, feats)
    return feats, saved


_MAIN_STREAM = contextlib.nullcontext()


def _is_dense(t, c):
    return t.shape[-1] == c and ops.cpad(c) != c


class _Backward:
    """One backward pass: what its steps read (the net, the saved activations, the storage dtype), the gradients they leave
    in `grads` under (block, 1 | 2 | 0 for conv1 | conv2 | the projection) or ("stem", 0), and the workspace policy."""

    def __init__(self, net, saved, dtype, allow_direct, want_dx, want_wgrad=True, rule=None):
        self.net, self.saved, self.dtype, self.want_dx = net, saved, dtype, want_dx
        # None: the LeakyReLU derivative at every activation.  "guided": guided backpropagation (encoder_pixel_gradient) — the
        # walk of `_guided_block_backward`, data gradients only
        self.rule = rule
        # False: a walk that is after the data gradient alone (encoder_pixel_gradient).  The stand-alone weight-gradient launches
        # are skipped; the one-pass kernels that make the data gradient still run, and what they leave in `grads` is dropped
        self.want_wgrad = want_wgrad
        self.blocks = list(net.blocks())
        self.grads = {}
        # in-place accumulation into the parameters' .grad: opt-in (dist.FlatParams sets direct_grad; plain loss.backward() only),
        # and only when autograd wants a gradient for every encoder parameter (allow_direct, from ctx.needs_input_grad)
        self.direct = net.direct_grad and allow_direct and all(p.grad is not None and p.grad.is_contiguous() for p in net.encoder_params())
        # Weight gradients only consume (x, dz) and nothing downstream waits for them, so under overlap_wgrad they run on
        # side streams (round-robin, one slab workspace each) beside the sequential dgrad chain: the small late-layer
        # and stride-2 launches do not fill 256 CUs alone.
        self.main = torch.cuda.current_stream()
        self.sides = net._side_streams()
        self.rr = 0                         # weight-gradient launches put on side streams so far
        self.ws = {}                        # the re-used buffers of a pass without deferred reductions
        self.batch = None
        self.bare_input = None              # encoder_stage_gradient: the entry block whose input gradient is left un-masked

    def reductions(self, device):
        """Context of the pass's weight-gradient launches.  With `batch_reductions` the producers record their slab reductions
        in the net's ReduceBatch instead of launching them; leaving the context runs them all in one launch."""
        net = self.net
        if not net.batch_reductions or net.overlap_wgrad:
            return contextlib.nullcontext()
        if net._reduce_batch is None or net._reduce_batch.device != device:
            net._reduce_batch = ops.ReduceBatch(device)
        self.batch = net._reduce_batch
        return self.batch

    def out(self, *params):
        """Destination gradient tensors (the parameters' own .grad) when accumulating in place, else None."""
        return tuple(None if p is None else p.grad for p in params) if self.direct else None

    def workspace(self, kind, key, need, launch, *args, **kw):
        """`launch(*args, workspace=<slab buffer>, **kw)` for call site (kind, key); kind "w": a weight-gradient kernel, "f": a
        fused backward, "p": the stage-entry pair.  The one place the three workspace policies are told apart.  need=None:
        the wrapper sizes the buffer itself and returns the one it used as its last result, which is kept here."""
        batch, side = self.batch, None
        if batch is not None:                # deferred reduction: a slab buffer of its own, alive until the batched launch
            store, slot = batch.ws, (kind, key)
        elif kind == "w" and self.net.overlap_wgrad:
            slot = self.rr % len(self.sides)
            self.rr += 1
            store, side = self.ws, self.sides[slot]
            side.wait_stream(self.main)                      # dz was produced on the main stream
        else:                                # one buffer, re-used; the fused backward's apart from the weight-gradient kernels'
            store, slot = self.ws, "f" if kind == "f" else "w"
        with (_MAIN_STREAM if side is None else torch.cuda.stream(side)):
            if need is None:
                buf = store.get(slot)
            elif batch is not None:
                buf = batch.workspace(slot, need)
            else:                            # (launches on one stream are serialised: one buffer per stream)
                buf = store[slot] = ops.workspace_for(store.get(slot), need, args[0].device)
            res = launch(*args, workspace=buf, **kw)
        if need is None and res is not None:
            store[slot] = res[-1]            # under deferred reductions: kept until the batched reduction has run
        if side is not None:
            args[0].record_stream(side)
            args[1].record_stream(side)
        return res

    def stem_allocator(self):
        """`ws_alloc` for ops.stem_backward, which sizes its slabs itself: under deferred reductions they must outlive the
        call and come from the ReduceBatch (key ("s", 0)); otherwise None, and the wrapper allocates."""
        return None if self.batch is None else functools.partial(self.batch.workspace, ("s", 0))

    def wgrad(self, conv, xin, dzz, key, stem=False):
        """dW and db of `conv` from its input and the gradient of its output, left in grads[key].  stem: conv1, which runs as
        a 4x4 stride-1 conv on the space-to-depth tensor.  Not launched without `want_wgrad`."""
        if not self.want_wgrad:
            return
        n, h, w, _ = xin.shape
        _, ho, wo, _ = dzz.shape
        cin, cout, bias = conv.in_channels, conv.out_channels, conv.bias
        ks, stride, pad = (4, 1, 2) if stem else (conv.kernel_size[0], conv.stride[0], conv.padding[0])
        need = ops.wgrad_workspace_bytes(n, h, w, cin, ho, wo, cout, ks, stride, pad, stem, xin.dtype)
        self.grads[key] = self.workspace("w", key, need, ops.conv_wgrad, xin, dzz, cin, cout, ks=ks, stride=stride, pad=pad, stem=stem,
                                         want_bias=bias is not None, out=self.out(conv.weight, bias))

    def fused(self, conv, dzz, xin, addend, mask, key):
        """The one-pass backward of block key[0]'s conv1 or conv2 (key[1]), both 3x3 stride-1: returns the data gradient
        and leaves dW, db in grads[key] — or returns None where there is no such kernel for the shape, or none is wanted."""
        if not self.net.fuse_backward:
            return None
        n, h, w, _ = dzz.shape
        cin, cout = conv.in_channels, conv.out_channels
        dense = _is_dense(dzz, cout)
        need = ops.bwd_fused_workspace_bytes(n, h, w, cout, cin, 3, 1, dzz.dtype, dense)
        if need is None:
            if dense:
                raise RuntimeError("dense gradient layout chosen for a shape without a fused backward kernel")
            return None
        wd, _ = self.net._packed(f"b{key[0]}.c{key[1]}", L.PACK_DGRAD)
        res = self.workspace("f", key, need, ops.conv_bwd_fused, dzz, wd, xin, cin, cout, addend=addend, mask=mask, out=self.out(conv.weight, conv.bias))
        if res is None:
            return None
        self.grads[key] = res[1:]
        return res[0]

    def join(self):
        if self.net.overlap_wgrad:          # the main stream waits for the weight gradients on the side streams
            for side in self.sides:
                self.main.wait_stream(side)


def _conv2_backward(bw, bi, dz):
    """conv2 of block `bi`: leaves dW2/db2, and returns dz1 where the one-pass kernel made it on the way — else None, and
    the caller picks the data-gradient kernel."""
    conv = bw.blocks[bi].conv2
    o1 = bw.saved["blocks"][bi][1]
    dz1 = bw.fused(conv, dz, o1, None, True, (bi, 2))
    if dz1 is None:
        if _is_dense(dz, conv.out_channels):
            raise RuntimeError("dense gradient layout without the fused backward")
        bw.wgrad(conv, o1, dz, (bi, 2))
    return dz1


def _identity_block_backward(bw, bi, dz):
    """Backward of identity-shortcut block `bi`: returns the gradient of its input."""
    net, conv = bw.net, bw.blocks[bi].conv1
    xin, o1, _out = bw.saved["blocks"][bi]
    cp = ops.cpad(conv.out_channels)
    w2d, _ = net._packed(f"b{bi}.c2", L.PACK_DGRAD)
    w1d, _ = net._packed(f"b{bi}.c1", L.PACK_DGRAD)
    mask = xin if bi > 0 else None          # block 0 reads the max-pool output (no activation in between)
    dz1 = _conv2_backward(bw, bi, dz)
    if dz1 is None:
        if net.fuse_backward:
            # 80 channels on 8x8 maps: the block's two transposed convs on the LDS-resident images, one launch:
            # dz1 = lrelu'(o1) * conv2^T(dz),  dz(prev) = lrelu'(x) * (conv1^T(dz1) + dz)
            chain = ops.conv_pair(dz, w2d, None, w1d, None, actA=o1, resB=dz, actB=mask)
            if chain is not None:
                bw.wgrad(conv, xin, chain[0], (bi, 1))
                return chain[1]
        dz1 = ops.conv(dz, w2d, None, cp, ks=3, stride=1, pad=1, act=o1)
    dz_prev = bw.fused(conv, dz1, xin, dz, mask is not None, (bi, 1))      # one pass: previous block's dz and dW1/db1
    if dz_prev is None:
        bw.wgrad(conv, xin, dz1, (bi, 1))
        dz_prev = ops.conv(dz1, w1d, None, cp, ks=3, stride=1, pad=1, res=dz, act=mask)
    return dz_prev


def _first_stage_dense(bw, bi):
    """Does the gradient chain of the first (20-channel) stage, below the stage-entry block `bi`, run in the dense layout?
    Only when every kernel of it that reads the layout exists for these shapes: the fused backward and the fused stem
    backward.  Not under want_dx: the tiles' gradient needs the un-pooled stem gradient in the padded layout (the dense one
    has no pool-gradient scatter)."""
    net, saved, dtype = bw.net, bw.saved, bw.dtype
    xin = saved["blocks"][bi][0]
    cin = bw.blocks[bi].conv1.in_channels
    return (net.dense_grads and not bw.want_dx and cin == STEM_WIDTH and ops.cpad(cin) != cin and (dtype == torch.bfloat16 or L.is_split(dtype)) and bi > 0 and
            all(b.stride == 1 and b.downsample is None for b in bw.blocks[:bi]) and
            ops.bwd_fused_workspace_bytes(xin.shape[0], xin.shape[1], xin.shape[2], cin, cin, 3, 1, dtype, True) is not None and
            ops.stem_bwd_dense_ok(saved["x"] if saved["xs"] is None else saved["xs"], dtype))


def _entry_block_backward(bw, bi, dz, dz1=None):
    """Backward of block `bi`, which has a projection shortcut (a stage entry): returns the gradient of its input.  dz1, the
    gradient behind conv2, is given when a stage-wide chain produced it (and dW2/db2 with it)."""
    net, blk = bw.net, bw.blocks[bi]
    xin, o1, _out = bw.saved["blocks"][bi]
    conv, proj, s = blk.conv1, blk.downsample[0], blk.stride
    cin, cout = conv.in_channels, conv.out_channels
    if dz1 is None:
        dz1 = _conv2_backward(bw, bi, dz)
        if dz1 is None:
            w2d, _ = net._packed(f"b{bi}.c2", L.PACK_DGRAD)
            dz1 = ops.conv(dz, w2d, None, ops.cpad(cout), ks=3, stride=1, pad=1, act=o1)
    # block 0 reads the max-pool output (no activation in between); bare_input: the gradient of the block's INPUT TENSOR is
    # wanted — the output of the stage below — not that of the pre-activation map behind it
    mask = xin if bi > 0 and bi != bw.bare_input else None
    pair = None

    def s2_operands():
        """The packed stride-2 filter and the dense-layout rule of the two fused data gradients below.  Asked where one of
        them is about to run, not before: `_first_stage_dense` queries the library, and those calls keep their place."""
        return net._packed(f"b{bi}.c1", L.PACK_DGRAD_S2)[0], (cin if _first_stage_dense(bw, bi) else None)

    if s == 2 and net.fuse_backward and not net.overlap_wgrad and bw.want_wgrad:
        # data gradient and both weight gradients in one launch, where there is such a kernel (bf16, the 20 -> 40 and 40 -> 60
        # entries): the same bits as the two launches below
        ws2, dense_cx = s2_operands()
        one = bw.workspace("p", bi, None, ops.conv_entry_bwd, dz1, dz, ws2, xin, cin, cout, masked=mask is not None, dense_cx=dense_cx,
                           out=bw.out(conv.weight, conv.bias, proj.weight))
        if one is not None:
            bw.grads[bi, 1], bw.grads[bi, 0] = one[1:3], (one[3], None)
            return one[0]
        # both weight gradients of the stage-entry convs from one pass over the block input
        pair = bw.workspace("p", bi, None, ops.conv_wgrad_pair, xin, dz1, dz, cin, cout, out=bw.out(conv.weight, conv.bias, proj.weight))
    if pair is not None:
        bw.grads[bi, 1], bw.grads[bi, 0] = pair[:2], (pair[2], None)
    else:
        bw.wgrad(conv, xin, dz1, (bi, 1))
        bw.wgrad(proj, xin, dz, (bi, 0))
    if s == 2 and net.fuse_backward:        # both transposed convs + the mask in one pass over the compact dz maps
        ws2, dense_cx = s2_operands()
        fused = ops.conv_dgrad_s2(dz1, dz, ws2, ops.cpad(cin), xin.shape[1:3], act=mask, dense_cx=dense_cx)
        if fused is not None:
            return fused
    w1d, _ = net._packed(f"b{bi}.c1", L.PACK_DGRAD)
    wdd, _ = net._packed(f"b{bi}.ds", L.PACK_DGRAD)
    up = dict(zero_insert=True, out_hw=xin.shape[1:3]) if s == 2 else {}        # a stride-2 conv transposed: on the zero-inserted dz
    addend = ops.conv(dz, wdd, None, ops.cpad(cin), ks=1, stride=1, pad=0, **up)
    return ops.conv(dz1, w1d, None, ops.cpad(cin), ks=3, stride=1, pad=1, res=addend, act=mask, **up)


def _guided_block_backward(bw, bi, dz):
    """Backward of block `bi` under guided backpropagation, identity or projection shortcut: returns the gradient of its input.
    At each of the block's two LeakyReLUs the gradient handed on is g where the saved output and g are positive, else 0, g
    being the TOTAL gradient arriving there (the shortcut's share included): `ops.conv_dgrad_rule(rule=1)`, the generic
    implicit-GEMM kernel with the gate in its store epilogue.  What carries no activation — the 1x1 projection's transposed
    conv, and conv1 of block 0, which reads the max-pool output — stays linear and goes through the plain `ops.conv`.  No
    one-pass kernel, no `conv_pair` / `conv_chain` / `conv_dgrad_s2`, no weight gradient."""
    net, blk = bw.net, bw.blocks[bi]
    xin, o1, _out = bw.saved["blocks"][bi]
    conv, s = blk.conv1, blk.stride
    cin_p, cout_p = ops.cpad(conv.in_channels), ops.cpad(conv.out_channels)
    w2d, _ = net._packed(f"b{bi}.c2", L.PACK_DGRAD)
    w1d, _ = net._packed(f"b{bi}.c1", L.PACK_DGRAD)
    dz1 = ops.conv_dgrad_rule(dz, w2d, cout_p, ks=3, pad=1, rule=1, act=o1)
    up = dict(zero_insert=True, out_hw=xin.shape[1:3]) if s == 2 else {}        # a stride-2 conv transposed: on the zero-inserted dz
    if blk.downsample is None:
        addend = dz
    else:
        wdd, _ = net._packed(f"b{bi}.ds", L.PACK_DGRAD)
        addend = ops.conv(dz, wdd, None, cin_p, ks=1, stride=1, pad=0, **up)
    if bi == 0:                             # the max-pool output: no activation in between, nothing to gate
        return ops.conv(dz1, w1d, None, cin_p, ks=3, stride=1, pad=1, res=addend, **up)
    return ops.conv_dgrad_rule(dz1, w1d, cin_p, ks=3, pad=1, rule=1, res=addend, act=xin, **up)


def _stage_dgrad_chain(bw, first, depth, dz_out):
    """Every 3x3 stride-1 data gradient of the stage in ONE launch (ops.conv_chain: whole images resident in LDS — the
    80-channel stage at 256x256 tiles), plus the weight gradients they feed.  Returns (dz of the entry block's output, its
    dz1) — or None when the stage / shape has no such kernel (then the stage is walked block by block)."""
    net, dtype, blocks, saved = bw.net, bw.dtype, bw.blocks, bw.saved
    last = first + depth - 1
    if depth < 2 or depth > 3 or not net.fuse_backward or not (dtype == torch.bfloat16 or L.is_split(dtype)):
        return None
    ent = blocks[first]
    if ent.stride != 2 or ent.downsample is None or any(b.stride != 1 or b.downsample is not None for b in blocks[first + 1:last + 1]):
        return None
    cout = ent.conv1.out_channels
    n, h, w, cp = dz_out.shape
    if (cp, h, w) not in ops.RESIDENT_SHAPES or ops.bwd_fused_workspace_bytes(n, h, w, cout, cout, 3, 1, dtype) is not None:
        return None                         # widths with a fused dgrad+wgrad kernel keep it
    convs, src = [], None                   # src: chain output that is the gradient entering the current block (None: dz_out)
    for k in range(last, first, -1):
        xin_k, o1_k, _ = saved["blocks"][k]
        w2d_k, _ = net._packed(f"b{k}.c2", L.PACK_DGRAD)
        w1d_k, _ = net._packed(f"b{k}.c1", L.PACK_DGRAD)
        convs.append(dict(w=w2d_k, act=o1_k))                                            # dmid_k = lrelu'(o1) * conv2^T(dz_k)
        convs.append(dict(w=w1d_k, res=dz_out if src is None else src, act=xin_k))       # dz_{k-1} = lrelu'(x) * (conv1^T(dmid_k) + dz_k)
        src = len(convs) - 1
    w2d_e, _ = net._packed(f"b{first}.c2", L.PACK_DGRAD)
    convs.append(dict(w=w2d_e, act=saved["blocks"][first][1]))                           # the entry block's dz1
    outs = ops.conv_chain(dz_out, convs)
    if outs is None:
        return None
    dz_k = dz_out
    for i, k in enumerate(range(last, first, -1)):
        xin_k, o1_k, _ = saved["blocks"][k]
        bw.wgrad(blocks[k].conv2, o1_k, dz_k, (k, 2))
        bw.wgrad(blocks[k].conv1, xin_k, outs[2 * i], (k, 1))
        dz_k = outs[2 * i + 1]
    bw.wgrad(ent.conv2, saved["blocks"][first][1], dz_k, (first, 2))
    return dz_k, outs[-1]


def _stage_backward(bw, stage, dz):
    """Backward of `stage` = (index of its first block, its blocks): the stage-wide data-gradient chain where there is one,
    else block by block, last to first.  Returns the gradient of the stage's input."""
    first, blks = stage
    if bw.rule is not None:
        for bi in range(first + len(blks) - 1, first - 1, -1):
            dz = _guided_block_backward(bw, bi, dz)
        return dz
    chain = _stage_dgrad_chain(bw, first, len(blks), dz)
    if chain is not None:                   # what is left is the entry block, from its dz1 on
        return _entry_block_backward(bw, first, *chain)
    for bi in range(first + len(blks) - 1, first - 1, -1):
        step = _identity_block_backward if blks[bi - first].downsample is None else _entry_block_backward
        dz = step(bw, bi, dz)
    return dz


def _stem_backward(bw, dz):
    """conv1's weight gradient from dz, the gradient of the max-pool output.  Returns the un-pooled stem gradient where it
    was made on the way (the fused kernel never materialises it), else None."""
    net, saved = bw.net, bw.saved
    fused_stem = None
    if net.fuse_backward:                   # pool backward + lrelu backward + stem wgrad in one pass (bf16 path)
        src, src_kind = (saved["x"], saved["kind"]) if saved["xs"] is None else (saved["xs"], "s2d")
        fused_stem = ops.stem_backward(src_kind, src, dz, saved["widx"], out=bw.out(net.conv1.weight, net.conv1.bias), ws_alloc=bw.stem_allocator())
    if fused_stem is not None:
        bw.grads["stem", 0] = fused_stem
        return None
    if _is_dense(dz, STEM_WIDTH):
        raise RuntimeError("dense gradient layout without the fused stem backward")
    dstem = ops.maxpool_bwd(dz, saved["widx"], saved["stem_hw"])
    if saved["xs"] is None:
        saved["xs"] = ops.stem_to_s2d(saved["kind"], saved["x"], dz.dtype)
    bw.wgrad(net.conv1, saved["xs"], dstem, ("stem", 0), stem=True)
    return dstem


# ---- the pieces of a backward walk, shared by encoder_backward, encoder_stage_gradient and encoder_pixel_gradient ----------
def _check_dx_args(want_dx, dx_reduce, dx_acc, gate=None):
    if dx_acc is not None and (dx_reduce is not None or not want_dx):
        raise ValueError("dx_acc accumulates the three-channel gradient: it goes with the tiles' gradient (want_dx=True) and without dx_reduce")
    if gate is not None and (dx_reduce is not None or dx_acc is not None):
        raise ValueError("gate multiplies the three-channel gradient as it is stored: it goes without dx_reduce and without dx_acc")


def _pool_gradient(net, saved, dfeats, masked=True, rule=None):
    """The seed of a walk that drops the fc layer's gradient: from dfeats [T,80] to the gradient behind stage 4."""
    # rule "guided": the gate at the last block's LeakyReLU in place of its derivative (the wrapper refuses it with masked=False)
    return ops.avgpool_fc_bwd_data(dfeats.contiguous(), net.fc.weight.detach(), saved["pooled"], saved["blocks"][-1][2], masked=masked,
                                   rule=0 if rule is None else 1)


def _walk(bw, stages, dz, stem=False):
    """`stages` backwards, last to first, from the gradient `dz` behind the last of them — and with `stem` conv1's weight
    gradient — inside the pass's reduction context; then the join of the side streams.  Returns (the gradient of the first
    stage's input, what `_stem_backward` returned or None)."""
    dstem = None
    with bw.reductions(dz.device):
        for stage in reversed(stages):
            dz = _stage_backward(bw, stage, dz)
        if stem:
            dstem = _stem_backward(bw, dz)
    bw.join()
    return dz, dstem


def _padded(dz, c, why):
    if _is_dense(dz, c):
        raise RuntimeError(why)
    return dz


def _tiles_gradient(bw, dz, dstem, dx_reduce, dx_acc, gate=None):
    """The tail of a walk under want_dx, from dz, the gradient of the max-pool output, to the tiles: `ops.maxpool_bwd` unless the
    un-pooled stem gradient `dstem` is at hand (the fused stem backward never materialises it), then `ops.stem_dgrad` -> (dx, sal)
    or, with dx_acc, `ops.stem_dgrad_acc` -> (None, None).  Under the guided rule the pool backward is its guided form; gate:
    `ops.stem_dgrad`'s."""
    net, saved = bw.net, bw.saved
    _padded(dz, STEM_WIDTH, "the tiles' gradient needs the padded layout of the pooled stem gradient")
    if dstem is None and bw.rule is not None:
        dstem = ops.maxpool_bwd(dz, saved["widx"], saved["stem_hw"], rule=1)
    if dstem is None:
        dstem = ops.maxpool_bwd(dz, saved["widx"], saved["stem_hw"])
    if dx_acc is not None:
        ops.stem_dgrad_acc(dstem, net.stem_dgrad_packed(bw.dtype), saved["tile_hw"], dx_acc[0], dx_acc[1])
        return None, None
    if gate is not None:
        return ops.stem_dgrad(dstem, net.stem_dgrad_packed(bw.dtype), saved["tile_hw"], gate=gate)
    return ops.stem_dgrad(dstem, net.stem_dgrad_packed(bw.dtype), saved["tile_hw"], reduce=dx_reduce)


def encoder_backward(net, saved, dfeats, dtype, allow_direct=True, want_dx=False, dx_reduce=None, dx_acc=None):
    """Gradients of every encoder parameter, in `encoder_params()` order.  want_dx=True: returns (those gradients, dx, sal)
    with the gradient of the tiles themselves behind the stem's weight gradient — `ops.maxpool_bwd` to the un-pooled stem
    gradient, then `ops.stem_dgrad`: dx [T,3,H,W] fp32 (dx_reduce=None), or sal [T,H,W] = max_c |dx| and dx None
    (dx_reduce="max_abs"); dx_acc=(acc, scale) (with want_dx; not with dx_reduce): `ops.stem_dgrad_acc` in place of
    `ops.stem_dgrad` — acc [T,3,H,W] fp32 += scale * dx in the kernel's store epilogue, no dx tensor is made, dx and sal are
    None (the inner step of `TileIntegratedGradients` / `TileSmoothGrad`).  The gradient chain of the 20-channel stage then keeps its padded layout (the dense one has no
    pool-gradient scatter), so the parameter gradients are those of `net.dense_grads = False`, bit for bit.  Without want_dx
    nothing of this is packed or launched (`Attention.forward` detaches its input as the reference does,
    gbm/model.py:194-196)."""
    _check_dx_args(want_dx, dx_reduce, dx_acc)
    if saved["x_src"] is not None and saved["x_src"]._version != saved["x_version"]:
        raise RuntimeError("the input tiles were modified in place between the encoder's forward and backward: conv1's gradient is "
                           "computed from them (no space-to-depth copy is kept).  Keep the tensor untouched until backward, or set "
                           "`net.cnn.module.keep_s2d = True` to have the forward keep its own copy (bf16: the space-to-depth records; "
                           "bf16x3: an fp32 clone of the tiles)")
    bw = _Backward(net, saved, dtype, allow_direct, want_dx)
    dz, dwfc = ops.avgpool_fc_bwd(dfeats.contiguous(), net.fc.weight.detach(), saved["pooled"], saved["blocks"][-1][2],
                                  STAGE_WIDTHS[-1], out=net.fc.weight.grad if bw.direct else None)
    dz, dstem = _walk(bw, net.stages(), dz, stem=True)
    dx, sal = _tiles_gradient(bw, dz, dstem, dx_reduce, dx_acc) if want_dx else (None, None)
    flat = list(bw.grads["stem", 0])
    for bi, blk in enumerate(bw.blocks):
        flat += [*bw.grads[bi, 1], *bw.grads[bi, 2]]
        if blk.downsample is not None:
            flat.append(bw.grads[bi, 0][0])
    flat.append(dwfc)
    if bw.direct:
        flat = [None] * len(flat)          # already accumulated into the parameters' .grad tensors
    return (flat, dx, sal) if want_dx else flat


def encoder_stage_gradient(net, saved, dfeats, dtype, stage):
    """Gradient of the OUTPUT of stage `stage` (1..4: layer1..layer4; `saved["blocks"][last block of the stage][2]`, the tensor
    behind the block's LeakyReLU) for the feature gradient `dfeats` [T,80], in that tensor's padded NHWC layout and dtype: the
    backward chain cut short.  `ops.avgpool_fc_bwd_data`, then `_stage_backward` for the stages above `stage`; the stem and the
    stages below are not run.  The chain itself carries gradients of PRE-activation maps (each step multiplies by lrelu' of the
    map it arrives at), so the last step of this walk — the pool gradient for stage 4, else the entry block of stage + 1 —
    runs without that factor.  The gradient keeps the padded layout as under `want_dx`; parameter gradients met on the way are
    dropped and never accumulated (`allow_direct=False`)."""
    if stage not in (1, 2, 3, 4):
        raise ValueError(f"stage must be 1..4, got {stage!r}")
    if stage == 4:
        return _pool_gradient(net, saved, dfeats, masked=False)
    stages = net.stages()
    bw = _Backward(net, saved, dtype, False, True)
    bw.bare_input = stages[stage][0]
    dz, _dstem = _walk(bw, stages[stage:], _pool_gradient(net, saved, dfeats))
    return _padded(dz, STAGE_WIDTHS[stage - 1], "a stage's gradient is returned in the padded layout")


BACKWARD_RULES = (None, "guided")         # encoder_pixel_gradient's rule: the LeakyReLU derivative, or guided backpropagation


def encoder_pixel_gradient(net, saved, dtype, *, dz=None, stage=None, dfeats=None, dx_reduce=None, dx_acc=None, rule=None, gate=None):
    """The gradient of the TILES alone, (dx, sal) as `ops.stem_dgrad` returns them: the data-gradient-only walk from a seed to the
    pixels.  The seed is either `dz`, the gradient of the pre-activation map behind the output of stage `stage` (1..4; what
    `ops.stage_seed` makes, in that tensor's padded NHWC layout and dtype) for a forward that ran at least that far
    (`encoder_forward(upto=stage)`), or `dfeats` [T,80], which goes through `ops.avgpool_fc_bwd_data` — the very launch of
    `ops.avgpool_fc_bwd`'s data half — into stage 4.  Then `_stage_backward` for the stages at and below the seed with
    `want_wgrad=False`: no `ops.conv_wgrad`, no `conv_wgrad_pair` / `conv_entry_bwd`, no `stem_backward`; the one-pass kernels
    that make a data gradient still run and their weight gradients are dropped.  Then `_tiles_gradient`, the tail that
    `encoder_backward` runs under want_dx: dx is bit for bit that function's.  Padded gradient layout, `allow_direct=False`: no
    `.grad` is read or written.
    rule="guided": guided backpropagation.  At every LeakyReLU the gradient handed on is g where the saved
    output and g are positive, else 0: `ops.avgpool_fc_bwd_data(rule=1)` for a dfeats seed (a dz seed is taken as given: the
    gradient behind the stage's last LeakyReLU), `_guided_block_backward` for every block — `ops.conv_dgrad_rule(rule=1)` on the
    generic kernel, the plain `ops.conv` for the two linear pieces — and `ops.maxpool_bwd(rule=1)`; no one-pass kernel,
    `conv_pair`, `conv_chain` or `conv_dgrad_s2` runs and no weight gradient is launched.  With rule=None nothing changes.
    gate: uint8 [T,H,W], handed to `ops.stem_dgrad`, which multiplies dx by gate / 255 as it stores it (without dx_reduce and
    dx_acc; under either rule)."""
    if (dz is None) == (dfeats is None):
        raise ValueError("the seed is either dz (with its stage) or dfeats")
    if rule not in BACKWARD_RULES:
        raise ValueError(f"rule must be one of {BACKWARD_RULES}, got {rule!r}")
    _check_dx_args(True, dx_reduce, dx_acc, gate)
    stages = net.stages()
    if dfeats is not None:
        if stage is not None:
            raise ValueError("dfeats enters behind the fc layer: it takes no stage")
        stage = len(stages)
        if "pooled" not in saved:
            raise ValueError("dfeats needs the whole forward (encoder_forward without upto)")
    elif stage not in (1, 2, 3, 4):
        raise ValueError(f"stage must be 1..4, got {stage!r}")
    first, blks = stages[stage - 1]
    if len(saved["blocks"]) < first + len(blks):
        raise ValueError(f"the forward stopped below stage {stage}")
    top = saved["blocks"][first + len(blks) - 1][2]
    if dfeats is not None:
        dz = _pool_gradient(net, saved, dfeats, rule=rule)
    elif dz.shape != top.shape or dz.dtype != top.dtype:
        raise ValueError(f"dz must be like the output of stage {stage}, {tuple(top.shape)} {top.dtype}, got {tuple(dz.shape)} {dz.dtype}")
    bw = _Backward(net, saved, dtype, False, True, want_wgrad=False, rule=rule)
    dz, _dstem = _walk(bw, stages[:stage], dz)
    return _tiles_gradient(bw, dz, None, dx_reduce, dx_acc, gate)


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, net, x, *params):
        mode = net.compute_dtype            # torch.bfloat16, torch.float32 (exact-f32 MFMA) or L.BF16X3 (fp32 tensors, split products)
        dtype = L.storage_dtype(mode)
        if ctx.needs_input_grad[1] and not (x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3):
            raise NotImplementedError("a gradient for the tiles exists for the fp32 [T,3,H,W] feed only: the bf16 space-to-depth "
                                      "tensor (S2dTiles) holds rounded values, and no kernel writes a gradient in its layout")
        with L.f32_mma(L.mma_code(mode)):
            feats, saved = encoder_forward(net, x.detach(), dtype)
        ctx.net, ctx.saved, ctx.dtype, ctx.mode = net, saved, dtype, mode
        return feats

    @staticmethod
    def backward(ctx, dfeats):
        want_dx = ctx.needs_input_grad[1]
        with L.f32_mma(L.mma_code(ctx.mode)):
            grads = encoder_backward(ctx.net, ctx.saved, dfeats, ctx.dtype, allow_direct=all(ctx.needs_input_grad[2:]), want_dx=want_dx)
        ctx.saved = None
        if want_dx:                         # x.requires_grad_(): the tiles' own gradient, behind the stem's weight gradient
            grads, dx, _sal = grads
            return (None, dx, *grads)
        return (None, None, *grads)
