"""Every call the narrow encoder makes into the C library, configuration by configuration (GPU box): run on two trees and
`diff` the outputs to show that a change of the host orchestration (encoder.py, ops.py) launches the same kernels in the same
order with the same arguments, and computes the same bits.

  python tools/dev/launch_trace.py [--tree DIR] [--only TEXT] [--out FILE]      the traces and digests
  python tools/dev/launch_trace.py --cover encoder_forward,encoder_backward     + on stderr, the lines of those functions that never ran
  python tools/dev/launch_trace.py --time                                       host time of two small steps, recording off

`--tree` (default: this repository) is where `mil_amd` is imported from; MIL_LIB_PATH selects the library as usual.  The
cached handle `_lib._lib` is replaced by a proxy that records, per call: the symbol, every scalar, for every pointer the
ordinal of that address's first appearance in the configuration (0: NULL; "host" for the caller's ctypes buffers) — aliasing
is compared, addresses are not —, the value a by-reference output holds afterwards, and the `ops._ChainConv` records of
`mil_conv_chain`.  An ordinal is meant to name one tensor, but the caching allocator hands a freed block to the next tensor of
its size, and two trees that drop a temporary one statement apart would then differ in ordinals though they pass the same
tensors.  So while a configuration runs, every tensor that any torch operator returns is kept alive (a dispatch mode; the
backward passes run on the calling thread for it): no block is freed, and none is handed out twice."""
import argparse
import ast
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch.utils._python_dispatch import TorchDispatchMode

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HOST_ARGS = {"mil_conv_chain": (1,), "mil_reduce_defer_begin": (0,), "mil_wgrad_reduce_all": (1,)}   # host addresses passed as ints
MODES = {"bf16": torch.bfloat16, "fp32": torch.float32, "x3": "bf16x3"}


class Recorder:
    """Stands in for the ctypes library handle: attribute lookup returns a recording wrapper around the real function."""

    def __init__(self, real, sigs, chain_struct):
        self._real, self._sigs, self._chain = real, sigs, chain_struct
        self.reset()

    def reset(self):
        self.lines, self._seen, self._count = [], {}, 0

    def _ordinal(self, a):
        if not a:
            return 0
        if a not in self._seen:
            self._count += 1
            self._seen[a] = self._count
        return self._seen[a]

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._sigs:
            return fn
        types = self._sigs[name][0]

        def call(*args):
            parts = []
            for i, (a, t) in enumerate(zip(args, types)):
                if t is ctypes.c_void_p and (i in HOST_ARGS.get(name, ()) or not isinstance(a, (int, type(None)))):
                    parts.append("host")        # a ctypes buffer of the caller's (job tables): a malloc address says nothing
                elif t is ctypes.c_void_p:
                    parts.append(f"p{self._ordinal(a)}")
                elif issubclass(t, ctypes._Pointer):
                    parts.append(None)          # a by-reference output: its value after the call
                else:
                    parts.append(format(a, ".9g") if isinstance(a, float) else str(int(a)))
            if name == "mil_conv_chain":
                arr = (self._chain * args[2]).from_address(args[1])
                parts.append("[" + " ".join(f"(w=p{self._ordinal(c.wpack)} bias=p{self._ordinal(c.bias)} res=p{self._ordinal(c.res)} "
                                            f"act=p{self._ordinal(c.act)} out=p{self._ordinal(c.out)} lrelu={c.lrelu})" for c in arr) + "]")
            rc = fn(*args)
            parts = [f"out={a._obj.value}" if p is None else p for p, a in zip(parts, args + (None,))]
            self.lines.append(f"{name}({', '.join(parts)}) -> {rc}")
            return rc
        return call


class keep_alive(TorchDispatchMode):
    """Inside the block, whatever any torch operator returns lives until the block is left — with backward passes run on the
    calling thread, so that the mode (which is per thread) sees them too."""

    def __enter__(self):
        self.kept = []
        self.single = torch.autograd.set_multithreading_enabled(False)
        self.single.__enter__()
        return super().__enter__()

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.kept.append(out)
        return out

    def __exit__(self, *exc):
        super().__exit__(*exc)
        self.single.__exit__(*exc)
        self.kept = []


def sha(t):
    return hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest()[:24]


def configurations():
    """(name, settings): mode, tile size, bag sizes, encoder attributes to set, and what drives the pass."""
    out = []
    for mode in MODES:
        for size in (64, 128, 256, 300):
            out.append((f"{mode}-{size}-defaults", dict(mode=mode, size=size)))
            out.append((f"{mode}-{size}-no_fuse_backward", dict(mode=mode, size=size, attrs=dict(fuse_backward=False))))
            out.append((f"{mode}-{size}-unfused", dict(mode=mode, size=size, attrs=dict(
                fuse_backward=False, fuse_stem_forward=False, fuse_stage_entry=False, fuse_block_forward=False))))
    for mode in ("bf16", "x3"):
        for size in (256, 300):
            for attr, val in (("dense_grads", False), ("batch_reductions", False), ("overlap_wgrad", True), ("keep_s2d", True)):
                out.append((f"{mode}-{size}-{attr}={val}", dict(mode=mode, size=size, attrs={attr: val})))
            for drive in ("direct_grad", "u8", "s2d", "want_dx", "saliency", "hooks"):
                if drive != "s2d" or mode == "bf16":
                    out.append((f"{mode}-{size}-{drive}", dict(mode=mode, size=size, drive=drive)))
    # the workspace queries that gate the fused paths depend on the launch size: both sides of the persistent-kernel threshold
    out.append(("x3-128-bags40+30-pf_min_tiles=1", dict(mode="x3", size=128, bags=(40, 30), env=dict(MIL_PF_MIN_TILES="1"))))
    out.append(("x3-128-bags40+30", dict(mode="x3", size=128, bags=(40, 30))))
    # un-fused passes of the remaining feeds and of the tiles' gradient, a kept copy under the u8 feed
    for drive in ("u8", "s2d", "want_dx"):
        out.append((f"bf16-64-{drive}-no_fuse_backward", dict(mode="bf16", size=64, drive=drive, attrs=dict(fuse_backward=False))))
    out.append(("x3-64-u8-keep_s2d", dict(mode="x3", size=64, drive="u8", attrs=dict(keep_s2d=True))))
    out.append(("x3-64-keep_s2d", dict(mode="x3", size=64, attrs=dict(keep_s2d=True))))
    out.append(("bf16-64-hooks-avgpool-fc", dict(mode="bf16", size=64, drive="hooks_tail")))
    out.append(("x3-64-activation_summary", dict(mode="x3", size=64, drive="summary")))
    # four blocks in the last stage: too deep for the stage-wide resident chains, so its identity blocks run them pair by pair
    out.append(("bf16-256-layer4_of_four", dict(mode="bf16", size=256, drive="deep_layer4")))
    out.append(("x3-256-layer4_of_four", dict(mode="x3", size=256, drive="deep_layer4")))
    return out


def make_net(mil_amd, mode):
    w = np.load(os.path.join(ROOT, "tests", "golden", "weights.npz"))
    net = mil_amd.Attention(3, compute_dtype=MODES[mode]).eval()
    net.load_state_dict({k: torch.tensor(w[k]) for k in w.keys()})
    return net


def run(mil_amd, rec, name, mode, size, bags=(5, 7), attrs=None, drive=None, env=None):
    """One configuration: returns the digest lines; the trace is in rec.lines."""
    from mil_amd import ops
    from mil_amd.preprocess import S2dTiles, U8Tiles
    gen = torch.Generator().manual_seed(1234)
    net = make_net(mil_amd, mode)
    enc = net.cnn.module
    for k, v in (attrs or {}).items():
        assert hasattr(enc, k), k
        setattr(enc, k, v)
    if drive == "deep_layer4":
        torch.manual_seed(5)
        enc.layer4.append(type(enc.layer4[1])(80, 80).to(enc.conv1.weight.device))
    if drive == "summary":
        mil_amd.ActivationSummary(net, taps="blocks")
    if drive in ("hooks", "hooks_tail"):
        seen = []
        mods = (enc.layer3, enc.layer1[1].relu, enc.conv1) if drive == "hooks" else (enc.avgpool, enc.fc, enc.layer2[0])
        for m in mods:
            m.register_forward_hook(lambda m, i, o: seen.append(tuple(o.shape)))
    labels = torch.tensor([k % 3 for k in range(len(bags))])
    if drive == "u8":
        xs = [U8Tiles(torch.randint(0, 256, (n, 3, size, size), generator=gen, dtype=torch.uint8)) for n in bags]
    else:
        xs = [torch.randn(n, 3, size, size, generator=gen).clamp_(-1, 1).cuda() for n in bags]
    if drive == "s2d":
        xs = [S2dTiles(ops.stem_s2d(x, torch.bfloat16)) for x in xs]
    for k, v in (env or {}).items():
        os.environ[k] = v
    digests = []
    torch.cuda.synchronize()
    rec.reset()
    try:
        if drive == "want_dx":                  # the model detaches its tiles (as the reference does): the encoder alone
            x = torch.cat(xs).requires_grad_()
            feats = enc(x)
            feats.backward(torch.randn(feats.shape, generator=gen).cuda())
            digests.append(f"dx {sha(x.grad)}")
        elif drive == "saliency":
            sal = mil_amd.TileSaliency(net)
            digests.append(f"sal {sha(sal.maps(xs[0], 1, 'gradient'))}")
            digests.append(f"dx {sha(sal.input_gradient(xs[1], 2))}")
            feats = None
        else:
            flat = mil_amd.FlatParams(net) if drive == "direct_grad" else None
            for _ in range(2 if flat is not None else 1):
                outs = net.forward_bags(xs, labels)
                outs.loss.sum().backward()
            feats = torch.stack([o["y_pred"].reshape(-1) for o in outs])
        torch.cuda.synchronize()
    finally:
        for k in (env or {}):
            del os.environ[k]
    if feats is not None:
        digests.insert(0, f"out {sha(feats)}")
    for pname, p in net.named_parameters():
        if p.grad is not None:
            digests.append(f"grad {pname} {sha(p.grad)}")
    if drive in ("hooks", "hooks_tail"):
        digests.append(f"hooks {seen}")
    return digests


class LineCover:
    """Which lines of the named functions of the tree's encoder.py ran (nested functions included).  The backward runs on
    autograd's own thread, which sys.settrace does not reach: the traced entry points install the tracer themselves."""

    def __init__(self, encoder, names, extra_modules):
        self.file = encoder.__file__
        self.src = open(self.file).read().split("\n")
        self.spans, self.skip = [], set()
        for node in ast.walk(ast.parse("\n".join(self.src))):
            if isinstance(node, ast.FunctionDef) and node.name in names:
                self.spans.append((node.lineno, node.end_lineno))
            if isinstance(node, ast.Raise):
                self.skip.update(range(node.lineno, node.end_lineno + 1))
        self.hit, self.code_lines = set(), set()
        for name in names:
            fn = getattr(encoder, name)
            self._collect(fn.__code__)
            for mod in (encoder,) + tuple(extra_modules):
                if getattr(mod, name, None) is fn:
                    setattr(mod, name, self._traced(fn))

    def _collect(self, code):
        self.code_lines.update(ln for _s, _e, ln in code.co_lines() if ln is not None and ln > code.co_firstlineno)
        for c in code.co_consts:
            if hasattr(c, "co_lines"):
                self._collect(c)

    def _traced(self, fn):
        def traced(*a, **k):
            prev = sys.gettrace()
            sys.settrace(self._global)
            try:
                return fn(*a, **k)
            finally:
                sys.settrace(prev)
        return traced

    def _global(self, frame, event, arg):
        if frame.f_code.co_filename == self.file and any(a <= frame.f_code.co_firstlineno <= b for a, b in self.spans):
            return self._local
        return None

    def _local(self, frame, event, arg):
        if event == "line":
            self.hit.add(frame.f_lineno)
        return self._local

    def report(self):
        missed = sorted(ln for ln in self.code_lines - self.hit if ln not in self.skip and self.src[ln - 1].strip() not in ("", "else:"))
        return [f"never executed (raise statements apart): {len(missed)} lines"] + [f"  {ln}: {self.src[ln - 1].strip()}" for ln in missed]


def time_steps(mil_amd):
    """Median host time per forward + backward step of two small bags (each step ends in a device synchronise)."""
    res = {}
    for label, n, size in (("8x64", 8, 64), ("200x300", 200, 300)):
        net = make_net(mil_amd, "x3")
        x = torch.randn(n, 3, size, size, generator=torch.Generator().manual_seed(3)).clamp_(-1, 1).cuda()
        y = torch.tensor([1])
        samples = []
        for it in range(220):
            t0 = time.perf_counter()
            net.forward_bags([x], y).loss.sum().backward()
            torch.cuda.synchronize()
            samples.append(time.perf_counter() - t0)
            net.zero_grad(set_to_none=True)
        res[label + "_median_ms"] = round(1e3 * statistics.median(samples[20:]), 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--only", default="", help="run the configurations whose name contains this text")
    ap.add_argument("--out", default=None, help="write the traces and digests here instead of to stdout")
    ap.add_argument("--cover", default="", help="comma-separated functions of encoder.py: list their lines that never ran")
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import mil_amd
    from mil_amd import _lib as L, encoder, ops, saliency
    assert os.path.abspath(mil_amd.__file__).startswith(os.path.abspath(args.tree)), mil_amd.__file__
    if args.time:
        print(json.dumps(dict(tree=os.path.abspath(args.tree), **time_steps(mil_amd))))
        return
    cover = LineCover(encoder, args.cover.split(","), (saliency,)) if args.cover else None
    rec = L._lib = Recorder(L.lib(), L._SIGS, ops._ChainConv)
    sink = open(args.out, "w") if args.out else sys.stdout
    t0 = time.perf_counter()
    for name, cfg in configurations():
        if args.only not in name:
            continue
        with keep_alive():
            digests = run(mil_amd, rec, name, **cfg)
        print(f"== {name}: {len(rec.lines)} calls", file=sink)
        print("\n".join(rec.lines + digests), file=sink)
        torch.cuda.empty_cache()
    if cover is not None:
        print("\n".join(cover.report()), file=sys.stderr)
    print(f"{time.perf_counter() - t0:.1f} s", file=sys.stderr)


if __name__ == "__main__":
    main()
