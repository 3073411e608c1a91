"""CPU (-m "not gpu"): the parts of the poisoned run (tests/test_gpu_poison.py) that need no GPU.
  * build() leaves the shipped and the poisoned library; the poisoned one exports the whole ABI plus the two probes, the
    shipped one no probe;
  * source audit: every LDS declaration of every kernel is poisoned at entry in the diagnostic build — a new kernel that
    forgets the macro fails here;
  * `gpu_util.poison_allocations()` on CPU tensors (its device predicate is a parameter)."""
import ctypes
import glob
import os
import re

import pytest
import torch

from gpu_util import allocations_poisoned, poison_allocations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBES = ("mil_poison_probe", "mil_poison_static_probe")


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "mil_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mil_[a-z0-9_]+)\s*\(", text)))


def test_build_leaves_both_libraries_and_only_the_poisoned_one_has_probes():
    import mil_amd
    from mil_amd import _lib
    assert os.path.basename(_lib.POISON_LIB_PATH) == "libmil_hip_poison.so"
    shipped = os.path.join(os.path.dirname(_lib.POISON_LIB_PATH), "libmil_hip.so")
    assert os.path.exists(shipped) and os.path.exists(_lib.POISON_LIB_PATH), "run __graft_entry__.build()"
    if not os.environ.get("MIL_LIB_PATH"):
        assert mil_amd.LIB_PATH == shipped                     # importing the package binds the shipped library
    ship, poison = ctypes.CDLL(shipped), ctypes.CDLL(_lib.POISON_LIB_PATH)
    declared = _header_symbols()
    assert len(declared) >= 15 and not set(PROBES) & set(declared)
    for name in declared:
        assert hasattr(poison, name), f"{name} missing from the poisoned library"
    for name in PROBES:
        assert hasattr(poison, name), f"the poisoned library lacks {name}"
        assert not hasattr(ship, name), f"the shipped library exports {name}"
    assert poison.mil_abi_version() == ship.mil_abi_version() == 2


# ---- source audit ------------------------------------------------------------------------------------------------------------
def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _enclosing_block_end(text, pos):
    """Index of the `}` that closes the block `pos` is in."""
    depth = 0
    for i in range(pos, len(text)):
        if text[i] == "{":
            depth += 1
        elif text[i] == "}":
            if depth == 0:
                return i
            depth -= 1
    return len(text)


def audit_lds_poison(text):
    """(number of dynamic declarations, number of static names, list of complaints) for one source text."""
    text = _strip_comments(text)
    complaints, n_dyn, n_static = [], 0, 0
    for m in re.finditer(r"\bextern\s+__shared__\b[^;]*?\b(\w+)\s*\[\s*\]\s*;", text):
        n_dyn += 1
        name = m.group(1)
        nxt = re.match(r"\s*([^;{}]*;)", text[m.end():])
        stmt = re.sub(r"\s+", "", nxt.group(1)) if nxt else ""
        if stmt != f"MIL_POISON({name});":
            complaints.append(f"extern __shared__ {name}[] is not followed by MIL_POISON({name}); but by `{stmt}`")
    for m in re.finditer(r"(?<![\w])__shared__\b([^;]*);", text):
        if re.search(r"\bextern\s*$", text[max(0, m.start() - 16):m.start()]):
            continue
        decl = re.sub(r"__attribute__\s*\(\((?:[^()]|\([^()]*\))*\)\)", " ", m.group(1))
        body = text[m.end():_enclosing_block_end(text, m.end())]
        for piece in decl.split(","):
            nm = re.search(r"(\w+)\s*(?:\[[^\]]*\]\s*)*$", piece.strip())
            assert nm, f"cannot parse the declaration `{m.group(0)}`"
            name = nm.group(1)
            n_static += 1
            first = re.search(rf"\b{name}\b", body)
            ok = first is not None and re.search(rf"MIL_POISON_STATIC\(\s*$", body[:first.start()]) is not None \
                and re.match(rf"{name}\s*\)", body[first.start():]) is not None
            if not ok:
                complaints.append(f"static __shared__ {name}: its first use in the kernel is not MIL_POISON_STATIC({name})")
    return n_dyn, n_static, complaints


def test_every_lds_declaration_is_poisoned_at_kernel_entry():
    csrc = glob.glob(os.path.join(ROOT, "*_amd", "csrc"))[0]
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cuh")))
    assert len(files) >= 30
    n_dyn = n_static = 0
    complaints = []
    for f in files:
        d, s, c = audit_lds_poison(open(f).read())
        n_dyn, n_static = n_dyn + d, n_static + s
        complaints += [f"{os.path.basename(f)}: {x}" for x in c]
    assert not complaints, "\n".join(complaints)
    assert n_dyn >= 31 and n_static >= 20, (n_dyn, n_static)          # what the sources hold today: the audit is not vacuous
    common = _strip_comments(open(os.path.join(csrc, "common.cuh")).read())
    # the shipped build's kernels are untouched: both macros expand to nothing without -DMIL_POISON_LDS
    tail = common[common.index("#else", common.index("#define MIL_POISON(base) mil_poison_lds")):]
    assert re.search(r"#define MIL_POISON\(base\) \(\(void\)0\)\s*#define MIL_POISON_STATIC\(arr\) \(\(void\)0\)\s*#endif", tail)


def test_the_audit_catches_a_forgotten_macro():
    good = """
    __global__ void k(float* o) {
        __shared__ __attribute__((aligned(16))) float a[4][8];   // per wave
        __shared__ float b[16], c;
        MIL_POISON_STATIC(a); MIL_POISON_STATIC(b); MIL_POISON_STATIC(c);
        a[0][0] = b[1] + c;
    }
    __global__ void d(float* o) {
        extern __shared__ __attribute__((aligned(16))) char smem[];
        MIL_POISON(smem);
        o[0] = smem[0];
    }"""
    assert audit_lds_poison(good) == (1, 3, [])
    assert len(audit_lds_poison(good.replace("MIL_POISON_STATIC(b); ", ""))[2]) == 1
    assert len(audit_lds_poison(good.replace("MIL_POISON_STATIC(c);", ""))[2]) == 1
    assert len(audit_lds_poison(good.replace("        MIL_POISON(smem);\n", ""))[2]) == 1
    # poisoned too late (after the first access), or by another kernel of the same file
    late = good.replace("MIL_POISON_STATIC(a); ", "").replace("a[0][0] = b[1] + c;", "a[0][0] = b[1] + c; MIL_POISON_STATIC(a);")
    assert len(audit_lds_poison(late)[2]) == 1
    other = good.replace("MIL_POISON_STATIC(a); ", "").replace("MIL_POISON(smem);", "MIL_POISON(smem); MIL_POISON_STATIC(a);")
    assert len(audit_lds_poison(other)[2]) == 1
    assert len(audit_lds_poison(good.replace("MIL_POISON(smem);", "const int t = 0; MIL_POISON(smem);"))[2]) == 1


# ---- poison_allocations() on CPU tensors ---------------------------------------------------------------------------------------
def _everywhere(t):
    return True


def _all_bytes_ff(t):
    return bool((t.contiguous().view(-1).view(torch.uint8) == 255).all())


def test_poison_patterns_per_dtype():
    with poison_allocations(device_predicate=_everywhere):
        assert allocations_poisoned()
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            for t in (torch.empty((3, 5, 7), dtype=dt), torch.empty_like(torch.zeros(11, dtype=dt)), torch.zeros(2, dtype=dt).new_empty((4, 3)),
                      torch.empty(6, dtype=dt).new_empty(5), torch.empty((), dtype=dt)):
                assert t.dtype == dt and bool(torch.isnan(t).all()) and _all_bytes_ff(t), dt
        assert torch.empty_like(torch.zeros(4), dtype=torch.bfloat16).dtype == torch.bfloat16
        u = torch.empty((9, 9), dtype=torch.uint8)
        assert bool((u == 255).all()) and bool((torch.empty_like(u) == 255).all()) and bool((u.new_empty(3) == 255).all())
        for dt in (torch.int32, torch.int64):                  # (left alone: test_int_tensors_are_not_written)
            assert torch.empty(8, dtype=dt).dtype == dt and torch.empty_like(torch.zeros(8, dtype=dt)).dtype == dt
    assert not allocations_poisoned()
    # the default predicate: CPU tensors are not touched at all
    with poison_allocations():
        t = torch.empty(4096, dtype=torch.float32)
        t.zero_()
        del t
        assert not bool(torch.isnan(torch.empty(4096, dtype=torch.float32)).any())


def test_int_tensors_are_not_written():
    """Stronger than "does not hold the pattern": the fill is not reached for int32 / int64 (and the narrower integers)."""
    import gpu_util
    seen = []
    orig = gpu_util._poison_fill

    def spy(t):
        before = t.clone()
        out = orig(t)
        seen.append((t.dtype, bool(torch.equal(before, out)) if not t.is_floating_point() else None))
        return out
    gpu_util._poison_fill, keep = spy, gpu_util._poison_fill
    try:
        with poison_allocations(device_predicate=_everywhere):
            for dt in (torch.int32, torch.int64, torch.int16, torch.int8):
                torch.empty(64, dtype=dt)
                torch.zeros(64, dtype=dt).new_empty(8)
    finally:
        gpu_util._poison_fill = keep
    assert len(seen) == 8 and all(same for _, same in seen)


def test_zero_size_set_idiom_and_non_contiguous():
    with poison_allocations(device_predicate=_everywhere):
        assert torch.empty(0).numel() == 0 and torch.empty((4, 0, 3), dtype=torch.bfloat16).shape == (4, 0, 3)
        # head.py: a zero-size tensor re-pointed at a run of gradient storage, then accumulated into
        g0 = torch.arange(12, dtype=torch.float32)
        view = torch.empty(0, dtype=torch.float32).set_(g0.untyped_storage(), 2, (5,))
        assert torch.equal(view, torch.arange(2, 7, dtype=torch.float32))          # the storage it points at was NOT filled
        view.add_(torch.ones(5))
        assert torch.equal(g0, torch.tensor([0, 1, 3, 4, 5, 6, 7, 7, 8, 9, 10, 11], dtype=torch.float32))
        # empty_like keeps the strides of a permuted (dense, non-contiguous) tensor: filled through them, no exception
        p = torch.zeros((2, 3, 4, 5)).permute(0, 2, 3, 1)
        e = torch.empty_like(p)
        assert not e.is_contiguous() and e.stride() == p.stride() and bool(torch.isnan(e).all())
        pu = torch.empty_like(torch.zeros((6, 4), dtype=torch.uint8).t())
        assert bool((pu == 255).all())
        # a leaf that wants a gradient, and the modules / optimizers that allocate through torch.empty
        w = torch.empty(3, requires_grad=True)
        assert w.requires_grad and w.is_leaf
        lin = torch.nn.Linear(7, 3)
        assert bool(torch.isfinite(lin.weight).all()) and bool(torch.isfinite(lin.bias).all())
        y = torch.nn.functional.conv2d(torch.ones(1, 2, 5, 5), torch.ones(3, 2, 3, 3), padding=1)
        assert bool(torch.isfinite(y).all())
        opt = torch.optim.Adam(lin.parameters(), lr=1e-2)
        lin(torch.ones(2, 7)).sum().backward()
        opt.step()
        assert bool(torch.isfinite(lin.weight).all())


def test_originals_are_restored_also_after_an_exception():
    import mil_amd  # noqa: F401
    from mil_amd import ops
    orig = (torch.empty, torch.empty_like, torch.Tensor.new_empty, ops.ReduceBatch.workspace)

    def now():
        return (torch.empty, torch.empty_like, torch.Tensor.new_empty, ops.ReduceBatch.workspace)
    with poison_allocations(device_predicate=_everywhere):
        assert all(a is not b for a, b in zip(now(), orig))
        with poison_allocations(device_predicate=_everywhere):          # nests
            assert bool(torch.isnan(torch.empty(3)).all())
        assert allocations_poisoned() and bool(torch.isnan(torch.empty(3)).all())
    assert all(a is b for a, b in zip(now(), orig))
    with pytest.raises(ZeroDivisionError):
        with poison_allocations(device_predicate=_everywhere):
            1 / 0
    assert all(a is b for a, b in zip(now(), orig)) and not allocations_poisoned()
    # the one-way switch: on from the call, until someone leaves it
    switch = poison_allocations(device_predicate=_everywhere, reduce_batch=False)
    try:
        assert allocations_poisoned() and ops.ReduceBatch.workspace is orig[3]
    finally:
        switch.__exit__(None, None, None)
    assert all(a is b for a, b in zip(now(), orig))


def test_reduce_batch_workspace_is_refilled_each_time_it_is_handed_out():
    import mil_amd  # noqa: F401
    from mil_amd import ops
    with poison_allocations(device_predicate=_everywhere):
        rb = ops.ReduceBatch(torch.device("cpu"))
        w = rb.workspace(("w", 0), 1000)
        assert w.numel() == 250 and bool(torch.isnan(w).all())
        w.zero_()                                                   # "last step's slabs"
        w2 = rb.workspace(("w", 0), 400)
        assert w2.data_ptr() == w.data_ptr() and bool(torch.isnan(w2).all())
        with rb:                                                    # the double-hand-out guard still fires
            rb.workspace(("f", 1), 64)
            with pytest.raises(RuntimeError, match="handed out twice"):
                rb.workspace(("f", 1), 64)
    rb2 = ops.ReduceBatch(torch.device("cpu"))
    w = rb2.workspace(("w", 0), 64)
    w.zero_()
    assert bool((rb2.workspace(("w", 0), 64) == 0).all())           # unwrapped again: the buffer keeps its contents
