"""The fixed-order sum of a tile in slices (csrc/slice_sum.cuh), restated in numpy fp32 with the summation tree include/mil_hip.h
writes down for `objective`, `energy`, `loss`, `terms` and `tile_sum` — every addition one correctly rounded fp32 operation:

  a tile's work items are cut into `slices` runs of `per` items, one workgroup of 256 threads each (the last runs short or empty);
  thread tid takes the items tid, tid + 256, ... of its run and adds their terms one by one, in the order given, to a sum that
  starts at +0; the 64 lanes of a wave then add s = s + s[lane ^ d] for d = 32, 16, ..., 1; the four waves are added in order,
  ((w0 + w1) + w2) + w3; a second pass adds the slices in order, again from +0; the entry's last operation (a quotient, a scaled
  quotient, or nothing) follows.

A term that a kernel skips (a padding channel, a pixel that owns no cell, the tail of a short group or slice) is a +0 here: a sum
that starts at +0 never becomes -0 under round-to-nearest, so adding +0 leaves every bit as it is.  Vectorised over tiles, slices
and threads: the Python loops run over a thread's rounds and the terms of an item only.

The five callers form their terms with the roundings of their kernels and hand them over in work-item order."""
import numpy as np

THREADS = 256
SEED_SLICES, REG_SLICES, ATTR_SLICES = 16, 16, 32


def tree_sum(terms, slices, per):
    """terms fp32 [T, items, k] — the k terms of every work item of a tile, in the order a thread adds them — cut into `slices`
    runs of `per` items -> fp32 [T], the tile's sum by the tree above."""
    terms = np.asarray(terms)
    assert terms.dtype == np.float32 and terms.ndim == 3 and terms.shape[1] <= slices * per
    n, items, k = terms.shape
    rounds = -(-per // THREADS)
    run = np.zeros((n, slices * per, k), dtype=np.float32)
    run[:, :items] = terms
    grid = np.zeros((n, slices, rounds * THREADS, k), dtype=np.float32)
    grid[:, :, :per] = run.reshape(n, slices, per, k)
    grid = grid.reshape(n, slices, rounds, THREADS, k)
    s = np.zeros((n, slices, THREADS), dtype=np.float32)
    for r in range(rounds):                                  # a thread's own chain
        for j in range(k):
            s = s + grid[:, :, r, :, j]
    s = s.reshape(n, slices, THREADS // 64, 64)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):                           # the butterfly: every lane ends with the wave's sum
        s = s + s[..., lane ^ d]
    w = s[..., 0]
    part = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
    assert part.dtype == np.float32
    total = np.zeros(n, dtype=np.float32)
    for i in range(slices):                                  # the second pass
        total = total + part[:, i]
    return total


def _stage(terms):
    """Per-element terms [T,h,w,cp] of a stage output -> the tile sums: a work item is one 8-channel group of one pixel, its
    terms in channel order; MIL_SEED_SLICES runs of ceil(h w / slices) pixels."""
    n, h, w, cp = terms.shape
    per = -(-(h * w) // SEED_SLICES)
    return tree_sum(terms.reshape(n, h * w * (cp // 8), 8), SEED_SLICES, per * (cp // 8))


def stage_seed_objective(act, channels):
    """mil_stage_seed's objective for act fp32 [T,h,w,cp] holding the STORED values: the tile's channel summed, / (h w)."""
    act = np.asarray(act, dtype=np.float32)
    terms = np.zeros_like(act)
    for t, ch in enumerate(channels):
        terms[t, :, :, ch] = act[t, :, :, ch]
    return _stage(terms) / np.float32(act.shape[1] * act.shape[2])


def _real(x, c):
    x = np.asarray(x, dtype=np.float32).copy()
    x[..., c:] = 0                                           # the padding channels do not count
    return x


def stage_energy(target, c):
    """mil_stage_energy's energy: a * a over the real channels."""
    a = _real(target, c)
    return _stage(a * a)


def stage_match_loss(act, target, c, energy, weight):
    """mil_stage_match's loss: (a - g) * (a - g) over the real channels, then weight * (D / E_t)."""
    d = _real(act, c) - _real(target, c)
    return np.float32(weight) * (_stage(d * d) / np.asarray(energy, dtype=np.float32))


def reg_terms(x, alpha):
    """mil_pixel_reg's terms [2,T] for x fp32 [T,3,H,W]: a work item is four consecutive elements of the tile's 3 H W (fewer in
    the last), MIL_REG_SLICES runs of ceil(groups / slices) of them.  Row 0: p * v with p = v^(alpha-1) by repeated products;
    row 1: dd * dd + dr * dr on the pixels that own a cell (not in the last row or column)."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    p = x.copy()
    for _ in range(alpha - 2):
        p = p * x
    tv = np.zeros_like(x)
    own = x[:, :, :-1, :-1]
    dd, dr = own - x[:, :, 1:, :-1], own - x[:, :, :-1, 1:]
    tv[:, :, :-1, :-1] = dd * dd + dr * dr
    groups = (x[0].size + 3) // 4
    per = -(-groups // REG_SLICES)

    def rows(e):
        flat = np.zeros((n, groups * 4), dtype=np.float32)
        flat[:, :x[0].size] = e.reshape(n, -1)
        return tree_sum(flat.reshape(n, groups, 4), REG_SLICES, per)
    return np.stack([rows(p * x), rows(tv)])


def attr_tile_sums(attr):
    """mil_attr_finish's tile_sum for attr fp32 [T,3,H,W]: (a0 + a1) + a2 per pixel; a work item is four consecutive pixels,
    MIL_ATTR_SLICES runs of ceil(h w / slices) pixels rounded up to a multiple of four."""
    a = np.asarray(attr, dtype=np.float32)
    n, hw = a.shape[0], a.shape[2] * a.shape[3]
    a = a.reshape(n, 3, hw)
    tot = (a[:, 0] + a[:, 1]) + a[:, 2]
    per = (-(-hw // ATTR_SLICES) + 3) & ~3
    flat = np.zeros((n, (hw + 3) // 4 * 4), dtype=np.float32)
    flat[:, :hw] = tot
    return tree_sum(flat.reshape(n, -1, 4), ATTR_SLICES, per // 4)
