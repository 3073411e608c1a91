"""The noise of `mil_path_point` restated in numpy: Philox4x32-10 (Salmon et al., SC'11; the Random123 generator) and the
Box-Muller transform in fp64 from the same bits.  Shared by tests/test_cpu_path_attr.py and tests/test_gpu_path_attr.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
# the three known answers (counter, key, output); the first two are Random123's own known-answer vectors (zeros, all ones), the
# third its "digits of pi" vector
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
# seed whose first counter (element group 0, sample 0) gives r0 >> 8 == 0xffffff, i.e. u1 == 1: elements 0 and 1 are exactly 0.
# Found by a search over seeds with `philox4x32_10`; tests/test_cpu_path_attr.py checks it.
SEED_WITH_U1_ONE = 16390493


def philox4x32_10(counter, key):
    """Four uint64 arrays holding the 32-bit output words for counter (c0, c1, c2, c3) and key (k0, k1), scalars or arrays."""
    u = np.uint64
    c = [np.asarray(v, dtype=u) for v in counter]
    k = [np.asarray(v, dtype=u) for v in key]
    mask, s32 = u(0xffffffff), u(32)
    for _ in range(10):
        p0, p1 = u(M0) * c[0], u(M1) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k[0], p1 & mask, (p0 >> s32) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + u(W0)) & mask, (k[1] + u(W1)) & mask]
    return c


def normals(n, seed=0, sample=0):
    """The first n standard normals of (seed, sample) in fp64, element i at index i: counter (i >> 2 low, i >> 2 high, sample, 0),
    key (seed low, seed high); elements 4q, 4q + 1 from (r0, r1), 4q + 2, 4q + 3 from (r2, r3)."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    zero = np.zeros_like(q)
    r = philox4x32_10((q & np.uint64(0xffffffff), q >> np.uint64(32), zero + np.uint64(sample), zero),
                      (np.uint64(seed & 0xffffffff), np.uint64(seed >> 32)))
    out = np.empty((len(q), 4), dtype=np.float64)
    for pair in (0, 1):
        u1 = ((r[2 * pair] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (r[2 * pair + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pair] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * pair + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[:n]
