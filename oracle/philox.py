"""numpy Philox4x32-10 (Salmon et al. 2011) and the uniform mapping of the kernels.  TEST INFRASTRUCTURE ONLY.

Restates csrc/lg_math.h:219-238 (philox4x32_10, u01) over arrays: every argument is broadcast, values are carried in
uint64 so that a 32 x 32-bit product keeps both halves.
"""
from __future__ import annotations

import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on counter (c0, c1, c2, c3) under key (k0, k1); returns the four 32-bit output words as uint64 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(np.asarray(v, np.uint64) & MASK for v in (c0, c1, c2, c3, k0, k1)))
    c0, c1, c2, c3, k0, k1 = (v.copy() for v in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):                       # lg_math.h:225-235
        p0, p1 = c0 * M0, c2 * M1             # < 2^64: exact
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def u01(r):
    """lg_math.h:238: the low 24 bits times 2^-24, as float32 (exact: every value is a multiple of 2^-24 below 1)."""
    return ((np.asarray(r, np.uint64) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
