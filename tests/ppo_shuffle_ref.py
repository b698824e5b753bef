"""Host restatement of hg_ppo_shuffle (TEST INFRASTRUCTURE): include/heligym_amd.h's keyed permutation of
0 .. B-1 in NumPy, exact (integer arithmetic only), with tests/philox_ref.py for Philox4x32-10.

  w = max(1, bit_length(B - 1)), half = ceil(w / 2), mask = 2^half - 1; element i starts at x = i; one pass is
  four Feistel rounds (L, R) <- (R, L ^ (F(R, j) & mask)) on L = x >> half, R = x & mask; passes repeat while
  x >= B.  F(R, j) = word 0 of Philox on the counter (R, j, e_lo, e_hi), key (seed_lo ^ 0x73687566,
  seed_hi ^ 0x666C655F), e = epoch (+ the device counter's value)."""
import numpy as np

from philox_ref import MASK, philox4x32_10

KEY_XOR = (0x73687566, 0x666C655F)


def shuffle_ref(B, seed, epoch=0):
    """(index [B] int32, passes [B] int64: how many passes each element took)."""
    B = int(B)
    w = max(1, (B - 1).bit_length())
    half = (w + 1) // 2
    mask = np.uint64((1 << half) - 1)
    e = int(epoch) & (2 ** 64 - 1)
    k0, k1 = (seed & MASK) ^ KEY_XOR[0], ((seed >> 32) & MASK) ^ KEY_XOR[1]
    x = np.arange(B, dtype=np.uint64)
    out = np.empty(B, dtype=np.int64)
    passes = np.zeros(B, dtype=np.int64)
    todo = np.arange(B)
    while len(todo):
        L, R = x >> np.uint64(half), x & mask
        for j in range(4):
            rows = np.empty((len(R), 6), dtype=np.uint64)
            rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = R, j, e & MASK, e >> 32
            rows[:, 4], rows[:, 5] = k0, k1
            f = philox4x32_10(rows)[:, 0].astype(np.uint64)
            L, R = R, L ^ (f & mask)
        x = (L << np.uint64(half)) | R
        passes[todo] += 1
        done = x < np.uint64(B)
        out[todo[done]] = x[done].astype(np.int64)
        todo, x = todo[~done], x[~done]
    return out.astype(np.int32), passes
