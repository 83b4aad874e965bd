"""Oracle of the counter-based dropout mask (csrc/dropout.hip, ops.dropout_apply), independent of the product code: numpy only, on the
Philox4x32-10 of tests/mesh_reference.py (uint64 arithmetic masked to 32 bits).

  element (r, c) is dropped  iff  (w >> 8) < threshold,   threshold = int(p * 2^24 + 0.5)
  w = word (c & 3) of Philox4x32-10(key = (seed & 0xffffffff, seed >> 32), counter = (c >> 2, (row0 + r) & 0xffffffff, step & 0xffffffff, tower))
  y = x * m in ONE fp32 multiply, m = 0 where dropped, fp32(1 / (1 - p)) elsewhere (0 at p = 1)
"""
import numpy as np

from tests.mesh_reference import philox4x32_10

M32 = 0xFFFFFFFF


def threshold(p):
    return int(float(p) * 16777216.0 + 0.5)


def scale32(p):
    return np.float32(0.0) if float(p) == 1.0 else np.float32(1.0 / (1.0 - float(p)))


def uniform_bits(rows, cols, seed, step, row0=0, tower=0):
    """uint64 [rows, cols]: the 24 bits (w >> 8) of every element; every element runs its own Philox call (four per group: the
    kernel's sharing of one call among four columns is not assumed here)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    c = np.broadcast_to(np.arange(cols, dtype=np.uint64)[None, :], (rows, cols))
    r = np.broadcast_to(np.array([(int(row0) + i) & M32 for i in range(rows)], dtype=np.uint64)[:, None], (rows, cols))
    words = philox4x32_10((c >> np.uint64(2), r, np.full((rows, cols), int(step) & M32, dtype=np.uint64),
                           np.full((rows, cols), int(tower) & M32, dtype=np.uint64)), (seed & M32, seed >> 32))
    w = np.choose((c & np.uint64(3)).astype(np.int64), words)
    return w >> np.uint64(8)


def dropped(rows, cols, p, seed, step, row0=0, tower=0, bits=None):
    """bool [rows, cols]: True where the element is dropped (bits: uniform_bits(...) of the same arguments, when already at hand)."""
    bits = uniform_bits(rows, cols, seed, step, row0, tower) if bits is None else bits
    return bits < np.uint64(threshold(p))


def multiplier(rows, cols, p, seed, step, row0=0, tower=0, bits=None):
    """float32 [rows, cols]: 0 where dropped, fp32(1 / (1 - p)) elsewhere."""
    return np.where(dropped(rows, cols, p, seed, step, row0, tower, bits), np.float32(0.0), scale32(p)).astype(np.float32)


def apply(x, p, seed, step, row0=0, tower=0, bits=None):
    """x float32 [rows, cols] -> x * m, one fp32 multiply per element (inf * 0 = NaN)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x * multiplier(x.shape[0], x.shape[1], p, seed, step, row0, tower, bits)).astype(np.float32)
