"""The host reference of the state digest (include/qingdai_hip.h: qd_state_digest), in NumPy uint64 arithmetic.  It is the
yardstick of tests/test_state_digest_cpu.py and tests/test_gpu_state_digest.py and imports nothing of the package.

    D(plane) = sum_{i = 0 .. n-1} mix64(w_i + (i + 1) * 0x9E3779B97F4A7C15)  mod 2^64

w_i: the element's stored bits zero-extended to 64 bits (f64 8 bytes, f32 4, u8 1), i: its row-major index in the global plane,
mix64: the splitmix64 finaliser.  The run digest of named planes is sum_e mix64(D_e ^ fnv1a64(name_e)) mod 2^64.
"""
import numpy as np

GOLD = np.uint64(0x9E3779B97F4A7C15)
M1, M2 = np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3
MASK = (1 << 64) - 1


def mix64(z):
    """splitmix64's finaliser on a uint64 array (or scalar), wrapping."""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z ^ (z >> np.uint64(30))
        z = z * M1
        z = z ^ (z >> np.uint64(27))
        z = z * M2
        z = z ^ (z >> np.uint64(31))
    return z


def words(a):
    """The stored bits of every element, zero-extended to uint64, in row-major order."""
    a = np.ascontiguousarray(a)
    if a.dtype.itemsize not in (8, 4, 1):
        raise TypeError(f"the digest is defined for 8-, 4- and 1-byte elements, not {a.dtype}")
    return a.reshape(-1).view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize]).astype(np.uint64)


def digest(a, index0=0):
    """The digest of a plane -> int.  index0: the global row-major index of a's first element, for a block of a larger plane (the
    digest of the plane is the sum of its blocks' digests mod 2^64)."""
    w = words(a)
    with np.errstate(over="ignore"):
        i1 = np.arange(w.size, dtype=np.uint64) + np.uint64(int(index0) + 1)
        return int(np.sum(mix64(w + i1 * GOLD), dtype=np.uint64))


def fnv1a64(name):
    h = FNV_OFFSET
    for b in str(name).encode("utf-8"):
        h = ((h ^ b) * FNV_PRIME) & MASK
    return h


def run_digest(digests):
    """{name: D} -> sum_e mix64(D_e ^ fnv1a64(name_e)) mod 2^64."""
    total = 0
    for name, d in digests.items():
        total = (total + int(mix64(np.uint64(int(d) ^ fnv1a64(name))))) & MASK
    return total
