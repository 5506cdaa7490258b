"""Host reference of the dropout mask of gta_block.hip (numpy): Philox4x32-10 and the keep rule, restated from the kernel's contract.

    key            the two 32-bit halves of the call's 64-bit seed (low, high)
    counter        unit i8 (elements 8 i8 .. 8 i8 + 7) draws two blocks, at the 64-bit counters 2 i8 and 2 i8 + 1, each split into
                   (low word, high word, 0, 0); the four output words of a block belong to four consecutive elements
    keep           word >= min(uint32(p 2^32), 0xffffffff), p as the fp32 value the C ABI receives; kept values are scaled by the
                   fp32 quotient 1 / (1 - p)

Nothing here touches the GPU or the library: the known answer of the generator is a CPU test (tests/test_philox_host.py), the masks of
the kernels are compared with `keep_mask` in tests/test_gpu_block.py and tests/test_gpu_block_regimes.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key schedule (Weyl constants)
_LOW = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds over arrays of counter words (uint32-valued, any common shape) under the key (k0, k1) -> four uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _LOW for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2                      # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _S32) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(p):
    """The word below which an element is dropped"""
    return min(int(float(np.float32(p)) * 4294967296.0), 0xFFFFFFFF)


def keep_scale(p):
    """What a kept element is multiplied by: 1 / (1 - p) in fp32"""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(n, p, seed, first_unit=0):
    """bool [n]: is element 8 first_unit + j kept, j < n, in a call with probability p and this seed (n a multiple of 8)"""
    assert n % 8 == 0 and n >= 0 and first_unit >= 0
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = (np.arange(n // 4, dtype=np.uint64) + np.uint64(2 * first_unit))   # block b of the window: counter 2 first_unit + b
    zero = np.zeros_like(ctr)
    words = np.stack(philox4x32_10(ctr & _LOW, ctr >> _S32, zero, zero, seed & 0xFFFFFFFF, seed >> 32), axis=1).reshape(-1)
    return words >= np.uint32(threshold(p))
