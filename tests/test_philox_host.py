"""CPU: the host reference of the dropout mask (tests/_philox.py) against the published known answers of Philox4x32-10, and the
bookkeeping of `keep_mask` (windows, threshold, the seed's halves).  The kernels are compared with it in the GPU tests."""
import numpy as np

from tests import _philox as P


def _words(counter, key):
    return [int(w[()]) for w in P.philox4x32_10(*[np.array(c, dtype=np.uint64) for c in counter], *key)]


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32 with 10 rounds: zeros, all ones, the digits of pi"""
    assert _words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = 0xffffffff
    assert _words((f, f, f, f), (f, f)) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert _words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_keep_mask_layout():
    seed, p = (0x1234567 << 32) | 0x89abcdef, 0.3
    m = P.keep_mask(64, p, seed)
    # element 8 i8 + j: word j % 4 of the block at counter 2 i8 + j // 4, keyed by the seed's (low, high) halves
    for e in (0, 3, 4, 13, 63):
        w = _words((e // 4, 0, 0, 0), (seed & 0xffffffff, seed >> 32))[e % 4]
        assert bool(m[e]) == (w >= P.threshold(p))
    assert np.array_equal(P.keep_mask(16, p, seed, first_unit=5), P.keep_mask(64, p, seed)[40:56])          # a window is a slice
    big = 1 << 31                                                                                           # counter 2^32: the high word
    hi = P.keep_mask(8, p, seed, first_unit=big)
    w = _words((0, 1, 0, 0), (seed & 0xffffffff, seed >> 32))
    assert [bool(x) for x in hi[:4]] == [x >= P.threshold(p) for x in w]
    assert not np.array_equal(m, P.keep_mask(64, p, seed + (1 << 32)))                                      # the high half is part of the key


def test_keep_mask_threshold_and_rate():
    assert P.threshold(0.0) == 0 and P.keep_mask(64, 0.0, 7).all()
    assert P.threshold(0.5) == 1 << 31
    assert P.threshold(0.3) == int(float(np.float32(0.3)) * 2.0 ** 32)                                      # p as fp32, not as a double
    assert P.threshold(np.nextafter(np.float32(1.0), np.float32(0.0))) <= 0xffffffff
    n = 1 << 20
    for p in (0.01, 0.3):
        kept = P.keep_mask(n, p, 1234).mean()
        assert abs(kept - (1 - p)) < 4 * (p * (1 - p) / n) ** 0.5
    assert P.keep_scale(0.0) == 1.0 and abs(float(P.keep_scale(0.3)) - 1 / 0.7) < 1e-6
