"""Philox4x32-10 written with one 64-bit product per multiplier (risvec_dev.hpp: `p = (uint64_t)M * c`, hi = p >> 32,
lo = (uint32_t)p) against the multiply-high / multiply-low pair it replaces: an exact integer identity, restated here in
NumPy and held against the oracle's philox4x32 (which every draw test of the device uses as its reference).  No GPU."""
import numpy as np

from oracle import risvec_oracle as orc

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
CORNERS = np.array([0, 1, 2 ** 32 - 1], dtype=np.uint32)


def _counters(n, seed):
    rng = np.random.default_rng(seed)
    return np.concatenate([CORNERS, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)])


def _mulhi_mullo(m, c):
    """the pair: the high word by 16-bit limbs (no 64-bit product anywhere), the low word by a wrapping 32-bit multiply"""
    c = c.astype(np.uint32)
    with np.errstate(over="ignore"):
        lo = np.uint32(m) * c
    a1, a0 = np.uint64(m >> 16), np.uint64(m & 0xFFFF)
    b1, b0 = (c >> np.uint32(16)).astype(np.uint64), (c & np.uint32(0xFFFF)).astype(np.uint64)
    mid = a1 * b0 + ((a0 * b0) >> np.uint64(16))                       # < 2^32 + 2^16
    mid2 = a0 * b1 + (mid & np.uint64(0xFFFF))
    hi = a1 * b1 + (mid >> np.uint64(16)) + (mid2 >> np.uint64(16))
    return hi.astype(np.uint32), lo


def _product(m, c):
    """the product: one uint64 multiply, split into halves by a shift and a truncating conversion"""
    p = np.uint64(m) * c.astype(np.uint64)
    return (p >> np.uint64(32)).astype(np.uint32), p.astype(np.uint32)


def _oracle_halves(m, c):
    """the halves as oracle.philox4x32 takes them: >> 32 and & 0xffffffff"""
    p = np.uint64(m) * c.astype(np.uint64)
    return (p >> np.uint64(32)).astype(np.uint32), (p & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _round(c, k, halves):
    hi0, lo0 = halves(M0, c[0])
    hi1, lo1 = halves(M1, c[2])
    return (hi1 ^ c[1] ^ np.uint32(k[0]), lo1, hi0 ^ c[3] ^ np.uint32(k[1]), lo0)


def _ten_rounds(c, seed, halves):
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    for _ in range(10):
        c = _round(c, (k0, k1), halves)
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def test_one_product_gives_the_pair():
    c = _counters(100_000, 1)
    for m in (M0, M1):
        hi_p, lo_p = _product(m, c)
        hi_o, lo_o = _oracle_halves(m, c)
        hi_m, lo_m = _mulhi_mullo(m, c)
        assert np.array_equal(hi_p, hi_o) and np.array_equal(lo_p, lo_o)
        assert np.array_equal(hi_p, hi_m) and np.array_equal(lo_p, lo_m)
    # the corner values by hand: 0, the multiplier itself, and M * (2^32 - 1) = (M - 1) * 2^32 + (2^32 - M)
    hi, lo = _product(M0, CORNERS)
    assert hi.tolist() == [0, 0, M0 - 1] and lo.tolist() == [0, M0, 2 ** 32 - M0]


def test_one_round_both_ways():
    c = tuple(_counters(100_000, s) for s in (2, 3, 4, 5))
    k = (0x243F6A88, 0x85A308D3)
    a = _round(c, k, _product)
    b = _round(c, k, _mulhi_mullo)
    o = _round(c, k, _oracle_halves)
    for x, y, z in zip(a, b, o):
        assert x.dtype == np.uint32 and np.array_equal(x, y) and np.array_equal(x, z)


def test_ten_rounds_against_the_oracle():
    c = tuple(_counters(100_000, s) for s in (6, 7, 8, 9))
    for seed in (0, 1, 0x0123456789ABCDEF, 2 ** 64 - 1):
        want = orc.philox4x32(*c, seed)
        got = _ten_rounds(c, seed, _product)
        pair = _ten_rounds(c, seed, _mulhi_mullo)
        for w, g, p in zip(want, got, pair):
            assert np.array_equal(w, g) and np.array_equal(w, p), hex(seed)
