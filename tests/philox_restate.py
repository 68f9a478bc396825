"""Plain Python / numpy restatement of the library's seeded noise generator (switch_nerf_amd/csrc/philox.hpp): Philox4x32-10 with the
standard constants, the (seed, step, stream, global element) addressing, the uniform map and the Box-Muller normal map.  Integers for
the words, float64 for the normals.  Shared by tests/test_device_noise_cpu.py and tests/test_device_noise_gpu.py."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF

KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (Python ints) -> the 4 output words."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def block_counter(block: int, step: int, stream: int):
    return block & MASK, (block >> 32) & MASK, step & MASK, stream & MASK


def element_word(seed: int, step: int, stream: int, e: int) -> int:
    """The word of global element e: word e & 3 of block e >> 2, counter {b_lo, b_hi, step, stream}, key {seed_lo, seed_hi}."""
    return philox4x32_10(block_counter(e >> 2, step, stream), (seed & MASK, (seed >> 32) & MASK))[e & 3]


def _philox_blocks(blocks, step, stream, seed):
    """Vectorised over an array of block indices (uint64) -> [n, 4] uint64 words."""
    blocks = np.asarray(blocks, dtype=np.uint64)
    m = np.uint64(MASK)
    c0, c1 = blocks & m, (blocks >> np.uint64(32)) & m
    c2 = np.full_like(blocks, step & MASK)
    c3 = np.full_like(blocks, stream & MASK)
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2        # 32 x 32 bit products fit 64 bits
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], 1)


def words(seed: int, step: int, stream: int, base: int, n: int):
    """The uint64-held 32-bit words of elements base .. base + n - 1."""
    b0, b1 = base >> 2, (base + n - 1) >> 2
    w = _philox_blocks(np.arange(b0, b1 + 1, dtype=np.uint64), step, stream, seed).reshape(-1)
    off = base - 4 * b0
    return w[off:off + n]


def uniform(seed, step, stream, base, n):
    """float32 [n]: (x >> 8) * 2^-24, exact in fp32 - compared bit for bit."""
    return ((words(seed, step, stream, base, n) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def normal(seed, step, stream, base, n, scale=1.0):
    """float64 [n]: Box-Muller over the word pairs (0,1) and (2,3) of every block; even word r cos(theta), odd word r sin(theta)."""
    e0 = base & ~1                                             # the pair partner of an odd base lies before it
    e1 = (base + n + 1) & ~1
    w = words(seed, step, stream, e0, e1 - e0).reshape(-1, 2)
    u1 = ((w[:, 0] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    theta = 2.0 * np.pi * (w[:, 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    out = np.stack([r * np.cos(theta), r * np.sin(theta)], 1).reshape(-1) * float(scale)
    return out[base - e0: base - e0 + n]
