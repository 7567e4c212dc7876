"""Philox4x32-10 from the paper's definition (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3",
SC'11, section 5.3 and the Random123 known-answer file), in Python integers, and the two maps the device puts on top of it:
counter (slot, step, lane, iter) + 64-bit seed -> two 53-bit uniforms, and Box-Muller pairs on lanes 1, 2, ...

Nothing here is taken from the product's host.py or rbpf_device.hpp: the tests compare those with this file.

One round of Philox-4x32 on the counter (c0, c1, c2, c3) with the round key (k0, k1):
    hi0:lo0 = M0 * c0,  hi1:lo1 = M1 * c2            (32 x 32 -> 64 bit products)
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0,  lo1,  hi0 ^ c3 ^ k1,  lo0)
and between rounds the key is bumped by the Weyl constants: k0 += W0, k1 += W1 (mod 2^32).  Ten rounds.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57            # multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85            # Weyl constants: golden ratio, sqrt(3) - 1
MASK = 0xFFFFFFFF

# Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, output)
KNOWN_ANSWERS = [
    ((0x00000000,) * 4, (0x00000000,) * 2, (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]

SEEDS = [0, 1, 2 ** 32 - 1, 2 ** 32, 0xDEADBEEFCAFEF00D, 2 ** 64 - 1]   # both key halves and the carry between them
BACKWARD_LANE = 0x42530000                                              # lane of the backward-simulation uniforms


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = (int(v) & MASK for v in counter)
    k0, k1 = (int(v) & MASK for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _unit53(hi, lo):
    """(float(a) + 0.5) * 2^-53 with a the top 53 bits of hi:lo, evaluated in IEEE doubles: for a >= 2^52 the sum
    a + 0.5 is not representable and rounds (to even), so the largest value is exactly 1.0."""
    a = ((hi << 32) | lo) >> 11
    return (np.float64(a) + np.float64(0.5)) * np.float64(2.0 ** -53)


def uniform2(seed, slot, step, lane, it):
    """The two uniforms of counter (slot, step, lane, iter) under key (low 32 bits of seed, high 32 bits of seed)."""
    seed = int(seed)
    c = philox4x32_10((slot, step, lane, it), (seed & MASK, (seed >> 32) & MASK))
    return float(_unit53(c[0], c[1])), float(_unit53(c[2], c[3]))


def normals(seed, slot, step, it, nw):
    """z [nw] in np.longdouble and the radius r [nw] of each element's pair: pair j/2 on lane 1 + j/2,
    r = sqrt(-2 ln u0), z[j] = r cos(2 pi u1), z[j+1] = r sin(2 pi u1), with a long-double pi."""
    ld = np.longdouble
    pi = ld(4) * np.arctan(ld(1))
    z = np.zeros(nw, dtype=ld)
    r = np.zeros(nw, dtype=ld)
    for j in range(0, nw, 2):
        u0, u1 = uniform2(seed, slot, step, 1 + j // 2, it)
        rad = np.sqrt(ld(-2) * np.log(ld(u0)))
        ang = ld(2) * pi * ld(u1)
        z[j], r[j] = rad * np.cos(ang), rad
        if j + 1 < nw:
            z[j + 1], r[j + 1] = rad * np.sin(ang), rad
    return z, r
