"""CPU: the two orders in which the step kernel of the symmetric storage can sum 64 lanes give the same bits.

`wave_sum` (rbpf_device.hpp) is the xor butterfly: six stages, lane l adds the value of lane l ^ 32, 16, 8, 4, 2, 1.  `wave_sum4`
(rbpf_step_sym.hip) sums four values at once: v_permlane32_swap and v_permlane16_swap fold four registers into one (two stages),
four DPP row rotations by 8, 4, 2, 1 finish the 16-lane rows.  Both pair the same lanes at every stage; an add may see its operands
swapped (IEEE addition is commutative), so after every stage all lanes of an xor class hold identical bits and a rotation by k
delivers what the xor by k would.  Emulated here in numpy float64, lane for lane."""
import numpy as np
import pytest

LANES = np.arange(64)
ROW_OF_VALUE = [0, 2, 1, 3]          # wave_sum4: value k ends in row rho with (rho & 1) * 2 + (rho >> 1) == k


def butterfly(x):
    v = x.copy()
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[LANES ^ off]
    return v


def fold32(a, b):
    """lanes 0..31: a[l] + a[l + 32]; lanes 32..63: b[l - 32] + b[l]"""
    r = np.empty(64)
    r[:32] = a[:32] + a[32:]
    r[32:] = b[:32] + b[32:]
    return r


def fold16(a, b):
    """rows of 16 lanes: [a.r0 + a.r1, b.r0 + b.r1, a.r2 + a.r3, b.r2 + b.r3]"""
    ar, br = a.reshape(4, 16), b.reshape(4, 16)
    return np.concatenate([ar[0] + ar[1], br[0] + br[1], ar[2] + ar[3], br[2] + br[3]])


def row_ror(x, k):
    """DPP row_ror:k -- lane l of a 16-lane row receives lane (l - k) mod 16 of it"""
    return x.reshape(4, 16)[:, (np.arange(16) - k) % 16].reshape(64)


def wave_sum4(x0, x1, x2, x3):
    x = fold16(fold32(x0, x1), fold32(x2, x3))
    for k in (8, 4, 2, 1):
        x = x + row_ror(x, k)
    return x


def packed(xs):
    """wave_sums_packed: groups of four through wave_sum4, a last group of 1-3 filled up with its first value; the value lane 16 rho stores"""
    nv = len(xs)
    out = np.empty(nv)
    for j in range((nv + 3) // 4):
        grp = [xs[4 * j + k] if 4 * j + k < nv else xs[4 * j] for k in range(4)]
        r = wave_sum4(*grp)
        for k in range(4):
            if 4 * j + k < nv:
                out[4 * j + k] = r[16 * ROW_OF_VALUE[k]]
    return out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def inputs(kind, rs, nv):
    tiny = np.finfo(np.float64).tiny
    if kind == "mixed":
        return rs.standard_normal((nv, 64)) * 10.0 ** rs.randint(-12, 13, size=(nv, 64))
    if kind == "cancel":
        x = rs.standard_normal((nv, 64)) * 10.0 ** rs.randint(-12, 13, size=(nv, 64))
        x[:, ::2] = -x[:, 1::2] * (1.0 + rs.randint(0, 2, size=(nv, 32)) * 2.0 ** -52)      # neighbours cancel (almost)
        x[:, :32] = np.where(rs.rand(nv, 32) < 0.3, -x[:, 32:], x[:, :32])                  # and partners of the first stage
        return x
    if kind == "zeros":
        x = np.where(rs.rand(nv, 64) < 0.5, 0.0, -0.0)
        x[0] = -0.0                                                                         # a total of -0 needs every term -0
        if nv > 1:
            x[1] = np.where(rs.rand(64) < 0.1, rs.standard_normal(64), x[1])
            x[1, 32:] = -x[1, :32]                                                          # exact cancellation -> +0
        return x
    if kind == "subnormal":
        x = rs.randint(-2 ** 20, 2 ** 20, size=(nv, 64)) * (tiny * 2.0 ** -40)             # subnormal terms, subnormal sums
        x[nv // 2] = rs.standard_normal(64) * tiny * 10.0 ** rs.randint(-3, 4, size=64)    # across the normal / subnormal border
        return x
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["mixed", "cancel", "zeros", "subnormal"])
def test_packed_order_equals_xor_butterfly_bitwise(kind):
    rs = np.random.RandomState({"mixed": 1, "cancel": 2, "zeros": 3, "subnormal": 4}[kind])
    for nv in list(range(1, 9)) + [9, 12, 14, 18, 27, 36]:
        for trial in range(20):
            xs = inputs(kind, rs, nv)
            got = packed(xs)
            for q in range(nv):
                b = butterfly(xs[q])
                assert same_bits(b, np.full(64, b[0])), "the xor butterfly leaves one value in every lane"
                assert same_bits(got[q], b[0]), (kind, nv, trial, q, got[q], b[0])


def test_every_lane_of_a_row_holds_the_rows_total():
    """what lets lane 16 rho store: wave_sum4 leaves the total of value k in all sixteen lanes of row ROW_OF_VALUE[k]"""
    rs = np.random.RandomState(5)
    for trial in range(200):
        xs = inputs("mixed" if trial % 2 else "cancel", rs, 4)
        r = wave_sum4(*xs)
        for k in range(4):
            rho = ROW_OF_VALUE[k]
            assert (rho & 1) * 2 + (rho >> 1) == k
            assert same_bits(r[16 * rho:16 * rho + 16], np.full(16, butterfly(xs[k])[0]))


def test_signed_zero_totals():
    x = np.full((4, 64), -0.0)
    x[1, 17] = 0.0
    x[2, :32] = 1.5
    x[2, 32:] = -1.5
    got = packed(x)
    assert np.signbit(got[0]) and not np.signbit(got[1]) and not np.signbit(got[2]) and np.signbit(got[3])
    for q in range(4):
        assert same_bits(got[q], butterfly(x[q])[0])
