"""GPU: the packed wave sums of the symmetric-storage step kernel (wave_sums_packed, rbpf_step_sym.hip: four sums per register
butterfly) give the bits of the xor butterfly through LDS (wave_sum) that they replaced -- one wave, NV = 1 .. 36 vectors of 64
doubles through rbpf_probe_wave_sums_packed.  36 covers the counts of the kernel (9, 18, 27 values of K_s' H', 12 and 14 innovation
statistics, 3 and 4 per border row, 1 and 2 in dense-radio) and every size of the last group."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)


def vectors(nv, rs):
    """mixed magnitudes; cancelling neighbours and first-stage partners; a row of signed zeros; a subnormal row"""
    x = rs.standard_normal((nv, 64)) * 10.0 ** rs.randint(-12, 13, size=(nv, 64))
    x[::3, ::2] = -x[::3, 1::2] * (1.0 + 2.0 ** -52)
    x[1::5, 32:] = -x[1::5, :32]
    if nv > 2:
        x[2] = np.where(rs.rand(64) < 0.5, 0.0, -0.0)
    if nv > 4:
        x[4] = rs.randint(-2 ** 20, 2 ** 20, size=64) * (np.finfo(np.float64).tiny * 2.0 ** -40)
    if nv > 6:
        x[6] = -0.0
    return np.ascontiguousarray(x)


@pytest.fixture(scope="module")
def probe(rbpf):
    lib = rbpf.load_library()
    lib.rbpf_probe_wave_sums_packed.argtypes = [C.c_int32, DP, DP, DP]
    lib.rbpf_probe_wave_sums_packed.restype = C.c_int

    def run(nv, x):
        ref, got = np.full(nv, np.nan), np.full(nv, np.nan)
        st = lib.rbpf_probe_wave_sums_packed(nv, x.ctypes.data_as(DP), ref.ctypes.data_as(DP), got.ctypes.data_as(DP))
        assert st == 0, st
        return ref, got
    return run


def test_packed_sums_equal_the_xor_butterfly_bitwise(probe):
    rs = np.random.RandomState(11)
    for nv in range(1, 37):
        x = vectors(nv, rs)
        ref, got = probe(nv, x)
        assert np.array_equal(ref.view(np.uint64), got.view(np.uint64)), (nv, ref, got)      # every slot, signs of zeros included
        np.testing.assert_array_equal(got, ref)
        # the butterfly itself: a sum of the 64 values (loose: any association order)
        np.testing.assert_allclose(ref, x.sum(axis=1), rtol=0, atol=1e-13 * np.abs(x).sum(axis=1).max() + 1e-300)


def test_exact_sums_reach_their_slots(probe):
    """integers (exact in any order), a different total per slot: every value lands in its own slot at every NV"""
    for nv in range(1, 37):
        x = np.ascontiguousarray((np.arange(nv * 64, dtype=np.float64).reshape(nv, 64) % 97.0) + 1000.0 * np.arange(nv)[:, None])
        ref, got = probe(nv, x)
        np.testing.assert_array_equal(ref, x.sum(axis=1))
        np.testing.assert_array_equal(got, x.sum(axis=1))
