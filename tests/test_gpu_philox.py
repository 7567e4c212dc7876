"""The device generator (philox4x32_10 / philox_uniform2 / philox_normals of csrc/rbpf_device.hpp, dumped by
rbpf_philox_fill) against the from-spec reference of philox_ref.py: uniforms bit for bit, Box-Muller normals against a
long-double evaluation, and the counter layout (slot, step, lane, iter) independent of the sizes of the call.

Bound on the normals: |Z - Z_ref| <= 4e-15 * max(1, r), r = sqrt(-2 ln u0) the pair's radius.  The angle 2 pi u1 carries one
rounding of the product (<= 4.4e-16 at angles up to 2 pi) and the double pi (<= 2.4e-16); sincos and log/sqrt add about
2 ulp each (<= 4.4e-16 each, relative to r): 1.6e-15 r in all, and the bound is 2.5 x that.

Measured on an MI355X (all seeds, k_iter 0 and 3, N = 300, T = 4): max |dZ| / max(1, r) = 6.97e-16, between 6.67e-16
and 6.97e-16 in each of the twelve (seed, k_iter) cases (each test prints its own).
"""
import ctypes as C

import numpy as np
import pytest

import philox_ref as P

pytestmark = pytest.mark.gpu

N, T, NW_MAX = 300, 4, 8
NWS = (1, 3, 6, 8)
K_ITERS = (0, 3)
Z_BOUND = 4e-15
_ref_cache = {}


def fill(rbpf, seed, k_iter, n, t, nw):
    """rbpf_philox_fill itself (PhiloxRNG.replay hides k_iter): U [t-1, n], Z [t-1, n, nw], Ufin."""
    lib = rbpf.load_library()
    U = np.full((t - 1, n), np.nan)
    Z = np.full((t - 1, n, nw), np.nan)
    uf = C.c_double(np.nan)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.rbpf_philox_fill(C.c_uint64(seed), k_iter, n, t, nw, dp(U), dp(Z), C.byref(uf))
    assert rc == rbpf.RBPF_OK, lib.rbpf_last_error()
    return U, Z, uf.value


def reference(seed, k_iter):
    """U [T-1, N], Z and the radii [T-1, N, 8] (long double), Ufin -- computed once per (seed, k_iter), never modified."""
    key = (seed, k_iter)
    if key not in _ref_cache:
        U = np.empty((T - 1, N))
        Z = np.empty((T - 1, N, NW_MAX), dtype=np.longdouble)
        R = np.empty((T - 1, N, NW_MAX), dtype=np.longdouble)
        for t in range(1, T):
            for i in range(N):
                U[t - 1, i] = P.uniform2(seed, i, t, 0, k_iter)[0]
                Z[t - 1, i], R[t - 1, i] = P.normals(seed, i, t, k_iter, NW_MAX)
        for a in (U, Z, R):
            a.setflags(write=False)
        _ref_cache[key] = (U, Z, R, P.uniform2(seed, 0, T, 0, k_iter)[0])
    return _ref_cache[key]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("k_iter", K_ITERS)
@pytest.mark.parametrize("seed", P.SEEDS)
def test_device_stream_equals_the_spec(rbpf, seed, k_iter):
    assert np.finfo(np.longdouble).eps < 1e-18
    U_ref, Z_ref, R_ref, uf_ref = reference(seed, k_iter)
    worst = 0.0
    for nw in NWS:
        U, Z, uf = fill(rbpf, seed, k_iter, N, T, nw)
        np.testing.assert_array_equal(bits(U), bits(U_ref))                        # lane 0, first uniform, every slot and step
        assert bits(np.array([uf]))[0] == bits(np.array([uf_ref]))[0]              # Ufin: slot 0 at step T
        assert np.all(np.isfinite(U)) and np.all(np.isfinite(Z)) and np.isfinite(uf)
        assert np.all(U > 0.0) and np.all(U <= 1.0) and 0.0 < uf <= 1.0
        err = np.abs(Z.astype(np.longdouble) - Z_ref[..., :nw]) / np.maximum(1.0, R_ref[..., :nw])
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= Z_BOUND, (nw, float(err.max()))
    print(f"philox seed={seed:#x} k_iter={k_iter}: max |dZ|/max(1,r) = {worst:.3e}")
    if k_iter == 0:                                 # the public wrapper sees the same stream
        rep = rbpf.PhiloxRNG(seed).replay(N, T, 6)
        np.testing.assert_array_equal(bits(rep.U[0]), bits(U_ref))
        assert bits(rep.Ufin)[0] == bits(np.array([uf_ref]))[0]


@pytest.mark.parametrize("seed", [1, 0xDEADBEEFCAFEF00D])
def test_counters_do_not_depend_on_the_sizes_of_the_call(rbpf, seed):
    """(N, T, nw) = (300, 4, 6) and (7, 9, 6) agree where they overlap (slots 0..6, steps 1..3); the first nw' < nw normals
    of a slot are the same numbers."""
    Ua, Za, _ = fill(rbpf, seed, 0, 300, 4, 6)
    Ub, Zb, ufb = fill(rbpf, seed, 0, 7, 9, 6)
    np.testing.assert_array_equal(bits(Ua[:3, :7]), bits(Ub[:3, :7]))
    np.testing.assert_array_equal(bits(Za[:3, :7]), bits(Zb[:3, :7]))
    assert ufb == P.uniform2(seed, 0, 9, 0, 0)[0]
    for t in range(4, 9):                                                          # steps only the long call has
        assert Ub[t - 1, 6] == P.uniform2(seed, 6, t, 0, 0)[0]
    _, Z8, _ = fill(rbpf, seed, 0, 300, 4, 8)
    for nw in (1, 3, 6):
        _, Zn, _ = fill(rbpf, seed, 0, 300, 4, nw)
        np.testing.assert_array_equal(bits(Zn), bits(Z8[..., :nw]))
