"""Localisation in the fixed map of a generic device-code model (rbpf.DeviceMap, rbpf_loc_generic_*): everything that holds
without a device -- the prototypes, the unchanged ABI, the refusals that come before any device is touched, the factorisation of
from_posterior, and the condition on the GPU tests' full-run cases (tests/device_map_ref.py): the float64 and the long-double
restatement draw identical ancestors at every step, so "indices exact" is a fair demand of the device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

import device_map_ref as dm
import generic_ny_cases as gc
from test_generic_device_cpu import ABI9_SIZES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rbpf_loc_generic_create", "rbpf_loc_generic_layout", "rbpf_loc_generic_ancestors_device", "rbpf_loc_generic_step_device",
       "rbpf_loc_generic_weights"]


def _ffi(rbpf):
    return importlib.import_module(rbpf.__name__ + "._ffi")


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _never(*a):
    raise AssertionError("a handle was called")


def test_prototypes_are_declared_exported_and_mirrored(rbpf):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rbpf.h")).read(), flags=re.S)
    lib = rbpf.load_library()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in rbpf.EXPORTS
        assert getattr(lib, name).argtypes is not None, name
    assert hasattr(rbpf, "DeviceMap") and hasattr(rbpf, "device_map_weights")


def test_abi_is_9_and_no_struct_changed_size(rbpf):
    lib = rbpf.load_library()
    assert lib.rbpf_abi_version() == 9
    assert [lib.rbpf_abi_sizeof(w) for w in range(len(ABI9_SIZES))] == ABI9_SIZES
    assert lib.rbpf_abi_sizeof(len(ABI9_SIZES)) == -1


class _Args:
    """Valid arguments of rbpf_loc_generic_create at (n_nonlin, n_y, n_lin) = (3, 2, 5), N_P = 4, N_T = 3; fields are replaced per test."""

    def __init__(self, rbpf, **kw):
        ffi = _ffi(rbpf)
        self.nN, self.d, self.n, self.N, self.T, self.cols = 3, 2, 5, 4, 3, 1
        self.mean, self.V, self.R = np.zeros(5), np.asfortranarray(np.eye(5)), np.asfortranarray(gc.full_R(2, 1))
        self.y, self.x0 = np.zeros((3, 2), order="F"), np.zeros((3, 1), order="F")
        self.U = np.full((1, 2, 4), 0.5)
        self.rng = ffi.rbpf_rng()
        self.rng.mode, self.rng.n_iter, self.rng.U = ffi.RBPF_RNG_REPLAY, 1, _dp(self.U)
        self.opt = ffi.rbpf_options(keep_history=1)
        self.null = set()
        for k, v in kw.items():
            setattr(self, k, v)

    def call(self, lib):
        ctx = C.c_void_p()
        p = lambda name: None if name in self.null else _dp(getattr(self, name))              # noqa: E731
        st = lib.rbpf_loc_generic_create(self.nN, self.d, self.n, p("mean"), p("V"), p("R"), self.N, self.T, p("y"), p("x0"), self.cols,
                                         None if "rng" in self.null else C.byref(self.rng), C.byref(self.opt),
                                         None if "ctx" in self.null else C.byref(ctx))
        assert not ctx.value or st == 0
        if ctx.value:
            lib.rbpf_destroy(ctx)
        return st


def test_null_arguments_are_invalid_before_a_device_is_needed(rbpf):
    lib = rbpf.load_library()
    for name in ("mean", "V", "R", "y", "x0", "rng", "ctx"):
        assert _Args(rbpf, null={name}).call(lib) == rbpf.RBPF_ERR_INVALID_ARG, name
    ldx, p1, p2 = C.c_int32(0), C.c_void_p(), C.c_void_p()
    assert lib.rbpf_loc_generic_layout(None, C.byref(ldx)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_generic_ancestors_device(None, C.byref(p1), C.byref(p2)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_generic_step_device(None, None, None, 0) == rbpf.RBPF_ERR_INVALID_ARG
    a = _Args(rbpf)
    dy = np.zeros((4, 2, 5))
    out = np.zeros(64)
    args = lambda dyp, layout: (2, 5, 4, dyp, layout, 0, _dp(a.mean), _dp(a.V), _dp(a.R), _dp(np.zeros(2)), _dp(out), None, None, 1, None)   # noqa: E731
    assert lib.rbpf_loc_generic_weights(*args(None, 2)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_loc_generic_weights(*args(_dp(dy), 3)) == rbpf.RBPF_ERR_INVALID_ARG


@pytest.mark.parametrize("field,value", [("d", 0), ("d", 9), ("n", 0), ("n", 1152), ("nN", 0), ("nN", 9), ("N", 0), ("T", 0), ("cols", 2)])
def test_sizes_out_of_range_are_refused(rbpf, field, value):
    st = _Args(rbpf, **{field: value}).call(rbpf.load_library())
    assert st in (rbpf.RBPF_ERR_INVALID_ARG, rbpf.RBPF_ERR_UNSUPPORTED)
    assert st == (rbpf.RBPF_ERR_UNSUPPORTED if value in (9, 1152) else rbpf.RBPF_ERR_INVALID_ARG)


def test_an_r_that_is_not_positive_definite_is_refused_at_creation(rbpf):
    lib = rbpf.load_library()
    R = np.asfortranarray(np.array([[1.0, 2.0], [2.0, 1.0]]))
    assert _Args(rbpf, R=R).call(lib) == rbpf.RBPF_ERR_CHOL_FAILED
    assert b"R must be positive definite" in lib.rbpf_last_error()
    a = _Args(rbpf)
    st = lib.rbpf_loc_generic_weights(2, 5, 4, _dp(np.zeros((4, 2, 5))), 2, 0, _dp(a.mean), _dp(a.V), _dp(R), _dp(np.zeros(2)), None, None,
                                      _dp(np.zeros(4)), 1, None)
    assert st == rbpf.RBPF_ERR_CHOL_FAILED


@pytest.mark.parametrize("field", ["lazy_depth", "n_devices", "inplace", "storage", "fix_p_mean", "chol_refresh"])
def test_foreign_options_are_unsupported(rbpf, field):
    a = _Args(rbpf)
    setattr(a.opt, field, 2)
    assert a.call(rbpf.load_library()) == rbpf.RBPF_ERR_UNSUPPORTED


def test_from_posterior_factors_p_and_refuses_an_indefinite_one(rbpf):
    rs = np.random.RandomState(0)
    n = 23
    B = rs.standard_normal((n, n))
    P = B @ B.T / n + 0.1 * np.eye(n)
    h = rbpf.DeviceHandles(_never, _never)
    mp = rbpf.DeviceMap.from_posterior(h, rs.standard_normal(n), P, gc.full_R(3, 1))
    assert np.array_equal(mp.V, np.tril(mp.V)) and mp.nLin == n and mp.ny == 3
    assert np.max(np.abs(mp.V.T @ mp.V - P)) <= 1e-12 * np.max(np.abs(P))
    mag = rbpf.DenseMagMap.from_posterior(rbpf.DenseMagModel(*reversed(rbpf.domain_cartesian_dx(n - 3, 3, [[-1, -1, -1], [1, 1, 1]]))),
                                          np.zeros(n), P, 1.0)
    np.testing.assert_array_equal(mag.V, mp.V)                            # one factorisation, shared
    P[0, 0] = -1.0
    with pytest.raises(ValueError):
        rbpf.DeviceMap.from_posterior(h, np.zeros(n), P, np.eye(3))
    with pytest.raises(TypeError):
        rbpf.DeviceMap(object(), np.zeros(n), np.eye(n), np.eye(3))
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.DeviceMap(rbpf.DeviceSparseHandles(_never, _never), np.zeros(n), np.eye(n), np.eye(3))
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED


def test_without_a_device_the_run_raises_no_device(rbpf):
    if rbpf.device_count() > 0:
        pytest.skip("a GPU is visible")
    m, p = dm.case((3, 3, 3, 2, 5), 4, 3)
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(_never, _never), p["mean"], p["V"], p["R"])
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilterLocalization(mp, None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
    assert _Args(rbpf).call(rbpf.load_library()) == rbpf.RBPF_ERR_NO_DEVICE
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.device_map_weights(np.zeros((4, 2, 5)), np.zeros(5), np.eye(5), np.eye(2), np.zeros(2))
    assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE


def test_smoothing_in_a_device_map_is_refused_with_the_reason(rbpf):
    m, p = dm.case((3, 3, 3, 2, 5), 4, 3)
    mp = rbpf.DeviceMap(rbpf.DeviceHandles(_never, _never), p["mean"], p["V"], p["R"])
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherLocalization(mp, None, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], 4, p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "transition density" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                             # a mixed pair
        rbpf.particleFilterLocalization(mp, _never, p["odometry"], p["y"], p["x0_nonLin"], p["Q"], p["R"], p["N_P"], p["dt"])
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


def test_the_restatement_equals_the_dense_formula():
    """weights() against H P H' + R formed directly and numpy's own Cholesky: the restatement is what section 1 says."""
    rs = np.random.RandomState(2)
    N, d, n = 7, 3, 11
    H, V, mean, y = rs.standard_normal((N, d, n)), np.tril(rs.standard_normal((n, n))), rs.standard_normal(n), rs.standard_normal(d)
    R = gc.full_R(d, 2)
    yhat, S, logw = dm.weights(H, mean, V, R, y)
    P = V.T @ V
    for i in range(N):
        Si = H[i] @ P @ H[i].T
        assert np.max(np.abs(S[i] - Si)) < 1e-12 * np.max(np.abs(Si))
        L = np.linalg.cholesky(Si + R)
        z = np.linalg.solve(L, y - H[i] @ mean)
        want = -np.sum(np.log(np.diag(L))) - 0.5 * z @ z - 0.5 * d * np.log(2 * np.pi)
        assert abs(logw[i] - want) < 1e-11 * abs(want)


@pytest.mark.parametrize("i", range(len(dm.FULL_RUNS)), ids=lambda i: "ny%d_n%d" % dm.FULL_RUNS[i][0][3:5])
def test_float64_and_long_double_draw_the_same_ancestors(i):
    m, p, ref = dm.full_run(i)
    ld = dm.run(m, p, dtype=np.longdouble)
    np.testing.assert_array_equal(ref["ai"], ld["ai"])
    assert not ref["degenerate"].any()
    assert len(np.unique(ref["ai"][1:])) > 1                                # the draws are not trivial
    e_ref = float(np.max(np.abs(ref["w"] - ld["w"].astype(np.float64))) / np.max(ref["w"]))
    print("restatement's own error |fp64 - long double| on the weights:", e_ref)
    assert e_ref < 1e-10
