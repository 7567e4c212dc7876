"""CPU: the C ABI and the Python surface of the covariance-form smoother's sparseFeatures branch with device handles
(rbpf_particle_smoother_sparse_device, rbpf.DeviceSparseSmootherHandles): what can be checked without a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rbpf_particle_smoother_sparse_device": "(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng, "
                                            "const rbpf_options* opt, int32_t N_K, rbpf_sparse_dyn_fn dyn_model, "
                                            "rbpf_sparse_meas_fn meas_model, rbpf_sparse_dyn_res_norm_fn dyn_res_norm, void* user, "
                                            "int32_t yhat_layout, int32_t dy_layout, int32_t max_future_per_call, "
                                            "rbpf_smoother_out* out)",
    "rbpf_sparse_smoother_timing": "(int32_t enable, double* build_ms, double* chol_ms, int64_t* steps)",
    "rbpf_sparse_ext_build_probe": "(int32_t N, int32_t n, int32_t M, int32_t d, const double* P_dev, const double* D_dev, "
                                   "const int32_t* pair_t_dev, const int32_t* pair_j_dev, const double* R_dev, int32_t reps, "
                                   "double* S_dev, double* ms)",
}
MEAS_TYPEDEF = ("typedef int (*rbpf_sparse_meas_fn)(void* user, int32_t n_cols, const double* xn, const double* xl, int32_t ldx, "
                "double* yhat, double* dy);")
# sizeof of every struct of include/rbpf.h in the order of rbpf_abi_sizeof(which), as of ABI 9: this entry point changes none
ABI9_SIZES = [80, 112, 40, 96, 120, 64, 32, 32, 16, 72, 72, 72, 112, 32]


def _ffi(rbpf):
    return importlib.import_module(rbpf.__name__ + "._ffi")


def _args(n=6, d=4, N=5, T=3):
    return (np.zeros((T - 1, 3)), np.zeros((T, d)), np.zeros(3), np.zeros(n), np.eye(n), 0.01 * np.eye(3), np.eye(d), N, 1.0)


def _never(*a):
    raise AssertionError("a refused run called a handle")


def test_entry_points_are_exported_with_their_prototypes(rbpf):
    lib = rbpf.load_library()
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rbpf.h")).read())
    for name, proto in NEW.items():
        assert hasattr(lib, name), name
        assert name in rbpf.EXPORTS
        assert f"int {name}{proto};" in header, name
        assert len(getattr(lib, name).argtypes) == proto.count(",") + 1
    assert MEAS_TYPEDEF in header


def _c_problem(rbpf, n=6, d=4, N=5, T=3):
    host = importlib.import_module(rbpf.__name__ + ".host")
    a = _args(n, d, N, T)
    model = rbpf.GenericSparseModel(3, n, d, 3, 3)
    prob = host._Problem(model, *a[:7], a[7], a[8])
    blk, keep = host._rng_block(rbpf.PhiloxRNG(1), N, T, 3, 2)
    return model.descriptor(), prob, blk, keep


def test_null_arguments_and_bad_layouts_are_refused_without_a_device(rbpf):
    lib, ffi = rbpf.load_library(), _ffi(rbpf)
    mdesc, prob, blk, _keep = _c_problem(rbpf)
    dyn = ffi.DYN_MODEL_FN(lambda *a: 1)
    meas = ffi.SPARSE_MEAS_MODEL_FN(lambda *a: 1)
    none_dyn, none_meas, none_drn = ffi.DYN_MODEL_FN(), ffi.SPARSE_MEAS_MODEL_FN(), ffi.DYN_RES_NORM_FN()
    out = ffi.rbpf_smoother_out()
    f = lib.rbpf_particle_smoother_sparse_device

    def call(model=C.byref(mdesc), p=C.byref(prob.c), rng=C.byref(blk), N_K=2, d=dyn, m=meas, yl=2, dl=2, mf=0, o=C.byref(out)):
        return f(model, p, rng, None, N_K, d, m, none_drn, None, yl, dl, mf, o)

    for kw in (dict(model=None), dict(p=None), dict(rng=None), dict(o=None), dict(d=none_dyn), dict(m=none_meas), dict(N_K=0)):
        assert call(**kw) == rbpf.RBPF_ERR_INVALID_ARG, kw
    for kw, word in ((dict(yl=1), b"yhat_layout"), (dict(yl=3), b"yhat_layout"), (dict(dl=3), b"dy_layout"), (dict(dl=-1), b"dy_layout"),
                     (dict(mf=-1), b"max_future_per_call")):
        assert call(**kw) == rbpf.RBPF_ERR_INVALID_ARG, kw
        assert word in lib.rbpf_last_error()
    dense = rbpf.GenericDenseModel(3, 6, 4, 3, 3).descriptor()                # another kind
    assert call(model=C.byref(dense)) == rbpf.RBPF_ERR_INVALID_ARG and b"RBPF_MODEL_GENERIC_SPARSE" in lib.rbpf_last_error()
    some = C.c_void_p(8)
    assert lib.rbpf_sparse_ext_build_probe(1, 4, 4, 2, None, some, some, some, some, 1, some, None) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_sparse_ext_build_probe(1, 97, 4, 2, some, some, some, some, some, 1, some, None) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_sparse_ext_build_probe(1, 4, 1024, 2, some, some, some, some, some, 1, some, None) == rbpf.RBPF_ERR_INVALID_ARG


def test_unsupported_options_and_sizes_are_refused_without_a_device(rbpf):
    """n_devices, storage, lazy_depth, inplace, n_y > 32, nLin > 96 and M > 1023: RBPF_ERR_UNSUPPORTED from the C entry point
    itself, whether or not a device is visible (no handle is called: they return an error)."""
    lib, ffi = rbpf.load_library(), _ffi(rbpf)
    dyn, meas, none_drn = ffi.DYN_MODEL_FN(_never), ffi.SPARSE_MEAS_MODEL_FN(_never), ffi.DYN_RES_NORM_FN()
    out = ffi.rbpf_smoother_out()
    f = lib.rbpf_particle_smoother_sparse_device
    mdesc, prob, blk, _keep = _c_problem(rbpf)
    for kw, word in ((dict(n_devices=2), b"n_devices"), (dict(storage=1), b"storage"), (dict(lazy_depth=2), b"lazy_depth"),
                     (dict(inplace=1), b"inplace")):
        opt = ffi.rbpf_options(keep_history=1, **kw)
        assert f(C.byref(mdesc), C.byref(prob.c), C.byref(blk), C.byref(opt), 2, dyn, meas, none_drn, None, 2, 2, 0,
                 C.byref(out)) == rbpf.RBPF_ERR_UNSUPPORTED, kw
        assert word in lib.rbpf_last_error()
    for (n, d, T), word in (((66, 33, 3), b"n_y must be 1 .. 32"), ((97, 4, 3), b"nLin must be 1 .. 96"), ((64, 32, 40), b"more than 1023")):
        mdesc, prob, blk, _keep = _c_problem(rbpf, n=n, d=d, T=T)
        assert f(C.byref(mdesc), C.byref(prob.c), C.byref(blk), None, 2, dyn, meas, none_drn, None, 2, 2, 0,
                 C.byref(out)) == rbpf.RBPF_ERR_UNSUPPORTED, (n, d, T)
        assert word in lib.rbpf_last_error()


def test_the_timing_switch_needs_no_device(rbpf):
    assert rbpf.sparse_smoother_timing(True) == dict(build_ms=0.0, chol_ms=0.0, steps=0)
    assert rbpf.sparse_smoother_timing(False) == dict(build_ms=0.0, chol_ms=0.0, steps=0)
    assert rbpf.load_library().rbpf_sparse_smoother_timing(0, None, None, None) == rbpf.RBPF_OK


def test_abi_version_and_struct_sizes_are_unchanged(rbpf):
    lib = rbpf.load_library()
    assert lib.rbpf_abi_version() == 9 == _ffi(rbpf).ABI_VERSION
    assert [lib.rbpf_abi_sizeof(w) for w in range(len(ABI9_SIZES))] == ABI9_SIZES
    assert lib.rbpf_abi_sizeof(len(ABI9_SIZES)) == -1


def test_the_new_class_validates_its_arguments(rbpf):
    h = rbpf.DeviceSparseSmootherHandles(_never, _never)
    assert isinstance(h, rbpf.DeviceSparseHandles) and not isinstance(h, rbpf.DeviceSmootherHandles)
    assert h.dynResNorm is None and h.future_chunk is None
    assert rbpf.DeviceSparseSmootherHandles(_never, _never, [], 3).future_chunk == 3
    assert rbpf.DeviceSparseSmootherHandles(_never, _never, _never).dynResNorm is _never
    for bad in ((None, _never), (_never, 3), (_never, _never, 5), (_never, _never, None, 0), (_never, _never, None, 1.5),
                (_never, _never, None, True)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.DeviceSparseSmootherHandles(*bad)
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG, bad


@pytest.mark.parametrize("smoother", ["particleSmoother", "particleSmootherInformationForm"])
def test_device_sparse_handles_are_still_refused_by_both_smoothers(rbpf, smoother):
    h = rbpf.DeviceSparseHandles(_never, _never)
    with pytest.raises(rbpf.RBPFError) as ei:
        getattr(rbpf, smoother)(h, None, None, *_args()[:8], 2, 1.0, True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "smoother" in str(ei.value)


def test_the_information_form_refuses_the_new_object_before_a_device_is_touched(rbpf):
    h = rbpf.DeviceSparseSmootherHandles(_never, _never)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmootherInformationForm(h, None, None, *_args()[:8], 2, 1.0, True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "particleSmoother" in str(ei.value) and "dense features" in str(ei.value)


def test_python_refusals_come_before_any_handle_call(rbpf):
    h = rbpf.DeviceSparseSmootherHandles(_never, _never)
    a = _args()
    cases = [
        (dict(sparse=False), "RBPF_ERR_INVALID_ARG", "sparseFeatures"),
        (dict(n_devices=2), "RBPF_ERR_UNSUPPORTED", "n_devices"),
        (dict(storage="fp32"), "RBPF_ERR_UNSUPPORTED", "storage"),
        (dict(lazy_depth=2), "RBPF_ERR_UNSUPPORTED", "lazy_depth"),
        (dict(inplace=1), "RBPF_ERR_UNSUPPORTED", "inplace"),
    ]
    for kw, status, word in cases:
        kw = dict(kw)
        sparse = kw.pop("sparse", True)
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.particleSmoother(h, None, None, *a[:8], 2, 1.0, sparse, **kw)
        assert ei.value.status == getattr(rbpf, status) and word in str(ei.value), (kw, str(ei.value))
    big = (np.zeros((39, 3)), np.zeros((40, 32)), np.zeros(3), np.zeros(64), np.eye(64), 0.01 * np.eye(3), np.eye(32), 4)
    with pytest.raises(rbpf.RBPFError) as ei:                                  # 39 x 32 = 1248 future observations at step 1
        rbpf.particleSmoother(h, None, None, *big, 2, 1.0, True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "more than 1023 future observations" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                                  # the object replaces all three handles
        rbpf.particleSmoother(h, _never, None, *a[:8], 2, 1.0, True)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
