"""CPU: the C ABI and the Python surface of the sparseFeatures branch with device handles (RBPF_MODEL_GENERIC_SPARSE,
rbpf.DeviceSparseHandles): what can be checked without a device."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    "rbpf_filter_sparse_gathered_device": "(rbpf_ctx* ctx, const double** xl_dev, int32_t* ldx)",
    "rbpf_filter_step_sparse_device": "(rbpf_ctx* ctx, const double* xn_new_dev, const double* yhat_dev, int32_t yhat_layout, "
                                      "const double* dy_dev, int32_t dy_layout)",
    "rbpf_filter_sparse_yhattraj": "(rbpf_ctx* ctx, double* yhattraj)",
}
# sizeof of every struct of include/rbpf.h in the order of rbpf_abi_sizeof(which), as of ABI 9: this family changes none
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
    assert "RBPF_MODEL_GENERIC_SPARSE = 5" in header and _ffi(rbpf).RBPF_MODEL_GENERIC_SPARSE == 5


def test_a_null_context_is_refused(rbpf):
    lib = rbpf.load_library()
    p, ldx = C.c_void_p(), C.c_int32(0)
    some = (C.c_double * 8)()
    assert lib.rbpf_filter_sparse_gathered_device(None, C.byref(p), C.byref(ldx)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_filter_step_sparse_device(None, some, some, 2, some, 2) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_filter_sparse_yhattraj(None, some) == rbpf.RBPF_ERR_INVALID_ARG
    assert b"NULL" in lib.rbpf_last_error()


def test_abi_version_and_struct_sizes_are_unchanged(rbpf):
    lib = rbpf.load_library()
    assert lib.rbpf_abi_version() == 9 == _ffi(rbpf).ABI_VERSION
    assert [lib.rbpf_abi_sizeof(w) for w in range(len(ABI9_SIZES))] == ABI9_SIZES
    assert lib.rbpf_abi_sizeof(len(ABI9_SIZES)) == -1


def test_device_sparse_handles_validate_their_arguments(rbpf):
    h = rbpf.DeviceSparseHandles(_never, _never)
    assert isinstance(h, rbpf.DeviceHandles) and not isinstance(h, rbpf.DeviceSmootherHandles)
    assert h.dy_layout is None and h.native_out is False
    for bad in ((None, _never), (_never, 3)):
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.DeviceSparseHandles(*bad)
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
    m = rbpf.GenericSparseModel(3, 6, 4, 3, 3)
    d = m.descriptor()
    assert d.kind == 5 and not d.callbacks and m.sparse and (m.nNonLin, m.nLin, m.ny, m.nw, m.n_odo) == (3, 6, 4, 3, 3)


@pytest.mark.parametrize("smoother", ["particleSmoother", "particleSmootherInformationForm"])
def test_the_smoothers_refuse_them_before_a_device_is_touched(rbpf, smoother):
    h = rbpf.DeviceSparseHandles(_never, _never)
    with pytest.raises(rbpf.RBPFError) as ei:
        getattr(rbpf, smoother)(h, None, None, *_args()[:8], 2, 1.0, True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "smoother" in str(ei.value)


def test_sharding_and_the_dense_convention_refuse_them_before_a_device_is_touched(rbpf):
    h = rbpf.DeviceSparseHandles(_never, _never)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilter(h, None, *_args(), True, n_devices=2)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "n_devices" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleFilter(h, None, *_args(), False)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG and "sparseFeatures" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                                 # a plain DeviceHandles stays refused as it was
        rbpf.particleFilter(rbpf.DeviceHandles(_never, _never), None, *_args(), True)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "sparse-visual family only" in str(ei.value)
