"""The device entry points of the generic family (rbpf_filter_external_layout, rbpf_filter_ancestors_device,
rbpf_filter_step_device, rbpf_filter_set_device_callbacks) are additions to ABI 9: declared in include/rbpf.h with the
prototypes below, exported by the built library, no interface struct changed, and a NULL context is refused before anything
touches a device.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "rbpf_filter_external_layout": "int rbpf_filter_external_layout(const rbpf_ctx* ctx, int32_t* ldx);",
    "rbpf_filter_ancestors_device":
        "int rbpf_filter_ancestors_device(rbpf_ctx* ctx, const int32_t** ai_dev, const double** xn_anc_dev);",
    "rbpf_filter_step_device":
        "int rbpf_filter_step_device(rbpf_ctx* ctx, const double* xn_new_dev, const double* dy_dev, int32_t dy_layout);",
    "rbpf_filter_set_device_callbacks":
        "int rbpf_filter_set_device_callbacks(rbpf_ctx* ctx, const rbpf_callbacks* callbacks, int32_t dy_layout);",
}
# rbpf_abi_sizeof(0..13) of ABI 9 (rbpf_model, rbpf_problem, rbpf_rng, rbpf_options, rbpf_filter_out, rbpf_smoother_out,
# rbpf_timing, rbpf_callbacks, rbpf_view, rbpf_loc_map, rbpf_loc_problem, rbpf_loc_out, rbpf_ekf_problem, rbpf_ekf_out)
ABI9_SIZES = [80, 112, 40, 96, 120, 64, 32, 32, 16, 72, 72, 72, 112, 32]


def _header():
    src = open(os.path.join(ROOT, "include", "rbpf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_entry_point_is_declared_exported_and_mirrored(rbpf, name):
    assert PROTOTYPES[name] in _header()
    assert hasattr(rbpf.load_library(), name)
    assert name in rbpf.EXPORTS


def test_abi_version_and_struct_sizes_are_unchanged(rbpf):
    lib = rbpf.load_library()
    assert lib.rbpf_abi_version() == 9
    assert re.search(r"#define RBPF_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "rbpf.h")).read()).group(1) == "9"
    assert [lib.rbpf_abi_sizeof(w) for w in range(len(ABI9_SIZES))] == ABI9_SIZES
    assert lib.rbpf_abi_sizeof(len(ABI9_SIZES)) == -1


def test_null_context_is_an_invalid_argument(rbpf):
    """Checked before anything touches a device: holds on a machine without one."""
    lib = rbpf.load_library()
    ffi = __import__("importlib").import_module(rbpf.__name__ + "._ffi")
    ldx, p, q = C.c_int32(0), C.c_void_p(), C.c_void_p()
    buf = (C.c_double * 4)()
    addr = C.c_void_p(C.addressof(buf))
    cb = ffi.rbpf_callbacks()
    cb.dyn_model = ffi.DYN_MODEL_FN(lambda *a: 0)
    cb.meas_model = ffi.MEAS_MODEL_FN(lambda *a: 0)
    assert lib.rbpf_filter_external_layout(None, C.byref(ldx)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_filter_ancestors_device(None, C.byref(p), C.byref(q)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_filter_step_device(None, addr, addr, 0) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_filter_set_device_callbacks(None, C.byref(cb), 0) == rbpf.RBPF_ERR_INVALID_ARG
    assert b"NULL" in lib.rbpf_last_error()


def test_device_handles_are_refused_outside_the_single_gpu_filter(rbpf):
    """Smoothers and sharded sessions: RBPF_ERR_UNSUPPORTED with a message that says so, before any device is touched."""
    h = rbpf.DeviceHandles(lambda xn, dx, dt, Q: xn, lambda xn: xn)
    import numpy as np
    a = (np.zeros((2, 1)), np.zeros((3, 1)), np.zeros(1), np.zeros(1), np.eye(1), np.eye(1), np.eye(1), 4)
    for call in (lambda: rbpf.particleSmoother(h, None, None, *a, 2, 1.0),
                 lambda: rbpf.particleSmootherInformationForm(h, None, None, *a, 2, 1.0),
                 lambda: rbpf.particleFilter(h, None, *a, 1.0, n_devices=2)):
        with pytest.raises(rbpf.RBPFError) as ei:
            call()
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceHandles" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.DeviceHandles(lambda *a: 0, lambda *a: 0, dy_layout=7)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
