"""rbpf.DeviceSmootherHandles and the two entry points behind it (rbpf_particle_smoother_device,
rbpf_ext_pack_whiten_probe): argument validation, the class relation the filter relies on, the prototypes of include/rbpf.h
against the ctypes mirror, and the refusals that come before anything touches a device.  No GPU needed."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOTYPES = {
    "rbpf_particle_smoother_device":
        "int rbpf_particle_smoother_device(const rbpf_model* model, const rbpf_problem* prob, const rbpf_rng* rng, "
        "const rbpf_options* opt, int32_t N_K, int32_t info_form, const rbpf_callbacks* device_callbacks, int32_t dy_layout, "
        "rbpf_smoother_out* out);",
    "rbpf_ext_pack_whiten_probe":
        "int rbpf_ext_pack_whiten_probe(int32_t dy_layout, int32_t rows, int32_t d, int32_t n, const double* dy_host, "
        "const double* W_host, int32_t fused, double* G_host);",
}


def _header():
    src = open(os.path.join(ROOT, "include", "rbpf.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def _ctype(ffi, text):
    """The ctypes type a parameter of the header is mirrored by."""
    text = text.strip()
    structs = {"rbpf_model": ffi.rbpf_model, "rbpf_problem": ffi.rbpf_problem, "rbpf_rng": ffi.rbpf_rng, "rbpf_options": ffi.rbpf_options,
               "rbpf_callbacks": ffi.rbpf_callbacks, "rbpf_smoother_out": ffi.rbpf_smoother_out}
    m = re.match(r"(?:const )?(\w+)(\*?) \w+$", text)
    base, ptr = m.group(1), m.group(2)
    if base in structs:
        assert ptr
        return C.POINTER(structs[base])
    scalar = {"int32_t": C.c_int32, "double": C.c_double}[base]
    return C.POINTER(scalar) if ptr else scalar


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_entry_point_is_declared_exported_and_mirrored(rbpf, name):
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    header = _header()
    assert PROTOTYPES[name] in header
    lib = rbpf.load_library()
    assert hasattr(lib, name) and name in rbpf.EXPORTS
    params = re.search(re.escape(name) + r"\((.*?)\);", header).group(1).split(",")
    assert list(getattr(lib, name).argtypes) == [_ctype(ffi, t) for t in params]


def test_device_smoother_handles_validate_their_arguments(rbpf):
    ok = lambda *a: 0                                                     # noqa: E731
    h = rbpf.DeviceSmootherHandles(ok, ok)
    assert isinstance(h, rbpf.DeviceHandles)
    assert h.dy_layout == 0 and h.native_out is False and h.dynResNorm is None
    assert rbpf.DeviceSmootherHandles(ok, ok, ok, dy_layout=1, native_out=True).dynResNorm is ok
    assert rbpf.DeviceSmootherHandles(ok, ok, []).dynResNorm is None       # isempty(dynResNorm)
    for bad in (lambda: rbpf.DeviceSmootherHandles(1, ok), lambda: rbpf.DeviceSmootherHandles(ok, None),
                lambda: rbpf.DeviceSmootherHandles(ok, ok, 3), lambda: rbpf.DeviceSmootherHandles(ok, ok, dy_layout=7),
                lambda: rbpf.DeviceSmootherHandles(ok, ok, dy_layout=None)):
        with pytest.raises(rbpf.RBPFError) as ei:
            bad()
        assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG


def test_refusals_come_before_any_device(rbpf):
    ok = lambda *a: 0                                                     # noqa: E731
    h = rbpf.DeviceSmootherHandles(ok, ok)
    a = (np.zeros((2, 1)), np.zeros((3, 1)), np.zeros(1), np.zeros(1), np.eye(1), np.eye(1), np.eye(1), 4)
    for call in (lambda: rbpf.particleSmootherInformationForm(h, None, None, *a, 2, 1.0, n_devices=2),
                 lambda: rbpf.particleSmootherInformationForm(h, None, None, *a, 2, 1.0, sparseFeatures=True),
                 lambda: rbpf.particleSmoother(h, None, None, *a, 2, 1.0, sparseFeatures=True)):
        with pytest.raises(rbpf.RBPFError) as ei:
            call()
        assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceSmootherHandles" in str(ei.value)
    with pytest.raises(rbpf.RBPFError) as ei:                              # the object replaces all three handles
        rbpf.particleSmoother(h, ok, None, *a, 2, 1.0)
    assert ei.value.status == rbpf.RBPF_ERR_INVALID_ARG
    # a plain DeviceHandles is still refused, and is told where to go
    with pytest.raises(rbpf.RBPFError) as ei:
        rbpf.particleSmoother(rbpf.DeviceHandles(ok, ok), None, None, *a, 2, 1.0)
    assert ei.value.status == rbpf.RBPF_ERR_UNSUPPORTED and "DeviceSmootherHandles" in str(ei.value)


def test_c_entry_points_check_their_arguments_first(rbpf):
    ffi = importlib.import_module(rbpf.__name__ + "._ffi")
    lib = rbpf.load_library()
    out = ffi.rbpf_smoother_out()
    cb = ffi.rbpf_callbacks()
    keep = (ffi.DYN_MODEL_FN(lambda *a: 0), ffi.MEAS_MODEL_FN(lambda *a: 0))
    cb.dyn_model, cb.meas_model = keep
    mdl = ffi.rbpf_model(kind=ffi.RBPF_MODEL_GENERIC_DENSE)
    opt = ffi.rbpf_options(n_devices=2)
    assert lib.rbpf_particle_smoother_device(C.byref(mdl), None, None, C.byref(opt), 2, 1, None, 0, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_particle_smoother_device(C.byref(mdl), None, None, C.byref(opt), 2, 1, C.byref(cb), 3, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_particle_smoother_device(C.byref(mdl), None, None, C.byref(opt), 0, 1, C.byref(cb), 0, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    mag = ffi.rbpf_model(kind=ffi.RBPF_MODEL_DENSE_MAG_6D)
    assert lib.rbpf_particle_smoother_device(C.byref(mag), None, None, C.byref(opt), 2, 1, C.byref(cb), 0, C.byref(out)) == rbpf.RBPF_ERR_INVALID_ARG
    assert lib.rbpf_particle_smoother_device(C.byref(mdl), None, None, C.byref(opt), 2, 1, C.byref(cb), 0, C.byref(out)) == rbpf.RBPF_ERR_UNSUPPORTED
    assert b"one GPU" in lib.rbpf_last_error()
    sp = C.c_void_p()
    assert lib.rbpf_stream_get(None, C.byref(sp)) == rbpf.RBPF_ERR_INVALID_ARG      # no device callback is running
    if rbpf.device_count() == 0:
        with pytest.raises(rbpf.RBPFError) as ei:
            rbpf.pack_whiten_probe(np.zeros((1, 1, 1)), np.eye(1))
        assert ei.value.status == rbpf.RBPF_ERR_NO_DEVICE
