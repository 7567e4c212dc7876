"""GPU: every instantiation of the transition term GsTerm<NR, ANG, QP> that gs_pick can select (16 Gaussian, 9 with a quaternion
block), through the one-step probes rbpf.device_map_backward_step (backward_logp_kernel; backward_pass_kernel + backward_locate_kernel)
and rbpf.device_map_map_step (viterbi_pass_kernel + merge), on the 25 layouts of tests/transition_sweep_ref.py at 300 x 70, against
the existing restatements (tests/device_map_smoother_ref.py, pose_transition_ref.py, map_trajectory_ref.py).

Tolerances: logp 1e-9 of max |logp|, the TOL of tests/test_gpu_device_map_smoother.py for this arithmetic class; best 1e-9
max(1, |best|) as tests/test_gpu_map_trajectory.py; indices and arg exact.  tests/test_transition_sweep_cpu.py asserts what makes
exact indices a fair demand of every input used here (every draw 100 eps_ref from a cdf edge, every near-best set a singleton) and
that far_first / far_last put their displaced pairs before / behind each term's skip test.  The clamped-draw counter is not part
of the probes and is not checked.

Measured on an MI355X: 25 of 25 layouts compared; largest logp error 1.2e-14 of max |logp| (g1a), largest best error 2.1e-14
(p4a, 74 MAP steps: 25 base, 49 far); every index and arg equal."""
import numpy as np
import pytest

import transition_sweep_ref as T

pytestmark = pytest.mark.gpu

TOL = 1e-9


def _backward(rbpf, p, **kw):
    a = dict(T.probe_args(p), w=p["w"], u=p["u"])
    a.update(kw)
    return rbpf.device_map_backward_step(**a)


def _check_map_step(rbpf, p, o, label):
    """The _check_step of tests/test_gpu_map_trajectory.py with the cap at 0: arg equals the one member of every near-best set."""
    best, arg, _ = rbpf.device_map_map_step(delta=p["delta"], **T.probe_args(p))
    assert best.shape == (T.M,) and arg.shape == (T.M,)
    want = o["best"]
    assert np.all(np.isfinite(best))
    err = float(np.max(np.abs(best.astype(np.longdouble) - want) / np.maximum(1.0, np.abs(want))))
    print(f"best {label}: device vs long double {err:.2e}")
    assert err < TOL
    assert all(n.size == 1 for n in o["near"])
    np.testing.assert_array_equal(arg, [n[0] for n in o["near"]])
    np.testing.assert_array_equal(arg, o["arg"])
    return arg


@pytest.mark.parametrize("name", T.NAMES)
def test_logp(rbpf, name):
    p, o = T.inputs(name), T.reference(name)
    _, logp, _ = _backward(rbpf, p, want_logp=True)
    want = o["logp_ld"]
    assert logp.shape == (T.N, T.M)
    err = float(np.max(np.abs(logp.astype(np.longdouble) - want)) / np.max(np.abs(want)))
    print(f"logp {name} {T.layout(name).type}: device vs long double {err:.2e}")
    assert err <= TOL


@pytest.mark.parametrize("name", T.NAMES)
def test_indices(rbpf, name):
    p, o = T.inputs(name), T.reference(name)
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    index, _, _ = _backward(rbpf, p)
    np.testing.assert_array_equal(index, o["index"])                       # every draw
    for u in (2.0 ** -60, 1.0 - 2.0 ** -53):
        index, _, _ = _backward(rbpf, p, u=np.full(T.M, u))
        assert np.all(index >= 0) and np.all(index < T.N) and np.all(p["w"][index] > 0)


@pytest.mark.parametrize("name", T.NAMES)
def test_map_step(rbpf, name):
    _check_map_step(rbpf, T.inputs(name), T.reference(name), name)


@pytest.mark.parametrize("name,variant", T.FAR_CASES)
def test_displaced_pairs_leave_no_trace(rbpf, name, variant):
    """far_first: the pairs of every second live predecessor fall to the skip test; far_last: they pass it and vanish through exp
    (in the MAP pass: through the comparison with the running best).  A test on a sum that is not yet final, or none, fails one."""
    p, o = T.inputs(name, variant), T.reference(name, variant)
    np.testing.assert_array_equal(o["index"], o["index_ld"])
    index, _, _ = _backward(rbpf, p)
    np.testing.assert_array_equal(index, o["index"])
    assert not np.any(np.isin(index, p["displaced"]))
    arg = _check_map_step(rbpf, p, o, f"{name} {variant}")
    assert not np.any(np.isin(arg, p["displaced"]))
