"""CPU: the numpy oracle's particleFilter on the no-noise synthetic model of tests/generic_model.py against the
extended-precision batch posterior (generic_model.batch_posterior), at the shapes tests/test_gpu_generic_shapes.py runs the
device's generic family at.  The oracle is the reference of those GPU tests; this pins its own agreement with an answer that
does not restate the filter."""
import numpy as np
import pytest

import generic_model as gm
import rbpf_oracle as O


@pytest.mark.parametrize("shape,N_T", [((4, 3, 4, 3, 256), 150), ((2, 1, 2, 1, 128), 150), ((6, 4, 6, 3, 639), 120),
                                       ((3, 3, 3, 3, 1151), 100)])
def test_oracle_filter_equals_the_long_double_batch_posterior(shape, N_T):
    """No process noise, one x0_lin column: every particle follows the same path, so the final xl / P of every particle are
    the batch posterior and the summed log-weights the log marginal likelihood, to the conditioning bound of kat_tolerance."""
    N_P = 2
    m, p, ref = gm.kat_case(shape, N_P, N_T)
    out = O.particleFilter(m, p["odometry"], p["y"], p["x0_nonLin"], p["x0_lin"], p["P0_lin"], p["Q"], p["R"], N_P, p["dt"],
                           O.ReplayRNG(p["U"], p["Z"]), trace=True)
    np.testing.assert_array_equal(out["xn_traj"], np.repeat(gm.path_of(m, p)[:, None, :], N_P, axis=1))
    tol = gm.kat_tolerance(ref, N_T)
    assert tol < 1e-9                                                    # the problems are well conditioned (kappa ~ 1e3)
    xl, P, ll = ref["xl"].astype(np.float64), ref["P"].astype(np.float64), float(ref["loglik"])
    xscale = np.max(np.abs(xl)) + np.max(np.abs(xl - p["x0_lin"]))
    assert np.max(np.abs(P - p["P0_lin"])) > 0.1 * ref["P0max"]          # the data moved the map: not a trivial answer
    tr = out["trace"]
    for i in range(N_P):
        assert np.max(np.abs(tr["xl"][:, i] - xl)) <= tol * xscale
        assert np.max(np.abs(tr["P"][:, :, i] - P)) <= tol * ref["P0max"]
        assert abs(float(np.sum(tr["logw"][:, i])) - ll) <= tol * (abs(ll) + ref["M"])


def test_long_double_reference_is_not_fp64():
    """The reference really carries more than 53 bits: the same batch formulas in fp64 differ from it by more than the
    long-double rounding and far less than the tolerance (a reference that agreed to the last bit with fp64 arithmetic
    would not be an independent answer)."""
    m, p, ref = gm.kat_case((2, 1, 2, 1, 128), 2, 150)
    assert np.finfo(gm.LD).eps < 1e-18
    Phi = m.measModel(gm.path_of(m, p)).reshape(-1, m.nLin)
    C = Phi @ p["P0_lin"] @ Phi.T + np.kron(np.eye(150), p["R"])
    V = np.linalg.solve(np.linalg.cholesky(C), Phi @ p["P0_lin"])
    P64 = p["P0_lin"] - V.T @ V
    d = np.max(np.abs(P64 - ref["P"].astype(np.float64)))
    assert 0.0 < d <= gm.kat_tolerance(ref, 150) * ref["P0max"]
