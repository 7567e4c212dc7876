"""Problems of the synthetic family of tests/generic_model.py at measurement widths other than 1 and 3, with a FULL
symmetric positive definite R: generic_model.problem gives n_y != 3 a diagonal one, under which R^-1 and the innovation
Cholesky never see an off-diagonal term.  Here

    R = 0.01 B B' / n_y + 0.02 I,   B (n_y x n_y) standard normal from RandomState(3000 + seed)

(eigenvalues in [0.02, 0.02 + 0.01 |B|^2 / n_y]: the scale of the diagonal 0.03 I it replaces, so the y simulated under that
one stays plausible data).  The long-double known answer is built from this same R.  Shared by
tests/test_oracle_generic_ny_kat.py (CPU) and tests/test_gpu_generic_ny.py."""
import numpy as np

import generic_model as gm

# (n_nonlin, n_w, n_odo, n_y, nLin) -> N_T of the known-answer problems
KAT = {(3, 3, 3, 2, 64): 60, (3, 2, 3, 4, 129): 60, (4, 3, 4, 5, 200): 50, (3, 3, 3, 8, 256): 40}


def full_R(n_y, seed):
    B = np.random.RandomState(3000 + seed).standard_normal((n_y, n_y))
    return 0.01 * (B @ B.T) / n_y + 0.02 * np.eye(n_y)


def case(shape, N_P, N_T, N_K=1, seed=3, additive=False):
    """(model, problem) as test_gpu_generic_shapes.case, R replaced by full_R."""
    m = gm.GenericModel(*shape, seed=seed, additive=additive)
    p = gm.problem(m, N_P, N_T, N_K=N_K, seed=seed)
    p["R"] = full_R(m.ny, seed)
    return m, p


_KAT = {}


def kat_case(shape, N_P, N_T, seed=1):
    """generic_model.kat_case with the full R: (model, problem, long-double batch posterior), the answer computed once."""
    key = (tuple(shape), N_T, seed)
    if key not in _KAT:
        m = gm.GenericModel(*shape, seed=seed, noise=False)
        p0 = gm.problem(m, 1, N_T, seed=seed)
        p0["R"] = full_R(m.ny, seed)
        _KAT[key] = (m, p0, gm.batch_posterior(m, p0, gm.path_of(m, p0)))
    m, p0, ref = _KAT[key]
    rs = np.random.RandomState(seed)
    p = dict(p0, N_P=N_P, U=rs.random_sample((1, N_T - 1, N_P)), Z=np.zeros((1, N_T - 1, N_P, m.nw)), Ufin=None)
    return m, p, ref


def check_kat(ref, p, N_T, xl_of, P_of, logw_of, N_P):
    """The assertions of the known-answer tests: xl, P and the summed log-weights of every particle within
    generic_model.kat_tolerance of the long-double batch posterior; the data moved the map."""
    tol = gm.kat_tolerance(ref, N_T)
    assert tol < 1e-9, tol
    xl, P, ll = ref["xl"].astype(np.float64), ref["P"].astype(np.float64), float(ref["loglik"])
    xscale = np.max(np.abs(xl)) + np.max(np.abs(xl - p["x0_lin"]))
    assert np.max(np.abs(P - p["P0_lin"])) > 0.1 * ref["P0max"]          # the data moved the map: not a trivial answer
    for i in range(N_P):
        ex, eP, el = np.max(np.abs(xl_of(i) - xl)), np.max(np.abs(P_of(i) - P)), abs(float(np.sum(logw_of(i))) - ll)
        assert ex <= tol * xscale, (i, ex / xscale, tol)
        assert eP <= tol * ref["P0max"], (i, eP / ref["P0max"], tol)
        assert el <= tol * (abs(ll) + ref["M"]), (i, el / (abs(ll) + ref["M"]), tol)
    return tol
